"""The delta survey on the MI355X: gpuar_hip_survey_delta / gpuar_hip_survey_delta_batch, batch.survey_delta, delta="survey" and
`gpuar c --delta=auto`.

The oracle is the composition that already ships and is pinned elsewhere: row j of the delta survey of x is, by definition,
estimate_host(split_delta_host(x, w_j)).  Every comparison is exact; every status word is read and a canary sits behind each
of the four rows."""
import os
import subprocess

import numpy as np
import pytest

import delta_ref as D
from test_delta_survey_host import oracle
from test_survey_host import KINDS, MIB, WIDTHS, data_of, one_mib, totals_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")
HOST_CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")
PACKET = 8192
SG = 8 * PACKET
CANARY = 0x5A5A5A5A
PAD = 2                                      # canaries behind every row
LENGTHS = [1, 15, 16, 17, 8191, 8192, 8193, 16384, 16385, 32768, 65535, 65536, 65537, SG + 3 * PACKET + 77, 3 * SG + 24653]
KINDS = KINDS + ["sorted"]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


def kind_of(kind, n, seed=0):
    """test_survey_host's kinds and a sorted int64 walk: what the filter is for (constant high planes, borrows in the low ones)"""
    if kind == "sorted":
        return np.cumsum(np.random.default_rng(7 + seed).integers(0, 64, n // 8 + 1)).astype(np.int64).view(np.uint8)[:n].copy()
    return data_of(kind, n, seed)


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _rows(npk):
    return torch.full((4, npk + PAD), CANARY, dtype=torch.int32, device="cuda")


def _check_rows(d_est, npk, want, what):
    """want[j]: the row of width j, or None for a row that was not asked for and keeps its canary"""
    got = d_est.cpu().tolist()
    for j in range(4):
        assert got[j][:npk] == (want[j] if want[j] is not None else [CANARY] * npk), (what, WIDTHS[j])
        assert got[j][npk:] == [CANARY] * PAD, (what, WIDTHS[j], "wrote behind the row")


@pytest.mark.parametrize("kind", KINDS)
def test_one_buffer_is_the_estimate_of_every_filtered_split_at_every_length(H, kind):
    for n in LENGTHS:
        host = kind_of(kind, n)
        npk = H.packet_count(n)
        d_est = _rows(npk)
        H.survey_delta(torch.from_numpy(host).cuda(), d_est=d_est)
        _check_rows(d_est, npk, oracle(H, host), (kind, n))
    assert H.status() == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_a_single_width_leaves_the_other_rows_alone(H, w):
    for kind in ("sorted", "uniform", "by_eighth", "last_differs"):
        for n in (8193, 65536, SG + 3 * PACKET + 77, 3 * SG + 24653):
            host = kind_of(kind, n)
            npk = H.packet_count(n)
            d_est = _rows(npk)
            H.survey_delta(torch.from_numpy(host).cuda(), d_est=d_est, widths=(w,))
            _check_rows(d_est, npk, oracle(H, host, (w,)), (kind, n, w))
    assert H.status() == 0


def test_borrows_through_every_byte_and_across_planes(H):
    for kind in ("ramp", "ones"):
        for w in WIDTHS:
            n = 2 * SG + w * PACKET + 4097
            host = D.bytes_of(kind, n, w)
            npk = H.packet_count(n)
            d_est = _rows(npk)
            H.survey_delta(torch.from_numpy(host).cuda(), d_est=d_est)
            _check_rows(d_est, npk, oracle(H, host), (kind, w))
    assert H.status() == 0


def test_more_supergroups_than_workgroups_are_resident(H):
    """1100 supergroups and a tail, sorted int64 and zeros in alternating supergroups: the 512 persistent workgroups go round more
    than twice."""
    n_sg = 1100
    walk = kind_of("sorted", (n_sg // 2 + 1) * SG)
    host = np.zeros(n_sg * SG + 3 * PACKET + 1001, dtype=np.uint8)
    blocks = host[:n_sg * SG].reshape(n_sg, SG)
    blocks[0::2] = walk[:n_sg // 2 * SG].reshape(-1, SG)
    host[n_sg * SG:] = walk[n_sg // 2 * SG:n_sg // 2 * SG + host.size - n_sg * SG]
    npk = H.packet_count(host.size)
    d_est = _rows(npk)
    H.survey_delta(torch.from_numpy(host).cuda(), d_est=d_est)
    _check_rows(d_est, npk, oracle(H, host), "1100 supergroups")
    assert H.status() == 0


def test_more_short_buffers_than_one_pass_of_the_grid(H):
    """70 000 buffers of 64 bytes in one call: every supergroup is a short tail, eight of them start in every window."""
    n, size = 70000, 64
    rng = np.random.default_rng(9)
    host = rng.integers(0, 256, n * size, dtype=np.uint8) & rng.choice(np.array([0xFF, 0x0F, 0x01, 0x00], dtype=np.uint8), n).repeat(size)
    data = torch.from_numpy(host).cuda()
    ptrs = data.data_ptr() + size * torch.arange(n, dtype=torch.int64, device="cuda")
    sizes = torch.full((n,), size, dtype=torch.int64, device="cuda")
    fp = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    status = _status()
    d_est = _rows(n)
    H.survey_delta_batch(ptrs, sizes, fp, n, n, d_est=d_est, d_status=status)
    assert int(status.item()) == 0
    # a buffer of 64 bytes is one packet at every width and the split only permutes its bytes: row j is the estimate of the
    # buffer's differences at width j (the first element of every buffer as it is), formed here for all buffers at once
    raw = host.tobytes()
    rows = []
    for w in WIDTHS:
        v = host.reshape(n, size).view("<u%d" % w)
        d = v.copy()
        d[:, 1:] = v[:, 1:] - v[:, :-1]
        flat = d.view(np.uint8).tobytes()
        rows.append([H.estimate_host(flat[i * size:(i + 1) * size])[0] for i in range(n)])
    for i in (0, 1, n // 2, n - 1):
        assert [row[0] for row in oracle(H, raw[i * size:(i + 1) * size])] == [row[i] for row in rows]
    _check_rows(d_est, n, rows, "70000 buffers")


def _batch(H, hosts):
    """The buffers back to back (each 16-byte aligned) on the device and their descriptors."""
    offs, at = [], 0
    for h in hosts:
        offs.append(at)
        at += (h.size + 15) // 16 * 16
    data = torch.zeros(max(at, 16), dtype=torch.uint8, device="cuda")
    for o, h in zip(offs, hosts):
        data[o:o + h.size] = torch.from_numpy(h).cuda()
    sizes = [h.size for h in hosts]
    fp, npk = H.batch_packet_count(sizes)
    return data, offs, sizes, fp, npk


def test_a_batch_gives_what_its_buffers_give_alone(H):
    rng = np.random.default_rng(5)
    sizes = [0, 1, 17, 3000, 8192, 8193, 8191, 16384, 0, 3 * 8192 + 5] + [int(v) for v in rng.integers(0, 40000, 53)] + [65536, 65537]
    assert len(sizes) == 65
    hosts = [kind_of(KINDS[i % len(KINDS)], n, seed=i) if n else np.empty(0, dtype=np.uint8) for i, n in enumerate(sizes)]
    data, offs, sizes, fp, npk = _batch(H, hosts)
    n = len(sizes)
    desc = torch.tensor([data.data_ptr() + o for o in offs] + sizes + fp, dtype=torch.int64, device="cuda")
    status = _status()
    d_est = _rows(npk)
    H.survey_delta_batch(desc[:n], desc[n:2 * n], desc[2 * n:], n, npk, d_est=d_est, d_status=status)
    assert int(status.item()) == 0
    got = d_est.cpu().tolist()
    for j in range(4):
        assert got[j][npk:] == [CANARY] * PAD
    for b, (o, h) in enumerate(zip(offs, hosts)):
        want = oracle(H, h)
        assert [got[j][fp[b]:fp[b + 1]] for j in range(4)] == want, (b, h.size)
        if h.size:
            assert H.survey_delta(data[o:o + h.size]).cpu().tolist() == want, (b, h.size)
    assert H.status() == 0


def test_an_unusable_descriptor_is_bad_batch_and_its_columns_keep_their_canary(H):
    hosts = [kind_of("text", 2 * PACKET + 9), kind_of("sorted", SG + PACKET + 1), kind_of("zeros", 3 * PACKET)]
    data, offs, sizes, fp, npk = _batch(H, hosts)
    ptrs = [data.data_ptr() + o for o in offs]
    assert fp == [0, 3, 13, 16]

    def call(ptrs, fp=fp, npk=npk):
        desc = torch.tensor(ptrs + sizes + fp, dtype=torch.int64, device="cuda")
        status = _status()
        d_est = _rows(npk)
        H.survey_delta_batch(desc[:3], desc[3:6], desc[6:], 3, npk, d_est=d_est, d_status=status)
        got = d_est.cpu().tolist()
        for j in range(4):
            assert got[j][npk:] == [CANARY] * PAD
        return int(status.item()), [row[:npk] for row in got]

    want = [oracle(H, h) for h in hosts]
    flags, got = call(ptrs)
    assert flags == 0 and got == [want[0][j] + want[1][j] + want[2][j] for j in range(4)]
    flags, got = call([ptrs[0], ptrs[1] + 8, ptrs[2]])                      # a misaligned buffer: all ten of its packets
    assert flags == H.STATUS_BAD_BATCH
    assert got == [want[0][j] + [CANARY] * 10 + want[2][j] for j in range(4)]
    flags, got = call(ptrs, [0, 3, 14, 17], 17)                             # buffer 1 owns a packet past its end: the whole buffer
    assert flags == H.STATUS_BAD_BATCH
    assert got == [want[0][j] + [CANARY] * 11 + want[2][j] for j in range(4)]


def test_the_host_side_checks(H):
    lib = H.load()
    d = torch.zeros(2 * PACKET, dtype=torch.uint8, device="cuda")
    est = torch.full((16,), CANARY, dtype=torch.int32, device="cuda")
    desc = torch.zeros(8, dtype=torch.int64, device="cuda")
    p, e, q = d.data_ptr(), est.data_ptr(), desc.data_ptr()
    assert lib.gpuar_hip_survey_delta(None, 0, 0, None, 0, None) == 0                      # nothing to do comes first
    assert lib.gpuar_hip_survey_delta(None, PACKET, 15, e, 1, None) == -2 and lib.gpuar_hip_survey_delta(p, PACKET, 15, None, 1, None) == -2
    assert lib.gpuar_hip_survey_delta(p, 2 * PACKET, 15, e, 1, None) == -2                 # a stride below the packet count
    assert lib.gpuar_hip_survey_delta(p, PACKET, 0, e, 1, None) == -2 and lib.gpuar_hip_survey_delta(p, PACKET, 16, e, 1, None) == -2
    assert lib.gpuar_hip_survey_delta(p + 4, PACKET, 15, e, 1, None) == -1 and lib.gpuar_hip_survey_delta(p, PACKET, 15, e + 2, 1, None) == -1
    assert lib.gpuar_hip_survey_delta_batch(None, None, None, 1, 0, 0, None, 0, None, None) == 0
    assert lib.gpuar_hip_survey_delta_batch(None, q, q, 1, 1, 15, e, 1, None, None) == -2
    assert lib.gpuar_hip_survey_delta_batch(q, q, q, 1, 1, 15, None, 1, None, None) == -2
    assert lib.gpuar_hip_survey_delta_batch(q, q, q, 1, 2, 15, e, 1, None, None) == -2
    assert lib.gpuar_hip_survey_delta_batch(q, q, q, 1, 1, 0, e, 1, None, None) == -2
    assert lib.gpuar_hip_survey_delta_batch(q, q, q, 1, 1, 0x11, e, 1, None, None) == -2
    assert lib.gpuar_hip_survey_delta_batch(q + 4, q, q, 1, 1, 15, e, 1, None, None) == -1
    assert lib.gpuar_hip_survey_delta_batch(q, q, q, 1, 1, 15, e + 2, 1, None, None) == -1
    torch.cuda.synchronize()
    assert est.cpu().tolist() == [CANARY] * 16


@pytest.fixture(scope="module")
def table(H):
    """The nine 1 MiB inputs of DESIGN.md 4.9's table: (names, element widths, host bytes, tensors of their own type)."""
    inputs = D.table_inputs()
    names = list(inputs)
    return names, [inputs[k][1] for k in names], [D.raw_bytes(inputs[k][0]) for k in names], [torch.from_numpy(inputs[k][0]).cuda() for k in names]


def test_batch_survey_delta_is_the_filtered_estimate_at_every_width(H, table):
    from gpuar_amd import batch
    _names, _widths, hosts, tensors = table
    tensors = tensors + [torch.empty(0, dtype=torch.uint8, device="cuda"), torch.from_numpy(kind_of("sorted", 3000)).cuda()]
    hosts = hosts + [np.empty(0, dtype=np.uint8), kind_of("sorted", 3000)]
    for stored in (None, "auto"):
        got = batch.survey_delta(tensors, stored=stored)
        per_width = [batch.estimate(tensors, planes=w, delta=True, stored=stored) for w in WIDTHS]
        assert got == [[per_width[j][b] for j in range(4)] for b in range(len(tensors))], stored
        assert got == [totals_of(oracle(H, h), h.size, stored == "auto") for h in hosts], stored
    some = batch.survey_delta(tensors, widths=(2, 8))
    assert some == [[None, row[1], None, row[3]] for row in batch.survey_delta(tensors)]
    with pytest.raises(H.GpuarError):
        batch.survey_delta(tensors, widths=(3,))


def test_delta_survey_flags_what_delta_auto_flags(H, table):
    from gpuar_amd import batch
    names, widths, hosts, tensors = table
    survey = batch.compress(tensors, planes=widths, delta="survey")
    auto = batch.compress(tensors, planes=widths, delta="auto")
    assert survey.delta == auto.delta == [name in D.TABLE_DELTA_WINS for name in names]
    assert survey.planes == auto.planes == widths
    assert torch.equal(survey.stream, auto.stream) and torch.equal(survey.offsets, auto.offsets)
    assert batch.estimate(tensors, planes=widths, delta="survey") == batch.estimate(tensors, planes=widths, delta="auto")
    for w in WIDTHS:                                            # one width for all: the widths the inputs were not made for, too
        assert batch.compress(tensors, planes=w, delta="survey").delta == batch.compress(tensors, planes=w, delta="auto").delta, w
    assert batch.compress(tensors, delta="survey").delta == batch.compress(tensors, delta="auto").delta       # planes=None: bytes
    for kwargs in ({"checksum": True}, {"stored": "auto"}):
        c = batch.compress(tensors, planes=widths, delta="survey", **kwargs)
        assert c.delta == auto.delta
        for h, out in zip(hosts, batch.decompress(c)):
            assert np.array_equal(out.cpu().numpy(), h), kwargs
    with pytest.raises(H.GpuarError):
        batch.compress(tensors, delta="survey", base=[None] * len(tensors))
    with pytest.raises(H.GpuarError):
        batch.compress(tensors, delta="measure")


def test_width_and_filter_are_chosen_together(H, table):
    from gpuar_amd import batch
    names, _widths, hosts, _tensors = table
    views = [torch.from_numpy(h).cuda() for h in hosts] + [torch.empty(0, dtype=torch.uint8, device="cuda")]      # uint8 views: no dtype to go by
    hosts = hosts + [np.empty(0, dtype=np.uint8)]
    at = names.index("position_ids")
    joint = batch.compress(views, planes="survey", delta="survey")
    want = [H.choose_filter(totals_of(H.survey_planes_host(h.tobytes()), h.size), totals_of(oracle(H, h), h.size), H.packet_count(h.size)) for h in hosts]
    assert list(zip(joint.planes, joint.delta)) == want
    assert want[at] == (4, True) and want[-1] == (1, False)
    fixed = batch.compress(views, planes=joint.planes, delta=joint.delta)
    assert torch.equal(joint.stream, fixed.stream) and torch.equal(joint.offsets, fixed.offsets)
    blind = batch.compress(views, planes="survey", delta="auto")
    assert (blind.planes[at], blind.delta[at]) == (8, True)
    one_joint = batch.compress([views[at]], planes="survey", delta="survey")
    one_blind = batch.compress([views[at]], planes="survey", delta="auto")
    assert (one_joint.planes, one_joint.delta, one_blind.planes, one_blind.delta) == ([4], [True], [8], [True])
    assert one_joint.nbytes < one_blind.nbytes
    assert batch.estimate(views, planes="survey", delta="survey") == batch.estimate(views, planes=joint.planes, delta=joint.delta)
    for kwargs in ({"checksum": True}, {"stored": "auto"}):
        c = batch.compress(views, planes="survey", delta="survey", **kwargs)
        assert (c.planes[at], c.delta[at]) == (4, True)
        for h, out in zip(hosts, batch.decompress(c)):
            assert np.array_equal(out.cpu().numpy(), h), kwargs


@pytest.mark.parametrize("name", ["position_ids", "uniform"])
def test_the_cli_on_the_gpu_writes_the_hosts_file(H, tmp_path, name):
    src, host_gip = tmp_path / "in.dat", tmp_path / "host.gip"
    x = D.raw_bytes(D.table_inputs()[name][0]) if name == "position_ids" else one_mib(name)
    assert x.size == MIB
    x.tofile(src)
    r = subprocess.run([HOST_CLI, "c", "--host", "--delta=auto", "--planes=auto", f"--in={src}", f"--out={host_gip}"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert ("delta=auto: filter on, width 4 " if name == "position_ids" else "delta=auto: filter off, width 1 ") in r.stdout
    env = dict(os.environ, GPUAR_OVERSUBSCRIBE_DEVICES="1")
    for tag, flag in (("batch", "--batch=64"), ("gpus", "--gpus=2")):
        gip = tmp_path / f"{tag}.gip"
        r = subprocess.run([CLI, "c", "--delta=auto", "--planes=auto", flag, f"--in={src}", f"--out={gip}"], capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Attention" not in r.stdout and "delta=auto: filter" in r.stdout
        assert gip.read_bytes() == host_gip.read_bytes(), (name, flag)
