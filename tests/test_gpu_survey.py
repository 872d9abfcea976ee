"""The plane-width survey on the MI355X: gpuar_hip_survey_planes / gpuar_hip_survey_planes_batch, batch.survey, planes="survey" and
`gpuar c --planes=auto`.

The oracle is the composition that already ships and is pinned elsewhere: row j of the survey of x is, by definition,
estimate_host(split_planes_host(x, w_j)).  Every comparison is exact; every status word is read and a canary sits behind each
of the four rows."""
import os
import subprocess

import numpy as np
import pytest

import planes_ref as PR
from test_survey_host import KINDS, MIB, WIDTHS, data_of, one_mib, oracle, totals_of

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


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _rows(npk):
    return torch.full((4, npk + PAD), CANARY, dtype=torch.int32, device="cuda")


def _check_rows(d_est, npk, want, what):
    got = d_est.cpu().tolist()
    for j in range(4):
        assert got[j][:npk] == want[j], (what, WIDTHS[j])
        assert got[j][npk:] == [CANARY] * PAD, (what, WIDTHS[j], "wrote behind the row")


@pytest.mark.parametrize("kind", KINDS)
def test_one_buffer_is_the_estimate_of_every_split_at_every_length(H, kind):
    for n in LENGTHS:
        host = data_of(kind, n)
        npk = H.packet_count(n)
        d_est = _rows(npk)
        H.survey_planes(torch.from_numpy(host).cuda(), d_est=d_est)
        _check_rows(d_est, npk, oracle(H, host), (kind, n))
    assert H.status() == 0


def test_more_supergroups_than_workgroups_are_resident(H):
    """1100 supergroups and a tail, bf16 and zeros in alternating supergroups: the persistent workgroups go round more than once."""
    n_sg = 1100
    bf16 = PR.typed_input("bf16", (n_sg // 2 + 1) * SG)
    host = np.zeros(n_sg * SG + 3 * PACKET + 1001, dtype=np.uint8)
    blocks = host[:n_sg * SG].reshape(n_sg, SG)
    blocks[0::2] = bf16[:n_sg // 2 * SG].reshape(-1, SG)
    host[n_sg * SG:] = bf16[n_sg // 2 * SG:n_sg // 2 * SG + host.size - n_sg * SG]
    npk = H.packet_count(host.size)
    d_est = _rows(npk)
    H.survey_planes(torch.from_numpy(host).cuda(), d_est=d_est)
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
    H.survey_planes_batch(ptrs, sizes, fp, n, n, d_est=d_est, d_status=status)
    assert int(status.item()) == 0
    raw = host.tobytes()
    # a buffer of 64 bytes is one packet at every width: the split only permutes its bytes
    one = [H.estimate_host(raw[i * size:(i + 1) * size])[0] for i in range(n)]
    for i in (0, 1, n // 2, n - 1):
        assert [row[0] for row in oracle(H, host[i * size:(i + 1) * size])] == [one[i]] * 4
    _check_rows(d_est, n, [one] * 4, "70000 buffers")


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
    hosts = [data_of(KINDS[i % len(KINDS)], n, seed=i) if n else np.empty(0, dtype=np.uint8) for i, n in enumerate(sizes)]
    data, offs, sizes, fp, npk = _batch(H, hosts)
    n = len(sizes)
    desc = torch.tensor([data.data_ptr() + o for o in offs] + sizes + fp, dtype=torch.int64, device="cuda")
    status = _status()
    d_est = _rows(npk)
    H.survey_planes_batch(desc[:n], desc[n:2 * n], desc[2 * n:], n, npk, d_est=d_est, d_status=status)
    assert int(status.item()) == 0
    got = d_est.cpu().tolist()
    for j in range(4):
        assert got[j][npk:] == [CANARY] * PAD
    for b, (o, h) in enumerate(zip(offs, hosts)):
        want = oracle(H, h)
        assert [got[j][fp[b]:fp[b + 1]] for j in range(4)] == want, (b, h.size)
        if h.size:
            assert H.survey_planes(data[o:o + h.size]).cpu().tolist() == want, (b, h.size)
    assert H.status() == 0


def test_an_unusable_descriptor_is_bad_batch_and_its_columns_keep_their_canary(H):
    hosts = [data_of("text", 2 * PACKET + 9), data_of("bf16", SG + PACKET + 1), data_of("zeros", 3 * PACKET)]
    data, offs, sizes, fp, npk = _batch(H, hosts)
    ptrs = [data.data_ptr() + o for o in offs]
    assert fp == [0, 3, 13, 16]

    def call(ptrs, fp=fp, npk=npk):
        desc = torch.tensor(ptrs + sizes + fp, dtype=torch.int64, device="cuda")
        status = _status()
        d_est = _rows(npk)
        H.survey_planes_batch(desc[:3], desc[3:6], desc[6:], 3, npk, d_est=d_est, d_status=status)
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
    assert lib.gpuar_hip_survey_planes(None, 0, None, 0, None) == 0                    # nothing to do comes first
    assert lib.gpuar_hip_survey_planes(None, PACKET, e, 1, None) == -2 and lib.gpuar_hip_survey_planes(p, PACKET, None, 1, None) == -2
    assert lib.gpuar_hip_survey_planes(p, 2 * PACKET, e, 1, None) == -2                # a stride below the packet count
    assert lib.gpuar_hip_survey_planes(p + 4, PACKET, e, 1, None) == -1 and lib.gpuar_hip_survey_planes(p, PACKET, e + 2, 1, None) == -1
    assert lib.gpuar_hip_survey_planes_batch(None, None, None, 1, 0, None, 0, None, None) == 0
    assert lib.gpuar_hip_survey_planes_batch(None, q, q, 1, 1, e, 1, None, None) == -2
    assert lib.gpuar_hip_survey_planes_batch(q, q, q, 1, 1, None, 1, None, None) == -2
    assert lib.gpuar_hip_survey_planes_batch(q, q, q, 1, 2, e, 1, None, None) == -2
    assert lib.gpuar_hip_survey_planes_batch(q + 4, q, q, 1, 1, e, 1, None, None) == -1
    assert lib.gpuar_hip_survey_planes_batch(q, q, q, 1, 1, e + 2, 1, None, None) == -1
    torch.cuda.synchronize()
    assert est.cpu().tolist() == [CANARY] * 16


@pytest.fixture(scope="module")
def typed(H):
    """uint8 views of the 1 MiB bf16, fp32, int64, uniform and text inputs, an empty tensor and one of 3000 bytes: (hosts, tensors)."""
    hosts = [np.ascontiguousarray(one_mib(name)) for name in ("bf16", "fp32", "int64", "uniform", "text")]
    hosts += [np.empty(0, dtype=np.uint8), data_of("bf16", 3000)]
    return hosts, [torch.from_numpy(h).cuda() for h in hosts]


def test_batch_survey_is_the_estimate_at_every_width(H, typed):
    from gpuar_amd import batch
    hosts, tensors = typed
    for stored in (None, "auto"):
        got = batch.survey(tensors, stored=stored)
        per_width = [batch.estimate(tensors, planes=w, stored=stored) for w in WIDTHS]
        assert got == [[per_width[j][b] for j in range(4)] for b in range(len(tensors))], stored
        assert got == [totals_of(oracle(H, h), h.size, stored == "auto") for h in hosts], stored


def test_planes_survey_compresses_as_the_chosen_widths_do(H, typed):
    from gpuar_amd import batch
    hosts, tensors = typed
    small = hosts[-1]
    widths = [2, 4, 8, 1, 1, 1, H.choose_planes(totals_of(oracle(H, small), small.size), 1)]
    c = batch.compress(tensors, planes="survey")
    assert c.planes == widths
    fixed = batch.compress(tensors, planes=widths)
    assert torch.equal(c.stream, fixed.stream) and torch.equal(c.offsets, fixed.offsets)
    for kwargs in ({}, {"checksum": True}, {"stored": "auto"}):
        cc = batch.compress(tensors, planes="survey", **kwargs)
        assert cc.planes[:6] == widths[:6]
        for h, out in zip(hosts, batch.decompress(cc)):
            assert np.array_equal(out.cpu().numpy(), h), kwargs
    assert batch.estimate(tensors, planes="survey") == batch.estimate(tensors, planes=widths)
    assert batch.plane_widths(tensors, "auto") == [1] * len(tensors)         # the dtype rule sees bytes


@pytest.mark.parametrize("name", ["bf16", "uniform"])
def test_the_cli_on_the_gpu_writes_the_hosts_file(H, tmp_path, name):
    src, host_gip = tmp_path / "in.dat", tmp_path / "host.gip"
    one_mib(name).tofile(src)
    r = subprocess.run([HOST_CLI, "c", "--host", "--planes=auto", f"--in={src}", f"--out={host_gip}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, GPUAR_OVERSUBSCRIBE_DEVICES="1")
    for tag, flag in (("batch", "--batch=64"), ("gpus", "--gpus=2")):
        gip = tmp_path / f"{tag}.gip"
        r = subprocess.run([CLI, "c", "--planes=auto", flag, f"--in={src}", f"--out={gip}"], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Attention" not in r.stdout and "planes=auto: width" in r.stdout
        assert gip.read_bytes() == host_gip.read_bytes(), (name, flag)
