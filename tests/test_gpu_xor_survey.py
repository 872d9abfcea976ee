"""The XOR-base survey on the MI355X: gpuar_hip_survey_xor / gpuar_hip_survey_xor_batch.

Two oracles, both exact.  The host twin (gpuar_hip_survey_xor_host, pinned against a numpy restatement in test_xor_survey_host.py),
and, where the buffers are too large for the host, the kernels that were there before, on the device: with y = x ^ b the est rows
are survey_planes(y) and scan row j is sparse_scan(split_planes(y, w_j)).  Every status word is read and canaries sit behind the
rows."""
import numpy as np
import pytest

import xor_survey_ref as XS
from test_survey_host import KINDS, WIDTHS, data_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
SG = 8 * PACKET
CANARY = 0x5A5A5A5A
PAD = 2                                      # canaries behind every row
# tests/test_gpu_survey.py's lengths, and tails with (n mod G) mod w != 0
LENGTHS = [1, 15, 16, 17, 8191, 8192, 8193, 16384, 16385, 32768, 65535, 65536, 65537, SG + 3 * PACKET + 77, 3 * SG + 24653,
           3 * SG + 5 * PACKET + 4099]


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


def _u32(rows):
    return [[v & 0xFFFFFFFF for v in row] for row in rows]


def _check_rows(d_rows, npk, want, what):
    got = _u32(d_rows.cpu().tolist())
    for j in range(4):
        assert got[j][:npk] == want[j], (what, WIDTHS[j])
        assert got[j][npk:] == [CANARY] * PAD, (what, WIDTHS[j], "wrote behind the row")


def _base_of(kind, n):
    """a base for data_of(kind, n): unrelated in the first half of every packet pair, equal to the buffer elsewhere"""
    x = data_of(kind, n)
    b = x.copy()
    other = data_of("uniform", n, seed=11)
    pick = (np.arange(n) // (PACKET // 2)) % 3 == 0
    b[pick] = other[pick]
    return x, b


def _device_oracle(H, d_x, d_b):
    """(est rows, scan rows) as int32 tensors (4, packets), from the plane survey and the scan of the plane splits of x ^ b"""
    y = torch.bitwise_xor(d_x, d_b)
    est = H.survey_planes(y)
    scan = torch.stack([H.sparse_scan(H.split_planes(y, w)).view(torch.int32) for w in WIDTHS])
    return est, scan


@pytest.mark.parametrize("kind", KINDS)
def test_one_buffer_is_the_host_twin_in_both_rows_at_every_length(H, kind):
    for n in LENGTHS:
        x, b = _base_of(kind, n)
        npk = H.packet_count(n)
        d_est, d_scan = _rows(npk), _rows(npk)
        d_x, d_b = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
        H.survey_xor(d_x, d_b, d_est=d_est, d_scan=d_scan)
        want_est, want_scan = H.survey_xor_host(x.tobytes(), b.tobytes())
        _check_rows(d_est, npk, want_est, (kind, n, "est"))
        _check_rows(d_scan, npk, want_scan, (kind, n, "scan"))
        if n >= PACKET:                                     # the device checker agrees (its supergroups are the same: one buffer)
            est, scan = _device_oracle(H, d_x, d_b)
            assert torch.equal(d_est[:, :npk], est) and torch.equal(d_scan[:, :npk], scan), (kind, n)
    assert H.status() == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_the_scan_edges(H, w):
    j = WIDTHS.index(w)
    for tag, x, b, packet, want in XS.scan_edges(w):
        npk = H.packet_count(x.size)
        d_est, d_scan = _rows(npk), _rows(npk)
        H.survey_xor(torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda(), d_est=d_est, d_scan=d_scan)
        want_est, want_scan = H.survey_xor_host(x.tobytes(), b.tobytes())
        _check_rows(d_est, npk, want_est, (w, tag, "est"))
        _check_rows(d_scan, npk, want_scan, (w, tag, "scan"))
        if tag in ("equal to its base", "fill 0x5A everywhere"):
            assert want_scan == [[want] * npk] * 4, (w, tag)
        else:
            assert want_scan[j][packet] == want, (w, tag)
    assert H.status() == 0


def test_a_missing_output_is_not_written_and_the_other_is_the_same(H):
    x, b = _base_of("bf16", SG + 3 * PACKET + 77)
    npk = H.packet_count(x.size)
    d_x, d_b = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
    want_est, want_scan = H.survey_xor_host(x.tobytes(), b.tobytes())
    d_est = _rows(npk)
    assert H.survey_xor(d_x, d_b, d_est=d_est, d_scan=False) == (d_est, None)
    _check_rows(d_est, npk, want_est, "est alone")
    d_scan = _rows(npk)
    assert H.survey_xor(d_x, d_b, d_est=False, d_scan=d_scan)[0] is None
    _check_rows(d_scan, npk, want_scan, "scan alone")
    est, scan = H.survey_xor(d_x, d_b)
    assert _u32(est.cpu().tolist()) == want_est and _u32(scan.cpu().tolist()) == want_scan
    with pytest.raises(H.GpuarError):
        H.survey_xor(d_x, d_b, d_est=False, d_scan=False)
    with pytest.raises(H.GpuarError):
        H.survey_xor(d_x, d_b[:-1])
    assert H.status() == 0


def test_more_supergroups_than_workgroups_are_resident(H):
    """1100 supergroups and a tail, alternately equal to the base and unrelated to it: the persistent workgroups go round more
    than once.  Checked on the device, and the first, a middle and the last supergroups against the host twin."""
    n_sg = 1100
    n = n_sg * SG + 3 * PACKET + 1001
    g = torch.Generator(device="cuda").manual_seed(3)
    d_x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    d_b = d_x.clone()
    blocks = d_b[:n_sg * SG].view(n_sg, SG)
    blocks[1::2] = torch.randint(0, 256, (n_sg // 2, SG), dtype=torch.uint8, device="cuda", generator=g)
    npk = H.packet_count(n)
    d_est, d_scan = _rows(npk), _rows(npk)
    H.survey_xor(d_x, d_b, d_est=d_est, d_scan=d_scan)
    est, scan = _device_oracle(H, d_x, d_b)
    assert torch.equal(d_est[:, :npk], est) and torch.equal(d_scan[:, :npk], scan)
    assert d_est[:, npk:].eq(CANARY).all() and d_scan[:, npk:].eq(CANARY).all()
    assert d_scan[:, 0:8].eq(0).all() and d_scan[:, 8:16].eq(-1).all()          # equal to the base: fill 0, k = 0; unrelated: none
    for first_sg, count in ((0, 2), (511, 3), (1098, 3)):                       # (the last one with the tail)
        lo, hi = first_sg * SG, min(n, (first_sg + count) * SG)
        want_est, want_scan = H.survey_xor_host(d_x[lo:hi].cpu().numpy().tobytes(), d_b[lo:hi].cpu().numpy().tobytes())
        p0, p1 = lo // PACKET, H.packet_count(hi)
        assert _u32(d_est[:, p0:p1].cpu().tolist()) == want_est and _u32(d_scan[:, p0:p1].cpu().tolist()) == want_scan, first_sg
    assert H.status() == 0


def test_more_short_buffers_than_one_pass_of_the_grid(H):
    """70 000 buffers of 64 bytes in one call, bases alternately present and 0: every supergroup is a short tail, eight of them
    start in every window."""
    n, size = 70000, 64
    rng = np.random.default_rng(9)
    x = rng.integers(0, 256, n * size, dtype=np.uint8) & rng.choice(np.array([0xFF, 0x0F, 0x01, 0x00], dtype=np.uint8), n).repeat(size)
    b = x.copy()
    flip = rng.random(n * size) < 0.3
    b[flip] ^= 0x5A
    d_x, d_b = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
    at = size * torch.arange(n, dtype=torch.int64, device="cuda")
    ptrs = d_x.data_ptr() + at
    bases = (d_b.data_ptr() + at) * (torch.arange(n, device="cuda") % 2 == 0)
    sizes = torch.full((n,), size, dtype=torch.int64, device="cuda")
    fp = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    status = _status()
    d_est, d_scan = _rows(n), _rows(n)
    H.survey_xor_batch(ptrs, sizes, fp, bases, n, n, d_est=d_est, d_scan=d_scan, d_status=status)
    assert int(status.item()) == 0
    # a buffer of 64 bytes is one packet at every width: the split only permutes its bytes
    y = x.copy().reshape(n, size)
    y[0::2] ^= b.reshape(n, size)[0::2]
    values = [XS.packet_values(row) for row in y]
    _check_rows(d_est, n, [[v[0] for v in values]] * 4, "70000 buffers, est")
    _check_rows(d_scan, n, [[v[1] for v in values]] * 4, "70000 buffers, scan")
    for i in (0, 1, n // 2, n - 1):
        base = b[i * size:(i + 1) * size] if i % 2 == 0 else np.zeros(size, dtype=np.uint8)
        est, scan = H.survey_xor_host(x[i * size:(i + 1) * size].tobytes(), base.tobytes())
        assert [r[0] for r in est] == [values[i][0]] * 4 and [r[0] for r in scan] == [values[i][1]] * 4


def _batch(H, hosts):
    """The buffers back to back (each 16-byte aligned) on the device: (tensor, offsets)"""
    offs, at = [], 0
    for h in hosts:
        offs.append(at)
        at += (h.size + 15) // 16 * 16
    data = torch.zeros(max(at, 16), dtype=torch.uint8, device="cuda")
    for o, h in zip(offs, hosts):
        data[o:o + h.size] = torch.from_numpy(h).cuda()
    return data, offs


def test_a_batch_gives_what_its_buffers_give_alone(H):
    rng = np.random.default_rng(5)
    sizes = [0, 1, 17, 3000, 8192, 8193, 8191, 16384, 0, 3 * 8192 + 5] + [int(v) for v in rng.integers(0, 40000, 53)] + [65536, 65537]
    pairs = [_base_of(KINDS[i % len(KINDS)], n) if n else (np.empty(0, dtype=np.uint8),) * 2 for i, n in enumerate(sizes)]
    based = [i % 3 != 1 for i in range(len(sizes))]                          # every third buffer has no base
    data, offs = _batch(H, [p[0] for p in pairs])
    bdata, boffs = _batch(H, [p[1] for p in pairs])
    fp, npk = H.batch_packet_count(sizes)
    n = len(sizes)
    desc = torch.tensor([data.data_ptr() + o for o in offs] + sizes + fp + [bdata.data_ptr() + o if on else 0 for o, on in zip(boffs, based)],
                        dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    status = _status()
    d_est, d_scan = _rows(npk), _rows(npk)
    side.wait_stream(torch.cuda.current_stream())
    H.survey_xor_batch(desc[:n], desc[n:2 * n], desc[2 * n:3 * n + 1], desc[3 * n + 1:], n, npk, d_est=d_est, d_scan=d_scan, d_status=status, stream=side)
    side.synchronize()
    assert int(status.item()) == 0                                           # a side stream with a status word of its own
    got_est, got_scan = _u32(d_est.cpu().tolist()), _u32(d_scan.cpu().tolist())
    for j in range(4):
        assert got_est[j][npk:] == [CANARY] * PAD and got_scan[j][npk:] == [CANARY] * PAD
    for i, ((x, b), on, o, bo) in enumerate(zip(pairs, based, offs, boffs)):
        want_est, want_scan = H.survey_xor_host(x.tobytes(), (b if on else np.zeros_like(x)).tobytes())
        assert [got_est[j][fp[i]:fp[i + 1]] for j in range(4)] == want_est, (i, x.size)
        assert [got_scan[j][fp[i]:fp[i + 1]] for j in range(4)] == want_scan, (i, x.size)
        if x.size and on:
            est, scan = H.survey_xor(data[o:o + x.size], bdata[bo:bo + x.size])
            assert _u32(est.cpu().tolist()) == want_est and _u32(scan.cpu().tolist()) == want_scan, (i, x.size)
        if x.size and not on:                                                # no base: the plane survey's rows
            assert H.survey_planes(data[o:o + x.size]).cpu().tolist() == want_est, (i, x.size)
    # one output alone: the other's canaries stay
    d_est, d_scan = _rows(npk), _rows(npk)
    H.survey_xor_batch(desc[:n], desc[n:2 * n], desc[2 * n:3 * n + 1], desc[3 * n + 1:], n, npk, d_est=d_est, d_scan=False, d_status=status)
    H.survey_xor_batch(desc[:n], desc[n:2 * n], desc[2 * n:3 * n + 1], desc[3 * n + 1:], n, npk, d_est=False, d_scan=d_scan, d_status=status)
    assert _u32(d_est.cpu().tolist()) == got_est and _u32(d_scan.cpu().tolist()) == got_scan
    assert int(status.item()) == 0 and H.status() == 0


def test_an_unusable_descriptor_is_bad_batch_and_its_columns_keep_their_canary_in_both_outputs(H):
    pairs = [_base_of("text", 2 * PACKET + 9), _base_of("bf16", SG + PACKET + 1), _base_of("zeros", 3 * PACKET)]
    data, offs = _batch(H, [p[0] for p in pairs])
    bdata, boffs = _batch(H, [p[1] for p in pairs])
    sizes = [p[0].size for p in pairs]
    fp, npk = H.batch_packet_count(sizes)
    ptrs, bases = [data.data_ptr() + o for o in offs], [bdata.data_ptr() + o for o in boffs]
    assert fp == [0, 3, 13, 16]

    def call(ptrs, bases, fp=fp, npk=npk, **outputs):
        desc = torch.tensor(ptrs + sizes + fp + bases, dtype=torch.int64, device="cuda")
        status = _status()
        d_est, d_scan = _rows(npk), _rows(npk)
        H.survey_xor_batch(desc[:3], desc[3:6], desc[6:10], desc[10:], 3, npk, **{"d_est": d_est, "d_scan": d_scan, **outputs}, d_status=status)
        got = [_u32(t.cpu().tolist()) for t in (d_est, d_scan)]
        for rows in got:
            for j in range(4):
                assert rows[j][npk:] == [CANARY] * PAD
        return int(status.item()), [[row[:npk] for row in rows] for rows in got]

    want = [H.survey_xor_host(x.tobytes(), b.tobytes()) for x, b in pairs]                # [buffer][est | scan][j]

    def joined(middle):
        return [[want[0][k][j] + (want[1][k][j] if middle is None else [CANARY] * middle) + want[2][k][j] for j in range(4)] for k in range(2)]

    flags, got = call(ptrs, bases)
    assert flags == 0 and got == joined(None)
    flags, got = call(ptrs, [bases[0], bases[1] + 8, bases[2]])                           # a misaligned base: all ten of its packets
    assert flags == H.STATUS_BAD_BATCH and got == joined(10)
    flags, got = call([ptrs[0], ptrs[1] + 8, ptrs[2]], bases)                             # a misaligned buffer
    assert flags == H.STATUS_BAD_BATCH and got == joined(10)
    flags, got = call(ptrs, bases, [0, 3, 14, 17], 17)                                    # buffer 1 owns a packet past its end
    assert flags == H.STATUS_BAD_BATCH and got == joined(11)
    flags, got = call(ptrs, [bases[0], bases[1] + 8, bases[2]], d_scan=False)             # an output that was not asked for
    assert flags == H.STATUS_BAD_BATCH and got[0] == joined(10)[0]
    assert H.status() == 0


def test_one_buffer_and_its_base_past_4_gib(H):
    """4 GiB + 2 supergroups + 4099 bytes: packet indices and byte offsets beyond 32 bits.  The est rows and the scan row of width 8
    against the kernels that were there before over the whole buffer; the supergroups either side of 2^32 against the host twin."""
    n = (1 << 32) + 2 * SG + 4099
    g = torch.Generator(device="cuda").manual_seed(4)
    d_x = H.generate("uniform", 34, n)
    d_b = d_x.clone()
    d_b[SG::3 * SG] ^= 0x21                                                  # one byte in every third supergroup ...
    for lo in ((1 << 32) - SG - 4096, (1 << 32) + SG + 100):                  # ... and a stretch of noise either side of the line
        d_b[lo:lo + 3 * PACKET] = torch.randint(0, 256, (3 * PACKET,), dtype=torch.uint8, device="cuda", generator=g)
    npk = H.packet_count(n)
    d_est, d_scan = _rows(npk), _rows(npk)
    H.survey_xor(d_x, d_b, d_est=d_est, d_scan=d_scan)
    y = torch.bitwise_xor(d_x, d_b)
    assert torch.equal(d_est[:, :npk], H.survey_planes(y))
    assert torch.equal(d_scan[3, :npk], H.sparse_scan(H.split_planes(y, 8)).view(torch.int32))
    assert d_est[:, npk:].eq(CANARY).all() and d_scan[:, npk:].eq(CANARY).all()
    del y
    lo, hi = (1 << 32) - 2 * SG, n
    want_est, want_scan = H.survey_xor_host(d_x[lo:hi].cpu().numpy().tobytes(), d_b[lo:hi].cpu().numpy().tobytes())
    p0 = lo // PACKET
    assert _u32(d_est[:, p0:npk].cpu().tolist()) == want_est and _u32(d_scan[:, p0:npk].cpu().tolist()) == want_scan
    assert H.status() == 0


def test_the_host_side_checks(H):
    lib = H.load()
    d = torch.zeros(2 * PACKET, dtype=torch.uint8, device="cuda")
    rows = torch.full((32,), CANARY, dtype=torch.int32, device="cuda")
    desc = torch.zeros(8, dtype=torch.int64, device="cuda")
    p, e, s, q = d.data_ptr(), rows.data_ptr(), rows.data_ptr() + 64, desc.data_ptr()
    assert lib.gpuar_hip_survey_xor(None, None, 0, None, None, 0, None) == 0              # nothing to do comes first
    assert lib.gpuar_hip_survey_xor(p, None, PACKET, e, s, 1, None) == -2 and lib.gpuar_hip_survey_xor(p, p, PACKET, None, None, 1, None) == -2
    assert lib.gpuar_hip_survey_xor(p, p, 2 * PACKET, e, s, 1, None) == -2                # a stride below the packet count
    assert lib.gpuar_hip_survey_xor(p, p + 8, PACKET, e, s, 1, None) == -1 and lib.gpuar_hip_survey_xor(p, p, PACKET, e, s + 2, 1, None) == -1
    assert lib.gpuar_hip_survey_xor_batch(None, None, None, None, 1, 0, None, None, 0, None, None) == 0
    assert lib.gpuar_hip_survey_xor_batch(q, q, q, None, 1, 1, e, s, 1, None, None) == -2
    assert lib.gpuar_hip_survey_xor_batch(q, q, q, q, 1, 1, None, None, 1, None, None) == -2
    assert lib.gpuar_hip_survey_xor_batch(q, q, q, q + 4, 1, 1, e, s, 1, None, None) == -1
    torch.cuda.synchronize()
    assert rows.cpu().tolist() == [CANARY] * 32
