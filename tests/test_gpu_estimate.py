"""The packet size estimate on the MI355X: gpuar_hip_estimate / gpuar_hip_estimate_batch against gpuar_hip_estimate_host (the same
integer definition on the CPU, itself checked in tests/test_estimate_host.py) -- exactly, at every packet length at which the
kernel takes another path, on data that spreads over the histogram and data that hits one counter 8192 times, through the
batch descriptors, and with an unusable descriptor.  Every status word is read and every output has a canary behind it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
CANARY = 0x5A5A5A5A
LENGTHS = [1, 15, 16, 17, 127, 128, 129, 8191, 8192, 8193, 3 * 8192 + 5]
KINDS = ["uniform", "text", "zeros", "ones", "alternating", "last_differs"]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


def data_of(kind, n, seed=0):
    from gpuar_amd import synth
    if kind == "uniform":
        return np.random.default_rng(1000 + n + seed).integers(0, 256, n, dtype=np.uint8)
    if kind == "text":
        return synth.text(3 + seed, n)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "ones":
        return np.full(n, 0xFF, dtype=np.uint8)                  # the last bin
    if kind == "alternating":
        return np.tile(np.array([0x41, 0xC2], dtype=np.uint8), n // 2 + 1)[:n]
    if kind == "last_differs":                                   # one counter takes all but one byte of every packet
        x = np.full(n, 0x10, dtype=np.uint8)
        x[PACKET - 1::PACKET] = 0xEF
        x[-1] = 0xEF
        return x
    raise KeyError(kind)


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("kind", KINDS)
def test_one_buffer_is_the_host_estimate_at_every_length(H, kind):
    for n in LENGTHS:
        host = data_of(kind, n)
        npk = H.packet_count(n)
        d_est = torch.full((npk + 2,), CANARY, dtype=torch.int32, device="cuda")
        H.estimate(torch.from_numpy(host).cuda(), d_est=d_est)
        got = d_est.cpu().tolist()
        assert got[:npk] == H.estimate_host(host.tobytes()), (kind, n)
        assert got[npk:] == [CANARY, CANARY], (kind, n, "wrote behind the last packet")


def test_more_short_packets_than_one_pass_of_the_grid(H):
    """70 000 buffers of 64 bytes in one call: every packet is short, and the persistent workgroups go round more than once."""
    n, size = 70000, 64
    rng = np.random.default_rng(9)
    host = rng.integers(0, 256, n * size, dtype=np.uint8) & rng.choice(np.array([0xFF, 0x0F, 0x01, 0x00], dtype=np.uint8), n).repeat(size)
    data = torch.from_numpy(host).cuda()
    ptrs = data.data_ptr() + size * torch.arange(n, dtype=torch.int64, device="cuda")
    sizes = torch.full((n,), size, dtype=torch.int64, device="cuda")
    fp = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    status = _status()
    d_est = torch.full((n + 2,), CANARY, dtype=torch.int32, device="cuda")
    H.estimate_batch(ptrs, sizes, fp, n, n, d_est=d_est, d_status=status)
    assert int(status.item()) == 0
    got = d_est.cpu().tolist()
    raw = host.tobytes()
    want = [H.estimate_host(raw[i * size:(i + 1) * size])[0] for i in range(n)]
    assert got[:n] == want
    assert got[n:] == [CANARY, CANARY]


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
    sizes = [0, 1, 17, 3000, 8192, 8193, 8191, 16384, 0, 3 * 8192 + 5] + [int(v) for v in rng.integers(0, 40000, 55)]
    assert len(sizes) == 65
    hosts = [data_of(KINDS[i % len(KINDS)], n, seed=i) if n else np.empty(0, dtype=np.uint8) for i, n in enumerate(sizes)]
    data, offs, sizes, fp, npk = _batch(H, hosts)
    n = len(sizes)
    desc = torch.tensor([data.data_ptr() + o for o in offs] + sizes + fp, dtype=torch.int64, device="cuda")
    status = _status()
    d_est = torch.full((npk + 2,), CANARY, dtype=torch.int32, device="cuda")
    H.estimate_batch(desc[:n], desc[n:2 * n], desc[2 * n:], n, npk, d_est=d_est, d_status=status)
    assert int(status.item()) == 0
    got = d_est.cpu().tolist()
    assert got[npk:] == [CANARY, CANARY]
    for b, (o, h) in enumerate(zip(offs, hosts)):
        want = H.estimate_host(h.tobytes())
        assert got[fp[b]:fp[b + 1]] == want, (b, h.size)
        if h.size:
            assert H.estimate(data[o:o + h.size]).cpu().tolist() == want, (b, h.size)


def test_an_unusable_descriptor_is_bad_batch_and_its_estimates_keep_their_canary(H):
    hosts = [data_of("text", 2 * PACKET + 9), data_of("uniform", PACKET + 1), data_of("zeros", 3 * PACKET)]
    data, offs, sizes, fp, npk = _batch(H, hosts)
    ptrs = [data.data_ptr() + o for o in offs]

    def call(ptrs, fp=fp):
        desc = torch.tensor(ptrs + sizes + fp, dtype=torch.int64, device="cuda")
        status = _status()
        d_est = torch.full((npk,), CANARY, dtype=torch.int32, device="cuda")
        H.estimate_batch(desc[:3], desc[3:6], desc[6:], 3, npk, d_est=d_est, d_status=status)
        return int(status.item()), d_est.cpu().tolist()

    want = [H.estimate_host(h.tobytes()) for h in hosts]
    flags, got = call(ptrs)
    assert flags == 0 and got == want[0] + want[1] + want[2]
    flags, got = call([ptrs[0], ptrs[1] + 8, ptrs[2]])                      # a misaligned buffer: both of its packets
    assert flags == H.STATUS_BAD_BATCH
    assert got == want[0] + [CANARY, CANARY] + want[2]
    flags, got = call(ptrs, [0, 3, 6, 9])                                   # buffer 1 owns a packet past its end
    assert flags == H.STATUS_BAD_BATCH
    assert got == want[0] + want[1] + [CANARY] + want[2][:2]


def test_the_host_side_checks(H):
    lib = H.load()
    d = torch.zeros(2 * PACKET, dtype=torch.uint8, device="cuda")
    est = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    desc = torch.zeros(8, dtype=torch.int64, device="cuda")
    p, e, q = d.data_ptr(), est.data_ptr(), desc.data_ptr()
    assert lib.gpuar_hip_estimate(None, 0, None, None) == 0                 # nothing to do comes first, as in gpuar_hip_crc32
    assert lib.gpuar_hip_estimate(None, PACKET, e, None) == -2 and lib.gpuar_hip_estimate(p, PACKET, None, None) == -2
    assert lib.gpuar_hip_estimate(p + 4, PACKET, e, None) == -1 and lib.gpuar_hip_estimate(p, PACKET, e + 2, None) == -1
    assert lib.gpuar_hip_estimate_batch(None, None, None, 1, 0, None, None, None) == 0
    assert lib.gpuar_hip_estimate_batch(None, q, q, 1, 1, e, None, None) == -2
    assert lib.gpuar_hip_estimate_batch(q, q, q, 1, 1, None, None, None) == -2
    assert lib.gpuar_hip_estimate_batch(q + 4, q, q, 1, 1, e, None, None) == -1
    assert lib.gpuar_hip_estimate_batch(q, q, q, 1, 1, e + 2, None, None) == -1
    torch.cuda.synchronize()
    assert est.cpu().tolist() == [CANARY] * 4
