"""Raw storage of incompressible packets on the MI355X: gpuar_hip_move_packets byte for byte with canaries behind every
destination, and batch.compress(stored=...) / decompress / estimate: the round trip, the flags against the host rule applied to
the split bytes, the coded packets against the same call without `stored` (the codec is untouched), forced masks, and what
Compressed.gip(b) does with a buffer that holds a raw packet."""
import numpy as np
import pytest

import planes_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
GUARD = 64


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


# ---- move_packets -----------------------------------------------------------------------------------------------------

def test_regions_arrive_byte_exact_and_nothing_behind_them_is_written(H):
    sizes = [1, 15, 16, 17, 8191, 8192, 4097, 0]
    rng = np.random.default_rng(11)
    hosts = [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]
    # every source in an allocation of its own that ends with the 16-byte piece that holds its last byte
    srcs = [torch.zeros(max((n + 15) // 16 * 16, 16), dtype=torch.uint8, device="cuda") for n in sizes]
    for s, h in zip(srcs, hosts):
        s[:h.size] = torch.from_numpy(h).cuda()
    offs, at = [], 0
    for n in sizes:
        offs.append(at)
        at += (n + GUARD + 15) // 16 * 16
    dst = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    n = len(sizes)
    desc = torch.tensor([s.data_ptr() for s in srcs] + [dst.data_ptr() + o for o in offs] + sizes, dtype=torch.int64, device="cuda")
    status = _status()
    H.move_packets(desc[:n], desc[n:2 * n], desc[2 * n:], n, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    for r, (o, h) in enumerate(zip(offs, hosts)):
        assert (got[o:o + h.size] == h).all(), (r, h.size)
        end = offs[r + 1] if r + 1 < n else at
        assert (got[o + h.size:end] == 0x5A).all(), (r, h.size, "wrote behind the region")
    for s, h in zip(srcs, hosts):
        assert (s.cpu().numpy()[:h.size] == h).all()


def test_a_misaligned_or_over_long_region_is_bad_batch_and_is_skipped(H):
    src = torch.arange(4 * PACKET, device="cuda").to(torch.uint8)
    dst = torch.full((4 * PACKET,), 0x5A, dtype=torch.uint8, device="cuda")
    s, d = src.data_ptr(), dst.data_ptr()

    def call(srcs, dsts, sizes):
        dst.fill_(0x5A)
        desc = torch.tensor(srcs + dsts + sizes, dtype=torch.int64, device="cuda")
        status = _status()
        H.move_packets(desc[:2], desc[2:4], desc[4:], 2, d_status=status)
        return int(status.item()), dst.cpu().numpy()

    want = src.cpu().numpy()
    flags, got = call([s, s + PACKET], [d, d + 2 * PACKET], [100, 50])
    assert flags == 0 and (got[:100] == want[:100]).all() and (got[2 * PACKET:2 * PACKET + 50] == want[PACKET:PACKET + 50]).all()
    for bad in ([[s + 8, s + PACKET], [d, d + 2 * PACKET], [100, 50]],             # source
                [[s, s + PACKET], [d + 4, d + 2 * PACKET], [100, 50]],             # destination
                [[s, s + PACKET], [d, d + 2 * PACKET], [PACKET + 1, 50]]):         # more than a packet
        flags, got = call(*bad)
        assert flags == H.STATUS_BAD_BATCH, bad
        assert (got[:2 * PACKET] == 0x5A).all(), "the refused region was written"
        assert (got[2 * PACKET:2 * PACKET + 50] == want[PACKET:PACKET + 50]).all() and (got[2 * PACKET + 50:] == 0x5A).all()


def test_move_packets_host_side_checks(H):
    lib = H.load()
    desc = torch.zeros(8, dtype=torch.int64, device="cuda")
    q = desc.data_ptr()
    assert lib.gpuar_hip_move_packets(None, None, None, 0, None, None) == 0
    assert lib.gpuar_hip_move_packets(None, q, q, 1, None, None) == -2 and lib.gpuar_hip_move_packets(q, None, q, 1, None, None) == -2
    assert lib.gpuar_hip_move_packets(q, q, None, 1, None, None) == -2
    assert lib.gpuar_hip_move_packets(q + 4, q, q, 1, None, None) == -1 and lib.gpuar_hip_move_packets(q, q, q + 4, 1, None, None) == -1
    assert lib.gpuar_hip_move_packets(q, q, q, 1, q + 2, None) == -1


# ---- batch.compress(stored=...) ---------------------------------------------------------------------------------------

def raw(t):
    """the tensor's bytes on the host"""
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1) if t.numel() else np.empty(0, dtype=np.uint8)


@pytest.fixture(scope="module")
def mixed(H):
    """bf16 and fp32 weights (groups and a tail), uniform bytes, zeros, text, an empty tensor and a short uniform one --
    with what batch.compress makes of them with and without stored="auto" (shared by the tests below, never modified)."""
    from gpuar_amd import batch, synth
    g = torch.Generator().manual_seed(1)
    ts = [
        (torch.randn((3 * 16384 + 6) // 2, generator=g) * 0.02).to(torch.bfloat16).cuda(),
        (torch.randn((2 * 32768 + 40) // 4, generator=g) * 0.02).cuda(),
        torch.randint(0, 256, (3 * PACKET,), generator=g, dtype=torch.uint8).cuda(),
        torch.zeros(2 * PACKET + 100, dtype=torch.uint8, device="cuda"),
        torch.from_numpy(synth.text(4, 20000)).cuda(),
        torch.empty(0, dtype=torch.float32, device="cuda"),
        torch.randint(0, 256, (3000,), generator=g, dtype=torch.uint8).cuda(),
    ]
    plain = batch.compress(ts, planes="auto", checksum=True)
    auto = batch.compress(ts, planes="auto", checksum=True, stored="auto")
    return ts, plain, auto


def host_flags(H, ts, widths):
    flags = []
    for t, w in zip(ts, widths):
        split = R.numpy_split(raw(t), w)
        est = H.estimate_host(split.tobytes())
        flags += [1 if H.stored_rule(e, min(PACKET, split.size - p * PACKET)) else 0 for p, e in enumerate(est)]
    return flags


def test_auto_round_trips_and_stores_what_the_host_rule_stores(H, mixed):
    from gpuar_amd import batch
    ts, plain, auto = mixed
    assert auto.planes == [2, 4, 1, 1, 1, 4, 1] and auto.sizes == plain.sizes and auto.first_packet == plain.first_packet
    flags = auto.stored.cpu().tolist()
    assert auto.stored.dtype == torch.uint8 and flags == host_flags(H, ts, auto.planes)
    n_stored = sum(flags)
    assert 0 < n_stored < auto.n_packets                                      # both kinds of packet are in this batch
    assert auto.offsets.numel() == auto.n_packets - n_stored + 1 and auto.raw_offsets.numel() == n_stored + 1
    assert int(auto.raw_offsets[-1].item()) == auto.raw.numel() and auto.stream.numel() == int(auto.offsets[-1].item())
    assert auto.nbytes == auto.stream.numel() + auto.raw.numel() and plain.nbytes == plain.stream.numel()
    assert auto.nbytes < plain.nbytes
    assert torch.equal(auto.crc32, plain.crc32)                               # the CRCs of the original bytes, all packets
    for b, (o, t) in enumerate(zip(batch.decompress(auto), ts)):
        assert o.dtype == torch.uint8 and (o.cpu().numpy() == raw(t)).all(), b


def test_the_coded_packets_are_the_packets_of_the_call_without_stored(H, mixed):
    ts, plain, auto = mixed
    flags = auto.stored.cpu().tolist()
    off_c, off_p = auto.offsets.cpu().tolist(), plain.offsets.cpu().tolist()
    stream_c, stream_p = auto.stream.cpu().numpy(), plain.stream.cpu().numpy()
    rank = 0
    for p, flag in enumerate(flags):
        if not flag:
            assert stream_c[off_c[rank]:off_c[rank + 1]].tobytes() == stream_p[off_p[p]:off_p[p + 1]].tobytes(), p
            rank += 1
    assert rank == len(off_c) - 1
    # and the raw packets are the split bytes themselves
    raw_off, raw_bytes = auto.raw_offsets.cpu().tolist(), auto.raw.cpu().numpy()
    split = [R.numpy_split(raw(t), w) for t, w in zip(ts, auto.planes)]
    kept = 0
    for b in range(len(ts)):
        for j in range(auto.first_packet[b + 1] - auto.first_packet[b]):
            if flags[auto.first_packet[b] + j]:
                want = split[b][j * PACKET:(j + 1) * PACKET]
                assert raw_off[kept] % 16 == 0 and (raw_bytes[raw_off[kept]:raw_off[kept] + want.size] == want).all(), (b, j)
                kept += 1
    assert kept == len(raw_off) - 1


def test_decompress_into_the_callers_tensors_leaves_what_is_behind_them(H, mixed):
    from gpuar_amd import batch
    ts, _plain, auto = mixed
    outs = [torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda") for n in auto.sizes]
    assert batch.decompress(auto, out=outs) is outs
    for b, (o, t) in enumerate(zip(outs, ts)):
        got = o.cpu().numpy()
        n = auto.sizes[b]
        assert (got[:n] == raw(t)).all(), b
        assert (got[n:] == 0x5A).all(), (b, "wrote behind the buffer")


def test_gip_and_payload_refuse_a_buffer_with_a_raw_packet(H, mixed):
    ts, plain, auto = mixed
    flags = auto.stored.cpu().tolist()
    for b in range(len(ts)):
        mine = flags[auto.first_packet[b]:auto.first_packet[b + 1]]
        if any(mine):
            with pytest.raises(H.GpuarError, match="stored"):
                auto.gip(b)
            with pytest.raises(H.GpuarError, match="stored"):
                auto.payload(b)
        else:
            assert auto.gip(b) == plain.gip(b), b
            assert torch.equal(auto.payload(b), plain.payload(b)), b
    assert any(flags[auto.first_packet[0]:auto.first_packet[1]]) and not any(flags[auto.first_packet[3]:auto.first_packet[4]])


def test_forced_masks_round_trip(H, mixed):
    from gpuar_amd import batch, synth
    text = [torch.from_numpy(synth.text(8, 5 * PACKET + 77)).cuda()]
    c = batch.compress(text, stored=[True, False] * 3, checksum=True)
    assert c.stored.cpu().tolist() == [1, 0] * 3 and c.offsets.numel() == 4 and c.raw_offsets.cpu().tolist() == [0, PACKET, 2 * PACKET, 3 * PACKET]
    assert torch.equal(batch.decompress(c)[0], text[0])
    assert c.nbytes > batch.compress(text).nbytes                             # (text shrinks: storing it is what the mask is for)
    ts, plain, _auto = mixed
    for value in (True, False):
        c = batch.compress(ts, planes="auto", checksum=True, stored=[value] * plain.n_packets)
        assert c.stored.cpu().tolist() == [int(value)] * plain.n_packets
        for b, (o, t) in enumerate(zip(batch.decompress(c), ts)):
            assert (o.cpu().numpy() == raw(t)).all(), (value, b)
        if value:
            assert c.stream.numel() == 0 and c.offsets.cpu().tolist() == [0]
            assert c.raw.numel() == sum((min(PACKET, n - j * PACKET) + 15) // 16 * 16 for n in c.sizes for j in range((n + PACKET - 1) // PACKET))
        else:
            assert torch.equal(c.stream, plain.stream) and torch.equal(c.offsets, plain.offsets)
            assert c.raw.numel() == 0 and c.raw_offsets.cpu().tolist() == [0]
            assert c.gip(0) == plain.gip(0)


def test_a_mask_of_the_wrong_length_or_kind_raises_before_any_launch(H, mixed):
    from gpuar_amd import batch
    ts, plain, _auto = mixed
    with pytest.raises(H.GpuarError, match="stored"):
        batch.compress(ts, stored=[True] * (plain.n_packets - 1))
    with pytest.raises(H.GpuarError, match="stored"):
        batch.compress(ts, stored="always")


def test_stored_none_is_the_call_without_the_keyword(H, mixed):
    from gpuar_amd import batch
    ts, plain, _auto = mixed
    c = batch.compress(ts, planes="auto", checksum=True, stored=None)
    assert torch.equal(c.stream, plain.stream) and torch.equal(c.offsets, plain.offsets)
    assert c.stored is None and c.raw is None and c.raw_offsets is None


def test_estimate_is_the_sum_of_the_host_estimates(H, mixed):
    from gpuar_amd import batch
    ts, plain, auto = mixed
    for planes in (None, "auto"):
        widths = batch.plane_widths(ts, planes) or [1] * len(ts)
        want, want_stored = [], []
        for t, w in zip(ts, widths):
            split = R.numpy_split(raw(t), w)
            est = H.estimate_host(split.tobytes())
            ulen = [min(PACKET, split.size - p * PACKET) for p in range(len(est))]
            want.append(sum(est))
            want_stored.append(sum(u if H.stored_rule(e, u) else e for e, u in zip(est, ulen)))
        assert batch.estimate(ts, planes=planes) == want
        assert batch.estimate(ts, planes=planes, stored="auto") == want_stored
    # within a byte per packet of what compress really makes of every tensor
    off = plain.offsets.cpu().tolist()
    predicted = batch.estimate(ts, planes="auto")
    for b in range(len(ts)):
        lo, hi = plain.first_packet[b], plain.first_packet[b + 1]
        assert abs(off[hi] - off[lo] - predicted[b]) <= hi - lo, b
    assert batch.estimate([]) == []
