"""Batches of many buffers in one launch (gpuar_hip_encode_batch / decode_batch / decode_stream_batch, gpuar_amd.batch).

1. Slot equality: in both encode modes and auto, every buffer's slots are byte-identical to hip.encode of that buffer
   alone (status 0); a seeded sample of buffers is checked against the reference codec as well.
2. Compaction: each buffer's subrange of compact() over the batch is its single-buffer stream; batch.gip(b) is its file.
3. Round trips through both batch decoders into views of one canary-filled arena.
4. The room check: too little room, or a damaged ulen, is BAD_PACKET and writes nothing past the room.
5. Bad descriptors: BAD_BATCH, that packet's slot untouched, the other buffers right.  The table mode, which only the
   single-buffer encoder has, is refused as an argument before any launch.
6. Scale: over 2 GiB in ~2000 buffers (offsets past 4 GiB, several scan tiles).
7. Two batches on two streams with status words of their own.
Fixed seeds throughout.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
CANARY = 0xA5
MODES = ["throughput", "latency", "auto"]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    codec = O.require_best()
    assert codec.kind == O.expected_kind()
    return codec


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _bytes_for(rng, n, kind):
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 1:
        return (rng.integers(0, 4, n) * 7 + 65).astype(np.uint8)             # low entropy
    return np.minimum(rng.geometric(0.05, n), 255).astype(np.uint8)            # skewed


class Arena:
    """Buffers as 16-byte aligned views of one device arena, canary-filled gaps between them."""
    def __init__(self, sizes, gap=48, fill=None, seed=0):
        self.sizes = list(sizes)
        self.starts, at = [], gap
        for n in self.sizes:
            self.starts.append(at)
            at = (at + n + gap + 15) // 16 * 16
        self.total = at + gap
        self.mem = torch.full((self.total,), CANARY, dtype=torch.uint8, device="cuda")
        self.host = []
        if fill is not False:
            rng = np.random.default_rng(seed)
            for b, (s, n) in enumerate(zip(self.starts, self.sizes)):
                h = _bytes_for(rng, n, b % 3)
                self.host.append(h)
                if n:
                    self.mem[s:s + n] = torch.from_numpy(h).cuda()

    def views(self):
        return [self.mem[s:s + n] for s, n in zip(self.starts, self.sizes)]

    def gaps_intact(self):
        ends = [s + n for s, n in zip(self.starts, self.sizes)]
        gaps = [(0, self.starts[0] if self.starts else self.total)] + list(zip(ends, self.starts[1:] + [self.total]))
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        for a, b in gaps:
            bad += (self.mem[a:b] != CANARY).sum()
        return int(bad) == 0


def _desc(H, views, sizes=None):
    sizes = [v.numel() for v in views] if sizes is None else sizes
    fp, npk = H.batch_packet_count(sizes)
    ptrs = [v.data_ptr() if v.numel() else 0 for v in views]
    d = torch.tensor(ptrs + sizes + fp, dtype=torch.int64).cuda()
    k = len(views)
    return d[:k], d[k:2 * k], d[2 * k:], fp, npk


def _encode_batch(H, views, mode):
    d_ptrs, d_bytes, d_fp, fp, npk = _desc(H, views)
    st = _status()
    slots = H.encode_batch(d_ptrs, d_bytes, d_fp, len(views), npk, stream=None, d_status=st, mode=mode, device="cuda")
    torch.cuda.synchronize()
    return slots, fp, npk, int(st.item())


def _single_slots(H, v, mode):
    st = _status()
    s = H.encode(v, stream=None, d_status=st, mode=mode)
    assert int(st.item()) == 0
    return s


def _check_slots_equal(H, views, slots, fp, mode, sample=None):
    """every buffer's slots (their defined bytes: clen) equal the single-buffer encoding's"""
    idx = range(len(views)) if sample is None else sample
    for b in idx:
        n_pk = fp[b + 1] - fp[b]
        if n_pk == 0:
            continue
        want = _single_slots(H, views[b], mode)[:n_pk * SLOT].view(n_pk, SLOT)
        got = slots[fp[b] * SLOT:fp[b + 1] * SLOT].view(n_pk, SLOT)
        clen = want[:, 0].long() | (want[:, 1].long() << 8)
        cols = torch.arange(SLOT, device="cuda")[None, :] < clen[:, None]
        ok = ((got == want) | ~cols).all(dim=1)
        if not bool(ok.all()):
            j = int((~ok).nonzero()[0])
            pytest.fail(f"mode {mode}: buffer {b} ({views[b].numel()} bytes), packet {j} (batch packet {fp[b] + j}, lane {(fp[b] + j) % 64}) differs")


def _short_lanes(sizes):
    """the lane positions (packet % 64) of the packets shorter than 8192 bytes"""
    lanes, p = set(), 0
    for n in sizes:
        k = (n + PACKET - 1) // PACKET
        if n % PACKET:
            lanes.add((p + k - 1) % 64)
        p += k
    return lanes


def _short_at_every_lane():
    """one-packet buffers of 1 .. 8191 bytes, each followed by a multi-packet buffer (whole packets, or with a tail of its own)
    sized so that the next short buffer lands on the next lane position; every lane 0 .. 63 gets one"""
    sizes, p = [], 0
    for i in range(64):
        target = (i * 29) % 64                                     # visit the lanes out of order
        whole = (target - p) % 64 + 64 * (i % 2)                   # packets in front of it
        if whole:
            sizes.append(whole * PACKET)
            p += whole
        sizes.append((i * 131 + 7) % 8191 + 1)                     # the short one, at lane `target`
        p += 1
        tail = 2 * PACKET + (i * 977) % 8191 + 1 if i % 3 == 0 else 0
        if tail:                                                   # a multi-packet buffer with a tail of its own
            sizes.append(tail)
            p += 3
    return sizes


def test_short_at_every_lane_composition_covers_every_lane():
    assert _short_lanes(_short_at_every_lane()) == set(range(64))
    assert _short_lanes(_compositions()["residues"]) == set(range(64))


def _compositions():
    rng = np.random.default_rng(11)
    comps = {
        "k1": [3 * PACKET + 1000],
        "zeros_start_mid_end": [0, 0, 20000, 0, 8192, 0, 5, 0],
        "k64_tiny": [int(x) for x in rng.integers(1, 200, 64)],
        "k65_tiny": [int(x) for x in rng.integers(1, 200, 65)],
        # a short packet at every lane position of a wavefront: buffers of 1 .. 8191 bytes between multi-packet ones
        "short_at_every_lane": _short_at_every_lane(),
        # tail residues: every value mod 8, 16 and 64
        "residues": [PACKET * (1 + (r % 2)) + 64 * (r % 5) + r for r in range(64)] + [r for r in range(1, 64)],
    }
    return comps


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("comp", sorted(_compositions()))
def test_batch_slots_equal_single_buffer_encoding(H, mode, comp):
    sizes = _compositions()[comp]
    a = Arena(sizes, seed=len(sizes))
    views = a.views()
    slots, fp, npk, st = _encode_batch(H, views, mode)
    assert st == 0 and npk == fp[-1]
    _check_slots_equal(H, views, slots, fp, mode)


def test_batch_above_the_auto_switch(H):
    """more than 32768 packets: auto takes the throughput kernel; equal to single-buffer encoding on a sample"""
    sizes = [PACKET * 500 + (i * 1237) % PACKET for i in range(70)]                # ~35000 packets
    a = Arena(sizes, seed=3)
    views = a.views()
    slots, fp, npk, st = _encode_batch(H, views, "auto")
    assert st == 0 and npk > 32768
    _check_slots_equal(H, views, slots, fp, "throughput", sample=[0, 1, 33, 68, 69])


def test_batch_matches_the_reference_codec(H, oracle):
    from gpuar_amd import batch
    sizes = _compositions()["short_at_every_lane"]
    a = Arena(sizes, seed=5)
    c = batch.compress(a.views())
    for b in np.random.default_rng(2).choice(len(sizes), 12, replace=False):
        want = oracle.encode_stream(a.host[b])
        got = c.payload(int(b)).cpu().numpy()
        assert got.size == want.size and np.array_equal(got, want), f"buffer {b}"


@pytest.mark.parametrize("mode", ["throughput", "latency"])
def test_batch_compaction_and_gip_equal_the_single_path(H, mode):
    from gpuar_amd import batch
    sizes = [0, 1, 8191, 8192, 8193, 0, 40000, 77, 0]
    a = Arena(sizes, seed=9)
    c = batch.compress(a.views(), mode=mode)
    for b, v in enumerate(a.views()):
        npk = H.packet_count(v.numel())
        if npk == 0:
            assert c.payload(b).numel() == 0
            assert c.gip(b) == H.gip_header(0, 0)
            continue
        s, off = H.compact(_single_slots(H, v, mode), npk)
        want = s[:int(off[-1])]
        assert torch.equal(c.payload(b), want), b
        assert c.gip(b) == H.gip_header(v.numel(), want.numel()) + bytes(want.cpu().numpy().tobytes())


@pytest.mark.parametrize("via", ["slots", "stream"])
def test_batch_round_trip_into_an_arena(H, via):
    sizes = _compositions()["short_at_every_lane"] + [0, 3, 0]
    a = Arena(sizes, seed=21)
    views = a.views()
    slots, fp, npk, st = _encode_batch(H, views, None)
    assert st == 0
    out = Arena(sizes, fill=False)
    d_ptrs, d_room, d_fp, _, _ = _desc(H, out.views())
    st = _status()
    if via == "slots":
        H.decode_batch(slots, d_fp, len(sizes), npk, d_ptrs, d_room, d_status=st)
    else:
        s, off = H.compact(slots, npk)
        H.decode_stream_batch(s, off, d_fp, len(sizes), npk, d_ptrs, d_room, d_status=st)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    for b, v in enumerate(out.views()):
        assert np.array_equal(v.cpu().numpy(), a.host[b]), b
    assert out.gaps_intact()


def test_batch_of_one_decodes_as_hip_decode(H):
    n = 5 * PACKET + 123
    a = Arena([n], seed=4)
    slots, fp, npk, st = _encode_batch(H, a.views(), None)
    want = H.decode(slots, npk)[:n]
    out = Arena([n], fill=False)
    d_ptrs, d_room, d_fp, _, _ = _desc(H, out.views())
    st = _status()
    H.decode_batch(slots, d_fp, 1, npk, d_ptrs, d_room, d_status=st)
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and torch.equal(out.views()[0], want) and out.gaps_intact()


@pytest.mark.parametrize("via", ["slots", "stream"])
def test_room_check(H, via):
    """buffer 1 gets 100 bytes less room than it needs; buffer 2's last packet carries a damaged ulen (8192) past its room"""
    sizes = [20000, 3 * PACKET + 500, 2 * PACKET + 300, 9000]
    a = Arena(sizes, seed=8)
    slots, fp, npk, st = _encode_batch(H, a.views(), None)
    assert st == 0
    last2 = fp[3] - 1
    slots[last2 * SLOT + 2] = 0x00
    slots[last2 * SLOT + 3] = 0x20                                            # ulen = 8192 > its room (300)
    room = list(sizes)
    room[1] -= 100
    out = Arena(room, fill=False)
    d_ptrs, d_room, d_fp, _, _ = _desc(H, out.views(), room)
    st = _status()
    if via == "slots":
        H.decode_batch(slots, d_fp, len(sizes), npk, d_ptrs, d_room, d_status=st)
    else:
        s, off = H.compact(slots, npk)
        H.decode_stream_batch(s, off, d_fp, len(sizes), npk, d_ptrs, d_room, d_status=st)
    torch.cuda.synchronize()
    assert int(st.item()) & H.STATUS_BAD_PACKET
    assert out.gaps_intact()                                                  # nothing written past any room
    got = [v.cpu().numpy() for v in out.views()]
    assert np.array_equal(got[0], a.host[0]) and np.array_equal(got[3], a.host[3])
    assert np.array_equal(got[1][:3 * PACKET], a.host[1][:3 * PACKET])      # the packets that fit
    assert (got[1][3 * PACKET:] == CANARY).all()                              # the one that did not: unwritten
    assert np.array_equal(got[2][:2 * PACKET], a.host[2][:2 * PACKET]) and (got[2][2 * PACKET:] == CANARY).all()


@pytest.mark.parametrize("mode", ["throughput", "latency"])
def test_bad_descriptors(H, mode):
    """buffer 1 claims one packet more than its bytes have; buffer 3's pointer is misaligned"""
    sizes = [10000, 2 * PACKET + 5, 7000, 30000, 4000]
    a = Arena(sizes, seed=13)
    views = a.views()
    fp, _ = H.batch_packet_count(sizes)
    fp = fp[:2] + [x + 1 for x in fp[2:]]                                      # buffer 1: one packet too many
    npk = fp[-1]
    ptrs = [v.data_ptr() for v in views]
    ptrs[3] += 8                                                              # misaligned
    d = torch.tensor(ptrs + sizes + fp, dtype=torch.int64).cuda()
    k = len(sizes)
    slots = torch.full((npk * SLOT,), 0x5A, dtype=torch.uint8, device="cuda")
    st = _status()
    H.encode_batch(d[:k], d[k:2 * k], d[2 * k:], k, npk, d_slots=slots, d_status=st, mode=mode)
    torch.cuda.synchronize()
    assert int(st.item()) == H.STATUS_BAD_BATCH
    untouched = [fp[2] - 1] + list(range(fp[3], fp[4]))                       # the extra packet, buffer 3's packets
    for p in untouched:
        assert bool((slots[p * SLOT:(p + 1) * SLOT] == 0x5A).all()), p
    good = {0: views[0], 2: views[2], 4: views[4]}
    for b, v in good.items():
        n_pk = H.packet_count(v.numel())
        want = _single_slots(H, v, mode)
        for j in range(n_pk):
            w = want[j * SLOT:(j + 1) * SLOT]
            clen = int(w[0]) | (int(w[1]) << 8)
            p = fp[b] + j
            assert torch.equal(slots[p * SLOT:p * SLOT + clen], w[:clen]), (b, j)
    # buffer 1's real packets are right too
    want = _single_slots(H, views[1], mode)
    for j in range(3):
        w = want[j * SLOT:(j + 1) * SLOT]
        clen = int(w[0]) | (int(w[1]) << 8)
        assert torch.equal(slots[(fp[1] + j) * SLOT:(fp[1] + j) * SLOT + clen], w[:clen])


def test_batch_encoders_refuse_the_table_mode(H):
    """GPUAR_MODE_TABLE is gpuar_hip_encode_mode's alone (include/gpuar_hip.h): gpuar_hip_encode_batch returns
    GPUAR_ERR_ARGUMENT for it before it looks at anything else -- through the argument and through GPUAR_ENCODE_MODE, which
    tests/test_gpu_parity.py sets to "table" around its single-buffer cases --, nothing is launched: the slots and the
    caller's status word keep what they held, and the fallback word stays 0."""
    import os
    sizes = [10000, PACKET, 3 * PACKET + 5]
    a = Arena(sizes, seed=17)
    d_ptrs, d_bytes, d_fp, fp, npk = _desc(H, a.views())
    slots = torch.full((npk * SLOT,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), 0x1234, dtype=torch.int32, device="cuda")
    assert H.status() == 0
    with pytest.raises(H.GpuarError, match=r"gpuar_hip_encode_batch.*code -2\)"):
        H.encode_batch(d_ptrs, d_bytes, d_fp, len(sizes), npk, d_slots=slots, d_status=st, mode="table")
    old = os.environ.get("GPUAR_ENCODE_MODE")
    os.environ["GPUAR_ENCODE_MODE"] = "table"
    try:
        with pytest.raises(H.GpuarError, match=r"gpuar_hip_encode_batch.*code -2\)"):
            H.encode_batch(d_ptrs, d_bytes, d_fp, len(sizes), npk, d_slots=slots, d_status=st)
    finally:
        if old is None:
            del os.environ["GPUAR_ENCODE_MODE"]
        else:
            os.environ["GPUAR_ENCODE_MODE"] = old
    assert H.load().gpuar_hip_encode_batch(d_ptrs.data_ptr(), d_bytes.data_ptr(), d_fp.data_ptr(), len(sizes), npk, slots.data_ptr(),
                                           st.data_ptr(), None, 3) == -2
    torch.cuda.synchronize()
    assert int(st.item()) == 0x1234 and bool((slots == 0x5A).all()) and a.gaps_intact()
    assert H.status() == 0
    # the same descriptors are fine in a mode the batch encoder has
    st.zero_()
    H.encode_batch(d_ptrs, d_bytes, d_fp, len(sizes), npk, d_slots=slots, d_status=st, mode="throughput")
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    _check_slots_equal(H, a.views(), slots, fp, "table")


def test_scale_past_4_gib_of_stream_offsets(H):
    """~2000 seeded random-size buffers, ~5 GiB of mostly incompressible input: the compacted stream's offsets pass 4 GiB (the
    high half of decode_stream_batch_kernel's wave-uniform base is used) and compaction spans many scan tiles; both batch
    decoders restore every buffer; single-buffer equality on a sample"""
    rng = np.random.default_rng(2024)
    sizes = [int(x) for x in rng.integers(1, 5 * 2**20, 2000)]
    assert sum(sizes) > 4.5 * 2**30
    a = Arena(sizes, fill=False, gap=16)
    for b, (s, n) in enumerate(zip(a.starts, a.sizes)):                       # device-generated contents (16-aligned starts)
        H.generate("text" if b % 4 == 0 else "uniform", 77 + b, n, out=a.mem[s:s + n])
    views = a.views()
    slots, fp, npk, st = _encode_batch(H, views, None)
    assert st == 0
    s, off = H.compact(slots, npk)
    assert int(off[-1]) > 2**32
    out = Arena(sizes, fill=False, gap=16)
    d_ptrs, d_room, d_fp, _, _ = _desc(H, out.views())
    for via in ("stream", "slots"):
        out.mem.fill_(CANARY)
        st = _status()
        if via == "stream":
            H.decode_stream_batch(s, off, d_fp, len(sizes), npk, d_ptrs, d_room, d_status=st)
        else:
            H.decode_batch(slots, d_fp, len(sizes), npk, d_ptrs, d_room, d_status=st)
        torch.cuda.synchronize()
        assert int(st.item()) == 0, via
        for b in range(len(sizes)):
            assert torch.equal(out.views()[b], views[b]), (via, b)
        assert out.gaps_intact(), via
    _check_slots_equal(H, views, slots, fp, "throughput", sample=[0, 999, 1999])


@pytest.mark.parametrize("via", ["slots", "stream"])
def test_bad_output_descriptors(H, via):
    """decode: buffer 1's output pointer misaligned, buffer 2 given a first_packet that claims one packet more than its
    bytes: those packets are BAD_BATCH and write nothing; the other buffers are restored"""
    sizes = [10000, 3 * PACKET + 7, 2 * PACKET, 5000]
    a = Arena(sizes, seed=17)
    slots, fp, npk, st = _encode_batch(H, a.views(), None)
    assert st == 0
    extra = torch.zeros(SLOT, dtype=torch.uint8, device="cuda")
    extra[:8] = torch.tensor([8, 0, 4, 0, 0, 0, 0, 0], dtype=torch.uint8)       # a well-formed 4-byte packet, ulen 4
    at = fp[3] * SLOT                                                         # slot behind buffer 2's packets
    slots2 = torch.cat([slots[:at], extra, slots[at:npk * SLOT]])
    fp2 = fp[:3] + [x + 1 for x in fp[3:]]
    npk2 = fp2[-1]
    out = Arena(sizes, fill=False)
    views = out.views()
    ptrs = [v.data_ptr() for v in views]
    ptrs[1] += 8
    k = len(sizes)
    d = torch.tensor(ptrs + sizes + fp2, dtype=torch.int64).cuda()
    st = _status()
    if via == "slots":
        H.decode_batch(slots2, d[2 * k:], k, npk2, d[:k], d[k:2 * k], d_status=st)
    else:
        s, off = H.compact(slots2, npk2)
        H.decode_stream_batch(s, off, d[2 * k:], k, npk2, d[:k], d[k:2 * k], d_status=st)
    torch.cuda.synchronize()
    assert int(st.item()) == H.STATUS_BAD_BATCH
    assert out.gaps_intact()
    got = [v.cpu().numpy() for v in views]
    assert (got[1] == CANARY).all()                                           # nothing written at the misaligned pointer
    for b in (0, 2, 3):
        assert np.array_equal(got[b], a.host[b]), b


def test_two_batches_on_two_streams(H):
    from gpuar_amd import batch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a1 = Arena([PACKET * 40 + 1, 17, 0, 9999], seed=31)
    a2 = Arena([3, PACKET * 64, 12345], seed=32)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c1 = batch.compress(a1.views(), stream=s1)
    with torch.cuda.stream(s2):
        c2 = batch.compress(a2.views(), stream=s2)
    with torch.cuda.stream(s1):
        o1 = batch.decompress(c1, stream=s1)
    with torch.cuda.stream(s2):
        o2 = batch.decompress(c2, stream=s2)
    torch.cuda.synchronize()
    for o, a in ((o1, a1), (o2, a2)):
        for b, v in enumerate(o):
            assert np.array_equal(v.cpu().numpy(), a.host[b]), b
