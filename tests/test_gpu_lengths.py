"""Packet lengths, lane mixes and ragged tails through the HIP kernels, against the pinned reference codec.

1. Every packet length 1 ... 8192 through both decoders (decode_stream and the slot decoder), in lane layouts built to
   drive the decoder's divergent whole-block loop, its handoff to the plain step and its partial last block.
2. Every tail residue through the three encode kernels (throughput: encode_kernel, latency: encode_small_kernel, table:
   encode_kernel_t16, the table walk).
3. The auto-mode switch (32768 packets: the latency kernel; 32769: the table-walk kernel encode_kernel_t16) against all
   three forced modes.
4. Compaction (scans + gather) against a plain concatenation of synthetic slots.
5. Every packet length through both batch encoders (throughput and latency mode): each lane its own one-packet buffer,
   the buffers scattered over a canary arena in permuted address order with zero-byte buffers among them, the bytes
   between buffers 0x00 and then 0xFF; the slots equal the reference's, and decode back through both batch decoders.
6. Every packet length through both batch decoders (slots; stream at pointer skew 0 and 4): one output buffer per packet
   with a room of exactly its ulen, in permuted rows, and buffers of 1-5 packets whose packets in front of the last one
   have a room of 8192 behind a shorter ulen.

The packets of parts 1, 2, 5 and 6 come from tests/length_sweep.py (six source models in turn), the batch descriptors
from tests/batch_sweep.py; the host half is tests/test_lane_emulation.py::test_lane_decoder_at_every_packet_length.
Fixed seeds throughout.
"""
import numpy as np
import pytest

import batch_sweep as BS
import length_sweep as LS
from gpuar_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
CANARY = 0xC3


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()          # raises if the HIP library is missing: no fallback
    return hip


@pytest.fixture(scope="module")
def oracle():
    """The checker: the reference's own codec wherever the golden vectors pin it (as in tests/test_gpu_parity.py)."""
    from oracle import oracle as O
    codec = O.require_best()
    assert codec.kind == O.expected_kind()
    return codec


@pytest.fixture(scope="module")
def sweep(oracle):
    """The 8192 sweep packets, their oracle encodings, and on the device: each packet's expected 8192-byte output row
    (canary after ulen), its slot (encoding, zeros after clen), clen and ulen."""
    pkts = LS.packets()
    encs, clens = LS.encode_all(oracle, pkts)
    rows = np.full((PACKET, PACKET), CANARY, dtype=np.uint8)
    slots = np.zeros((PACKET, SLOT), dtype=np.uint8)
    for i, (p, e) in enumerate(zip(pkts, encs)):
        rows[i, :p.size] = p
        slots[i, :e.size] = e
    ulens = np.arange(1, PACKET + 1, dtype=np.int64)
    return dict(pkts=pkts, encs=encs, clens=clens, ulens=ulens, rows=torch.from_numpy(rows).cuda(),
                slots=torch.from_numpy(slots).cuda(), d_clens=torch.from_numpy(clens).cuda())


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _first_wrong_row(got, want, order, sweep, what, rooms=None):
    """pytest.fail with the packet, lane, ulen (and room) and first differing byte of the first output row that is wrong."""
    bad = (got != want).any(dim=1).nonzero().flatten()
    lane = int(bad[0])
    i = int(order[lane])
    ulen = int(sweep["ulens"][i])
    room = "" if rooms is None else f", room {int(rooms[lane])}"
    g, w = got[lane].cpu().numpy(), want[lane].cpu().numpy()
    at = int(np.flatnonzero(g != w)[0])
    where = "inside ulen" if at < ulen else "after ulen (canary overwritten)"
    pytest.fail(f"{what}: {bad.numel()} rows wrong; first: packet {i} at row {lane} (wavefront {lane // 64}, lane {lane % 64}), "
                f"ulen {ulen}{room}, byte {at} {where}: got {g[at]:#04x}, want {w[at]:#04x}")


def _check_rows(d_out, order, sweep, what):
    n = order.size
    idx = torch.from_numpy(order).cuda()
    got = d_out[:n * PACKET].view(n, PACKET)
    want = sweep["rows"].index_select(0, idx)
    if not torch.equal(got, want):
        _first_wrong_row(got, want, order, sweep, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every packet length through both decoders
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = LS.layouts()


def _device_stream(sweep, order, skew):
    """The packets of `order` back to back on the device at an address that is `skew` mod 16 (its own allocation, 64 bytes
    of slack): (allocation, stream, offsets)."""
    stream = np.concatenate([sweep["encs"][i] for i in order])
    offs = np.zeros(order.size + 1, dtype=np.int64)
    offs[1:] = np.cumsum(sweep["clens"][order])
    assert offs[-1] == stream.size
    raw = torch.zeros(stream.size + 64, dtype=torch.uint8, device="cuda")
    base = (-raw.data_ptr()) % 16 + skew
    raw[base:base + stream.size] = torch.from_numpy(stream).cuda()
    d_stream = raw[base:base + stream.size]
    assert d_stream.data_ptr() % 16 == skew
    return raw, d_stream, torch.from_numpy(offs).cuda()


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_stream_at_every_packet_length(H, sweep, layout, skew):
    order = LAYOUTS[layout]
    n = order.size
    raw, d_stream, d_offs = _device_stream(sweep, order, skew)
    d_out = torch.full((n * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    word = _status()
    H.decode_stream(d_stream, d_offs, n, d_out, d_status=word)
    torch.cuda.synchronize()
    assert int(word.item()) == 0, f"{layout} skew {skew}: status {int(word.item()):#x}"
    _check_rows(d_out, order, sweep, f"decode_stream {layout} skew {skew}")


@pytest.mark.parametrize("after_clen", ["garbage", "zeros"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_slots_at_every_packet_length(H, sweep, layout, after_clen):
    """A well-formed packet decodes the same whatever its slot holds after clen."""
    order = LAYOUTS[layout]
    n = order.size
    idx = torch.from_numpy(order).cuda()
    d_slots = sweep["slots"].index_select(0, idx)
    if after_clen == "garbage":
        gen = torch.Generator(device="cuda")
        gen.manual_seed(LS.SEED + n)
        junk = torch.randint(0, 256, (n, SLOT), dtype=torch.uint8, device="cuda", generator=gen)
        keep = torch.arange(SLOT, device="cuda")[None, :] < sweep["d_clens"].index_select(0, idx)[:, None]
        d_slots = torch.where(keep, d_slots, junk)
    d_slots = d_slots.reshape(-1).contiguous()
    d_out = torch.full((n * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    word = _status()
    H.decode(d_slots, n, d_out, d_status=word)
    torch.cuda.synchronize()
    assert int(word.item()) == 0, f"{layout} {after_clen}: status {int(word.item()):#x}"
    _check_rows(d_out, order, sweep, f"decode (slots) {layout}, {after_clen} after clen")


# ---------------------------------------------------------------------------------------------------------------------
# 2. every tail residue through the three encoders
# ---------------------------------------------------------------------------------------------------------------------
TAILS = sorted(set(range(1, 257)) | set(range(7936, 8192)) | {64 * j + j % 64 for j in range(4, 124)})
FULL = 63


def _clen_bytes_equal(d_slots, d_want, d_clens):
    """Device-side: rows of slots equal on their clen bytes (and on the clens themselves)."""
    keep = torch.arange(SLOT, device=d_slots.device)[None, :] < d_clens[:, None]
    return torch.where(keep, d_slots, 0).eq(torch.where(keep, d_want, 0)).all()


@pytest.mark.parametrize("mode", ["throughput", "latency", "table"])
def test_encode_every_tail_residue(H, oracle, sweep, mode):
    """n = 63*8192 + r (one wavefront whose last lane is short) and n = r (one live lane): the last slot equals the
    oracle's encoding of the last packet on its clen bytes, the 63 full packets equal a prefix encoded once, and every
    case decodes back to its input.  r covers 1 ... 256, 7936 ... 8191 and every residue mod 64 at every depth.  In the
    throughput and table kernels the top modeler leaves its whole-phase form after r / 64 chunks and the low modeler and
    the coder after r / 8 phases, so with 63 full packets in front every residue mod 64 puts the two hand-offs in a
    different relation; with none the group is not full and the one live lane runs in the ragged form from its first
    symbol on (host half: tests/test_encode_table.py)."""
    kinds = ("text", "zipf", "uniform")
    prefix = np.concatenate([synth.generate(kinds[k % 3], 40 + k, PACKET) for k in range(FULL)])
    stream = oracle.encode_stream(prefix)
    ref = np.zeros((FULL, SLOT), dtype=np.uint8)
    off = 0
    for p in range(FULL):
        c = int(stream[off]) | (int(stream[off + 1]) << 8)
        ref[p, :c] = stream[off:off + c]
        off += c
    assert off == stream.size
    d_ref = torch.from_numpy(ref).cuda()
    d_ref_clens = d_ref[:, 0].to(torch.int64) | (d_ref[:, 1].to(torch.int64) << 8)

    d_buf = torch.empty((FULL + 1) * PACKET, dtype=torch.uint8, device="cuda")
    d_buf[:FULL * PACKET] = torch.from_numpy(prefix).cuda()
    d_slots = torch.empty((FULL + 1) * SLOT, dtype=torch.uint8, device="cuda")
    d_back = torch.empty((FULL + 1) * PACKET, dtype=torch.uint8, device="cuda")
    word = _status()
    verdicts = []                                     # (case, last slot ok, full packets ok, round trip ok): checked at the end
    for r in TAILS:
        d_tail = sweep["rows"][r - 1, :r]
        want_slot = sweep["slots"][r - 1]
        for lead in (FULL, 0):
            n = lead * PACKET + r
            npk = lead + 1
            d_buf[FULL * PACKET:FULL * PACKET + r] = d_tail
            d_in = d_buf[:n] if lead else d_buf[FULL * PACKET:FULL * PACKET + r]     # (both 16-byte aligned)
            assert d_in.data_ptr() % 16 == 0
            d_slots.fill_(0xEE)
            H.encode(d_in, d_slots, d_status=word, mode=mode)
            last = d_slots[lead * SLOT:(lead + 1) * SLOT]
            clen = int(sweep["clens"][r - 1])
            ok_last = last[:clen].eq(want_slot[:clen]).all()
            ok_full = (_clen_bytes_equal(d_slots[:FULL * SLOT].view(FULL, SLOT), d_ref, d_ref_clens) if lead
                       else torch.ones((), dtype=torch.bool, device="cuda"))
            d_back.fill_(CANARY)
            H.decode(d_slots, npk, d_back, d_status=word)
            ok_back = d_back[:n].eq(d_in).all() & d_back[n:npk * PACKET].eq(CANARY).all()
            verdicts.append(((r, lead), torch.stack([ok_last, ok_full, ok_back])))
    torch.cuda.synchronize()
    assert int(word.item()) == 0, f"{mode}: status {int(word.item()):#x}"
    table = torch.stack([v for _, v in verdicts]).cpu().numpy()
    wrong = [(case, what) for (case, _), row in zip(verdicts, table)
             for what, ok in zip(("last slot vs oracle", "full packets vs oracle", "round trip"), row) if not ok]
    assert not wrong, f"{mode}: {len(wrong)} failures, first {wrong[:8]} ((r, full packets in front), check)"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the auto-mode boundary between the encode kernels
# ---------------------------------------------------------------------------------------------------------------------
SMALL_GROUPS_PACKETS = 512 * 64          # gpuar_hip_encode_mode: auto sends up to kSmallGroups groups to the latency kernel


@pytest.mark.parametrize("npk", [SMALL_GROUPS_PACKETS, SMALL_GROUPS_PACKETS + 1])
def test_encode_modes_agree_across_the_auto_boundary(H, oracle, npk):
    """At 32768 packets auto takes the latency kernel, at 32769 the table-walk kernel (encode_kernel_t16): auto and the
    three forced modes give the same slots on their clen bytes (compared on the device), 64-packet windows of them equal
    the oracle, and the slots decode back.  The input mixes three source models packet by packet and ends in a short
    packet."""
    n = (npk - 1) * PACKET + 4321
    d_in = torch.empty(npk * PACKET, dtype=torch.uint8, device="cuda")
    rows = d_in.view(npk, PACKET)
    for k, kind in enumerate(("text", "zipf", "uniform")):
        rows[k::3] = H.generate(kind, 70 + k, npk * PACKET).view(npk, PACKET)[k::3]
    d_in = d_in[:n]
    out = {}
    for mode in ("auto", "throughput", "latency", "table"):
        word = _status()
        out[mode] = H.encode(d_in, mode=mode, d_status=word).view(npk, SLOT)
        torch.cuda.synchronize()
        assert int(word.item()) == 0, (npk, mode)
    d_clens = out["auto"][:, 0].to(torch.int64) | (out["auto"][:, 1].to(torch.int64) << 8)
    for mode in ("throughput", "latency", "table"):
        assert _clen_bytes_equal(out[mode], out["auto"], d_clens).item(), f"{npk} packets: {mode} differs from auto"
    for first in (0, npk - 64, 32704):
        last = min(first + 65, npk) if first == 32704 else first + 64
        want = oracle.encode_stream(d_in[first * PACKET:last * PACKET].cpu().numpy())
        got = out["auto"][first:last]
        clens = d_clens[first:last].cpu().numpy()
        stream = np.concatenate([got[j, :int(clens[j])].cpu().numpy() for j in range(last - first)])
        assert np.array_equal(stream, want), f"{npk} packets: window {first}..{last - 1} differs from the oracle"
    word = _status()
    back = H.decode(out["auto"].reshape(-1), npk, d_status=word)
    assert torch.equal(back[:n], d_in)
    assert int(word.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. compaction against a plain concatenation
# ---------------------------------------------------------------------------------------------------------------------
def _synthetic_clens(n: int, seed: int) -> np.ndarray:
    """clens in 4 ... 8704: the extremes, 5 ... 19, runs that walk the destination offset through all 16 alignments
    (16 x 17, 16 x 4099, 16 x 8703), then uniform draws."""
    lead = [4, 8704, *range(5, 20), *[17] * 16, *[4099] * 16, *[8703] * 16, 8704, 4]
    rng = np.random.default_rng([LS.SEED, 3, seed])
    body = rng.integers(4, 8705, max(n - len(lead), 0))
    return np.concatenate([lead, body])[:n].astype(np.int64)


COMPACT_COUNTS = [1, 63, 64, 65, 4095, 4096, 4097, 16 * 4096 - 1, 16 * 4096 + 1, 257 * 4096 + 1]


@pytest.mark.parametrize("n", COMPACT_COUNTS)
def test_compact_equals_a_plain_concatenation(H, n):
    """Synthetic slots (random bytes, the clen field set; the scans and the gather read nothing else): offsets are the
    exclusive cumsum of the clens, the stream is the clen prefixes back to back byte for byte, and nothing is written
    past offsets[n] (a canary behind it in an oversized buffer) nor past offsets[n] in the offsets array.  257*4096 + 1
    packets is more than 256 tiles: two passes of scan_tile_prefix_kernel."""
    clens = _synthetic_clens(n, n)
    d_clens = torch.from_numpy(clens).cuda()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(LS.SEED + n)
    d_slots = torch.randint(0, 256, (n, SLOT), dtype=torch.uint8, device="cuda", generator=gen)
    d_slots[:, 0] = (d_clens & 0xFF).to(torch.uint8)
    d_slots[:, 1] = (d_clens >> 8).to(torch.uint8)
    total = int(clens.sum())
    d_stream = torch.full((total + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    d_offsets = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    H.compact(d_slots.view(-1), n, d_stream, d_offsets)
    torch.cuda.synchronize()
    want_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    want_offs[1:] = torch.cumsum(d_clens, 0)
    assert torch.equal(d_offsets[:n + 1], want_offs), f"{n} packets: offsets differ from the exclusive cumsum"
    assert int(d_offsets[n + 1].item()) == -7, f"{n} packets: written past offsets[{n}]"
    tail = d_stream[total:]
    assert bool(tail.eq(0xA5).all()), \
        f"{n} packets: {int(tail.ne(0xA5).sum())} bytes written past offsets[n] = {total}, first at +{int(tail.ne(0xA5).nonzero()[0])}"
    # the stream, a chunk of packets at a time (masked_select keeps the clen prefixes of the rows in order)
    cols = torch.arange(SLOT, device="cuda")[None, :]
    step = 16384
    for a in range(0, n, step):
        b = min(a + step, n)
        want = d_slots[a:b].masked_select(cols < d_clens[a:b, None])
        got = d_stream[int(want_offs[a]):int(want_offs[b])]
        if not torch.equal(got, want):
            rows = torch.repeat_interleave(torch.arange(a, b, device="cuda"), d_clens[a:b])
            p = int(rows[(got != want).nonzero()[0]])
            at = int((got != want).nonzero()[0]) - int(want_offs[p] - want_offs[a])
            pytest.fail(f"{n} packets: packet {p} (clen {clens[p]}, destination offset {int(want_offs[p])}, "
                        f"alignment {int(want_offs[p]) % 16}) differs first at byte {at}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. and 6. every packet length through the batch kernels
# ---------------------------------------------------------------------------------------------------------------------
PAD = 4096                                             # canary bytes in front of and behind every output arena


def _batch_desc(bufs, base):
    """tests/batch_sweep.py's buffers at device address `base` as the three descriptor arrays (one upload), and their count."""
    ptrs, nbytes, first = BS.columns(bufs, base)
    d = torch.tensor(ptrs + nbytes + first, dtype=torch.int64).cuda()
    k = len(bufs)
    return d[:k], d[k:2 * k], d[2 * k:], k


def _decode_batch(H, via, d_src, d_offs, n, bufs, rows):
    """One launch of decode_batch (via "slots") or decode_stream_batch over n packets into `bufs`, laid out in the rows of a
    canary arena with PAD canary bytes on either side: (the rows in batch order, the launch's status word, pads intact)."""
    d_out = torch.full((n * PACKET + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    d_ptrs, d_bytes, d_fp, k = _batch_desc(bufs, d_out.data_ptr() + PAD)
    word = _status()
    if via == "slots":
        H.decode_batch(d_src, d_fp, k, n, d_ptrs, d_bytes, d_status=word)
    else:
        H.decode_stream_batch(d_src, d_offs, d_fp, k, n, d_ptrs, d_bytes, d_status=word)
    torch.cuda.synchronize()
    pads = bool(d_out[:PAD].eq(CANARY).all()) and bool(d_out[PAD + n * PACKET:].eq(CANARY).all())
    got = d_out[PAD:PAD + n * PACKET].view(n, PACKET).index_select(0, torch.from_numpy(np.asarray(rows)).cuda())
    return got, int(word.item()), pads


def _check_batch_rows(got, word, pads, order, sweep, rooms, what):
    assert word == 0, f"{what}: status {word:#x}"
    assert pads, f"{what}: written in front of the first or behind the last output row"
    want = sweep["rows"].index_select(0, torch.from_numpy(order).cuda())
    if not torch.equal(got, want):
        _first_wrong_row(got, want, order, sweep, what, rooms)


@pytest.mark.parametrize("mode", ["throughput", "latency"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_encode_batch_at_every_packet_length(H, sweep, layout, mode):
    """encode_batch_kernel / encode_small_batch_kernel with lanes of any lengths side by side: lane i is its own buffer
    holding packet order[i] + 1, so a wavefront's lanes own different numbers of whole phases and each partial phase waits
    for the final one.  The buffers lie 16-byte aligned in one arena in a seeded permuted address order, with zero-byte
    buffers at the front, the end and in runs between them; the bytes between buffers are 0x00 in one run and 0xFF in a
    second.  Each run: status 0, the input arena unchanged, every slot's clen bytes equal to the reference's encoding.  Both
    runs give the same slots byte for byte (nothing behind a buffer's end reaches its packet), and the slots decode back
    through both batch decoders."""
    order = LAYOUTS[layout]
    n = order.size
    sizes = sweep["ulens"][order]
    bufs, total = BS.scattered_inputs(sizes, n)
    starts = [off for off, _, _ in bufs if off is not None]               # lane order
    idx = torch.from_numpy(order).cuda()
    want = sweep["slots"].index_select(0, idx)
    keep = torch.arange(SLOT, device="cuda")[None, :] < sweep["d_clens"].index_select(0, idx)[:, None]
    runs = []
    for fill in (0x00, 0xFF):
        host = np.full(total, fill, dtype=np.uint8)
        for at, i in zip(starts, order):
            host[at:at + i + 1] = sweep["pkts"][i]
        d_arena = torch.from_numpy(host).cuda()
        d_before = d_arena.clone()
        assert d_arena.data_ptr() % 16 == 0
        d_ptrs, d_bytes, d_fp, k = _batch_desc(bufs, d_arena.data_ptr())
        d_slots = torch.full((n * SLOT,), 0xEE, dtype=torch.uint8, device="cuda")
        word = _status()
        H.encode_batch(d_ptrs, d_bytes, d_fp, k, n, d_slots=d_slots, d_status=word, mode=mode)
        torch.cuda.synchronize()
        what = f"encode_batch {mode}, {layout}, {fill:#04x} between buffers"
        assert int(word.item()) == 0, f"{what}: status {int(word.item()):#x}"
        assert torch.equal(d_arena, d_before), f"{what}: the input arena changed"
        got = d_slots.view(n, SLOT)
        if not torch.equal(torch.where(keep, got, 0), torch.where(keep, want, 0)):
            bad = (torch.where(keep, got, 0) != torch.where(keep, want, 0)).any(dim=1).nonzero().flatten()
            lane = int(bad[0])
            i = int(order[lane])
            at = int((got[lane] != want[lane])[:int(sweep["clens"][i])].nonzero()[0])
            pytest.fail(f"{what}: {bad.numel()} slots wrong; first: packet {i} (ulen {i + 1}, clen {int(sweep['clens'][i])}) "
                        f"at batch packet {lane} (wavefront {lane // 64}, lane {lane % 64}), byte {at}: "
                        f"got {int(got[lane, at]):#04x}, want {int(want[lane, at]):#04x}")
        runs.append(d_slots)
    if not torch.equal(runs[0], runs[1]):
        lane = int((runs[0].view(n, SLOT) != runs[1].view(n, SLOT)).any(dim=1).nonzero()[0])
        pytest.fail(f"encode_batch {mode}, {layout}: the slots depend on the bytes between buffers; first at batch packet {lane} "
                    f"(packet {int(order[lane])}, wavefront {lane // 64}, lane {lane % 64})")
    out_bufs, rows = BS.one_packet_outputs(sizes, n + 1)
    d_stream, d_offs = H.compact(runs[0], n)
    for via, d_src in (("slots", runs[0]), ("stream", d_stream)):
        got, word, pads = _decode_batch(H, via, d_src, d_offs, n, out_bufs, rows)
        _check_batch_rows(got, word, pads, order, sweep, sizes, f"encode_batch {mode}, {layout}: round trip through {via}")


@pytest.mark.parametrize("outputs", ["one_per_packet", "multi_packet"])
@pytest.mark.parametrize("source", ["slots", "stream_skew0", "stream_skew4"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_batch_at_every_packet_length(H, sweep, layout, source, outputs):
    """decode_slots_batch_kernel / decode_stream_batch_kernel on the sweep's reference slots, and on them back to back at
    pointer skew 0 and 4.  one_per_packet: each packet its own buffer, out_bytes = its ulen exactly (the room boundary at
    every length), in a seeded permutation of the arena's rows.  multi_packet: consecutive packets in buffers of 1-5,
    out_bytes = (k - 1) * 8192 + the last one's ulen, so the others have a room of 8192 and a canary behind their ulen.
    Zero-byte buffers among them.  Every row equals its packet with the canary behind it, status 0."""
    order = LAYOUTS[layout]
    n = order.size
    ulens = sweep["ulens"][order]
    if outputs == "one_per_packet":
        bufs, rows = BS.one_packet_outputs(ulens, n + 2)
    else:
        bufs, rows = BS.grouped_outputs(ulens, n + 3), np.arange(n)
    rooms = BS.lane_rooms(bufs)
    assert rooms.size == n and (rooms >= ulens).all()
    if source == "slots":
        via, raw, d_offs = "slots", None, None
        d_src = sweep["slots"].index_select(0, torch.from_numpy(order).cuda()).reshape(-1)
    else:
        via = "stream"
        raw, d_src, d_offs = _device_stream(sweep, order, int(source[-1]))
    got, word, pads = _decode_batch(H, via, d_src, d_offs, n, bufs, rows)
    _check_batch_rows(got, word, pads, order, sweep, rooms, f"decode_{via}_batch {layout}, {source}, {outputs}")
