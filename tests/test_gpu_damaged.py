"""Damaged packets through the HIP decoders, against the reference decoder (arDecompress through the pinned checker).

A damaged packet is ordinary input: what comes out is what arDecompress makes of it, which reads ulen from the header
and nothing else, and reads zeros behind its input.  tests/damage_sweep.py makes one damaged packet per length
1 ... 8192 (bit flips, bursts, cuts, raised and lowered ulen, random bodies, empty bodies, spliced headers), laid out
with the lane orders of tests/length_sweep.py: damage sits at lane 0 and lane 63, next to clean-length neighbours in the
same wavefront and in ragged last wavefronts.  Every row is compared to its ulen, with a canary behind it, and every
launch has a status word of its own.

Coverage of the hand-scheduled step: the whole sweep holds 30.9 million damaged symbols, 30.7 million of them in whole
64-symbol blocks (the asm step, its stream ring and its handoff to the plain step); part 1 sends about 405 million
damaged symbols through that step (five layouts, each through the slot decoder and four stream forms).

1. decode (slots), decode_stream (slot-spaced and back-to-back, pointer skew 0 and 4), garDecompressExecutor; and the
   batch decoders (decode_batch, decode_stream_batch) on the same forms, each packet its own output buffer (in permuted
   rows of a canary arena, zero-byte buffers among them) under three room rules: a room of 8192 (every row as the
   single-buffer decoders give it), the clean length n the packet was made from (what batch.decompress passes: a
   header whose ulen is above it is BAD_PACKET and its row keeps its canary), and ulen or ulen - 1 (exactly the second
   kind refused).  A one-packet buffer of 0 bytes is BAD_BATCH, not BAD_PACKET.
2. The 200 bit-flipped packets of tests/golden/seeded_vectors.json through both decoders.
3. Invalid headers (ulen > 8192, clen < 4): the row keeps its canary, BAD_PACKET lands in that launch's word only,
   every other row is right -- at every lane position, in a ragged last wavefront, in a wavefront of nothing else;
   through both single-buffer and both batch decoders.
4. What lies behind the end of the caller's buffer (garDecompressExecutor's `size`, decode_stream's offsets[n]), as
   include/gpuar_hip.h states it.  A packet shorter than 64 bytes is decoded by DecoderLane alone, which sees zeros
   there: cut by the end, it decodes as the reference decodes its bytes and zeros, whatever lies behind the end.  The
   stream ring of the hand-scheduled step repeats the 16-byte piece that holds the last byte instead (masking it was
   measured at +1.5 % decode time, gpuar_kernels.hip), so for an 8192-byte packet only this holds: bytes more than 16
   behind the end never change any row, the cut packet stays in its row and nothing is flagged.  A packet whose header
   is cut is flagged and writes nothing.  decode_stream_batch (64 one-packet buffers of room 8192) is held to the same.

The batch descriptors come from tests/batch_sweep.py.
"""
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import batch_sweep as BS
import damage_sweep as DS
import length_sweep as LS
from gpuar_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
CANARY = 0xC3
HERE = os.path.dirname(os.path.abspath(__file__))


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


def _ref_rows(oracle, views, ulens):
    """(len(views), 8192) uint8: the reference's decode of each staged packet, CANARY behind it.  Each decode must be
    exactly the header's ulen long: the reference stopping early would contradict the off < range argument that lets
    the hand-scheduled step skip the check (gpuar_kernels.hip, decode_wave)."""
    with ThreadPoolExecutor(16) as pool:                # (ctypes lets go of the GIL during the call)
        outs = list(pool.map(oracle.decode_packet, views))
    rows = np.full((len(views), PACKET), CANARY, dtype=np.uint8)
    for r, (o, u) in enumerate(zip(outs, ulens)):
        assert len(o) == u, f"the reference stopped after {len(o)} of {u} bytes on staged packet {r}"
        rows[r, :u] = np.frombuffer(o, dtype=np.uint8)
    return rows


@pytest.fixture(scope="module")
def dmg(oracle):
    """The 8192 damaged packets, their classes and ulens, and the rows the slot form must give (the reference on the
    packet and zeros behind it), on the device."""
    cache = {}

    def encode(m):
        if m not in cache:
            cache[m] = oracle.encode_stream(LS.packet(m))
        return cache[m]
    pkts, classes = DS.sweep(encode)
    ulens = np.asarray([DS.fields(p)[1] for p in pkts], dtype=np.int64)
    rows = _ref_rows(oracle, [p.tobytes() for p in pkts], ulens)
    return dict(pkts=pkts, classes=classes, ulens=ulens, encode=encode, rows=torch.from_numpy(rows).cuda())


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _first_wrong_row(got, want, order, dmg, what, rooms=None):
    """pytest.fail with the packet, lane, damage class, ulen (and room) and first differing byte of the first wrong row."""
    bad = (got != want).any(dim=1).nonzero().flatten()
    lane = int(bad[0])
    i = int(order[lane])
    ulen = int(dmg["ulens"][i]) if i >= 0 else 0
    cls = dmg["classes"][i] if i >= 0 else "invalid header"
    room = "" if rooms is None else f", room {int(rooms[lane])}"
    g, w = got[lane].cpu().numpy(), want[lane].cpu().numpy()
    at = int(np.flatnonzero(g != w)[0])
    where = "inside ulen" if at < ulen else "after ulen (canary overwritten)"
    pytest.fail(f"{what}: {bad.numel()} rows wrong; first: packet {i + 1 if i >= 0 else '-'} ({cls}) at row {lane} "
                f"(wavefront {lane // 64}, lane {lane % 64}), ulen {ulen}{room}, byte {at} {where}: got {g[at]:#04x}, want {w[at]:#04x}")


def _check_rows(d_out, want, order, dmg, what, rooms=None):
    """d_out: the output arena (rows in lane order from its start), or the rows themselves as an (n, 8192) tensor."""
    n = order.size
    got = d_out if d_out.dim() == 2 else d_out[:n * PACKET].view(n, PACKET)
    if not torch.equal(got, want):
        _first_wrong_row(got, want, order, dmg, what, rooms)


def _device_stream(stream: np.ndarray, skew: int):
    """The stream on the device at an address that is `skew` mod 16 (its own allocation, 64 bytes of slack)."""
    raw = torch.zeros(stream.size + 64, dtype=torch.uint8, device="cuda")
    base = (-raw.data_ptr()) % 16 + skew
    raw[base:base + stream.size] = torch.from_numpy(stream).cuda()
    d = raw[base:base + stream.size]
    assert d.data_ptr() % 16 == skew
    return raw, d


PAD = 4096                                              # canary bytes in front of and behind every batch output arena


def _launch_batch(H, via, d_src, d_offs, n, rooms, seed):
    """Launch decode_batch (via "slots") or decode_stream_batch over n packets, packet i into its own output buffer of
    rooms[i] bytes (tests/batch_sweep.py: seeded permuted rows of a canary arena, zero-byte buffers among them); no wait.
    Returns what _batch_rows needs."""
    bufs, rows = BS.one_packet_outputs(rooms, seed)
    d_out = torch.full((n * PACKET + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    ptrs, nbytes, first = BS.columns(bufs, d_out.data_ptr() + PAD)
    d = torch.tensor(ptrs + nbytes + first, dtype=torch.int64).cuda()
    k = len(bufs)
    word = _status()
    if via == "slots":
        H.decode_batch(d_src, d[2 * k:], k, n, d[:k], d[k:2 * k], d_status=word)
    else:
        H.decode_stream_batch(d_src, d_offs, d[2 * k:], k, n, d[:k], d[k:2 * k], d_status=word)
    return d_out, rows, word, (d, d_src, d_offs)


def _batch_rows(launched, n, what):
    """After the launch: (its output rows in batch order, its status word); asserts nothing was written into the pads."""
    d_out, rows, word, _ = launched
    torch.cuda.synchronize()
    assert bool(d_out[:PAD].eq(CANARY).all()) and bool(d_out[PAD + n * PACKET:].eq(CANARY).all()), \
        f"{what}: written in front of the first or behind the last output row"
    return d_out[PAD:PAD + n * PACKET].view(n, PACKET).index_select(0, torch.from_numpy(rows).cuda()), int(word.item())


def _decode_stream(H, stream, offs, n, skew):
    raw, d_stream = _device_stream(stream, skew)
    d_out = torch.full((n * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    word = _status()
    H.decode_stream(d_stream, torch.from_numpy(offs).cuda(), n, d_out, d_status=word)
    torch.cuda.synchronize()
    return d_out, int(word.item())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the damage sweep through every decoder
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = LS.layouts()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_slots_on_damaged_packets(H, dmg, layout):
    """Slot form (zeros to each slot's end): each row equals the reference to ulen, the canary behind it survives,
    and the status word stays 0 (every header here is one the decoders accept)."""
    order = LAYOUTS[layout]
    n = order.size
    d_slots = torch.from_numpy(DS.slot_form([dmg["pkts"][i] for i in order])).cuda()
    d_out = torch.full((n * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    word = _status()
    H.decode(d_slots, n, d_out, d_status=word)
    torch.cuda.synchronize()
    assert int(word.item()) == 0, f"{layout}: status {int(word.item()):#x}"
    _check_rows(d_out, dmg["rows"].index_select(0, torch.from_numpy(order).cuda()), order, dmg, f"decode (slots) {layout}")


_STREAM_ROWS = {}


def _stream_rows(oracle, dmg, layout, spacing):
    """The packets of `layout` in stream form and what the reference makes of each, shown the bytes that really follow
    it (damage_sweep.reference_view): in a back-to-back stream a damaged packet reads on into its neighbours."""
    key = (layout, spacing)
    if key not in _STREAM_ROWS:
        order = LAYOUTS[layout]
        stream, offs = DS.stream_form([dmg["pkts"][i] for i in order], spacing)
        views = [DS.reference_view(stream, int(offs[p]), int(offs[-1])) for p in range(order.size)]
        rows = _ref_rows(oracle, views, dmg["ulens"][order])
        _STREAM_ROWS[key] = (stream, offs, torch.from_numpy(rows).cuda())     # (kept for the batch tests: 340 MiB in all)
    return _STREAM_ROWS[key]


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("spacing", ["slot_spaced", "back_to_back"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_stream_on_damaged_packets(H, oracle, dmg, layout, spacing, skew):
    """decode_stream on the packets every 8704 bytes (zeros between) and back to back, pointer skew 0 and 4: each row
    equals the reference shown the same following bytes, the canary survives, the status word stays 0."""
    order = LAYOUTS[layout]
    stream, offs, want = _stream_rows(oracle, dmg, layout, SLOT if spacing == "slot_spaced" else None)
    d_out, word = _decode_stream(H, stream, offs, order.size, skew)
    assert word == 0, f"{layout} {spacing} skew {skew}: status {word:#x}"
    _check_rows(d_out, want, order, dmg, f"decode_stream {layout}, {spacing}, skew {skew}")


def test_garDecompressExecutor_on_damaged_packets(H, dmg):
    """The reference-named entry point (slots, NULL stream, the device's fallback status word) on the packets of the
    ragged layout whose last wavefront has 63 live lanes."""
    lib = H.load()
    order = LAYOUTS["last_wave_63_live"]
    n = order.size
    d_slots = torch.from_numpy(DS.slot_form([dmg["pkts"][i] for i in order])).cuda()
    d_out = torch.full((n * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    H.status()                                          # (clears what earlier launches left in the fallback word)
    lib.garDecompressExecutor(d_slots.data_ptr(), n * SLOT, d_out.data_ptr(), (n + 31) // 32)
    torch.cuda.synchronize()
    assert lib.gpuar_hip_last_error() == 0
    assert H.status() == 0
    _check_rows(d_out, dmg["rows"].index_select(0, torch.from_numpy(order).cuda()), order, dmg, "garDecompressExecutor")


ROOM_RULES = ("8192", "clean_length", "ulen_or_ulen_minus_1")


def _rooms(rule, order, dmg):
    """Each lane's room under `rule`, and which lanes the batch decoders must refuse (ulen > room).  Every room is >= 1:
    a one-packet buffer of 0 bytes is BAD_BATCH (test_batch_zero_room_is_bad_batch)."""
    ulens = dmg["ulens"][order]
    if rule == "8192":
        rooms = np.full(order.size, PACKET, dtype=np.int64)
    elif rule == "clean_length":                        # the packet was made from packet(n), n = order + 1
        rooms = order + 1
    else:                                               # a seeded half of the lanes with ulen >= 2 one byte short
        short = (np.random.default_rng([DS.SEED, order.size]).random(order.size) < 0.5) & (ulens >= 2)
        rooms = np.where(short, ulens - 1, np.maximum(ulens, 1))
    return rooms, ulens > rooms


def _check_batch_rules(H, via, d_src, d_offs, order, want, dmg, rule, what):
    """One batch launch under room rule `rule`: the refused rows keep their whole canary, every other row is `want`'s, the
    status word is exactly BAD_PACKET if any lane is refused and 0 otherwise."""
    n = order.size
    rooms, refused = _rooms(rule, order, dmg)
    assert rule == "8192" or refused.any(), f"{what}: rule {rule} refuses nothing here"
    what = f"{what}, rooms {rule}"
    got, word = _batch_rows(_launch_batch(H, via, d_src, d_offs, n, rooms, n + len(rule)), n, what)
    want_word = H.STATUS_BAD_PACKET if refused.any() else 0
    assert word == want_word, f"{what}: status {word:#x}, want {want_word:#x} ({int(refused.sum())} lanes refused)"
    want = want.clone()
    if refused.any():
        want[torch.from_numpy(np.flatnonzero(refused)).cuda()] = CANARY
    _check_rows(got, want, order, dmg, what, rooms)


@pytest.mark.parametrize("rule", ROOM_RULES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_slots_batch_on_damaged_packets(H, dmg, layout, rule):
    """decode_slots_batch_kernel on the slot form, one output buffer per packet, under each room rule (_rooms); with rooms
    of 8192 exactly what test_decode_slots_on_damaged_packets demands of the single-buffer decoder."""
    order = LAYOUTS[layout]
    d_slots = torch.from_numpy(DS.slot_form([dmg["pkts"][i] for i in order])).cuda()
    want = dmg["rows"].index_select(0, torch.from_numpy(order).cuda())
    _check_batch_rules(H, "slots", d_slots, None, order, want, dmg, rule, f"decode_batch {layout}")


@pytest.mark.parametrize("rule", ROOM_RULES)
@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("spacing", ["slot_spaced", "back_to_back"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_stream_batch_on_damaged_packets(H, oracle, dmg, layout, spacing, skew, rule):
    """decode_stream_batch_kernel on the stream forms of test_decode_stream_on_damaged_packets (the same rows, the reference
    shown the same following bytes), one output buffer per packet, under each room rule."""
    order = LAYOUTS[layout]
    stream, offs, want = _stream_rows(oracle, dmg, layout, SLOT if spacing == "slot_spaced" else None)
    raw, d_stream = _device_stream(stream, skew)
    _check_batch_rules(H, "stream", d_stream, torch.from_numpy(offs).cuda(), order, want, dmg, rule,
                       f"decode_stream_batch {layout}, {spacing}, skew {skew}")


@pytest.mark.parametrize("via", ["slots", "stream"])
def test_batch_zero_room_is_bad_batch(H, dmg, via):
    """A one-packet buffer of 0 bytes (at lanes 0, 37 and 63 of one wavefront and lane 63 of the next) starts at its
    buffer's end: BAD_BATCH exactly, not BAD_PACKET, and its row keeps its canary; the rest (room 8192) is right."""
    order = LAYOUTS["permuted"][:128]
    n = order.size
    rooms = np.full(n, PACKET, dtype=np.int64)
    zero = [0, 37, 63, 127]
    rooms[zero] = 0
    pkts = [dmg["pkts"][i] for i in order]
    if via == "slots":
        d_src, d_offs = torch.from_numpy(DS.slot_form(pkts)).cuda(), None
    else:
        stream, offs = DS.stream_form(pkts, DS.STREAM_TAIL)
        raw, d_src = _device_stream(stream, 4)
        d_offs = torch.from_numpy(offs).cuda()
    what = f"decode_{via}_batch, zero-byte buffers at {zero}"
    got, word = _batch_rows(_launch_batch(H, via, d_src, d_offs, n, rooms, 7), n, what)
    assert word == H.STATUS_BAD_BATCH, f"{what}: status {word:#x}"
    want = dmg["rows"].index_select(0, torch.from_numpy(order).cuda()).clone()
    want[zero] = CANARY
    _check_rows(got, want, order, dmg, what, rooms)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the golden bit-flipped packets
# ---------------------------------------------------------------------------------------------------------------------
def test_corrupted_golden_packets_through_both_decoders(H, oracle):
    """The 200 packets with 1-3 flipped bits of tests/golden/seeded_vectors.json (what host_codec.cpp is held to):
    each decoder's row has the reference's decoded length and md5, and the canary behind it.  Slot form, and a stream
    whose packets lie STREAM_TAIL bytes apart (zeros behind each, as the stored decode assumes)."""
    with open(os.path.join(HERE, "golden", "seeded_vectors.json")) as f:
        cases = json.load(f)["corrupted_packets"]
    assert len(cases) == 200
    pkts = []
    for trial, c in enumerate(cases):
        pkt = oracle.encode_stream(synth.generate(c["kind"], c["seed"], c["n"]))
        assert hashlib.md5(pkt.tobytes()).hexdigest() == c["packet_md5"], trial
        for byte, bit in c["flips"]:
            pkt[byte] ^= np.uint8(1 << bit)
        pkts.append(pkt)
    n = len(pkts)
    d_out = torch.full((n * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    word = _status()
    H.decode(torch.from_numpy(DS.slot_form(pkts)).cuda(), n, d_out, d_status=word)
    torch.cuda.synchronize()
    outs = {"decode (slots)": (d_out.cpu().numpy(), int(word.item()))}
    stream, offs = DS.stream_form(pkts, DS.STREAM_TAIL)
    d_out, w = _decode_stream(H, stream, offs, n, 4)
    outs["decode_stream"] = (d_out.cpu().numpy(), w)
    for what, (out, w) in outs.items():
        assert w == 0, f"{what}: status {w:#x}"
        rows = out.reshape(n, PACKET)
        for trial, c in enumerate(cases):
            k = c["decoded_len"]
            assert hashlib.md5(rows[trial, :k].tobytes()).hexdigest() == c["decoded_md5"], \
                f"{what}: corrupted packet {trial} (ulen {k}, flips {c['flips']}) differs from the reference"
            assert (rows[trial, k:] == CANARY).all(), f"{what}: corrupted packet {trial}: written after ulen {k}"


# ---------------------------------------------------------------------------------------------------------------------
# 3. invalid headers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def invalid(dmg):
    return DS.invalid(dmg["encode"])


def _launch_with_invalid(H, dmg, order, bad_at, decoder):
    """One launch over the sweep packets `order`, with the invalid packets `bad_at` = {row: (packet, what)} in place of
    theirs; and a second launch in flight behind it over the same packets without them.  Slot form, or a stream whose
    packets lie STREAM_TAIL apart (so every valid row's expectation is the slot form's); through decode / decode_stream,
    or (decoder "slots_batch" / "stream_batch") their batch kernels, each packet its own output buffer of 8192 bytes.
    Returns nothing: asserts."""
    n = order.size
    pkts = [bad_at[r][0] if r in bad_at else dmg["pkts"][i] for r, i in enumerate(order)]
    clean = [dmg["pkts"][i] for i in order]
    via = decoder.split("_")[0]
    results = []
    for ps in (pkts, clean):
        if via == "slots":
            d_in, d_offs = torch.from_numpy(DS.slot_form(ps)).cuda(), None
        else:
            stream, offs = DS.stream_form(ps, DS.STREAM_TAIL)
            raw, d_in = _device_stream(stream, 4)
            d_offs = torch.from_numpy(offs).cuda()
        if decoder.endswith("_batch"):
            results.append(_launch_batch(H, via, d_in, d_offs, n, np.full(n, PACKET), n))
            continue
        d_out = torch.full((n * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
        word = _status()
        if via == "slots":
            H.decode(d_in, n, d_out, d_status=word)
        else:
            H.decode_stream(d_in, d_offs, n, d_out, d_status=word)
        results.append((d_out, word, (d_in, d_offs)))
    where = f"{decoder}, invalid rows {sorted((r, bad_at[r][1]) for r in bad_at)[:4]}"
    if decoder.endswith("_batch"):
        (d_out, word), (d_clean, word_clean) = (_batch_rows(r, n, where) for r in results)
    else:
        torch.cuda.synchronize()
        (d_out, word, _), (d_clean, word_clean, _) = results
        word, word_clean = int(word.item()), int(word_clean.item())
    assert word == H.STATUS_BAD_PACKET, f"{where}: status {word:#x}"
    assert word_clean == 0, f"{where}: the flag reached the launch behind it"
    want = dmg["rows"].index_select(0, torch.from_numpy(order).cuda()).clone()
    rows = torch.tensor(sorted(bad_at), dtype=torch.int64, device="cuda")
    want[rows] = CANARY                                  # an invalid packet's whole 8192-byte row keeps its canary
    marked = order.copy()
    marked[sorted(bad_at)] = -1
    _check_rows(d_out, want, marked, dmg, where)
    _check_rows(d_clean, dmg["rows"].index_select(0, torch.from_numpy(order).cuda()), order, dmg, where + " (clean launch)")


@pytest.mark.parametrize("decoder", ["slots", "stream", "slots_batch", "stream_batch"])
def test_invalid_header_at_every_lane(H, dmg, invalid, decoder):
    """One wavefront per lane position 0 ... 63, the invalid header there (the six kinds in turn), damaged packets
    with valid headers in the other 63 lanes."""
    perm = LAYOUTS["permuted"]
    for lane in range(64):
        order = perm[64 * lane:64 * lane + 64]
        _launch_with_invalid(H, dmg, order, {lane: invalid[lane % len(invalid)]}, decoder)


@pytest.mark.parametrize("decoder", ["slots", "stream", "slots_batch", "stream_batch"])
def test_invalid_headers_in_ragged_and_all_invalid_wavefronts(H, dmg, invalid, decoder):
    """Invalid headers at lane 0 of a last wavefront with one live lane, at lane 62 of one with 63, and a wavefront
    in which every lane is invalid, between two wavefronts of valid packets."""
    for layout, row in (("last_wave_1_live", 64 * 5), ("last_wave_63_live", 64 * 3 + 62)):
        order = LAYOUTS[layout]
        _launch_with_invalid(H, dmg, order, {row: invalid[row % len(invalid)], 0: invalid[1]}, decoder)
    order = LAYOUTS["permuted"][:64 * 3]
    _launch_with_invalid(H, dmg, order, {64 + j: invalid[j % len(invalid)] for j in range(64)}, decoder)


def test_zero_ulen_writes_nothing_and_is_not_flagged(H, oracle):
    """ulen = 0 behind a valid clen: no byte of the row is written and nothing is flagged, at lanes 0, 31 and 63; through
    both decoders and both batch decoders (each packet its own output buffer of 8192 bytes)."""
    pkt = oracle.encode_stream(LS.packet(5000))
    pkt[2:4] = 0
    clean = [oracle.encode_stream(LS.packet(m)) for m in range(1, 65)]
    ps = [pkt if r in (0, 31, 63) else clean[r] for r in range(64)]
    for decoder in ("slots", "stream", "slots_batch", "stream_batch"):
        if decoder == "slots_batch":
            launched = _launch_batch(H, "slots", torch.from_numpy(DS.slot_form(ps)).cuda(), None, 64, np.full(64, PACKET), 64)
            d_out, word = _batch_rows(launched, 64, decoder)
        elif decoder == "stream_batch":
            stream, offs = DS.stream_form(ps)
            raw, d_stream = _device_stream(stream, 0)
            launched = _launch_batch(H, "stream", d_stream, torch.from_numpy(offs).cuda(), 64, np.full(64, PACKET), 64)
            d_out, word = _batch_rows(launched, 64, decoder)
        elif decoder == "slots":
            d_out = torch.full((64 * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
            word = _status()
            H.decode(torch.from_numpy(DS.slot_form(ps)).cuda(), 64, d_out, d_status=word)
            torch.cuda.synchronize()
            word = int(word.item())
        else:
            stream, offs = DS.stream_form(ps)
            d_out, word = _decode_stream(H, stream, offs, 64, 0)
        assert word == 0, decoder
        rows = d_out.reshape(64, PACKET).cpu().numpy()
        for r in range(64):
            if r in (0, 31, 63):
                assert (rows[r] == CANARY).all(), (decoder, r)
            else:
                assert np.array_equal(rows[r, :r + 1], LS.packet(r + 1)) and (rows[r, r + 1:] == CANARY).all(), (decoder, r)


# ---------------------------------------------------------------------------------------------------------------------
# 4. behind the end of the caller's buffer
# ---------------------------------------------------------------------------------------------------------------------
# (last packet, cut): where the last packet is cut (bytes of it still readable).  "full": 8192 bytes, decoded through the
# hand-scheduled step and its stream ring; "short": 40 bytes, decoded by the plain step (DecoderLane) alone.  Cuts of 1-3
# bytes leave the header itself behind the end.
CASES = ([("full", c) for c in (1, 2, 3, 4, 8, 17, 30, 1001, 2048, 4099, 6000, 7777)]
         + [("short", c) for c in (1, 3, 4, 5, 8, 13, 20, 29)])


@pytest.fixture(scope="module")
def tail_packets(oracle):
    """63 well-formed 8192-byte packets (three source models in turn) and a last one of each kind: data and encodings."""
    data = [synth.generate(synth.KINDS[k % 3], 900 + k, PACKET) for k in range(64)]
    last = {"full": data[63], "short": synth.generate("text", 977, 40)}
    encs = [oracle.encode_stream(d) for d in data[:63]]
    return data[:63], encs, {k: (d, oracle.encode_stream(d)) for k, d in last.items()}


def _cut_expectation(oracle, enc, cut):
    """The row the cut packet must give: the reference's decode of its first `cut` bytes followed by zeros (CANARY
    behind ulen), or -- when the header itself is cut -- no byte at all, and BAD_PACKET."""
    row = np.full(PACKET, CANARY, dtype=np.uint8)
    if cut < 4:
        return row, H_BAD
    back = oracle.decode_packet(enc[:cut].tobytes())
    assert len(back) == DS.fields(enc)[1], "the reference stopped early"
    row[:len(back)] = np.frombuffer(back, dtype=np.uint8)
    return row, 0


H_BAD = 0x2                                                # GPUAR_STATUS_BAD_PACKET


def _check_cut_run(out, data, want_row, what, exact=True):
    """The 63 packets in front of the cut one decode to their data, nothing is written past the last row, and (exact)
    the cut packet's row is `want_row`."""
    assert (out[64 * PACKET:] == CANARY).all(), f"{what}: written past the last row"
    assert np.array_equal(out[:63 * PACKET], np.concatenate(data)), f"{what}: a packet in front of the cut one is wrong"
    got = out[63 * PACKET:64 * PACKET]
    if exact and not np.array_equal(got, want_row):
        at = int(np.flatnonzero(got != want_row)[0])
        pytest.fail(f"{what}: the cut packet differs from the reference's zero-padded decode first at byte {at}: "
                    f"got {got[at]:#04x}, want {want_row[at]:#04x}")


# The runs of one case: what the 16 bytes right behind the end hold, and what lies further behind.  A short packet (and a
# cut header) must give the reference's row in every run; an 8192-byte one must give the same row in the first two.
RUNS = ((0x00, 0x00), (0x00, 0xEE), (0xEE, 0xEE))


def _behind(near: int, far: int, n: int) -> np.ndarray:
    out = np.full(n, far, dtype=np.uint8)
    out[:16] = near
    return out


def _same_far_behind(rows, what):
    assert np.array_equal(rows[0], rows[1]), f"{what}: bytes more than 16 behind the end changed the cut packet's row"


@pytest.mark.parametrize("last,cut", CASES)
def test_garDecompressExecutor_behind_size(H, oracle, tail_packets, last, cut):
    """`size` ends `cut` bytes into the last slot's packet (its header kept), each run its own allocation with RUNS
    behind source + size.  The 63 packets in front decode to their data; the status word is 0, or BAD_PACKET for a cut
    header (whose row keeps its canary)."""
    lib = H.load()
    data, encs, lasts = tail_packets
    enc = lasts[last][1]
    assert cut < enc.size
    slots = DS.slot_form(encs + [enc])
    size = 63 * SLOT + cut
    want_row, want_word = _cut_expectation(oracle, enc, cut)
    exact = last == "short" or cut < 4
    H.status()
    rows = []
    for near, far in RUNS:
        buf = np.concatenate([slots[:size], _behind(near, far, SLOT + 256 - cut)])
        d_buf = torch.from_numpy(buf).cuda()
        d_out = torch.full((64 * PACKET + 4096,), CANARY, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        lib.garDecompressExecutor(d_buf.data_ptr(), size, d_out.data_ptr(), 2)
        torch.cuda.synchronize()
        assert lib.gpuar_hip_last_error() == 0
        assert H.status() == want_word, (last, cut, near, far)
        out = d_out.cpu().numpy()
        _check_cut_run(out, data, want_row, f"{last} packet cut at {cut}, {near:#04x}/{far:#04x} behind `size`", exact)
        rows.append(out[63 * PACKET:64 * PACKET])
    _same_far_behind(rows, f"{last} packet cut at {cut}")


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("last,cut", CASES)
def test_decode_stream_behind_the_stream_end(H, oracle, tail_packets, last, cut, skew):
    """A back-to-back stream of 64 packets whose offsets[n] lies `cut` bytes into the last one: the same runs and
    expectations as above, with this launch's own status word, at pointer skew 0 and 4; through decode_stream and through
    decode_stream_batch (64 one-packet buffers of 8192 bytes in the rows of the same canary arena)."""
    data, encs, lasts = tail_packets
    enc = lasts[last][1]
    stream = np.concatenate(encs + [enc])
    offs = np.zeros(65, dtype=np.int64)
    offs[1:] = np.cumsum([e.size for e in encs + [enc]])
    end = int(offs[63]) + cut
    offs[64] = end
    want_row, want_word = _cut_expectation(oracle, enc, cut)
    exact = last == "short" or cut < 4
    for decoder in ("decode_stream", "decode_stream_batch"):
        rows = []
        for near, far in RUNS:
            buf = np.concatenate([stream[:end], _behind(near, far, 256)])
            raw, d_buf = _device_stream(buf, skew)
            d_offs = torch.from_numpy(offs).cuda()
            d_out = torch.full((64 * PACKET + 4096,), CANARY, dtype=torch.uint8, device="cuda")
            word = _status()
            if decoder == "decode_stream":
                H.decode_stream(d_buf, d_offs, 64, d_out, d_status=word)
            else:
                d = torch.tensor([d_out.data_ptr() + r * PACKET for r in range(64)] + [PACKET] * 64 + list(range(65)),
                                 dtype=torch.int64).cuda()
                H.decode_stream_batch(d_buf, d_offs, d[128:], 64, 64, d[:64], d[64:128], d_status=word)
            torch.cuda.synchronize()
            assert int(word.item()) == want_word, (decoder, last, cut, near, far)
            out = d_out.cpu().numpy()
            _check_cut_run(out, data, want_row, f"{decoder}: {last} packet cut at {cut}, {near:#04x}/{far:#04x} behind offsets[n]", exact)
            rows.append(out[63 * PACKET:64 * PACKET])
        _same_far_behind(rows, f"{decoder}: {last} packet cut at {cut}")
