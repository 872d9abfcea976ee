"""Where the buffers lie and how far into a buffer a kernel works: every entry point of include/gpuar_hip.h at the weakest
pointer alignment its contract allows, with the address line 2^32 (where a pointer's low word carries into its high word)
inside each of its buffers in turn, and -- the filter, CRC, estimate and survey kernels -- at offsets past 2^32 inside one buffer.
The other GPU modules vary packet lengths, contents and concurrency and hand over the first byte of a fresh allocation.

Every buffer of parts A and B is a slice of ONE arena of 2^32 + 128 MiB bytes, which therefore holds a multiple of 2^32 with
64 MiB on both sides (tests/address_edges.py::line_in; asserted, not skipped).  A slice has GUARD canary bytes on both sides,
checked after the call; an output starts as canaries, so whatever a call must leave alone (behind a packet's ulen, behind
clen in a stream, the stride gap and the unasked rows of a survey) is compared too; an input must come back unchanged.  Only
the windows in use are ever touched, and nothing is placed at the end of the allocation.  Before each launch the placement
asserts ptr % (2 * align) == align (weak, straddling) and ptr < line < ptr + nbytes (part B).  Comparisons are exact and run on
the device; one copy of the verdicts per test.  Every status word is read and compared (0 unless the case says otherwise); the
calls without a word report into the fallback word, which must be 0 at the end of each test.

A. Weakest alignment.  All pointer arguments weak at once, then each in turn while the others are 4096-aligned, so a failure
   names the argument.  Codec (130 packets + 4097 bytes of synth text and uniform: encode in its three modes -- throughput, latency and table,
   the table-walk kernel that auto takes for large inputs --, decode, compact,
   decode_stream with the stream at 4 and at 12 mod 16, the reference-named executors), the batch codec over the lengths of
   length_sweep's layout "last_wave_1_live" (inputs from batch_sweep.scattered_inputs, outputs 16 bytes apart, permuted, none
   32-aligned, the stream at skew 4, descriptor arrays 8- but not 16-aligned), CRC-32 (9 packets + 77 bytes; batch pointers
   16-weak, not packet-aligned), the filters (planes, delta, xor; w = 1, 2, 4, 8; out of place and in place; 3 * 65536 + 4097 + 5
   bytes), estimate and both surveys (d_est 4-weak, odd stride P + 1, mask 15 and the single width 8), move_packets (1, 15, 16,
   17, 8191, 8192 bytes), generate and gpuar_hip_copy.  generate's d_out must be 8-byte aligned (its kernels store 8 bytes at a
   time): at offsets 1 and 4 it returns GPUAR_ERR_ALIGNMENT and writes nothing, which the header now says.
B. The same shapes and references with the line inside one pointer argument at a time, the others weak elsewhere: in the
   middle of a packet of the second wavefront group, inside a slot's coded bytes, inside the compacted stream, the offsets
   array, a survey's rows, a filter's tail, the XOR base; and with a packet / slot / group boundary exactly on the line.  (A
   boundary on the line makes the start a multiple of the unit, 8192 or 512 bytes for slots: those placements cannot be weak
   as well and assert the boundary instead.)  Batch calls: one buffer straddles; in a second layout one buffer ends exactly
   at the line and the next begins at it.
C. One buffer of 2^32 + 3 * 65536 + 4097 + 5 bytes (packet 524288 starts at byte 2^32), generated on the device, three
   windows overwritten with sorted 64-bit integers (so the delta filter's borrows run through every byte): split / merge of
   planes (w = 8, 2), delta (w = 8) and xor (w = 8, in place, against a base of the same size that is freed right after), crc32
   and verify_crc32 with one byte flipped at 2^32 + 5 (first_bad = 524288), estimate and both surveys.  Compared against the
   *_host functions on three windows ([0, 128 KiB), 128 KiB either side of 2^32, the last group with the tail); over the
   whole buffer merge(split(x)) == x and the canary behind n holds.  The codec is not repeated (the 5 GiB tests cover it).

Time, pytest --durations=0 on an MI355X, the module alone: 24 passed in 3.8 s (605 placed launches in parts A and B; the
table-mode encode cases added since make it 625).
    0.50 s  setup of test_codec_at_the_weakest_alignment[text] (the arena, the reference encoder on 2 x 1 MiB)
    0.39 s  test_filters_past_4gib[delta-8] (the first of part C: generates and fills the 4 GiB buffer)
    0.29 s  test_codec_at_the_weakest_alignment[text] (the first launches of the process)
    0.10 s  setup of test_batch_codec_at_the_weakest_alignment (321 reference packets)
    0.06 s  test_codec_across_the_address_line[text], [uniform]
    0.04 s  test_codec_at_the_weakest_alignment[uniform], test_batch_codec_at_the_weakest_alignment, test_xor_in_place_past_4gib
    0.03 s  test_batch_codec_across_the_address_line
    0.02 s  test_filters_past_4gib[planes-8], test_filters_across_the_address_line[xor]
    0.01 s  test_filters_past_4gib[planes-2], test_estimate_and_surveys_past_4gib, test_crc32_at_the_weakest_alignment, the other
            filter tests; every remaining test and setup is under 0.005 s.
No shape had to shrink: no case of parts A and B comes near 5 s.  Memory: 4.1 GiB for the arena, at most 8.5 GiB more during
part C.  Fixed seeds throughout.
"""
import zlib

import numpy as np
import pytest

import address_edges as AE
import batch_sweep as BS
import length_sweep as LS
from concurrency_checks import _fail_on, _same
from gpuar_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
MiB = 1 << 20
MARGIN = 64 * MiB
GUARD = 256
CANARY = 0xA5
CANARY32 = 0xA5A5A5A5
LOW = 48 * MiB                        # the buffers that do not straddle are taken from [0, LOW): below the line's margin
WIDTHS = (1, 2, 4, 8)
FAMILIES = ("planes", "delta", "xor")
GROUP = 8 * PACKET                    # 65536: a group of w = 8, a supergroup of the surveys
BIG = AE.LINE + 3 * GROUP + 4097 + 5  # part C's buffer
SEED = 20261018


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()          # raises if the HIP library is missing: no fallback
    return hip


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    codec = O.require_best()
    assert codec.kind == O.expected_kind()
    return codec


# ---------------------------------------------------------------------------------------------------------------------
# the arena and the placements
# ---------------------------------------------------------------------------------------------------------------------
class Arena:
    """Slices of one allocation, each between two guards of canaries; see the module docstring."""

    def __init__(self, t):
        self.t, self.base, self.size = t, t.data_ptr(), t.numel()
        self.L = AE.line_in(self.base, self.size, MARGIN)
        self.line = self.base + self.L
        assert self.line % AE.LINE == 0 and self.base < self.line < self.base + self.size
        self.reset()

    def reset(self):
        self.cursor, self.held = 0, []

    def _take(self, off, nbytes):
        lo, hi = off - GUARD, off + nbytes + GUARD
        assert 0 <= lo and hi <= self.size, f"[{lo}, {hi}) leaves the arena"
        for o, n in self.held:
            assert hi <= o - GUARD or o + n + GUARD <= lo, "two placements overlap"
        self.held.append((off, nbytes))
        self.t[lo:hi].fill_(CANARY)
        return self.t[off:off + nbytes]

    def _bump(self, nbytes, multiple, residue):
        at = self.base + self.cursor + GUARD
        off = (AE.weak(at, residue) if multiple == 2 * residue else at + (residue - at) % multiple) - self.base
        self.cursor = off + nbytes + GUARD
        assert self.cursor <= LOW
        return off

    def put(self, nbytes, align, how="weak", block=False):
        """`nbytes` at a placement: "weak" (aligned to `align` and to nothing coarser; a block: a multiple of `align`), "page"
        (4096-aligned), ("skew", m, r) (address % m == r), ("in", k) (straddling the line, about k bytes in front of it, weak),
        ("on", k) (exactly k bytes in front of the line).  Asserts what it promises."""
        if how == "weak":
            off = self._bump(nbytes, align, 0) if block else self._bump(nbytes, 2 * align, align)
        elif how == "page":
            off = self._bump(nbytes, 4096, 0)
        elif how[0] == "skew":
            off = self._bump(nbytes, how[1], how[2])
        elif how[0] == "in":
            assert not block
            off = AE.straddle(self.L, nbytes, how[1] / nbytes, align)
        else:
            assert how[0] == "on"
            off = self.L - how[1]
        v = self._take(off, nbytes)
        ptr = v.data_ptr()
        assert ptr == self.base + off and ptr % align == 0
        if how == "page":
            assert ptr % 4096 == 0
        elif how[0] == "skew":
            assert ptr % how[1] == how[2]
        elif not block and (how == "weak" or how[0] == "in"):
            assert ptr % (2 * align) == align, f"{ptr:#x} is not aligned to {align} and nothing coarser"
        if how[0] in ("in", "on") and how != "weak":
            assert ptr < self.line < ptr + nbytes, f"the line {self.line:#x} is not inside [{ptr:#x}, +{nbytes})"
        return v

    def guards(self, tag):
        ok = torch.ones((), dtype=torch.bool, device="cuda")
        for off, n in self.held:
            ok = ok & self.t[off - GUARD:off].eq(CANARY).all() & self.t[off + n:off + n + GUARD].eq(CANARY).all()
        return (f"{tag}: canaries in front of or behind a buffer are gone", ok)


@pytest.fixture(scope="module")
def A(H):
    """The arena.  If it cannot be allocated the allocator's error fails the tests: no skip."""
    t = torch.empty(AE.LINE + 2 * MARGIN, dtype=torch.uint8, device="cuda")
    yield Arena(t)
    del t
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()


def _i32(v):
    return v.view(torch.int32)


def _i64(v):
    return v.view(torch.int64)


class Arg:
    """One pointer argument: nbytes, the alignment of its contract, what it holds before the call (`init`; None: canaries) and
    what it must hold after it (`want`; None: what it held before; `keep`: the bytes that are compared).  block: a block of
    buffers with their own offsets (placed at a multiple of `align`).  check=False: the test writes it itself (descriptors)."""

    def __init__(self, name, nbytes, align, init=None, want=None, keep=None, block=False, check=True):
        self.name, self.nbytes, self.align, self.block, self.check = name, int(nbytes), align, block, check
        self.init = None if init is None else _u8(init)
        if want is not None:
            self.want = _u8(want)
        elif init is not None:
            self.want = self.init
        else:
            self.want = torch.full((self.nbytes,), CANARY, dtype=torch.uint8, device="cuda")
        self.keep = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep).reshape(-1)).cuda()
        assert self.want.numel() == self.nbytes and (self.init is None or self.init.numel() == self.nbytes)


class Case:
    """A call under test: its pointer arguments, call(v) with v[name] the placed uint8 views, `moving`: the arguments part A
    moves one at a time (default: all), `lines`: part B's placements [(argument, ("in" | "on", k))], `fixed`: where an argument lies whenever it is not the one that moves."""

    def __init__(self, name, args, call, lines=(), moving=None, extra=(), fixed=None):
        self.name, self.args, self.call, self.lines, self.extra, self.fixed = name, args, call, list(lines), list(extra), dict(fixed or {})
        self.moving = [a.name for a in args] if moving is None else moving


def _run(A, case, place, tag, verdicts):
    A.reset()
    v = {}
    for arg in case.args:
        view = A.put(arg.nbytes, arg.align, place.get(arg.name, "weak"), arg.block)
        if arg.init is not None:
            view.copy_(arg.init)
        v[arg.name] = view
    case.call(v)
    for arg in case.args:
        if not arg.check:
            continue
        got = v[arg.name]
        ok = _same(got, arg.want) if arg.keep is None else (got.eq(arg.want) | ~arg.keep).all()
        verdicts.append((f"{case.name} [{tag}]: {arg.name} is not what it must be after the call", ok))
    verdicts.append(A.guards(f"{case.name} [{tag}]"))


def _part_a(H, A, cases):
    """All arguments weak at once; then each in turn with the others 4096-aligned; then the case's extra placements."""
    verdicts = []
    for case in cases:
        _run(A, case, case.fixed, "all weak", verdicts)
        for name in case.moving:
            place = {a.name: "page" for a in case.args if a.name != name and not a.block}
            place.update({k: how for k, how in case.fixed.items() if k != name})
            _run(A, case, place, f"{name} weak, the others 4096-aligned", verdicts)
        for place, tag in case.extra:
            _run(A, case, place, tag, verdicts)
    _fail_on(verdicts)
    assert H.status() == 0, "a launch reported into the fallback word"


def _part_b(H, A, cases):
    """The line inside one argument at a time, the others weak elsewhere."""
    verdicts, n = [], 0
    for case in cases:
        for name, how in case.lines:
            _run(A, case, {**case.fixed, name: how}, f"the line {how[1]} bytes into {name} ({how[0]})", verdicts)
            n += 1
    assert n, "no placement on the line"
    _fail_on(verdicts)
    assert H.status() == 0, "a launch reported into the fallback word"


def _status_arg(want=0):
    return Arg("d_status", 4, 4, init=np.zeros(1, np.uint32), want=np.array([want], np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the codec
# ---------------------------------------------------------------------------------------------------------------------
CODEC_N = 130 * PACKET + 4097
CODEC_NPK = 131


def _walk(stream, npk):
    """(slots image with canaries behind each clen, the mask of the coded bytes, offsets) of a packet stream."""
    slots = np.full((npk, SLOT), CANARY, dtype=np.uint8)
    keep = np.zeros((npk, SLOT), dtype=bool)
    offs = np.zeros(npk + 1, dtype=np.int64)
    at = 0
    for p in range(npk):
        c = int(stream[at]) | int(stream[at + 1]) << 8
        slots[p, :c] = stream[at:at + c]
        keep[p, :c] = True
        at += c
        offs[p + 1] = at
    assert at == stream.size
    return slots, keep, offs


def _boundary(offs, first, multiple):
    """The first packet from `first` on whose offset in the stream is a multiple of `multiple` (so it can lie on the line)."""
    for p in range(first, offs.size - 1):
        if offs[p] % multiple == 0:
            return int(offs[p])
    raise AssertionError(f"no packet from {first} on starts at a multiple of {multiple}")


def _codec_cases(H, oracle, kind):
    n, npk = CODEC_N, CODEC_NPK
    host = synth.generate(kind, 11, n)
    stream = oracle.encode_stream(host)
    slots, keep, offs = _walk(stream, npk)
    total = int(offs[-1])
    out_img = np.full(npk * PACKET, CANARY, dtype=np.uint8)
    out_img[:n] = host
    room = (total + 7) // 8 * 8
    stream_img = np.full(room, CANARY, dtype=np.uint8)
    stream_img[:total] = stream
    mid_in, mid_slot = 74 * PACKET + 4096, 70 * SLOT + 100              # inside packet 74 / the coded bytes of slot 70: second group
    assert 70 * SLOT + 100 < 70 * SLOT + (offs[71] - offs[70])
    in_lines = lambda name: [(name, ("in", mid_in)), (name, ("on", 64 * PACKET)), (name, ("on", 65 * PACKET))]
    slot_lines = lambda name: [(name, ("in", mid_slot)), (name, ("on", 64 * SLOT)), (name, ("on", 65 * SLOT))]
    off_lines = [("d_offsets", ("in", 66 * 8))]
    lib = H.load()

    def d_in():
        return Arg("d_in", n, 16, init=host)

    def d_slots_out():
        return Arg("d_slots", npk * SLOT, 16, want=slots, keep=keep)

    def d_slots_in():
        return Arg("d_slots", npk * SLOT, 16, init=slots)

    def d_out():
        return Arg("d_out", npk * PACKET, 16, want=out_img)

    cases = []
    for mode in ("throughput", "latency", "table"):
        cases.append(Case(f"encode {mode}, {kind}", [d_in(), d_slots_out(), _status_arg()],
                          lambda v, mode=mode: H.encode(v["d_in"], v["d_slots"], d_status=_i32(v["d_status"]), mode=mode),
                          lines=in_lines("d_in") + slot_lines("d_slots")))
    cases.append(Case(f"decode, {kind}", [d_slots_in(), d_out(), _status_arg()],
                      lambda v: H.decode(v["d_slots"], npk, v["d_out"], d_status=_i32(v["d_status"])),
                      lines=slot_lines("d_slots") + in_lines("d_out"), moving=["d_slots", "d_out"]))
    cases.append(Case(f"compact, {kind}", [d_slots_in(), Arg("d_stream", room, 8, want=stream_img), Arg("d_offsets", 8 * (npk + 1), 8, want=offs)],
                      lambda v: H.compact(v["d_slots"], npk, v["d_stream"], _i64(v["d_offsets"])),
                      lines=slot_lines("d_slots") + off_lines + [("d_stream", ("in", int(offs[70]) + 50)), ("d_stream", ("on", _boundary(offs, 64, 8)))]))
    cases.append(Case(f"decode_stream, {kind}", [Arg("d_stream", total, 4, init=stream), Arg("d_offsets", 8 * (npk + 1), 8, init=offs), d_out(),
                                                 _status_arg()],
                      lambda v: H.decode_stream(v["d_stream"], _i64(v["d_offsets"]), npk, v["d_out"], d_status=_i32(v["d_status"])),
                      lines=in_lines("d_out") + off_lines + [("d_stream", ("in", int(offs[70]) + 50)), ("d_stream", ("on", _boundary(offs, 64, 4)))],
                      moving=["d_stream", "d_offsets", "d_out"],
                      extra=[({"d_stream": ("skew", 16, r)}, f"d_stream at {r} mod 16") for r in (4, 12)] +
                            [({"d_stream": ("skew", 16, r), "d_offsets": "page", "d_out": "page", "d_status": "page"},
                              f"d_stream at {r} mod 16, the others 4096-aligned") for r in (4, 12)]))

    def compress(v):
        lib.initConstantRange()
        lib.garCompressExecutor(v["source"].data_ptr(), n, v["destination"].data_ptr(), 0)
        assert lib.gpuar_hip_last_error() == 0

    def decompress(v):
        lib.initConstantRange()
        lib.garDecompressExecutor(v["source"].data_ptr(), npk * SLOT, v["destination"].data_ptr(), 0)
        assert lib.gpuar_hip_last_error() == 0

    cases.append(Case(f"initConstantRange + garCompressExecutor, {kind}", [Arg("source", n, 16, init=host), Arg("destination", npk * SLOT, 16, want=slots, keep=keep)],
                      compress, lines=in_lines("source") + slot_lines("destination")))
    cases.append(Case(f"initConstantRange + garDecompressExecutor, {kind}", [Arg("source", npk * SLOT, 16, init=slots), Arg("destination", npk * PACKET, 16, want=out_img)],
                      decompress, lines=slot_lines("source") + in_lines("destination")))
    return cases


@pytest.fixture(scope="module")
def codec_cases(H, oracle):
    return {kind: _codec_cases(H, oracle, kind) for kind in ("text", "uniform")}


@pytest.mark.parametrize("kind", ["text", "uniform"])
def test_codec_at_the_weakest_alignment(H, A, codec_cases, kind):
    _part_a(H, A, codec_cases[kind])


@pytest.mark.parametrize("kind", ["text", "uniform"])
def test_codec_across_the_address_line(H, A, codec_cases, kind):
    _part_b(H, A, codec_cases[kind])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the batch codec
# ---------------------------------------------------------------------------------------------------------------------
def _desc_args(k):
    return [Arg("d_ptrs", 8 * k, 8, check=False), Arg("d_bytes", 8 * k, 8, check=False), Arg("d_fp", 8 * (k + 1), 8, check=False)]


def _fill_desc(v, bufs, block, weak=None):
    """Writes batch_sweep's descriptor columns for `bufs` in the block at `block` into the placed descriptor arrays; weak: the
    alignment every buffer pointer must have and no coarser (but for `weak[1]`, the buffer that begins on the line)."""
    ptrs, nbytes, first = BS.columns(bufs, block.data_ptr())
    if weak is not None:
        align, but = weak
        for p in ptrs:
            assert p == 0 or p % (2 * align) == align or p == but, f"buffer pointer {p:#x} is not aligned to {align} and nothing coarser"
    for name, col in (("d_ptrs", ptrs), ("d_bytes", nbytes), ("d_fp", first)):
        _i64(v[name]).copy_(torch.tensor(col, dtype=torch.int64))
        assert v[name].data_ptr() % 8 == 0
    return len(bufs)


def _block_image(offs, datas, total):
    img = np.full(total, CANARY, dtype=np.uint8)
    for o, d in zip(offs, datas):
        img[o:o + d.size] = d
    return img


def _batch_codec_cases(H, oracle):
    order = LS.layouts()["last_wave_1_live"]
    n = order.size                                             # 321 packets: five wavefronts and one live lane
    pkts = [LS.packet(int(i) + 1) for i in order]
    encs, clens = LS.encode_all(oracle, pkts)
    sizes = [p.size for p in pkts]
    slots = np.full((n, SLOT), CANARY, dtype=np.uint8)
    keep = np.zeros((n, SLOT), dtype=bool)
    for i, e in enumerate(encs):
        slots[i, :e.size] = e
        keep[i, :e.size] = True
    stream = np.concatenate(encs)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(clens)
    in_bufs, in_total = BS.scattered_inputs(sizes, n)
    in_offs = [off for off, _n, _k in in_bufs if off is not None]
    in_img = _block_image(in_offs, pkts, in_total)
    # lane 100 (second wavefront) straddles; `a` ends on the line and `b` begins on it
    big = max(range(64, 128), key=lambda i: sizes[i])
    a = next(i for i in range(64, n) if sizes[i] % 32 == 16 and sizes[i] > 256)
    b = next(i for i in range(64, n) if i != a and sizes[i] > 256)
    cases = []
    for join in (None, (a, b)):
        out_offs, out_total = AE.scattered(sizes, n + 1, align=16, gap=16, join=join)
        out_bufs = BS.with_empty([(o, s, 1) for o, s in zip(out_offs, sizes)], np.random.default_rng([SEED, 3]))
        out_img = _block_image(out_offs, pkts, out_total)
        k = len(out_bufs)
        tag = "" if join is None else f", buffer {a} ends where buffer {b} begins"
        on = ("on", out_offs[big] + AE.weak(sizes[big] // 2, 16)) if join is None else ("on", out_offs[b])

        def fill(v, out_bufs=out_bufs, join=join, out_offs=out_offs):
            but = None if join is None else v["outs"].data_ptr() + out_offs[join[1]]
            assert but is None or v["outs"].data_ptr() + out_offs[join[0]] + sizes[join[0]] == but
            return _fill_desc(v, out_bufs, v["outs"], weak=(16, but))

        def decode_batch(v, fill=fill):
            kk = fill(v)
            H.decode_batch(v["d_slots"], _i64(v["d_fp"]), kk, n, _i64(v["d_ptrs"]), _i64(v["d_bytes"]), d_status=_i32(v["d_status"]))

        def decode_stream_batch(v, fill=fill):
            kk = fill(v)
            assert v["d_stream"].data_ptr() % 8 == 4
            H.decode_stream_batch(v["d_stream"], _i64(v["d_offsets"]), _i64(v["d_fp"]), kk, n, _i64(v["d_ptrs"]), _i64(v["d_bytes"]),
                                  d_status=_i32(v["d_status"]))

        outs = lambda: Arg("outs", out_total, 32, want=out_img, block=True)
        cases.append(Case(f"decode_batch, {n} packets of every kind of length{tag}", [Arg("d_slots", n * SLOT, 16, init=slots), outs()] + _desc_args(k) + [_status_arg()],
                          decode_batch, lines=[("outs", on)] + ([("d_slots", ("in", 70 * SLOT + 40)), ("d_slots", ("on", 64 * SLOT))] if join is None else []),
                          moving=["d_slots", "d_ptrs", "d_bytes", "d_fp"] if join is None else []))
        cases.append(Case(f"decode_stream_batch, stream at skew 4{tag}",
                          [Arg("d_stream", stream.size, 4, init=stream), Arg("d_offsets", 8 * (n + 1), 8, init=offs), outs()] + _desc_args(k) + [_status_arg()],
                          decode_stream_batch, lines=[("outs", on)] + ([("d_stream", ("in", int(offs[100]) + 20)), ("d_offsets", ("in", 8 * 70))] if join is None else []),
                          moving=["d_stream", "d_offsets"] if join is None else [], fixed={"d_stream": ("skew", 16, 4)}))
    k_in = len(in_bufs)
    for mode in ("throughput", "latency"):
        def encode_batch(v, mode=mode):
            kk = _fill_desc(v, in_bufs, v["ins"])
            H.encode_batch(_i64(v["d_ptrs"]), _i64(v["d_bytes"]), _i64(v["d_fp"]), kk, n, d_slots=v["d_slots"], d_status=_i32(v["d_status"]), mode=mode)

        cases.append(Case(f"encode_batch {mode}, inputs of batch_sweep.scattered_inputs",
                          [Arg("ins", in_total, 16, init=in_img, block=True), Arg("d_slots", n * SLOT, 16, want=slots, keep=keep)] + _desc_args(k_in) + [_status_arg()],
                          encode_batch, lines=[("ins", ("on", in_offs[big] + AE.weak(sizes[big] // 2, 16))), ("d_slots", ("in", 70 * SLOT + 40))],
                          moving=["d_slots", "d_ptrs"]))
    return cases


@pytest.fixture(scope="module")
def batch_codec_cases(H, oracle):
    return _batch_codec_cases(H, oracle)


def test_batch_codec_at_the_weakest_alignment(H, A, batch_codec_cases):
    """Expects what test_gpu_lengths.py::test_decode_batch_at_every_packet_length expects: every output buffer equals its
    packet, the canaries between the buffers hold, status 0."""
    _part_a(H, A, batch_codec_cases)


def test_batch_codec_across_the_address_line(H, A, batch_codec_cases):
    _part_b(H, A, batch_codec_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 3. CRC-32
# ---------------------------------------------------------------------------------------------------------------------
def _crcs(data):
    return np.array([zlib.crc32(data[p:p + PACKET].tobytes()) for p in range(0, data.size, PACKET)], dtype=np.uint32)


def _crc_cases(H):
    rng = np.random.default_rng([SEED, 4])
    n = 9 * PACKET + 77
    npk = 10
    host = rng.integers(0, 256, n, dtype=np.uint8)
    crcs = _crcs(host)
    bad = host.copy()
    bad[6 * PACKET + 1234] ^= 0x10
    bad[8 * PACKET + 5] ^= 0x01
    minus1 = np.array([-1], dtype=np.int64)
    data_lines = lambda name: [(name, ("in", 4 * PACKET + 100)), (name, ("on", 4 * PACKET))]
    cases = [
        Case("crc32", [Arg("d_in", n, 16, init=host), Arg("d_crc", 4 * npk, 4, want=crcs)],
             lambda v: H.crc32(v["d_in"], n, d_crc=_i32(v["d_crc"])), lines=data_lines("d_in") + [("d_crc", ("in", 20))]),
        Case("verify_crc32 of intact bytes", [Arg("d_out", n, 16, init=host), Arg("d_crc", 4 * npk, 4, init=crcs), Arg("d_first_bad", 8, 8, init=minus1), _status_arg()],
             lambda v: H.verify_crc32(v["d_out"], _i32(v["d_crc"]), n, d_first_bad=_i64(v["d_first_bad"]), d_status=_i32(v["d_status"])),
             lines=data_lines("d_out") + [("d_crc", ("in", 20))]),
        Case("verify_crc32 with packets 6 and 8 damaged", [Arg("d_out", n, 16, init=bad), Arg("d_crc", 4 * npk, 4, init=crcs),
                                                         Arg("d_first_bad", 8, 8, init=minus1, want=np.array([6], np.int64)), _status_arg(H.STATUS_CHECKSUM)],
             lambda v: H.verify_crc32(v["d_out"], _i32(v["d_crc"]), n, d_first_bad=_i64(v["d_first_bad"]), d_status=_i32(v["d_status"])),
             lines=data_lines("d_out")),
    ]
    sizes = [0, 1, PACKET, PACKET + 1, 77, 3 * PACKET + 5, 16, 2 * PACKET + 8176, n]
    datas = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    fp, total_pk = H.batch_packet_count(sizes)
    want = np.concatenate([_crcs(d) for d in datas if d.size])
    assert want.size == total_pk
    for join in (None, (7, 5)):
        offs, total = AE.scattered(sizes, 5, align=16, gap=16, join=join)
        bufs = [(o, s, (s + PACKET - 1) // PACKET) for o, s in zip(offs, sizes)]
        img = _block_image(offs, datas, total)
        tag = "" if join is None else ", one buffer ends where the next begins"
        on = ("on", offs[8] + AE.weak(4 * PACKET + 100, 16)) if join is None else ("on", offs[5])

        def fill(v, bufs=bufs, join=join, offs=offs):
            return _fill_desc(v, bufs, v["block"], weak=(16, None if join is None else v["block"].data_ptr() + offs[join[1]]))

        def crc32_batch(v, fill=fill):
            k = fill(v)
            H.crc32_batch(_i64(v["d_ptrs"]), _i64(v["d_bytes"]), _i64(v["d_fp"]), k, total_pk, d_crc=_i32(v["d_crc"]), d_status=_i32(v["d_status"]))

        def verify_batch(v, fill=fill):
            k = fill(v)
            H.verify_crc32_batch(_i64(v["d_ptrs"]), _i64(v["d_bytes"]), _i64(v["d_fp"]), k, total_pk, _i32(v["d_crc"]),
                                 d_first_bad=_i64(v["d_first_bad"]), d_status=_i32(v["d_status"]))

        moving = ["d_crc", "d_ptrs", "d_bytes", "d_fp"] if join is None else []
        cases.append(Case(f"crc32_batch{tag}", [Arg("block", total, 32, init=img, block=True), Arg("d_crc", 4 * total_pk, 4, want=want)] + _desc_args(len(bufs)) +
                          [_status_arg()], crc32_batch, lines=[("block", on)], moving=moving))
        cases.append(Case(f"verify_crc32_batch{tag}", [Arg("block", total, 32, init=img, block=True), Arg("d_crc", 4 * total_pk, 4, init=want),
                                                       Arg("d_first_bad", 8, 8, init=minus1)] + _desc_args(len(bufs)) + [_status_arg()],
                          verify_batch, lines=[("block", on)], moving=moving + (["d_first_bad"] if join is None else [])))
    return cases


@pytest.fixture(scope="module")
def crc_cases(H):
    return _crc_cases(H)


def test_crc32_at_the_weakest_alignment(H, A, crc_cases):
    _part_a(H, A, crc_cases)


def test_crc32_across_the_address_line(H, A, crc_cases):
    _part_b(H, A, crc_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the filters
# ---------------------------------------------------------------------------------------------------------------------
FILTER_N = 3 * GROUP + 4097 + 5


def _filter_host(H, fam, merge, data, base, w):
    f = getattr(H, ("merge_" if merge else "split_") + fam + "_host")
    out = f(data.tobytes(), base.tobytes(), w) if fam == "xor" else f(data.tobytes(), w)
    return np.frombuffer(out, dtype=np.uint8).copy()


def _filter_call(H, fam, merge, w, n):
    f = getattr(H, ("merge_" if merge else "split_") + fam)
    if fam == "xor":
        return lambda v: f(v["d_in"] if "d_in" in v else v["x"], v["d_base"], w, d_out=v["d_out"] if "d_out" in v else v["x"], n_bytes=n)
    return lambda v: f(v["d_in"] if "d_in" in v else v["x"], w, d_out=v["d_out"] if "d_out" in v else v["x"], n_bytes=n)


def _filter_cases(H, fam):
    rng = np.random.default_rng([SEED, 5, FAMILIES.index(fam)])
    n = FILTER_N
    # sorted integers and noise, half and half: differences with borrows, and bytes no filter predicts
    x = np.cumsum(rng.integers(0, 1 << 20, n // 8 + 1, dtype=np.uint64)).view(np.uint8)[:n].copy()
    x[n // 2:] = rng.integers(0, 256, n - n // 2, dtype=np.uint8)
    base = rng.integers(0, 256, n, dtype=np.uint8)
    lines = lambda name: [(name, ("in", n - 2000)), (name, ("in", GROUP + 30000)), (name, ("on", 2 * GROUP))]
    cases = []
    for w in WIDTHS:
        split = _filter_host(H, fam, False, x, base, w)
        assert np.array_equal(_filter_host(H, fam, True, split, base, w), x)
        for merge in (False, True):
            src, dst = (split, x) if merge else (x, split)
            name = f"{'merge' if merge else 'split'}_{fam}, w = {w}"
            more = [Arg("d_base", n, 16, init=base)] if fam == "xor" else []
            more_lines = lines("d_base") if fam == "xor" else []
            cases.append(Case(name, [Arg("d_in", n, 16, init=src), Arg("d_out", n, 16, want=dst)] + more, _filter_call(H, fam, merge, w, n),
                              lines=lines("d_in") + lines("d_out") + more_lines))
            cases.append(Case(name + " in place", [Arg("x", n, 16, init=src, want=dst)] + more, _filter_call(H, fam, merge, w, n),
                              lines=lines("x") + more_lines))
    return cases


@pytest.fixture(scope="module")
def filter_cases(H):
    return {fam: _filter_cases(H, fam) for fam in FAMILIES}


@pytest.mark.parametrize("fam", FAMILIES)
def test_filters_at_the_weakest_alignment(H, A, filter_cases, fam):
    _part_a(H, A, filter_cases[fam])


@pytest.mark.parametrize("fam", FAMILIES)
def test_filters_across_the_address_line(H, A, filter_cases, fam):
    _part_b(H, A, filter_cases[fam])


# ---------------------------------------------------------------------------------------------------------------------
# 5. estimate and the surveys
# ---------------------------------------------------------------------------------------------------------------------
def _rows_image(rows, npk, stride):
    img = np.full((4, stride), CANARY32, dtype=np.uint32)
    for j, row in enumerate(rows):
        if row is not None:
            img[j, :npk] = row
    return img


def _rows(v, stride):
    return _i32(v["d_est"]).view(4, stride)


def _survey_cases(H):
    rng = np.random.default_rng([SEED, 6])
    n = 2 * GROUP + 3 * PACKET + 4097 + 5
    npk = H.packet_count(n)                                    # 20 packets: two supergroups and a ragged third
    stride = npk + 1
    assert stride % 2 == 1
    x = np.cumsum(rng.integers(0, 1 << 12, n // 4 + 1, dtype=np.uint32), dtype=np.uint32).view(np.uint8)[:n].copy()
    x[GROUP:GROUP + 3 * PACKET] = rng.integers(0, 256, 3 * PACKET, dtype=np.uint8)
    raw = x.tobytes()
    in_lines = [("d_in", ("in", 9 * PACKET + 100)), ("d_in", ("on", GROUP)), ("d_in", ("in", n - 2000))]
    est_lines = [("d_est", ("in", 4 * stride + 40)), ("d_est", ("in", 4 * (2 * stride + 3)))]
    cases = [Case("estimate", [Arg("d_in", n, 16, init=x), Arg("d_est", 4 * npk, 4, want=np.array(H.estimate_host(raw), np.uint32))],
                  lambda v: H.estimate(v["d_in"], n_bytes=n, d_est=_i32(v["d_est"])), lines=in_lines + [("d_est", ("in", 40))]),
             Case("survey_planes, odd stride", [Arg("d_in", n, 16, init=x), Arg("d_est", 16 * stride, 4, want=_rows_image(H.survey_planes_host(raw), npk, stride))],
                  lambda v: H.survey_planes(v["d_in"], d_est=_rows(v, stride), n_bytes=n), lines=in_lines + est_lines)]
    for widths in (WIDTHS, (8,)):
        cases.append(Case(f"survey_delta widths {widths}, odd stride",
                          [Arg("d_in", n, 16, init=x), Arg("d_est", 16 * stride, 4, want=_rows_image(H.survey_delta_host(raw, widths), npk, stride))],
                          lambda v, widths=widths: H.survey_delta(v["d_in"], d_est=_rows(v, stride), n_bytes=n, widths=widths), lines=in_lines + est_lines))
    return cases


@pytest.fixture(scope="module")
def survey_cases(H):
    return _survey_cases(H)


def test_estimate_and_surveys_at_the_weakest_alignment(H, A, survey_cases):
    _part_a(H, A, survey_cases)


def test_estimate_and_surveys_across_the_address_line(H, A, survey_cases):
    _part_b(H, A, survey_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 6. move_packets   7. generate and copy
# ---------------------------------------------------------------------------------------------------------------------
def _move_cases(H):
    rng = np.random.default_rng([SEED, 7])
    sizes = [1, 15, 16, 17, PACKET - 1, PACKET]
    datas = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    src_offs, src_total = AE.scattered(sizes, 8, align=16, gap=16)
    dst_offs, dst_total = AE.scattered(sizes, 9, align=16, gap=16)
    k = len(sizes)

    def move(v):
        src, dst = [v["src"].data_ptr() + o for o in src_offs], [v["dst"].data_ptr() + o for o in dst_offs]
        assert all(p % 32 == 16 for p in src + dst)
        for name, col in (("d_src_ptrs", src), ("d_dst_ptrs", dst), ("d_bytes", sizes)):
            _i64(v[name]).copy_(torch.tensor(col, dtype=torch.int64))
        H.move_packets(_i64(v["d_src_ptrs"]), _i64(v["d_dst_ptrs"]), _i64(v["d_bytes"]), k, d_status=_i32(v["d_status"]))

    args = [Arg("src", src_total, 32, init=_block_image(src_offs, datas, src_total), block=True),
            Arg("dst", dst_total, 32, want=_block_image(dst_offs, datas, dst_total), block=True),
            Arg("d_src_ptrs", 8 * k, 8, check=False), Arg("d_dst_ptrs", 8 * k, 8, check=False), Arg("d_bytes", 8 * k, 8, check=False), _status_arg()]
    lines = [(name, ("on", offs[r] + at)) for name, offs in (("src", src_offs), ("dst", dst_offs)) for r, at in ((4, 4112), (5, 16), (3, 16))]
    return [Case("move_packets, regions of 1, 15, 16, 17, 8191 and 8192 bytes", args, move, lines=lines,
                 moving=["d_src_ptrs", "d_dst_ptrs", "d_bytes", "d_status"])]


def _generate_cases(H):
    n = 3 * PACKET + 77
    n16 = 3 * PACKET + 48
    rng = np.random.default_rng([SEED, 10])
    cases = []
    for kind in ("uniform", "zipf", "text"):
        want = synth.generate(kind, 21, n, offset=8000)
        cases.append(Case(f"generate {kind}", [Arg("d_out", n, 8, want=want)],
                          lambda v, kind=kind: H.generate(kind, 21, n, offset=8000, out=v["d_out"]), lines=[("d_out", ("in", 10000)), ("d_out", ("in", n - 30))]))

        def refused(v, kind=kind):
            with pytest.raises(H.GpuarError, match=r"code -1\)"):
                H.generate(kind, 21, n, offset=8000, out=v["d_out"])

        cases.append(Case(f"generate {kind} into a destination that is not 8-byte aligned: GPUAR_ERR_ALIGNMENT, nothing written",
                          [Arg("d_out", n, 1)], refused, moving=[],
                          extra=[({"d_out": ("skew", 8, r)}, f"d_out at {r} mod 8") for r in (1, 4)]))
    data = rng.integers(0, 256, n16, dtype=np.uint8)
    cases.append(Case("gpuar_hip_copy", [Arg("d_src", n16, 16, init=data), Arg("d_dst", n16, 16, want=data)],
                      lambda v: H.device_copy(v["d_src"], v["d_dst"], n16), lines=[("d_src", ("in", 10000)), ("d_dst", ("in", 2 * PACKET + 16))]))
    return cases


@pytest.fixture(scope="module")
def small_cases(H):
    return _move_cases(H) + _generate_cases(H)


def test_move_generate_copy_at_the_weakest_alignment(H, A, small_cases):
    _part_a(H, A, small_cases)


def test_move_generate_copy_across_the_address_line(H, A, small_cases):
    _part_b(H, A, small_cases)


# ---------------------------------------------------------------------------------------------------------------------
# C. offsets past 2^32 inside one buffer
# ---------------------------------------------------------------------------------------------------------------------
TAIL = BIG % GROUP                                           # 4102 bytes behind the last whole group of w = 8
WINDOWS = ((0, 2 * GROUP), (AE.LINE - 2 * GROUP, AE.LINE + 2 * GROUP), (BIG - TAIL - GROUP, BIG))
CHUNK = 256 * MiB


def _equal_big(a, b):
    """a == b for two byte tensors of one size, 256 MiB at a time (torch.equal would allocate a mask as large as they are)."""
    assert a.numel() == b.numel()
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    for at in range(0, a.numel(), CHUNK):
        ok = ok & a[at:at + CHUNK].eq(b[at:at + CHUNK]).all()
    return bool(ok.item())


def _alloc_big():
    t = torch.empty(BIG + 4096, dtype=torch.uint8, device="cuda")
    t[BIG:].fill_(CANARY)
    return t


def _windows_of(t):
    return [t[a:b].cpu().numpy() for a, b in WINDOWS]


def _canary_holds(t):
    return bool(t[BIG:].eq(CANARY).all().item())


@pytest.fixture(scope="module")
def big(H, A):
    """Part C's buffer: synth text generated on the device, the three windows overwritten with sorted little-endian 64-bit
    integers (a seeded random walk: every byte of the differences varies and borrows); freed when the module ends."""
    x = _alloc_big()
    H.generate("text", 31, BIG, out=x)
    rng = np.random.default_rng([SEED, 11])
    for a, b in WINDOWS:
        k = (b - a) // 8
        walk = np.cumsum(rng.integers(0, 1 << 40, k, dtype=np.uint64), dtype=np.uint64) + np.uint64(0x0123456789ABCDEF)
        x[a:a + 8 * k].copy_(_u8(walk))
    torch.cuda.synchronize()
    state = {"x": x, "wins": _windows_of(x)}
    assert state["wins"][1].size == 4 * GROUP and WINDOWS[1][0] % GROUP == 0 and WINDOWS[2][0] % GROUP == 0
    yield state
    state.clear()
    del x
    torch.cuda.empty_cache()


def _check_windows(got, want, what):
    for (a, b), g, w in zip(WINDOWS, got, want):
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            pytest.fail(f"{what}: the window [{a}, {b}) differs from the host function first at byte {a + at} of the buffer (byte {at} of the window)")


@pytest.mark.parametrize("fam,w", [("planes", 8), ("planes", 2), ("delta", 8)])
def test_filters_past_4gib(H, big, fam, w):
    x, wins = big["x"], big["wins"]
    y = _alloc_big()
    getattr(H, "split_" + fam)(x, w, d_out=y, n_bytes=BIG)
    host = getattr(H, f"split_{fam}_host")
    _check_windows(_windows_of(y), [np.frombuffer(host(win.tobytes(), w), dtype=np.uint8) for win in wins], f"split_{fam} w = {w} of {BIG} bytes")
    getattr(H, "merge_" + fam)(y, w, d_out=y, n_bytes=BIG)
    assert _equal_big(y[:BIG], x[:BIG]), f"merge_{fam}(split_{fam}(x)) w = {w} in place is not x over the whole buffer"
    assert _canary_holds(x) and _canary_holds(y), "written behind byte n"
    assert _windows_of(x)[1].tobytes() == wins[1].tobytes(), "the input changed"
    assert H.status() == 0
    del y


def _packet_ranges():
    return [(a // PACKET, (b + PACKET - 1) // PACKET) for a, b in WINDOWS]


def test_crc32_past_4gib(H, A, big):
    x, wins = big["x"], big["wins"]
    npk = H.packet_count(BIG)
    assert npk == 524288 + 25
    A.reset()
    d_crc, first_bad, word = _i32(A.put(4 * npk, 4)), _i64(A.put(8, 8)), _i32(A.put(4, 4))
    H.crc32(x, BIG, d_crc=d_crc)
    got = d_crc.cpu().numpy().view(np.uint32)
    for (a, b), win in zip(_packet_ranges(), wins):
        assert np.array_equal(got[a:b], _crcs(win)), f"crc32 of {BIG} bytes: packets {a}..{b - 1} differ from zlib.crc32"
    for flip, want_word, want_bad in ((True, H.STATUS_CHECKSUM, 524288), (False, 0, -1)):
        if flip:
            x[AE.LINE + 5] ^= 0x40
        first_bad.fill_(-1)
        word.zero_()
        H.verify_crc32(x, d_crc, BIG, d_first_bad=first_bad, d_status=word)
        if flip:
            x[AE.LINE + 5] ^= 0x40
        assert (int(word.item()), int(first_bad.item())) == (want_word, want_bad), \
            f"verify_crc32 of {BIG} bytes{' with byte 2^32 + 5 flipped' if flip else ''}: status {int(word.item()):#x}, first_bad {int(first_bad.item())}"
    _fail_on([A.guards("crc32 / verify_crc32 past 4 GiB")])
    assert _windows_of(x)[1].tobytes() == wins[1].tobytes()
    assert H.status() == 0


def test_estimate_and_surveys_past_4gib(H, A, big):
    x, wins = big["x"], big["wins"]
    npk = H.packet_count(BIG)
    stride = npk + 2                                           # odd
    A.reset()
    d_est = _i32(A.put(4 * npk, 4))
    rows = {name: _i32(A.put(16 * stride, 4)).view(4, stride) for name in ("survey_planes", "survey_delta")}
    H.estimate(x, n_bytes=BIG, d_est=d_est)
    H.survey_planes(x, d_est=rows["survey_planes"], n_bytes=BIG)
    H.survey_delta(x, d_est=rows["survey_delta"], n_bytes=BIG)
    got = d_est.cpu().numpy()
    got_rows = {name: r.cpu().numpy() for name, r in rows.items()}
    for (a, b), win in zip(_packet_ranges(), wins):
        raw = win.tobytes()
        assert got[a:b].tolist() == H.estimate_host(raw), f"estimate of {BIG} bytes: packets {a}..{b - 1} differ from estimate_host"
        for name, host in (("survey_planes", H.survey_planes_host), ("survey_delta", H.survey_delta_host)):
            for j, want in enumerate(host(raw)):
                assert got_rows[name][j, a:b].tolist() == want, f"{name} of {BIG} bytes: row {j}, packets {a}..{b - 1} differ from {name}_host"
    for name in rows:
        assert (got_rows[name][:, npk:] == np.int32(CANARY32 - (1 << 32))).all(), f"{name}: written into the stride gap"
    _fail_on([A.guards("estimate and surveys past 4 GiB")])
    assert _canary_holds(x)
    assert H.status() == 0


def test_xor_in_place_past_4gib(H, big):
    x, wins = big["x"], big["wins"]
    base = _alloc_big()
    H.generate("uniform", 32, BIG, out=base)
    base_wins = _windows_of(base)
    H.split_xor(x, base, 8, d_out=x, n_bytes=BIG)
    _check_windows(_windows_of(x), [np.frombuffer(H.split_xor_host(win.tobytes(), bw.tobytes(), 8), dtype=np.uint8) for win, bw in zip(wins, base_wins)],
                   f"split_xor w = 8 in place of {BIG} bytes")
    H.merge_xor(x, base, 8, d_out=x, n_bytes=BIG)
    torch.cuda.synchronize()
    _check_windows(_windows_of(base), base_wins, "the base after split_xor and merge_xor")
    assert _canary_holds(base)
    del base
    torch.cuda.empty_cache()
    # the whole buffer against a second generation of it
    y = _alloc_big()
    H.generate("text", 31, BIG, out=y)
    for (a, b), win in zip(WINDOWS, wins):
        k = (b - a) // 8 * 8
        y[a:a + k].copy_(_u8(win[:k]))
    assert _equal_big(x[:BIG], y[:BIG]), "merge_xor(split_xor(x)) w = 8 in place is not x over the whole buffer"
    assert _canary_holds(x), "written behind byte n"
    assert H.status() == 0
    del y
