"""Where the buffers lie and how far into a buffer a kernel works: every entry point of include/gpuar_hip.h and of
include/gpuar_hip_gip.h at the weakest pointer alignment its contract allows, with the address line 2^32 (where a pointer's low
word carries into its high word) inside each of its buffers in turn, and -- the filter, CRC, estimate, survey, scan and kinds
kernels and move_bytes -- at offsets past 2^32 inside one buffer; and the kernels that keep 8192 wavefronts resident on three
packets per wavefront.
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
   bytes), estimate and both surveys (d_est 4-weak, odd stride P + 1, mask 15 and the single width 8), the XOR survey (the same
   20 packets against a base that equals them but for the first half of every third half-packet; d_in and d_base 16-weak, d_est
   and d_scan each 4-weak at the odd stride; both outputs, the est rows alone, the scan rows alone, the output that was not asked
   for keeping every canary; expected from survey_xor_host) and its batch form (buffers of 65536 + 8192 + 1, 3 * 8192 + 77, 17,
   0 and 65536 bytes, the second and the fourth with base pointer 0, buffers and bases in two blocks in different permuted
   address orders, 16-weak and not packet-aligned, the four descriptor arrays 8- but not 16-aligned), move_packets (1, 15, 16,
   17, 8191, 8192 bytes), generate and gpuar_hip_copy.  generate's d_out must be 8-byte aligned (its kernels store 8 bytes at a
   time): at offsets 1 and 4 it returns GPUAR_ERR_ALIGNMENT and writes nothing, which the header now says.
   The packet forms (sections 8 - 12; each section's docstring names the fault class it would catch): sparse_scan (9 packets +
   77 bytes: zeros, exceptions at bytes 0, 127, 128 and n - 1, count(f) at n / 2 and n / 2 + 1, uniform, text, 128 exceptions in
   one lane, one in every lane, a short last packet; d_scan 4-weak) and sparse_scan_batch (buffers 16-weak and not packet-aligned,
   descriptors as for the batch CRC); sparse_pack / sparse_unpack (regions of 1, 2, 3, 15, 16, 17, 129, 8191 and 8192 bytes with
   k = 0, 1, 64 over every lane, 128 in one lane and the largest k a small n allows; packets at 16 mod 32, the records back to
   back from an address that is 4 mod 8 with canaries only behind the last, expected from sparse_pack_host and
   sparse_unpack_host); kinds_store (stored on / off x d_scan given / NULL over raw, sparse and coded packets and a short last
   one of each non-coded kind; slots of canaries behind a made-up header, d_kind byte-weak); kinds_expand (a stream built from
   kinds_store_host's packets between kind-0 packets of odd lengths, raw and sparse packets starting at every residue mod 16,
   the stream byte-weak and at 1 and 15 mod 16); move_bytes (regions of 0, 1, 15, 16, 17, 31, 33, 4097 and 8704 bytes, sources
   at mixed residues, destinations back to back at byte grain, the blocks at five more residue pairs).
B. The same shapes and references with the line inside one pointer argument at a time, the others weak elsewhere: in the
   middle of a packet of the second wavefront group, inside a slot's coded bytes, inside the compacted stream, the offsets
   array, a survey's rows, a filter's tail, the XOR base; for the XOR survey inside a lane's 128-byte piece of a full
   supergroup, on a supergroup boundary and in the ragged tail of the base and of the buffer, in row 0 and on the word of the
   stride gap of the est rows and of the scan rows, inside the array of base pointers; and with a packet / slot / group boundary exactly on the line.  (A
   boundary on the line makes the start a multiple of the unit, 8192 or 512 bytes for slots: those placements cannot be weak
   as well and assert the boundary instead.)  Batch calls: one buffer straddles; in a second layout one buffer ends exactly
   at the line and the next begins at it (the XOR survey's batch: one BASE straddles, and one base ends at the line where the
   next begins; a base that ends on the line is a multiple of 16 bytes long, here 65536).  The packet forms: the line inside a record's pos[], exactly between pos[] and
   val[], on a record's start; inside a raw slot's body, a sparse record in a slot, on a slot boundary; in a stream inside a raw
   body, inside a sparse record and two bytes into a packet's header; inside d_kind, d_scan, d_offsets; and for move_bytes where
   a destination's head bytes end, inside its body, where its tail bytes begin, at its first byte and one byte behind its
   last, and the same for a source (the line is a multiple of 16: inside a destination it is always a quad boundary).
C. One buffer of 2^32 + 3 * 65536 + 4097 + 5 bytes (packet 524288 starts at byte 2^32), generated on the device, three
   windows overwritten with sorted 64-bit integers (so the delta filter's borrows run through every byte): split / merge of
   planes (w = 8, 2), delta (w = 8) and xor (w = 8, in place, against a base of the same size that is freed right after), crc32
   and verify_crc32 with one byte flipped at 2^32 + 5 (first_bad = 524288), estimate and both surveys.  Compared against the
   *_host functions on three windows ([0, 128 KiB), 128 KiB either side of 2^32, the last group with the tail); over the
   whole buffer merge(split(x)) == x and the canary behind n holds.  The codec is not repeated (the 5 GiB tests cover it).
   The packet forms: a second buffer of the same size of UNIFORM bytes (every whole packet raw) with four windows of 16 mixed
   packets -- at packet 0, at packet 493 448 where the slot offset r * 8704 passes 2^32, at packet 524 288 where r * 8192 does,
   and the last 16 with the short last packet -- through estimate, sparse_scan, kinds_store, compact and kinds_expand on one
   stream: the windows against the host twins, every scan word, kind, slot and output packet of the whole buffer on the
   device, the stream longer than 2^32 (asserted; at most 200 packets are not raw) and the packet that holds stream byte 2^32
   by itself.  move_bytes: one launch of 4096 regions from behind offset 2^32 of the first buffer to back-to-back destinations
   across offset 2^32 of another allocation, every residue pair, against numpy.
D. 3 * 8192 + 5 packets: sparse_scan, kinds_store and kinds_expand keep 8192 wavefronts resident, so each takes three packets
   (five take four) and kinds_expand builds them in the same 8 KiB of LDS: sparse, raw, coded and DAMAGED packets in orders
   chosen so that what one leaves behind would show in the next; BAD_PACKET / BAD_BATCH exactly when a defect is present.

Time, pytest --durations=0 on an MI355X, the module alone: 42 passed in 4.0 s (625 placed launches in parts A and B for the
older entry points, 151 for the packet forms, 59 for the XOR survey).
    0.49 s  setup of test_codec_at_the_weakest_alignment[text] (the arena, the reference encoder on 2 x 1 MiB)
    0.46 s  test_kinds_pipeline_past_4gib (4 GiB generated, 4.25 GiB of slots filled, five launches, four passes of comparisons)
    0.32 s  test_codec_at_the_weakest_alignment[text] (the first launches of the process)
    0.10 s  setup of test_batch_codec_at_the_weakest_alignment (321 reference packets)
    0.07 s  test_kinds_expand_second_trip[damaged], test_codec_across_the_address_line[text], [uniform]
    0.05 s  test_codec_at_the_weakest_alignment[uniform]
    0.04 s  test_xor_in_place_past_4gib, test_batch_codec_at_the_weakest_alignment
    0.03 s  test_batch_codec_across_the_address_line, test_filters_past_4gib[delta-8]
    0.02 s  test_filters_past_4gib[planes-8], test_kinds_expand_second_trip[intact], test_filters_across_the_address_line[xor],
            test_move_bytes_past_4gib
    0.01 s  test_xor_survey_at_the_weakest_alignment (24 placed launches), test_xor_survey_across_the_address_line (35; their
            setup, the host twin on six buffers, is under 0.005 s),
            the tests of sections 9 - 11, test_filters_past_4gib[planes-2], test_estimate_and_surveys_past_4gib,
            test_crc32_at_the_weakest_alignment, the other filter tests; every remaining test and setup is under 0.005 s
            (test_sparse_scan_and_kinds_store_second_trip, the scan and move_bytes sections among them).
No shape had to shrink: no case comes near 5 s.  Memory: 4.1 GiB for the arena; on top of it at most 8.5 GiB during the filter
tests of part C (its buffer and one more of that size) and, by the sizes allocated, 16.3 GiB during the kinds pipeline (part
C's buffer, which the module keeps, 4.0 GiB of uniform bytes, 4.25 GiB of slots and 4.0 GiB of stream; the slots are freed
before the 4.0 GiB output is made), 8.0 GiB during test_move_bytes_past_4gib and 4.9 GiB in part D.  Fixed seeds throughout.
"""
import struct
import zlib

import numpy as np
import pytest

import address_edges as AE
import batch_sweep as BS
import kinds_ref as K
import length_sweep as LS
import sparse_ref as S
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


def _rows(v, stride, name="d_est"):
    return _i32(v[name]).view(4, stride)


def _survey_input(H):
    """(n, packets, row stride, bytes): the section's one-buffer input"""
    rng = np.random.default_rng([SEED, 6])
    n = 2 * GROUP + 3 * PACKET + 4097 + 5
    npk = H.packet_count(n)                                    # 20 packets: two supergroups and a ragged third
    stride = npk + 1
    assert stride % 2 == 1
    x = np.cumsum(rng.integers(0, 1 << 12, n // 4 + 1, dtype=np.uint32), dtype=np.uint32).view(np.uint8)[:n].copy()
    x[GROUP:GROUP + 3 * PACKET] = rng.integers(0, 256, 3 * PACKET, dtype=np.uint8)
    return n, npk, stride, x


def _survey_cases(H):
    n, npk, stride, x = _survey_input(H)
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


def _survey_base(x, seed):
    """tests/test_gpu_xor_survey.py::_base_of: independent uniform bytes in the first half of every third half-packet, x elsewhere,
    so that full and short supergroups each hold packets whose XOR is all zeros, half zeros and neither"""
    b = x.copy()
    pick = (np.arange(x.size) // (PACKET // 2)) % 3 == 0
    b[pick] = np.random.default_rng([SEED, seed]).integers(0, 256, x.size, dtype=np.uint8)[pick]
    return b


def _joined_bases(sizes, seed, a, b):
    """AE.scattered, but bases a and b stand behind the others, b exactly where a ends.  sizes[a] is a multiple of 32 (a base that
    ends on the line and is 16-byte aligned has no other length here), so neither start is weak: a's is a multiple of 32, and the
    caller puts b's on the line."""
    assert sizes[a] and sizes[a] % 32 == 0 and sizes[b]
    offs, total = AE.scattered(sizes, seed, align=16, gap=16)
    offs[a] = (total + 31) // 32 * 32 + 32
    offs[b] = offs[a] + sizes[a]
    return offs, AE.weak(offs[b] + sizes[b] + 16, 16) + 16


def _xor_survey_cases(H):
    """The XOR survey is the first survey that reads two inputs in step, has a second output and, in a batch, an array of base
    pointers in which 0 is a value.  Would catch: the base's address formed from the buffer's high word or in 32 bits (the line
    inside a lane's 128-byte piece of the base, on a supergroup boundary of it, in its ragged tail -- and the same for the buffer
    while the base lies elsewhere), a store to the scan rows through the est rows' pointer or stride (each output 4-weak on its
    own, the line in row 0 and in the stride gap of each), a store to an output that was not asked for (it keeps every canary),
    a 16-byte load of a base that is only 16-aligned taken wider, a batch base located from a pointer read as two halves or from
    a 16-byte load of the 8-aligned pointer array (the line inside that array, a base that straddles the line, one that ends on it
    and the next that begins there), and a base pointer of 0 dereferenced."""
    n, npk, stride, x = _survey_input(H)
    base = _survey_base(x, 16)
    est, scan = H.survey_xor_host(x.tobytes(), base.tobytes())
    # packets that equal their base (scan word 0), that differ from it in half their bytes and, at the wider widths, in other
    # shares: in the full supergroups and in the ragged one
    for lo, hi in ((0, 16), (16, npk)):
        assert 0 in scan[0][lo:hi] and any(v >> 8 > 4000 for v in scan[0][lo:hi]) and len({tuple(r[p] for r in scan) for p in range(lo, hi)}) >= 3
    est_img, scan_img = _rows_image(est, npk, stride), _rows_image(scan, npk, stride)
    lane = GROUP + 3 * PACKET + 37 * 128 + 48                  # inside lane 37's piece of packet 3 of the second supergroup
    data_lines = lambda name: [(name, ("in", lane)), (name, ("on", GROUP)), (name, ("in", n - 2000))]
    row_lines = lambda name: [(name, ("in", 40)), (name, ("in", 4 * (stride + npk)))]         # in row 0; on the gap word behind row 1
    cases = []
    for tag, want_est, want_scan in (("both outputs", True, True), ("the est rows alone", True, False), ("the scan rows alone", False, True)):
        def call(v, want_est=want_est, want_scan=want_scan):
            got = H.survey_xor(v["d_in"], v["d_base"], d_est=_rows(v, stride) if want_est else False,
                               d_scan=_rows(v, stride, "d_scan") if want_scan else False, n_bytes=n)
            assert (got[0] is None) == (not want_est) and (got[1] is None) == (not want_scan)

        args = [Arg("d_in", n, 16, init=x), Arg("d_base", n, 16, init=base), Arg("d_est", 16 * stride, 4, want=est_img if want_est else None),
                Arg("d_scan", 16 * stride, 4, want=scan_img if want_scan else None)]
        cases.append(Case(f"survey_xor, {tag}, odd stride", args, call,
                          lines=data_lines("d_base") + data_lines("d_in") + row_lines("d_est") + row_lines("d_scan")))
    # the batch form: five buffers and their bases in two blocks, each in its own permuted address order
    sizes = [GROUP + PACKET + 1, 3 * PACKET + 77, 17, 0, GROUP]
    based = [True, False, True, False, True]
    rng = np.random.default_rng([SEED, 17])
    datas = [np.cumsum(rng.integers(0, 1 << 12, s // 4 + 1, dtype=np.uint32), dtype=np.uint32).view(np.uint8)[:s].copy() for s in sizes]
    bases = [_survey_base(d, 18 + b) for b, d in enumerate(datas)]
    fp, total_pk = H.batch_packet_count(sizes)
    bstride = total_pk + 2
    assert total_pk == 23 and bstride % 2 == 1
    rows = [[[], [], [], []], [[], [], [], []]]
    for d, q, on in zip(datas, bases, based):
        got = H.survey_xor_host(d.tobytes(), (q if on else np.zeros_like(d)).tobytes())                 # (no base: against zeros)
        for which in (0, 1):
            for j in range(4):
                rows[which][j] += got[which][j]
    best_img, bscan_img = _rows_image(rows[0], total_pk, bstride), _rows_image(rows[1], total_pk, bstride)
    offs, total = AE.scattered(sizes, 21, align=16, gap=16)
    img = _block_image(offs, datas, total)
    for join in (None, (4, 0)):
        boffs, btotal = AE.scattered(sizes, 22, align=16, gap=16) if join is None else _joined_bases(sizes, 22, *join)
        bimg = _block_image(boffs, [q if on else q[:0] for q, on in zip(bases, based)], btotal)      # (a base that is not used is not there)
        tag = ", base 0 straddles" if join is None else f", base {join[0]} ends where base {join[1]} begins"
        inside = AE.weak(3 * PACKET + 37 * 128 + 40, 16)       # inside a lane's piece of the first supergroup of buffer 0 / base 0
        on = ("on", boffs[0] + inside) if join is None else ("on", boffs[0])

        def call(v, boffs=boffs, join=join):
            ptrs = [v["block"].data_ptr() + o if s else 0 for o, s in zip(offs, sizes)]
            bptrs = [v["bases"].data_ptr() + o if f and s else 0 for o, s, f in zip(boffs, sizes, based)]
            assert all(p == 0 or (p % 32 == 16 and p % PACKET) for p in ptrs), "a buffer is not 16-weak, or is packet-aligned"
            strong = [] if join is None else [bptrs[i] for i in join]
            assert all(p == 0 or p % 32 == 16 or p in strong for p in bptrs), "a base is not 16-weak"
            assert join is None or bptrs[join[0]] + sizes[join[0]] == bptrs[join[1]]
            _put(v, d_ptrs=ptrs, d_bytes=sizes, d_fp=fp, d_base_ptrs=bptrs)
            H.survey_xor_batch(_i64(v["d_ptrs"]), _i64(v["d_bytes"]), _i64(v["d_fp"]), _i64(v["d_base_ptrs"]), len(sizes), total_pk,
                               d_est=_rows(v, bstride), d_scan=_rows(v, bstride, "d_scan"), d_status=_i32(v["d_status"]))

        args = [Arg("block", total, 32, init=img, block=True), Arg("bases", btotal, 32, init=bimg, block=True),
                Arg("d_est", 16 * bstride, 4, want=best_img), Arg("d_scan", 16 * bstride, 4, want=bscan_img)] + _desc_args(len(sizes)) + \
               [Arg("d_base_ptrs", 8 * len(sizes), 8, check=False), _status_arg()]
        cases.append(Case(f"survey_xor_batch{tag}", args, call,
                          lines=[("bases", on), ("d_base_ptrs", ("in", 24))] + ([("block", ("on", offs[0] + inside))] if join is None else []),
                          moving=["d_est", "d_scan", "d_ptrs", "d_bytes", "d_fp", "d_base_ptrs", "d_status"] if join is None else []))
    return cases


@pytest.fixture(scope="module")
def xor_survey_cases(H):
    return _xor_survey_cases(H)


def test_xor_survey_at_the_weakest_alignment(H, A, xor_survey_cases):
    _part_a(H, A, xor_survey_cases)


def test_xor_survey_across_the_address_line(H, A, xor_survey_cases):
    _part_b(H, A, xor_survey_cases)


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
# 8. sparse_scan and sparse_scan_batch
# ---------------------------------------------------------------------------------------------------------------------
FORMS_N = 9 * PACKET + 77
FORMS_NPK = 10


_filled = S._packet                                          # (n, fill, where): n bytes of `fill` with exceptions at `where`, none of them the fill


def _every_lane(n):
    """One position in each 128-byte lane of a packet of n bytes."""
    lanes = np.arange((n + 127) // 128)
    at = lanes * 128 + (lanes * 37) % 128
    return at[at < n]


def _form_packets(rng, last):
    """Nine whole packets -- zeros; fill 0x80 with exceptions at bytes 0, 127, 128 and n - 1; count(f) exactly n / 2 (no majority)
    and n / 2 + 1; uniform; text; 128 exceptions in one lane; one in every lane; 100 spread out -- and `last`, the short one."""
    return [np.zeros(PACKET, dtype=np.uint8), _filled(PACKET, 0x80, [0, 127, 128, PACKET - 1]),
            _filled(PACKET, 0x00, np.arange(PACKET // 2) * 2), _filled(PACKET, 0xFF, np.arange(PACKET // 2 - 1) * 2 + 1),
            rng.integers(0, 256, PACKET, dtype=np.uint8), np.frombuffer(K.TEXT[:PACKET], dtype=np.uint8).copy(),
            _filled(PACKET, 0xFF, np.arange(128) + 3 * 128), _filled(PACKET, 0x80, _every_lane(PACKET)),
            _filled(PACKET, 0x00, np.arange(100) * 81 + 7), last]


def _put(v, **columns):
    """Writes 64-bit descriptor columns into the placed arrays of the same names."""
    for name, col in columns.items():
        assert v[name].data_ptr() % 8 == 0
        _i64(v[name]).copy_(torch.tensor([int(c) for c in col], dtype=torch.int64))


def _scan_cases(H):
    """Would catch: a packet address formed in 32 bits or from the wrong base (the line inside a packet and on a packet
    boundary), a d_scan store wider than its word (d_scan 4-weak, the canary behind d_scan[npk]), a short last packet's bytes
    past its end counted, a batch buffer located from a pointer read as two halves (buffers ending and beginning on the line)."""
    rng = np.random.default_rng([SEED, 12])
    n, npk = FORMS_N, FORMS_NPK
    pkts = _form_packets(rng, _filled(77, 0x80, [0, 76]))
    host = np.concatenate(pkts)
    assert host.size == n
    want = np.array(H.sparse_scan_host(host.tobytes()), dtype=np.uint32)
    assert want.tolist() == [S.scan(x) for x in pkts] and want[2] == S.NONE and want[3] == ((PACKET // 2 - 1) << 8 | 0xFF) and want[4] == S.NONE
    cases = [Case("sparse_scan", [Arg("d_in", n, 16, init=host), Arg("d_scan", 4 * npk, 4, want=want)],
                  lambda v: H.sparse_scan(v["d_in"], n_bytes=n, d_scan=_i32(v["d_scan"])),
                  lines=[("d_in", ("in", 4 * PACKET + 100)), ("d_in", ("on", 4 * PACKET)), ("d_in", ("in", n - 40)), ("d_scan", ("in", 20))])]
    sizes = [0, 1, PACKET, PACKET + 1, 77, 3 * PACKET + 5, 16, 2 * PACKET + 8176, n]
    datas = [np.concatenate([pkts[(b + j) % 9] for j in range(s // PACKET + 1)])[:s] for b, s in enumerate(sizes)]
    fp, total_pk = H.batch_packet_count(sizes)
    want = np.concatenate([np.array(H.sparse_scan_host(d.tobytes()), dtype=np.uint32) for d in datas if d.size])
    assert want.size == total_pk
    for join in (None, (7, 5)):
        offs, total = AE.scattered(sizes, 15, align=16, gap=16, join=join)
        bufs = [(o, s, (s + PACKET - 1) // PACKET) for o, s in zip(offs, sizes)]
        img = _block_image(offs, datas, total)
        tag = "" if join is None else ", one buffer ends where the next begins"
        on = ("on", offs[8] + AE.weak(4 * PACKET + 100, 16)) if join is None else ("on", offs[5])

        def scan_batch(v, bufs=bufs, join=join, offs=offs):
            k = _fill_desc(v, bufs, v["block"], weak=(16, None if join is None else v["block"].data_ptr() + offs[join[1]]))
            assert join is not None or all(p % PACKET for p in BS.columns(bufs, v["block"].data_ptr())[0]), "a buffer is packet-aligned"
            H.sparse_scan_batch(_i64(v["d_ptrs"]), _i64(v["d_bytes"]), _i64(v["d_fp"]), k, total_pk, d_scan=_i32(v["d_scan"]), d_status=_i32(v["d_status"]))

        cases.append(Case(f"sparse_scan_batch{tag}", [Arg("block", total, 32, init=img, block=True), Arg("d_scan", 4 * total_pk, 4, want=want)] +
                          _desc_args(len(bufs)) + [_status_arg()], scan_batch, lines=[("block", on)],
                          moving=["d_scan", "d_ptrs", "d_bytes", "d_fp"] if join is None else []))
    return cases


@pytest.fixture(scope="module")
def scan_cases(H):
    return _scan_cases(H)


def test_sparse_scan_at_the_weakest_alignment(H, A, scan_cases):
    _part_a(H, A, scan_cases)


def test_sparse_scan_across_the_address_line(H, A, scan_cases):
    _part_b(H, A, scan_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 9. sparse_pack and sparse_unpack
# ---------------------------------------------------------------------------------------------------------------------
def _record_cases(H):
    """Packets at ptr % 32 == 16; their records back to back at 4-byte grain in one buffer that starts at ptr % 8 == 4 (a
    record's length is 4 or 0 mod 8, so the starts take both residues: asserted), canaries only behind the last: a pad that is
    a byte too long lands in the next record's head and shows.  Would catch: pos[] stored as dwords or val[] through pos's
    pointer type (2-byte and 1-byte stores at an address that is only 4-aligned), rec + 4 + 2 k formed in 32 bits (the line
    inside pos[], exactly between pos[] and val[], a record starting on it), descriptor arrays or d_scan read 16 bytes at a time."""
    regions = [(1, 0x00, []), (2, 0x80, []), (3, 0xFF, [1]), (15, 0x00, np.arange(7) * 2), (16, 0x80, [15]), (17, 0xFF, np.arange(8) * 2 + 1),
               (129, 0x00, [0, 127, 128]), (129, 0x80, np.arange(64) * 2), (8191, 0xFF, _every_lane(8191)), (PACKET, 0x00, np.arange(128) + 3 * 128),
               (PACKET, 0x80, []), (PACKET, 0xFF, [PACKET - 1]), (8191, 0x00, [0]), (PACKET, 0x80, _every_lane(PACKET))]
    pkts = [_filled(*r) for r in regions]
    sizes = [x.size for x in pkts]
    k = len(pkts)
    scans = [S.scan(x) for x in pkts]
    assert [s >> 8 for s in scans] == [0, 0, 1, 7, 1, 8, 3, 64, 64, 128, 0, 1, 1, 64] and all(2 * (s >> 8) < n for s, n in zip(scans, sizes))
    assert sorted(set(sizes)) == [1, 2, 3, 15, 16, 17, 129, 8191, 8192]
    recs = [np.frombuffer(H.sparse_pack_host(x.tobytes()), dtype=np.uint8) for x in pkts]
    assert all(r.tobytes() == S.pack(x) and r.size == S.sparse_len(s >> 8) for r, x, s in zip(recs, pkts, scans))
    back = [np.frombuffer(H.sparse_unpack_host(r.tobytes(), n), dtype=np.uint8) for r, n in zip(recs, sizes)]
    assert all(np.array_equal(b, x) for b, x in zip(back, pkts))
    rec_offs = np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
    rec_total, rec_offs = int(rec_offs[-1]), [int(o) for o in rec_offs[:-1]]
    assert {(4 + o) % 8 for o in rec_offs} == {0, 4}
    rec_img = np.concatenate(recs)
    src_offs, src_total = AE.scattered(sizes, 13, align=16, gap=16)
    dst_offs, dst_total = AE.scattered(sizes, 14, align=16, gap=16)
    lanes, one_lane, full = 13, 9, 10                        # k = 64 over every lane, k = 128 in one lane, a whole packet with k = 0
    rec_lines = [("recs", ("on", rec_offs[lanes] + 4 + 2 * 10)), ("recs", ("on", rec_offs[lanes] + 4 + 2 * 64)), ("recs", ("on", rec_offs[lanes])),
                 ("recs", ("on", rec_offs[one_lane] + 4 + 2 * 128 + 40)), ("recs", ("on", rec_offs[1]))]
    assert all(at % 4 == 0 and 0 < at < rec_total for _n, (_how, at) in rec_lines)

    def pack(v):
        src, dst = [v["src"].data_ptr() + o for o in src_offs], [v["recs"].data_ptr() + o for o in rec_offs]
        assert all(p % 32 == 16 for p in src) and all(p % 4 == 0 for p in dst) and v["d_scan"].data_ptr() % 4 == 0
        _put(v, d_src_ptrs=src, d_bytes=sizes, d_dst_ptrs=dst)
        H.sparse_pack(_i64(v["d_src_ptrs"]), _i64(v["d_bytes"]), _i32(v["d_scan"]), _i64(v["d_dst_ptrs"]), k, d_status=_i32(v["d_status"]))

    def unpack(v):
        rec, dst = [v["recs"].data_ptr() + o for o in rec_offs], [v["dst"].data_ptr() + o for o in dst_offs]
        assert all(p % 32 == 16 for p in dst) and all(p % 4 == 0 for p in rec)
        _put(v, d_rec_ptrs=rec, d_rec_bytes=[r.size for r in recs], d_dst_ptrs=dst, d_bytes=sizes)
        H.sparse_unpack(_i64(v["d_rec_ptrs"]), _i64(v["d_rec_bytes"]), _i64(v["d_dst_ptrs"]), _i64(v["d_bytes"]), k, d_status=_i32(v["d_status"]))

    desc = lambda *names: [Arg(name, 8 * k, 8, check=False) for name in names]
    in_packet = lambda name, offs: [(name, ("on", offs[full] + 4112)), (name, ("on", offs[lanes] + 16))]
    return [Case(f"sparse_pack, {k} regions of 1 .. 8192 bytes, k = 0 .. 128",
                 [Arg("src", src_total, 32, init=_block_image(src_offs, pkts, src_total), block=True), Arg("recs", rec_total, 4, want=rec_img),
                  Arg("d_scan", 4 * k, 4, init=np.array(scans, dtype=np.uint32))] + desc("d_src_ptrs", "d_bytes", "d_dst_ptrs") + [_status_arg()],
                 pack, lines=rec_lines + in_packet("src", src_offs), moving=["recs", "d_scan", "d_src_ptrs", "d_bytes", "d_dst_ptrs", "d_status"]),
            Case(f"sparse_unpack, {k} records",
                 [Arg("recs", rec_total, 4, init=rec_img), Arg("dst", dst_total, 32, want=_block_image(dst_offs, back, dst_total), block=True)] +
                 desc("d_rec_ptrs", "d_rec_bytes", "d_dst_ptrs", "d_bytes") + [_status_arg()],
                 unpack, lines=rec_lines + in_packet("dst", dst_offs), moving=["recs", "d_rec_ptrs", "d_rec_bytes", "d_dst_ptrs", "d_bytes", "d_status"])]


@pytest.fixture(scope="module")
def record_cases(H):
    return _record_cases(H)


def test_sparse_records_at_the_weakest_alignment(H, A, record_cases):
    _part_a(H, A, record_cases)


def test_sparse_records_across_the_address_line(H, A, record_cases):
    _part_b(H, A, record_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 10. kinds_store
# ---------------------------------------------------------------------------------------------------------------------
def _made_up_header(p, ulen):
    """What stands in a slot before kinds_store: a header nobody wrote (clen 4 .. 254), in front of canaries."""
    return np.frombuffer(struct.pack("<HH", 4 + (37 * p) % 251, ulen), dtype=np.uint8)


def _store_cases(H):
    """Slots of canaries with a made-up header each; a coded packet's slot must come back untouched in all 8704 bytes, a raw or
    sparse one holds kinds_store_host's bytes and canaries from clen on.  Would catch: slot + 4 stored with 16-byte-aligned
    stores (they would land at slot or slot + 16), d_kind written as a word (byte-weak, a canary behind kind[npk]), d_est or
    d_scan read as quads, slots + r * 8704 or in + r * 8192 formed in 32 bits (the line inside a raw body, inside a sparse
    record, on a slot boundary, inside d_in and d_kind)."""
    rng = np.random.default_rng([SEED, 16])
    n, npk = FORMS_N, FORMS_NPK
    text = np.frombuffer(K.TEXT[:77], dtype=np.uint8).copy()
    cases = []
    for stored, scanned, last, last_kind in ((True, True, _filled(77, 0x80, [0, 76]), K.SPARSE), (True, False, rng.integers(0, 256, 77, dtype=np.uint8), K.RAW),
                                             (False, True, np.zeros(77, dtype=np.uint8), K.SPARSE), (False, False, text, K.CODED)):
        pkts = _form_packets(rng, last)
        host = np.concatenate(pkts)
        raw = host.tobytes()
        est = np.array(H.estimate_host(raw), dtype=np.uint32)
        scan = np.array(H.sparse_scan_host(raw), dtype=np.uint32)
        before = np.full((npk, SLOT), CANARY, dtype=np.uint8)
        for p, x in enumerate(pkts):
            before[p, :4] = _made_up_header(p, x.size)
        after, kinds = before.copy(), []
        for p, x in enumerate(pkts):
            kind, pkt = H.kinds_store_host(x.tobytes(), stored, scanned)
            assert kind == H.sparse_rule(int(scan[p]) if scanned else S.NONE, int(est[p]), x.size, stored) == K.kind_of(x, stored, scanned)
            assert (kind == K.CODED) == (pkt == b"") and len(pkt) <= SLOT
            after[p, :len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
            kinds.append(kind)
        assert set(kinds) == {K.CODED} | ({K.RAW} if stored else set()) | ({K.SPARSE} if scanned else set()) and kinds[-1] == last_kind, kinds
        lines = [("d_slots", ("on", 4 * SLOT)), ("d_in", ("in", 4 * PACKET + 100)), ("d_in", ("on", 4 * PACKET)), ("d_in", ("in", n - 40)),
                 ("d_kind", ("in", 5))]
        if stored:
            p_raw = kinds.index(K.RAW)
            lines.append(("d_slots", ("in", p_raw * SLOT + 5000)))
        if scanned:
            p_sp = max((p for p in range(npk) if kinds[p] == K.SPARSE), key=lambda p: int(after[p, 0]) | int(after[p, 1]) << 8)
            assert (int(after[p_sp, 0]) | int(after[p_sp, 1]) << 8) >= 8 + 160, "no sparse record long enough to hold the line"
            lines.append(("d_slots", ("in", p_sp * SLOT + 8 + 100)))

        def store(v, stored=stored, scanned=scanned):
            H.kinds_store(v["d_in"], _i32(v["d_est"]), _i32(v["d_scan"]) if scanned else None, stored, v["d_slots"], n_bytes=n, d_kind=v["d_kind"],
                          d_status=_i32(v["d_status"]))

        args = [Arg("d_in", n, 16, init=host), Arg("d_est", 4 * npk, 4, init=est)] + ([Arg("d_scan", 4 * npk, 4, init=scan)] if scanned else []) + \
               [Arg("d_slots", npk * SLOT, 16, init=before, want=after), Arg("d_kind", npk, 1, want=np.array(kinds, dtype=np.uint8)), _status_arg()]
        cases.append(Case(f"kinds_store, stored {'on' if stored else 'off'}, d_scan {'given' if scanned else 'NULL'}, kinds {kinds}", args, store, lines=lines))
    return cases


@pytest.fixture(scope="module")
def store_cases(H):
    return _store_cases(H)


def test_kinds_store_at_the_weakest_alignment(H, A, store_cases):
    _part_a(H, A, store_cases)


def test_kinds_store_across_the_address_line(H, A, store_cases):
    _part_b(H, A, store_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 11. kinds_expand
# ---------------------------------------------------------------------------------------------------------------------
def _filler(length):
    """A coded packet of `length` bytes as far as anybody but the decoder can tell: its header and bytes nobody reads."""
    return struct.pack("<HH", length, PACKET) + bytes([0xC3]) * (length - 4)


def _expand_cases(H):
    """A compacted stream built on the host: kinds_store_host's raw and sparse packets, each behind a made-up kind-0 packet of
    an odd length chosen so that the raw and the sparse packets start at every residue mod 16 (asserted), and a short last
    packet.  A kind-0 packet's 8192 output bytes stay canaries, the stream comes back unchanged.  Would catch: the header or
    pos[] read through an aligned type (stream byte-weak, at 1 and 15 mod 16 too; the header two bytes either side of the
    line), stream + offsets[r] or out + r * 8192 formed in 32 bits, a raw tail read from offsets[p + 1] on, d_offsets read as
    quads (8-weak, the line inside it), d_kind read as words."""
    packets = dict(K.packets())
    rng = np.random.default_rng([SEED, 17])
    raws = [packets[f"uniform_n{PACKET}"], rng.integers(0, 256, PACKET, dtype=np.uint8)]
    sparses = [x for name, x in sorted(packets.items()) if x.size == PACKET and K.kind_of(x, False, True) == K.SPARSE]
    assert len(sparses) > 20
    cases = []
    for turn, last in enumerate(("ends_n4095", "uniform_n4095")):
        stream_packets, kinds, plain, at, starts = [], [], [], 0, {K.RAW: set(), K.SPARSE: set()}
        for i in range(32):                                  # a filler, then a raw or a sparse packet that starts at residue i % 16
            x = raws[(i + turn) % 2] if i < 16 else sparses[(i + 7 * turn) % len(sparses)]
            kind, pkt = H.kinds_store_host(x.tobytes(), i < 16, i >= 16)
            assert kind == (K.RAW if i < 16 else K.SPARSE) and (kind, pkt) == K.store(x, i < 16, i >= 16)
            length = 4 + 13 * i + turn
            length += (i % 16 - (at + length)) % 16
            stream_packets += [_filler(length), pkt]
            at += length
            starts[kind].add(at % 16)
            at += len(pkt)
            kinds += [K.CODED, kind]
            plain += [None, x]
        assert starts[K.RAW] == starts[K.SPARSE] == set(range(16))
        x = packets[last]
        kind, pkt = H.kinds_store_host(x.tobytes(), True, True)
        if kind == K.CODED:
            kind, pkt = K.RAW, struct.pack("<HH", 4 + x.size, x.size) + x.tobytes()
        stream_packets.append(pkt)
        kinds.append(kind)
        plain.append(x)
        npk = len(kinds)
        n_bytes = (npk - 1) * PACKET + x.size
        offs = np.concatenate([[0], np.cumsum([len(p) for p in stream_packets])]).astype(np.int64)
        stream = np.frombuffer(b"".join(stream_packets), dtype=np.uint8).copy()
        out = np.full(n_bytes, CANARY, dtype=np.uint8)
        for p, x in enumerate(plain):
            if x is not None:
                assert H.kinds_expand_host(stream_packets[p], kinds[p], x.size) == x.tobytes()
                out[p * PACKET:p * PACKET + x.size] = x
        p_raw, p_sp = 2 * 9 + 1, max(range(33, 64, 2), key=lambda p: len(stream_packets[p]))
        assert kinds[p_raw] == K.RAW and kinds[p_sp] == K.SPARSE and len(stream_packets[p_sp]) > 8 + 160
        lines = [("d_stream", ("on", int(offs[p_raw]) + 4 + 3001)), ("d_stream", ("on", int(offs[p_raw]) + 2)), ("d_stream", ("on", int(offs[p_sp]) + 2)),
                 ("d_stream", ("on", int(offs[p_sp]) + 8 + 51)), ("d_stream", ("on", int(offs[npk - 1]) + 2)),
                 ("d_out", ("in", p_sp * PACKET + 4096)), ("d_out", ("in", p_raw * PACKET + 100)), ("d_out", ("on", p_raw * PACKET)),
                 ("d_out", ("on", p_sp * PACKET)), ("d_out", ("in", n_bytes - 40)), ("d_offsets", ("in", 8 * 30))]

        def expand(v, npk=npk, n_bytes=n_bytes):
            H.kinds_expand(v["d_stream"], _i64(v["d_offsets"]), v["d_kind"], npk, v["d_out"], n_bytes, d_status=_i32(v["d_status"]))

        cases.append(Case(f"kinds_expand, {npk} packets, the last one {last}",
                          [Arg("d_stream", stream.size, 1, init=stream), Arg("d_offsets", 8 * (npk + 1), 8, init=offs),
                           Arg("d_kind", npk, 1, init=np.array(kinds, dtype=np.uint8)), Arg("d_out", n_bytes, 16, want=out), _status_arg()],
                          expand, lines=lines,
                          extra=[({"d_stream": ("skew", 16, r)}, f"d_stream at {r} mod 16") for r in (1, 15)]))
    return cases


@pytest.fixture(scope="module")
def expand_cases(H):
    return _expand_cases(H)


def test_kinds_expand_at_the_weakest_alignment(H, A, expand_cases):
    _part_a(H, A, expand_cases)


def test_kinds_expand_across_the_address_line(H, A, expand_cases):
    _part_b(H, A, expand_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 12. move_bytes
# ---------------------------------------------------------------------------------------------------------------------
def _move_bytes_cases(H):
    """Regions of 1 .. 8704 bytes and one of 0, twice over: the sources at mixed residues mod 16, the destinations back to back
    at byte grain in one block, so a store that leaves its region lands in a neighbour or in the canaries around the block.
    The line is a multiple of 16, so inside a destination it is always a boundary between 16-byte pieces: it is put where the
    head bytes end (3 bytes in), between two quads of the body, where the tail bytes begin, at the region's first byte and one
    byte behind its last; inside a source it falls in the middle of an unaligned 16-byte load.  Would catch: src + head + at or
    the tail's address formed in 32 bits, a whole-quad store over a ragged end, descriptor arrays read as quads."""
    rng = np.random.default_rng([SEED, 18])
    sizes = [1, 15, 16, 17, 31, 0, 33, 4097, SLOT]
    sizes = sizes + sizes[::-1]
    datas = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    k = len(sizes)
    dst_offs = [21 + int(o) for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    dst_total = dst_offs[-1] + sizes[-1] + 27
    src_offs, at = [], 7
    for i, s in enumerate(sizes):
        src_offs.append(at)
        at += s + 16 + (5 * i + 3) % 16
    src_total = at + 16
    assert len({o % 16 for o in src_offs}) >= 8 and len({o % 16 for o in dst_offs}) >= 5
    r = sizes.index(4097)
    lines = [("dst", ("on", dst_offs[r] + at)) for at in (3, 2051, 4083, 0, 4097)] + [("src", ("on", src_offs[r] + at)) for at in (2056, 0, 4097)] + \
            [("dst", ("on", dst_offs[8] + 5000)), ("src", ("on", src_offs[8] + 8699))]

    def move(v):
        _put(v, d_src_ptrs=[v["src"].data_ptr() + o for o in src_offs], d_dst_ptrs=[v["dst"].data_ptr() + o for o in dst_offs], d_bytes=sizes)
        H.move_bytes(_i64(v["d_src_ptrs"]), _i64(v["d_dst_ptrs"]), _i64(v["d_bytes"]), k, d_status=_i32(v["d_status"]))

    args = [Arg("src", src_total, 1, init=_block_image(src_offs, datas, src_total), block=True),
            Arg("dst", dst_total, 1, want=_block_image(dst_offs, datas, dst_total), block=True),
            Arg("d_src_ptrs", 8 * k, 8, check=False), Arg("d_dst_ptrs", 8 * k, 8, check=False), Arg("d_bytes", 8 * k, 8, check=False), _status_arg()]
    skews = ((0, 0), (9, 2), (15, 15), (3, 12), (6, 7))       # with the destinations' own offsets, 5 .. 9 mod 16: every residue
    return [Case(f"move_bytes, regions of {sizes[:9]} bytes and back", args, move, lines=lines,
                 moving=["d_src_ptrs", "d_dst_ptrs", "d_bytes", "d_status"],
                 extra=[({"src": ("skew", 16, rs), "dst": ("skew", 16, rd)}, f"src at {rs} and dst at {rd} mod 16") for rs, rd in skews])]


@pytest.fixture(scope="module")
def move_bytes_cases(H):
    return _move_bytes_cases(H)


def test_move_bytes_at_the_weakest_alignment(H, A, move_bytes_cases):
    _part_a(H, A, move_bytes_cases)


def test_move_bytes_across_the_address_line(H, A, move_bytes_cases):
    _part_b(H, A, move_bytes_cases)


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


# ---------------------------------------------------------------------------------------------------------------------
# C, continued: estimate -> sparse_scan -> kinds_store -> compact -> kinds_expand past 2^32, and move_bytes
# ---------------------------------------------------------------------------------------------------------------------
BIG_NPK = (BIG + PACKET - 1) // PACKET                       # 524313
BIG_LAST = BIG - (BIG_NPK - 1) * PACKET                      # 4102
SLOT_CROSSING = (AE.LINE + SLOT - 1) // SLOT                 # 493448: the first packet whose slot starts past byte 2^32 of d_slots
KW = 16                                                      # packets in a window
KINDS_WINDOWS = (0, SLOT_CROSSING - KW // 2, AE.LINE // PACKET - KW // 2, BIG_NPK - KW)
ROWS = 8192                                                  # packets per device comparison


def _window_mix(rng, w):
    """The 16 packets of window w: zeros, fills with k = 1 .. 100 exceptions, text (coded) and uniform (raw), in an order that
    depends on the window; the last window ends with a fill whose short form is the buffer's last packet."""
    text = np.frombuffer(K.TEXT[:PACKET], dtype=np.uint8)
    fills = lambda f, k: _filled(PACKET, f, np.arange(k) * (PACKET // 101) + 5 + w)
    mix = [np.zeros(PACKET, dtype=np.uint8), fills(0x80, 1), text.copy(), rng.integers(0, 256, PACKET, dtype=np.uint8), fills(0x00, 2), fills(0xFF, 17),
           np.roll(text, 3 + w), fills(0x00, 64), rng.integers(0, 256, PACKET, dtype=np.uint8), fills(0x80, 100), np.full(PACKET, 0xFF, dtype=np.uint8),
           np.roll(text, 100), fills(0xFF, 33), rng.integers(0, 256, PACKET, dtype=np.uint8), fills(0x00, 99), np.roll(text, 7)]
    mix = mix[w:] + mix[:w]
    if w == 3:
        j = next(j for j, q in enumerate(mix) if not q.any())
        mix[j], mix[-1] = mix[-1], mix[j][:BIG_LAST]
    return mix


def _made_up_slots(npk, last):
    """npk slots of canaries behind a made-up header (clen 4 + p % 251, the packet's ulen), and 4096 canaries behind them."""
    slots = torch.full((npk * SLOT + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    rows = slots[:npk * SLOT].view(npk, SLOT)
    rows[:, 0] = (4 + torch.arange(npk, device="cuda") % 251).to(torch.uint8)
    rows[:, 1] = 0
    rows[:, 2] = 0
    rows[:, 3] = PACKET >> 8
    rows[npk - 1, 2] = last & 255
    rows[npk - 1, 3] = last >> 8
    return slots, rows


def _all_equal(t, value):
    """Device verdict: every byte of t is `value`, 256 MiB at a time."""
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    for at in range(0, t.numel(), CHUNK):
        ok = ok & t[at:at + CHUNK].eq(value).all()
    return ok


def test_kinds_pipeline_past_4gib(H, A):
    """estimate, sparse_scan, kinds_store (stored on, d_scan given), compact and kinds_expand on one stream over 524 313 packets
    of uniform bytes -- every whole one raw: its estimate is 8249 .. 8265 against the threshold 8196 -- with four windows of 16
    mixed packets: at packet 0, where the slot offset r * 8704 passes 2^32 (packet 493 448), where the input offset r * 8192
    does (524 288), and the last 16 with the short last packet.  The slots start as canaries behind a made-up header of clen
    4 + p % 251, so the untouched (coded) packets of window 0 make later stream offsets odd, and with at most 200 packets that
    are not raw the stream itself passes 2^32 (asserted).  Would catch: a 32-bit product in slots + r * 8704, in + r * 8192,
    out + r * 8192 or stream + offsets[r] -- each writes a wrong but in-bounds place, so every slot, every kind and every
    output packet of the whole buffer is compared on the device --, and a scan loop whose 32-bit packet index goes wrong."""
    npk = BIG_NPK
    assert H.packet_count(BIG) == npk and (SLOT_CROSSING - 1) * SLOT < AE.LINE <= SLOT_CROSSING * SLOT
    x = _alloc_big()
    H.generate("uniform", 33, BIG, out=x)
    rng = np.random.default_rng([SEED, 19])
    wins = []
    for w, first in enumerate(KINDS_WINDOWS):
        pkts = _window_mix(rng, w)
        data = np.concatenate(pkts)
        assert first * PACKET + data.size <= BIG and (w < 3 or first * PACKET + data.size == BIG)
        x[first * PACKET:first * PACKET + data.size].copy_(_u8(data))
        wins.append((first, pkts))
    in_window = torch.zeros(npk, dtype=torch.bool, device="cuda")
    for first, _pkts in wins:
        in_window[first:first + KW] = True
    slots, rows = _made_up_slots(npk, BIG_LAST)
    room = npk * (4 + PACKET) + 4096
    d_stream = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    A.reset()
    d_est, d_scan, d_kind = _i32(A.put(4 * npk, 4)), _i32(A.put(4 * npk, 4)), A.put(npk, 1)
    d_offsets, word = _i64(A.put(8 * (npk + 1), 8)), _i32(A.put(4, 4))
    word.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    H.estimate(x, n_bytes=BIG, d_est=d_est, stream=s)
    H.sparse_scan(x, n_bytes=BIG, d_scan=d_scan, stream=s)
    H.kinds_store(x, d_est, d_scan, True, slots[:npk * SLOT], n_bytes=BIG, d_kind=d_kind, stream=s, d_status=word)
    H.compact(slots[:npk * SLOT], npk, d_stream, d_offsets, stream=s)
    s.synchronize()

    # the windows against the host twins
    got_scan, got_kind = d_scan.cpu().numpy().view(np.uint32), d_kind.cpu().numpy()
    host_kind = {}
    for first, pkts in wins:
        raw = np.concatenate(pkts).tobytes()
        scan_host, est_host = H.sparse_scan_host(raw), H.estimate_host(raw)
        assert got_scan[first:first + KW].tolist() == scan_host, f"scan words of packets {first} .. {first + KW - 1} differ from sparse_scan_host"
        want_kind = [H.sparse_rule(sc, e, q.size, True) for sc, e, q in zip(scan_host, est_host, pkts)]
        assert got_kind[first:first + KW].tolist() == want_kind, f"kinds of packets {first} .. {first + KW - 1} differ from sparse_rule"
        got_slots = rows[first:first + KW].cpu().numpy()
        for j, q in enumerate(pkts):
            kind, pkt = H.kinds_store_host(q.tobytes(), True, True)
            assert kind == want_kind[j]
            want = np.full(SLOT, CANARY, dtype=np.uint8)
            want[:4] = np.frombuffer(struct.pack("<HH", 4 + (first + j) % 251, q.size), dtype=np.uint8)
            want[:len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
            assert np.array_equal(got_slots[j], want), f"slot {first + j} (kind {kind}) differs from kinds_store_host or its canaries behind clen are gone"
            host_kind[first + j] = kind
        assert set(want_kind) == {K.CODED, K.RAW, K.SPARSE}
    not_raw = int(d_kind.ne(K.RAW).sum().item())
    assert 0 < not_raw == sum(k != K.RAW for k in host_kind.values()) <= 200, f"{not_raw} packets are not raw: the stream need not pass 2^32"

    # the whole buffer on the device
    verdicts = [("a scan word outside the windows is not NONE", (d_scan.eq(-1) | in_window).all()),
                ("a packet outside the windows is not raw", (d_kind.eq(K.RAW) | in_window).all())]
    header = torch.tensor([(4 + PACKET) & 255, (4 + PACKET) >> 8, 0, PACKET >> 8], dtype=torch.uint8, device="cuda")
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    for lo in range(0, npk - 1, ROWS):
        hi = min(lo + ROWS, npk - 1)
        r, xs = rows[lo:hi], x[lo * PACKET:hi * PACKET].view(-1, PACKET)
        good = r[:, :4].eq(header).all(1) & r[:, 4:4 + PACKET].eq(xs).all(1) & r[:, 4 + PACKET:].eq(CANARY).all(1)
        ok = ok & (good | in_window[lo:hi]).all()
    verdicts.append(("a slot outside the windows is not header(8196, 8192), the packet's bytes, canaries", ok))
    verdicts.append(("written behind the last slot", slots[npk * SLOT:].eq(CANARY).all()))
    offs = d_offsets.cpu().numpy()
    total = int(offs[-1])
    assert total > 1 << 32, f"the stream has {total} bytes: it does not pass 2^32"
    assert total == int((rows[:, 0].to(torch.int64) | rows[:, 1].to(torch.int64) << 8).sum().item()), "offsets[-1] is not the sum of the clens"
    verdicts.append(("written behind the stream", d_stream[total:].eq(CANARY).all()))
    _fail_on(verdicts)
    del r, xs, rows, slots
    torch.cuda.empty_cache()

    out = torch.full((BIG + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    s.wait_stream(torch.cuda.current_stream())
    H.kinds_expand(d_stream, d_offsets, d_kind, npk, out, BIG, stream=s, d_status=word)
    s.synchronize()
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    for lo in range(0, npk - 1, ROWS):
        hi = min(lo + ROWS, npk - 1)
        o, xs = out[lo * PACKET:hi * PACKET].view(-1, PACKET), x[lo * PACKET:hi * PACKET].view(-1, PACKET)
        ok = ok & torch.where(d_kind[lo:hi].ne(K.CODED), o.eq(xs).all(1), o.eq(CANARY).all(1)).all()
    tail = out[(npk - 1) * PACKET:BIG]
    assert host_kind[npk - 1] != K.CODED
    verdicts = [("an output packet is not the input's (kind 1, 2) or not canaries (kind 0)", ok),
                ("the short last packet is not the input's", _same(tail, x[(npk - 1) * PACKET:BIG])),
                ("written behind n_bytes", out[BIG:].eq(CANARY).all()), ("the input changed or was written behind", x[BIG:].eq(CANARY).all()),
                ("the status word is not 0", word.eq(0).all()), A.guards("the kinds pipeline past 4 GiB")]
    at = int(np.searchsorted(offs, 1 << 32, side="right")) - 1
    assert offs[at] <= 1 << 32 < offs[at + 1] and got_kind[at] == K.RAW, f"packet {at} holds stream byte 2^32 and is of kind {got_kind[at]}"
    verdicts += [(f"packet {at}, which holds stream byte 2^32: its output differs", _same(out[at * PACKET:(at + 1) * PACKET], x[at * PACKET:(at + 1) * PACKET])),
                 (f"packet {at}: its bytes in the stream differ", _same(d_stream[int(offs[at]) + 4:int(offs[at + 1])], x[at * PACKET:(at + 1) * PACKET]))]
    _fail_on(verdicts)
    assert H.status() == 0
    del out, d_stream, x, o, xs, tail


def test_move_bytes_past_4gib(H, A, big):
    """One launch of 4096 regions of 1 .. 8704 bytes whose sources lie behind offset 2^32 of part C's buffer and whose
    destinations stand back to back, at byte grain, across offset 2^32 of a second allocation, with every pair of residues
    mod 16 (asserted).  Expected: numpy over the region list; everything else in the second allocation stays canaries."""
    x, wins = big["x"], big["wins"]
    tail = np.concatenate([wins[1][2 * GROUP:], wins[2]])
    assert tail.size == BIG - AE.LINE
    rng = np.random.default_rng([SEED, 20])
    n = 4096
    sizes = np.concatenate([[1, 15, 16, 17, 31, 33, 4097, SLOT], rng.integers(1, SLOT + 1, n - 8)])[rng.permutation(n)].astype(np.int64)
    total = int(sizes.sum())
    start = AE.LINE - total // 2 + 3
    dst = start + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert dst[0] < AE.LINE < dst[-1]
    turn, src = [0] * 16, np.zeros(n, dtype=np.int64)
    for i in range(n):
        res = turn[dst[i] % 16] % 16
        turn[dst[i] % 16] += 1
        src[i] = int(rng.integers(0, tail.size - sizes[i] - 16)) // 16 * 16 + res
    assert len({(int(a) % 16, int(b) % 16) for a, b in zip(src, dst)}) == 256 and (src + sizes <= tail.size).all()
    want = np.full(total + 2 * 4096, CANARY, dtype=np.uint8)
    for a, b, m in zip(src, dst - start + 4096, sizes):
        want[b:b + m] = tail[a:a + m]
    d = torch.full((AE.LINE + total + 8192,), CANARY, dtype=torch.uint8, device="cuda")
    A.reset()
    d_src, d_dst, d_bytes, word = _i64(A.put(8 * n, 8)), _i64(A.put(8 * n, 8)), _i64(A.put(8 * n, 8)), _i32(A.put(4, 4))
    d_src.copy_(torch.from_numpy(src + AE.LINE + x.data_ptr()))
    d_dst.copy_(torch.from_numpy(dst + d.data_ptr()))
    d_bytes.copy_(torch.from_numpy(sizes))
    word.zero_()
    H.move_bytes(d_src, d_dst, d_bytes, n, d_status=word)
    lo, hi = start - 4096, start + total + 4096
    _fail_on([("the destinations differ from numpy's, or a byte next to them changed", _same(d[lo:hi], _u8(want))),
              ("written in front of the destinations", _all_equal(d[:lo], CANARY)), ("written behind the destinations", _all_equal(d[hi:], CANARY)),
              ("the sources changed", _same(x[AE.LINE:BIG], _u8(tail))), ("the status word is not 0", word.eq(0).all()),
              A.guards("move_bytes past 4 GiB")])
    assert _canary_holds(x) and H.status() == 0
    del d


# ---------------------------------------------------------------------------------------------------------------------
# D. the second and third trip of a wavefront: sparse_scan, kinds_store and kinds_expand over 3 * 8192 + 5 packets
# ---------------------------------------------------------------------------------------------------------------------
WAVES = 2048 * 4                                             # the persistent grid: 2048 workgroups of 4 wavefronts, a packet each
TRIPS_NPK = 3 * WAVES + 5
TRIPS_LAST = 77
TRIPS_N = (TRIPS_NPK - 1) * PACKET + TRIPS_LAST


def _sparse_packet(H, x):
    """x as a kind-2 packet of a stream, whatever the rule would make of it."""
    rec = H.sparse_pack_host(x.tobytes())
    return struct.pack("<HH", 4 + len(rec), x.size) + rec


def _patched(pkt, at, data):
    pkt = bytearray(pkt)
    pkt[at:at + len(data)] = data
    return bytes(pkt)


@pytest.mark.parametrize("damage", [True, False], ids=["damaged", "intact"])
def test_kinds_expand_second_trip(H, damage):
    """Wavefront w of kinds_expand's 8192 takes packets w, w + 8192 and w + 16384 (w < 5: a fourth) and builds every sparse one
    in the same 8 KiB of LDS.  What a packet leaves there must not show in the next: by w % 6 a wavefront meets 100 exceptions,
    then fill 0xFF with none, then a raw packet; a DAMAGED record -- positions not ascending at index 70 (the first turn of 64
    lanes has scattered its bytes), a value equal to the fill, a position >= n --, then a good packet with another fill and two
    exceptions; raw, kind 0 and sparse in other orders; and wavefront 4 a damaged full packet in front of the buffer's short last
    one.  Every packet that is not damaged must be exact (its template is pinned against kinds_expand_host), kind-0 packets stay
    canaries, the stream is unchanged, and BAD_PACKET is set exactly when a damaged packet is present.  Would catch: a missing
    ordering between one packet's scatter or read-back and the next packet's fill, a fill that covers only the next packet's
    bytes where the read-back covers more, a loop stride that is not the grid's."""
    rng = np.random.default_rng([SEED, 21])
    sp100 = _filled(PACKET, 0x00, np.arange(100) * 81 + 7)
    ff, two = np.full(PACKET, 0xFF, dtype=np.uint8), _filled(PACKET, 0x55, [9, 4000])
    uniform, text = rng.integers(0, 256, PACKET, dtype=np.uint8), np.frombuffer(K.TEXT[:PACKET], dtype=np.uint8).copy()
    last = _filled(TRIPS_LAST, 0x80, [0, TRIPS_LAST - 1])
    good = _sparse_packet(H, sp100)
    pos, val = 8, 8 + 2 * 100                                 # where pos[] and val[] begin in the packet
    bad = [_patched(good, pos + 2 * 70, good[pos + 2 * 69:pos + 2 * 70]), _patched(good, val + 70, b"\x00"), _patched(good, pos + 2 * 99, struct.pack("<H", PACKET))]
    for pkt in bad:
        assert K.expand(pkt, K.SPARSE, PACKET) is None and K.expand(good, K.SPARSE, PACKET) is not None
    raw_of = lambda q: struct.pack("<HH", 4 + q.size, q.size) + q.tobytes()
    # (bytes or None for canaries, kind, packet, damaged)
    T = [(sp100, K.SPARSE, good, False), (ff, K.SPARSE, _sparse_packet(H, ff), False), (uniform, K.RAW, raw_of(uniform), False),
         (text, K.RAW, raw_of(text), False), (None, K.CODED, _filler(4 + 13), False), (two, K.SPARSE, _sparse_packet(H, two), False)] + \
        [(sp100, K.SPARSE, pkt if damage else good, damage) for pkt in bad] + [(last, K.SPARSE, _sparse_packet(H, last), False)]
    for q, kind, pkt, damaged in T:
        if q is not None and not damaged:
            assert H.kinds_expand_host(pkt, kind, q.size) == q.tobytes()
    SP100, FF, RAW, TEXT, CODED, TWO, BAD_A, BAD_B, BAD_C, LAST = range(10)
    by_class = [(SP100, FF, RAW), (BAD_A, TWO, FF), (RAW, SP100, TWO), (BAD_B, FF, SP100), (CODED, BAD_C, TWO), (TEXT, CODED, SP100)]
    npk = TRIPS_NPK
    idx = np.array([by_class[(p % WAVES) % 6][p // WAVES] if p < 3 * WAVES else (TWO, SP100, FF, RAW, LAST)[p - 3 * WAVES] for p in range(npk)])
    idx[2 * WAVES + 4] = BAD_A                               # wavefront 4: a damaged full packet, then the short last one
    assert (idx[4::WAVES] == [CODED, BAD_C, BAD_A, LAST]).all()
    lens = np.array([len(t[2]) for t in T])
    offs = np.concatenate([[0], np.cumsum(lens[idx])]).astype(np.int64)
    stream = np.frombuffer(b"".join(T[t][2] for t in idx), dtype=np.uint8).copy()
    assert stream.size == offs[-1] and len({int(o) % 16 for o in offs}) == 16
    images = np.full((len(T), PACKET), CANARY, dtype=np.uint8)
    for t, (q, _kind, _pkt, _damaged) in enumerate(T):
        if q is not None:
            images[t, :q.size] = q
    d_idx = torch.from_numpy(idx).cuda()
    want = _u8(images).view(len(T), PACKET)[d_idx].view(-1)    # (the last packet's row: its 77 bytes, then canaries)
    skip = torch.tensor([t[3] for t in T], device="cuda")[d_idx]
    d_stream = torch.full((stream.size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    d_stream[:stream.size] = _u8(stream)
    before = d_stream.clone()
    d_offsets = torch.from_numpy(offs).cuda()
    d_kind = torch.tensor([t[1] for t in T], dtype=torch.uint8, device="cuda")[d_idx]
    out = torch.full((npk * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    H.kinds_expand(d_stream, d_offsets, d_kind, npk, out, TRIPS_N, d_status=word)
    same = out.view(npk, PACKET).eq(want.view(npk, PACKET)).all(1)
    n_bad = int(np.isin(idx, (BAD_A, BAD_B, BAD_C)).sum())
    assert n_bad > WAVES // 3 and int(skip.sum().item()) == (n_bad if damage else 0)
    _fail_on([("a packet that is not damaged differs from its template, a kind-0 packet is not canaries, or bytes behind the short last packet changed",
               (same | skip).all()),
              ("the stream changed", _same(d_stream, before)),
              (f"the status word is not {H.STATUS_BAD_PACKET if damage else 0:#x}", word.eq(H.STATUS_BAD_PACKET if damage else 0).all())])
    assert H.status() == 0


@pytest.mark.parametrize("defect", [True, False], ids=["wrong_scan_words", "right_scan_words"])
def test_sparse_scan_and_kinds_store_second_trip(H, defect):
    """The same for sparse_scan and kinds_store (stored on, d_scan given): each of their 8192 wavefronts takes three packets of
    the 3 * 8192 + 5, by w % 6 sparse, raw and coded ones in changing order.  The scan words are compared with the templates'
    (sparse_scan_host), the kinds with sparse_rule, every slot with kinds_store_host's bytes behind canaries and a made-up
    header.  With `defect`, the scan words of first-trip packets disagree with their bytes (a count that is one too many; a
    fill that is no majority): BAD_BATCH, kind 0, the slot untouched, and the good packets behind them in the same wavefront
    are stored as ever.  Would catch: state carried from one trip to the next (the prefix sum, the registers of a skipped
    packet), `continue` paths that skip the stride, a loop stride that is not the grid's."""
    rng = np.random.default_rng([SEED, 22])
    text = np.frombuffer(K.TEXT[:PACKET], dtype=np.uint8).copy()
    T = [_filled(PACKET, 0x00, np.arange(100) * 81 + 7), np.full(PACKET, 0xFF, dtype=np.uint8), rng.integers(0, 256, PACKET, dtype=np.uint8), text,
         _filled(PACKET, 0x55, [9, 4000]), np.zeros(PACKET, dtype=np.uint8), _filled(TRIPS_LAST, 0x80, [0, TRIPS_LAST - 1])]
    SP100, FF, RAW, TEXT, TWO, ZEROS, LAST = range(7)
    by_class = [(SP100, FF, RAW), (TWO, RAW, SP100), (RAW, SP100, TWO), (TWO, TEXT, FF), (TEXT, ZEROS, RAW), (FF, TWO, TEXT)]
    npk = TRIPS_NPK
    idx = np.array([by_class[(p % WAVES) % 6][p // WAVES] if p < 3 * WAVES else (TWO, SP100, FF, RAW, LAST)[p - 3 * WAVES] for p in range(npk)])
    scan_t = [H.sparse_scan_host(q.tobytes())[0] for q in T]
    est_t = [H.estimate_host(q.tobytes())[0] for q in T]
    kind_t, slot_t = [], np.full((len(T), SLOT), CANARY, dtype=np.uint8)
    for t, q in enumerate(T):
        kind, pkt = H.kinds_store_host(q.tobytes(), True, True)
        assert kind == H.sparse_rule(scan_t[t], est_t[t], q.size, True)
        slot_t[t, :len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
        kind_t.append(kind)
    assert [kind_t[t] for t in (SP100, FF, RAW, TEXT, TWO, ZEROS, LAST)] == [K.SPARSE, K.SPARSE, K.RAW, K.CODED, K.SPARSE, K.SPARSE, K.SPARSE]
    images = np.full((len(T), PACKET), CANARY, dtype=np.uint8)
    for t, q in enumerate(T):
        images[t, :q.size] = q
    d_idx = torch.from_numpy(idx).cuda()
    x = _u8(images).view(len(T), PACKET)[d_idx].view(-1)
    scans = np.array(scan_t, dtype=np.uint32)[idx]
    kinds = np.array(kind_t, dtype=np.uint8)[idx]
    wrong = np.zeros(npk, dtype=bool)
    if defect:
        first = np.arange(WAVES)
        one_more, no_majority = first[first % 6 == 1], first[first % 6 == 3]
        assert (idx[one_more] == TWO).all() and (idx[no_majority] == TWO).all()
        scans[one_more] = (3 << 8) | 0x55
        scans[no_majority] = (2 << 8) | 0x56
        wrong[one_more] = wrong[no_majority] = True
        kinds[wrong] = K.CODED
    d_est = torch.from_numpy(np.array(est_t, dtype=np.uint32)[idx].view(np.int32)).cuda()
    d_scan_in = torch.from_numpy(scans.view(np.int32)).cuda()
    got_scan = torch.full((npk + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    H.sparse_scan(x, n_bytes=TRIPS_N, d_scan=got_scan[:npk])
    slots, rows = _made_up_slots(npk, TRIPS_LAST)
    untouched = rows.clone()
    d_kind = torch.full((npk + 64,), CANARY, dtype=torch.uint8, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    H.kinds_store(x, d_est, d_scan_in, True, slots[:npk * SLOT], n_bytes=TRIPS_N, d_kind=d_kind[:npk], d_status=word)
    d_kinds = torch.from_numpy(kinds).cuda()
    want = torch.where(d_kinds.eq(K.CODED)[:, None], untouched, _u8(slot_t).view(len(T), SLOT)[d_idx])
    true_scans = torch.from_numpy(np.array(scan_t, dtype=np.uint32)[idx].view(np.int32)).cuda()
    _fail_on([("a scan word differs from sparse_scan_host's", _same(got_scan[:npk], true_scans)),
              ("written behind d_scan[npk]", got_scan[npk:].eq(-0x5A5A5A5B).all()),
              ("a kind differs from sparse_rule's (0 for a packet whose scan word is wrong)", _same(d_kind[:npk], d_kinds)),
              ("written behind d_kind[npk]", d_kind[npk:].eq(CANARY).all()),
              ("a slot differs: a coded packet's or a refused one's is not untouched, a raw or sparse one's is not kinds_store_host's bytes and canaries",
               rows.eq(want).all()),
              ("written behind the last slot", slots[npk * SLOT:].eq(CANARY).all()),
              (f"the status word is not {H.STATUS_BAD_BATCH if defect else 0:#x}", word.eq(H.STATUS_BAD_BATCH if defect else 0).all())])
    assert H.status() == 0
