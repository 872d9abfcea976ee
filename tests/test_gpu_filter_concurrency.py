"""The filter, estimate and survey kernels under concurrent streams and host threads: the contract of include/gpuar_hip.h that
tests/test_gpu_concurrency.py pins for the coders, compaction, CRC-32 and generate, here for the entry points added since --
split_ / merge_planes, split_ / merge_delta, split_ / merge_xor (each a full-group launch and a tail launch), estimate,
survey_planes, survey_delta, survey_xor, their batch forms and move_packets -- and for what gpuar_amd/batch.py composes from them
(planes=, delta=, stored=, base=, base_auto=, sparse=, "auto" and "survey").  Every call takes an explicit stream; a launch ORs its
flags into its own status word and into no other; a launch without a word uses the fallback word, which status() reports once.

Every test works the same way: a serial pass (one launch at a time, synchronised) is pinned against existing host code --
planes_ref.numpy_split, delta_ref.numpy_split_delta, xor_ref.numpy_split_xor, hip.estimate_host, hip.survey_planes_host,
hip.survey_delta_host, hip.survey_xor_host, the reference encoder on 64-packet windows, zlib.crc32 --; then the same work runs concurrently and must
give the same bytes, with every status word exactly what its own launch should report.  Everything is integer-exact.
Comparisons run on the device; one copy of the verdicts per test.

Stream / thread i runs WORKLOADS[i]: an element width, a kind of bytes and a byte count, each a different launch shape (tail
only; one group; one group and the longest tail; a tail without a whole element; four of 16 MiB and a ragged rest: 256 compute
units hold 1024 plane workgroups of 512 threads = 8 MiB of packets, or 512 workgroups of 64 KiB of LDS, so one such launch
goes round the chip two to four times and eight of them contend for it).

1. Stream order.  On a non-blocking stream s that is not the current stream a producer runs -- a chain of device_copy calls
   over 256 MiB, ending with the copy that puts the real input where the canary was --, the call under test is enqueued behind
   it with stream=s, and a copy of its output behind that.  An event behind the producer must still be pending after the last
   enqueue (otherwise the run says nothing and FAILS as "producer too short").  A launch that went to any other stream (the
   NULL stream, torch's current stream) reads the canary or is overwritten by the producer, and the result differs.  Every
   new entry point, out of place and in place, workloads 2 and 6.  A control sends split_planes to another stream on
   purpose and must differ.  The chain is sized at run time: its GPU time, in links measured with events, is at least four
   times the host time that the enqueue of chain, feeds, call and copies takes, the call's part of it as measured with
   perf_counter in the serial pass; and never under MIN_LINKS links, so that a pause of the host of a few milliseconds
   does not make a run inconclusive.  Measured on an MI355X: one link (a 256 MiB device_copy) runs 87.0 us on the GPU
   and takes 4.5 us of host time to enqueue; the slowest call's feeds, launch and copies took 107 us to enqueue.
2. Fan-out with status isolation, one family at a time, eight streams: planes / delta / XOR (single split, a copy, merge in
   place; the batch forms over a dozen buffers, stream 1's batch with one unusable descriptor), estimate and both surveys
   (single and batch, canaries behind every row and in the rows a widths mask leaves out, stream 1 with a misaligned buffer),
   the XOR survey (single and batch; both outputs, the est rows alone or the scan rows alone by stream, the output that was not
   asked for keeping every canary; base pointers of 0 in every batch; stream 1 with a base pointer that is 8 mod 16),
   move_packets (stream 1 with a region of 8193 bytes).  BAD_BATCH in stream 1's words and in no other.
3. The fallback word: each batch entry point with d_status=None and one unusable descriptor; status() reports BAD_BATCH once.
4. Mixed co-residency: a 256 MiB throughput encode next to survey_delta, estimate_batch, split_xor, merge_delta in place,
   move_packets, crc32_batch and survey_xor_batch, the encoder enqueued first or last.
5. batch.compress / decompress from seven threads, each with its own stream and one keyword family.

Time, pytest --durations=0 on an MI355X, with tests/test_gpu_batch_trace.py behind it: 13 passed in 10.6 s, 4.0 s of it that
module's one test and 2 s importing torch and collecting.
    1.39 s  test_thread_batch_compress_families (seven families; the host rule of the seventh -- eight numpy splits, estimates and
            scans of its 16 MiB tensor -- takes 0.7 s on one core)
    1.38 s  setup of test_stream_order[2] (the eight workloads and their references; survey_xor_host takes 0.3 s on one core for
            each of the four 16 MiB workloads)
    0.46 s, 0.39 s  test_stream_order[2], [6] (33 cases each, two of them the XOR survey's)
    0.50 s, 0.15 s  test_mixed_co_residency[encoder_first], [encoder_last]
    0.05 s  test_survey_xor_fan_out, test_estimate_and_survey_fan_out and each test_filter_fan_out
    0.04 s  test_fallback_word_of_the_batch_entry_points; 0.02 s test_move_packets_fan_out

Not covered here: the grid-stride loops of the plane, delta, XOR and move kernels start at 2^22 workgroups (32 GiB, or four million
buffers); tests/test_gpu_grid_cap.py runs their later passes on a build whose cap is 3.  Tensors on a device that is not the current one.  Fixed seeds throughout.
"""
import math
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import delta_ref as D
import planes_ref as P
import xor_ref as X
from concurrency_checks import _fail_on, _same, _status, _streams, _words
from test_survey_host import totals_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
MiB = 1 << 20
CANARY = 0xA5
CANARY32 = 0xA5A5A5A5
GUARD = 256
WIDTHS = (1, 2, 4, 8)
LINK = 256 * MiB                     # bytes one producer link copies
MIN_LINKS, MAX_LINKS = 64, 400       # a chain runs 5.6 .. 35 ms, whatever the serial pass measured
BAD = 7                              # the buffer of stream 1's batch that carries the unusable descriptor

# (element width, (source, kind), bytes): stream / thread i runs workload i
WORKLOADS = [
    (2, ("typed", "bf16"), 1),                                   # tail launch only, no whole element
    (8, ("bytes", "ramp"), 8 * PACKET),                          # exactly one group, no tail
    (4, ("typed", "fp32"), 8 * PACKET - 1),                      # one group and the longest tail
    (8, ("bytes", "uniform"), 8 * PACKET + 7),                   # one group and a tail without a whole element
    (1, ("typed", "uniform"), 16 * MiB + 8191),
    (2, ("bytes", "ones"), 16 * MiB + 2 * PACKET - 15),
    (4, ("typed", "bf16"), 16 * MiB + 3 * PACKET + 77),
    (8, ("bytes", "ramp"), 16 * MiB + 7 * PACKET + 8191),
]
MASKS = [(1, 2, 4, 8), (8,), (4,), (1, 2), (1,), (2, 8), (2, 4), (1, 2, 4, 8)]      # survey_delta's widths per stream
FAMILIES = ("planes", "delta", "xor")


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


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# inputs, references and their images on the device
# ---------------------------------------------------------------------------------------------------------------------
def _r16(n):
    return (n + 15) // 16 * 16


def _dev(host):
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


def _blank(n_bytes):
    return torch.full((n_bytes,), CANARY, dtype=torch.uint8, device="cuda")


def _image(host):
    """[host | canaries] on the device: the bytes up to the next multiple of 16 and GUARD more are canaries."""
    img = np.full(_r16(host.size) + GUARD, CANARY, dtype=np.uint8)
    img[:host.size] = host
    return _dev(img)


def _est_image(est, npk):
    """npk estimates and canaries behind them, as the bytes of a uint32 array (a multiple of 16 bytes)."""
    img = np.full((npk + 2 + 3) // 4 * 4, CANARY32, dtype=np.uint32)
    img[:npk] = est
    return _dev(img.view(np.uint8))


def _rows_image(rows, npk):
    """Four rows of npk estimates (None: a row that is left alone), canaries behind each: (bytes on the device, row stride)."""
    stride = (npk + 2 + 3) // 4 * 4
    img = np.full((4, stride), CANARY32, dtype=np.uint32)
    for j, row in enumerate(rows):
        if row is not None:
            img[j, :npk] = row
    return _dev(img.view(np.uint8).reshape(-1)), stride


def _as_est(buf):
    return buf.view(torch.int32)


def _as_rows(buf, stride):
    return buf.view(torch.int32).view(4, stride)


def _host_input(i):
    w, (source, kind), n = WORKLOADS[i]
    if source == "typed":
        return np.ascontiguousarray(P.typed_input(kind, n + 8, seed=100 + i)[:n])
    return D.bytes_of(kind, n, w, seed=100 + i)


def _describe(i, what):
    w, (_source, kind), n = WORKLOADS[i]
    return f"stream {i}: {what}, width {w}, {kind} {n} bytes ({(n + PACKET - 1) // PACKET} packets)"


@pytest.fixture(scope="module")
def W(H):
    """Each workload: its bytes, its XOR base, and the references of every single-buffer entry point at the workload's width
    (survey_delta at the stream's mask) as images on the device, canaries behind them.  The XOR survey has a base of its own
    (`xbase`, _survey_base): against the uniform base of the filters every packet of the XORed bytes is alike."""
    ws = []
    for i, (w, _kind, n) in enumerate(WORKLOADS):
        x = _host_input(i)
        assert x.size == n
        _other, b = X.pair(n, 500 + i)
        npk = H.packet_count(n)
        raw = x.tobytes()
        base = np.zeros(_r16(n), dtype=np.uint8)
        base[:n] = b
        sp_img, stride = _rows_image(H.survey_planes_host(raw), npk)
        sd_img, _stride = _rows_image(H.survey_delta_host(raw, MASKS[i]), npk)
        xb = _survey_base(x, 700 + i)
        xe, xs = H.survey_xor_host(raw, xb.tobytes())
        ws.append(dict(i=i, w=w, n=n, npk=npk, S=_r16(n) + GUARD, host=x, base=_dev(base), stride=stride,
                       img=dict(x=_image(x), planes=_image(P.numpy_split(x, w)), delta=_image(D.numpy_split_delta(x, w)),
                                xor=_image(X.numpy_split_xor(x, b, w))),
                       est=_est_image(H.estimate_host(raw), npk), sp=sp_img, sd=sd_img,
                       xbase=_image(xb), xe=_rows_image(xe, npk)[0], xs=_rows_image(xs, npk)[0]))
    torch.cuda.synchronize()
    return ws


def _survey_base(x, seed):
    """A base for the XOR survey of x (tests/test_gpu_xor_survey.py::_base_of): independent uniform bytes in the first half of every
    third half-packet, x elsewhere -- so that the XORed bytes have packets that are all zeros, half zeros and, at the wider widths,
    neither, and the scan rows are not one word throughout."""
    b = x.copy()
    pick = (np.arange(x.size) // (PACKET // 2)) % 3 == 0
    b[pick] = np.random.default_rng([71, seed]).integers(0, 256, x.size, dtype=np.uint8)[pick]
    return b


def _layout(sizes):
    at, offs = 0, []
    for n in sizes:
        offs.append(at)
        at += (n + GUARD + 15) // 16 * 16
    return offs, at


class Batch:
    """A dozen buffers in one arena (tests/test_gpu_delta.py::_layout: GUARD canaries behind each): an empty one, the packet
    boundaries, groups and tails, mixed widths, filter flags and bases; `extra`: one more buffer (bytes, base bytes, width).
    `bad`: buffer BAD carries an unusable descriptor -- "planes": width 3; "delta": filter word 2; "xor": a base pointer that
    is 8 mod 16; "ptr": a buffer pointer that is 8 mod 16 (for the calls that only read); "base_ptr": a base pointer of the XOR
    survey that is 8 mod 16 -- and the references leave it alone.  The XOR survey reads the bases of the filter through base
    pointers of its own (xbase_ptrs): 0, which is "no base", for the buffers without one and for every third buffer besides.  Every
    second base is a _survey_base of its buffer, the others are uniform bytes.
    Descriptors on the device; references as arena images."""

    def __init__(self, H, seed, mask, extra=None, bad=None):
        rng = np.random.default_rng([61, seed])
        sizes = [0, 1, 15, 17, 8191, 8192, 8193, 2 * PACKET + 5, 65536, 65537, 3 * 65536 + 4097, int(rng.integers(1, 200000))]
        widths = [8, 2, 8, 2, 4, 4, 1, 2, 8, 1, 8, 4]
        filt = [1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0]
        based = [1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1]
        hosts = [D.bytes_of(D.KINDS[(seed + b) % 3], n, widths[b], seed=1000 * seed + b) for b, n in enumerate(sizes)]
        bases = [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]
        bases = [_survey_base(h, 1000 * seed + b) if b % 2 == 0 else q for b, (h, q) in enumerate(zip(hosts, bases))]
        if extra is not None:
            hosts.append(extra[0])
            bases.append(extra[1])
            sizes.append(extra[0].size)
            widths.append(extra[2])
            filt.append(1)
            based.append(1)
        self.n, self.sizes, self.widths, self.filt, self.based, self.hosts, self.bad = len(sizes), sizes, widths, filt, based, hosts, bad
        self.offs, self.total = _layout(sizes)
        self.fp, self.npk = H.batch_packet_count(sizes)
        self.base = self._arena(bases, fill=0)
        self.src = self._arena(hosts)
        want = dict(planes=[P.numpy_split(h, w) for h, w in zip(hosts, widths)],
                    delta=[D.numpy_split_delta(h, w) if f else P.numpy_split(h, w) for h, w, f in zip(hosts, widths, filt)],
                    xor=[X.numpy_split_xor(h, q, w) if f else P.numpy_split(h, w) for h, q, w, f in zip(hosts, bases, widths, based)])
        skip = BAD if bad else None
        self.split = {fam: self._arena(want[fam], skip) for fam in FAMILIES}
        self.merged = self._arena(hosts, skip)                     # what merging `split` in place leaves
        self.xbased = [bool(f) and b % 3 != 2 for b, f in enumerate(based)]
        assert self.xbased[BAD] and True in self.xbased[:BAD] and False in self.xbased[BAD + 1:]
        est, sp, sd, xe, xs = [], [[], [], [], []], [[], [], [], []], [[], [], [], []], [[], [], [], []]
        for b, h in enumerate(hosts):
            mine = self.fp[b + 1] - self.fp[b]
            left = b == skip
            est += [CANARY32] * mine if left else H.estimate_host(h.tobytes())
            xor = H.survey_xor_host(h.tobytes(), (bases[b] if self.xbased[b] else np.zeros_like(h)).tobytes())
            for rows, got in ((sp, H.survey_planes_host(h.tobytes())), (sd, H.survey_delta_host(h.tobytes(), mask)), (xe, xor[0]), (xs, xor[1])):
                for j in range(4):
                    rows[j] += [CANARY32] * mine if left or got[j] is None else got[j]
        self.xe, self.xs = _rows_image(xe, self.npk)[0], _rows_image(xs, self.npk)[0]
        self.mask = mask
        self.est = _est_image(est, self.npk)
        self.sp, self.stride = _rows_image(sp, self.npk)
        self.sd, _stride = _rows_image([row if w in mask else None for w, row in zip(WIDTHS, sd)], self.npk)
        if bad == "planes":
            widths = widths[:BAD] + [3] + widths[BAD + 1:]
        if bad == "delta":
            filt = filt[:BAD] + [2] + filt[BAD + 1:]
        base_ptrs = [self.base.data_ptr() + o if f else 0 for o, f in zip(self.offs, based)]
        if bad == "xor":
            base_ptrs[BAD] += 8
        desc = torch.tensor(sizes + self.fp + widths + filt + base_ptrs, dtype=torch.int64, device="cuda")
        n = self.n
        self.d_bytes, self.d_fp, self.d_w, self.d_filt, self.d_base = desc[:n], desc[n:2 * n + 1], desc[2 * n + 1:3 * n + 1], \
            desc[3 * n + 1:4 * n + 1], desc[4 * n + 1:]

    def _arena(self, hosts, skip=None, fill=CANARY):
        img = np.full(self.total, fill, dtype=np.uint8)
        for b, (o, h) in enumerate(zip(self.offs, hosts)):
            if b != skip:
                img[o:o + h.size] = h
        return _dev(img)

    def ptrs(self, arena):
        """The buffers' pointers in `arena` (bad="ptr": buffer BAD's is misaligned)."""
        p = [arena.data_ptr() + o for o in self.offs]
        if self.bad == "ptr":
            p[BAD] += 8
        return torch.tensor(p, dtype=torch.int64, device="cuda")

    def xbase_ptrs(self, arena):
        """The XOR survey's base pointers into `arena`, which holds the bases as self.base does: 0 where xbased says none
        (bad="base_ptr": buffer BAD's is misaligned)."""
        p = [arena.data_ptr() + o if f else 0 for o, f in zip(self.offs, self.xbased)]
        if self.bad == "base_ptr":
            p[BAD] += 8
        return torch.tensor(p, dtype=torch.int64, device="cuda")

    def describe(self):
        return f"a batch of {self.n} buffers, {sum(self.sizes)} bytes ({self.npk} packets)"


class Moves:
    """Regions of 1 .. 8192 bytes, in shuffled order, from 8192-byte cells of a seeded source to a destination arena with GUARD
    canaries behind each; `bad`: region 5 is 8193 bytes long, which is BAD_BATCH, and is skipped."""

    def __init__(self, seed, regions, bad=False):
        rng = np.random.default_rng([67, seed])
        sizes = [1, 15, 16, 17, 8191, 8192] + [int(v) for v in rng.integers(1, PACKET + 1, regions - 6)]
        sizes = [sizes[j] for j in rng.permutation(regions)]
        if bad:
            sizes[5] = PACKET + 1
        cells = rng.permutation(regions)
        host = rng.integers(0, 256, regions * PACKET + 16, dtype=np.uint8)
        self.src = _dev(host)
        self.offs, self.total = _layout(sizes)
        img = np.full(self.total, CANARY, dtype=np.uint8)
        for r, (o, n) in enumerate(zip(self.offs, sizes)):
            if n <= PACKET:
                img[o:o + n] = host[int(cells[r]) * PACKET:int(cells[r]) * PACKET + n]
        self.want = _dev(img)
        self.n, self.sizes, self.bad = regions, sizes, bad
        self.dst = _blank(self.total)
        self.desc = torch.tensor([self.src.data_ptr() + int(c) * PACKET for c in cells] + [self.dst.data_ptr() + o for o in self.offs] + sizes,
                                 dtype=torch.int64, device="cuda")

    def run(self, H, stream, word):
        n = self.n
        H.move_packets(self.desc[:n], self.desc[n:2 * n], self.desc[2 * n:], n, stream=stream, d_status=word)

    def describe(self):
        return f"move_packets, {self.n} regions, {sum(self.sizes)} bytes"


def _single(H, fam, merge, k, src, dst, stream):
    """split_<fam> / merge_<fam> of workload k's n bytes from src to dst (the same tensor: in place)."""
    f = getattr(H, ("merge_" if merge else "split_") + fam)
    if fam == "xor":
        f(src, k["base"], k["w"], d_out=dst, n_bytes=k["n"], stream=stream)
    else:
        f(src, k["w"], d_out=dst, n_bytes=k["n"], stream=stream)


def _batched(H, fam, merge, bt, d_in, d_out, stream, word):
    """split_<fam>_batch / merge_<fam>_batch of batch bt from the pointers d_in to the pointers d_out."""
    f = getattr(H, ("merge_" if merge else "split_") + fam + "_batch")
    more = {"planes": [], "delta": [bt.d_filt], "xor": [bt.d_base]}[fam]
    f(d_in, bt.d_bytes, bt.d_fp, bt.d_w, *more, bt.n, bt.npk, d_out, stream=stream, d_status=word)


# ---------------------------------------------------------------------------------------------------------------------
# 1. stream order
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One call under test: `feeds` [(image, buffer)]: the copies that put its inputs in place; run(stream, word) enqueues it;
    `outs` [(buffer, the image it must equal afterwards)].  The buffers are shared by the cases of a workload and refilled."""

    def __init__(self, name, feeds, run, outs):
        self.name, self.feeds, self.run, self.outs = name, feeds, run, outs

    def reset(self):
        for _image, buf in self.feeds:
            buf.fill_(CANARY)
        for buf, _want in self.outs:
            buf.fill_(CANARY)


def _cases(H, k, bt, mv):
    """Every new entry point on workload k (single-buffer forms), on the batch bt that holds it (batch forms) and on the moves
    mv: out of place and, where allowed, in place."""
    S, n, tag = k["S"], k["n"], f"workload {k['i']} (width {k['w']}, {k['n']} bytes)"
    a, b = _blank(S), _blank(S)
    A, B = _blank(bt.total), _blank(bt.total)
    e, rows = _blank(k["est"].numel()), _blank(k["sp"].numel())
    E, ROWS = _blank(bt.est.numel()), _blank(bt.sp.numel())
    pa, pb = bt.ptrs(A), bt.ptrs(B)
    xe, xs, XE, XS = _blank(k["xe"].numel()), _blank(k["xs"].numel()), _blank(bt.xe.numel()), _blank(bt.xs.numel())
    xb = bt.xbase_ptrs(B)                                      # (the survey's bases stand in B, fed like the buffers in A)
    cases = []
    for fam in FAMILIES:
        for merge in (False, True):
            name = ("merge_" if merge else "split_") + fam
            before, after = (k["img"][fam], k["img"]["x"]) if merge else (k["img"]["x"], k["img"][fam])
            cases.append(Case(f"{name}, {tag}", [(before, a)], lambda s, _w, fam=fam, merge=merge: _single(H, fam, merge, k, a, b, s), [(b, after)]))
            cases.append(Case(f"{name} in place, {tag}", [(before, a)], lambda s, _w, fam=fam, merge=merge: _single(H, fam, merge, k, a, a, s),
                              [(a, after)]))
            before, after = (bt.split[fam], bt.src) if merge else (bt.src, bt.split[fam])
            cases.append(Case(f"{name}_batch, {bt.describe()} with {tag}", [(before, A)],
                              lambda s, word, fam=fam, merge=merge: _batched(H, fam, merge, bt, pa, pb, s, word), [(B, after)]))
            cases.append(Case(f"{name}_batch in place, {bt.describe()} with {tag}", [(before, A)],
                              lambda s, word, fam=fam, merge=merge: _batched(H, fam, merge, bt, pa, pa, s, word), [(A, after)]))
    cases += [
        Case(f"estimate, {tag}", [(k["img"]["x"], a)], lambda s, _w: H.estimate(a, n_bytes=n, d_est=_as_est(e), stream=s), [(e, k["est"])]),
        Case(f"survey_planes, {tag}", [(k["img"]["x"], a)],
             lambda s, _w: H.survey_planes(a, d_est=_as_rows(rows, k["stride"]), n_bytes=n, stream=s), [(rows, k["sp"])]),
        Case(f"survey_delta widths {MASKS[k['i']]}, {tag}", [(k["img"]["x"], a)],
             lambda s, _w: H.survey_delta(a, d_est=_as_rows(rows, k["stride"]), n_bytes=n, stream=s, widths=MASKS[k["i"]]), [(rows, k["sd"])]),
        Case(f"estimate_batch, {bt.describe()} with {tag}", [(bt.src, A)],
             lambda s, word: H.estimate_batch(pa, bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_est(E), stream=s, d_status=word), [(E, bt.est)]),
        Case(f"survey_planes_batch, {bt.describe()} with {tag}", [(bt.src, A)],
             lambda s, word: H.survey_planes_batch(pa, bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_rows(ROWS, bt.stride), stream=s, d_status=word),
             [(ROWS, bt.sp)]),
        Case(f"survey_delta_batch widths {bt.mask}, {bt.describe()} with {tag}", [(bt.src, A)],
             lambda s, word: H.survey_delta_batch(pa, bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_rows(ROWS, bt.stride), stream=s, d_status=word,
                                                  widths=bt.mask), [(ROWS, bt.sd)]),
        Case(f"survey_xor, {tag}", [(k["img"]["x"], a), (k["xbase"], b)],
             lambda s, _w: H.survey_xor(a, b, d_est=_as_rows(xe, k["stride"]), d_scan=_as_rows(xs, k["stride"]), n_bytes=n, stream=s),
             [(xe, k["xe"]), (xs, k["xs"])]),
        Case(f"survey_xor_batch, {bt.describe()} with {tag}", [(bt.src, A), (bt.base, B)],
             lambda s, word: H.survey_xor_batch(pa, bt.d_bytes, bt.d_fp, xb, bt.n, bt.npk, d_est=_as_rows(XE, bt.stride),
                                                d_scan=_as_rows(XS, bt.stride), stream=s, d_status=word), [(XE, bt.xe), (XS, bt.xs)]),
    ]
    # move_packets reads its own source, which the producer fills from a copy of it
    image = mv.src.clone()
    cases.append(Case(f"{mv.describe()}, beside {tag}", [(image, mv.src)], lambda s, word: mv.run(H, s, word), [(mv.dst, mv.want)]))
    return cases


@pytest.fixture(scope="module")
def producer(H):
    """The producer's scratch buffers and what one link costs: (source, destination, GPU seconds per link by events, host seconds
    per link to enqueue)."""
    p, q = torch.zeros(LINK, dtype=torch.uint8, device="cuda"), torch.empty(LINK, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    for _ in range(4):
        H.device_copy(p, q, stream=s)
    s.synchronize()
    links = 32
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    t0 = time.perf_counter()
    for _ in range(links):
        H.device_copy(p, q, stream=s)
    host = (time.perf_counter() - t0) / links
    e1.record(s)
    s.synchronize()
    gpu = e0.elapsed_time(e1) * 1e-3 / links
    print(f"producer link of {LINK >> 20} MiB: {gpu * 1e6:.1f} us on the GPU, {host * 1e6:.1f} us of host time to enqueue")
    assert gpu > 8 * host, f"a producer link runs {gpu * 1e6:.1f} us and takes {host * 1e6:.1f} us to enqueue: no chain of them outlasts its own enqueue"
    return p, q, gpu, host


def _links(producer, call_host):
    """How many links outlast four times the enqueue of the chain and of a call that took call_host seconds to enqueue."""
    _p, _q, gpu, host = producer
    return min(MAX_LINKS, max(MIN_LINKS, math.ceil(4 * call_host / (gpu - 4 * host))))


def _enqueue_behind_producer(H, producer, s, case, word, stream_of_call, links):
    """The producer (`links` links), the case's feeds, the call (on stream_of_call) and the copies of its outputs, enqueued on s
    (None: the current stream) without a synchronisation: (the copies, whether the producer was still pending after the last
    enqueue, the host seconds the enqueue took)."""
    p, q = producer[:2]
    case.reset()
    results = [torch.full_like(buf, 0x3C) for buf, _want in case.outs]
    behind_producer = torch.cuda.Event()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(links):
        H.device_copy(p, q, stream=s)
    for image, buf in case.feeds:
        H.device_copy(image, buf, stream=s)
    behind_producer.record(s if s is not None else torch.cuda.current_stream())
    case.run(stream_of_call, word)
    for (buf, _want), r in zip(case.outs, results):
        H.device_copy(buf, r, stream=s)
    pending = not behind_producer.query()
    return results, pending, time.perf_counter() - t0


@pytest.mark.parametrize("i", [2, 6])
def test_stream_order(H, W, producer, i):
    """Every new entry point reads what the work in front of it on ITS stream wrote and is read by what comes behind it there.
    Serial pass: feeds, call, synchronise, against the references; its enqueue is timed.  Ordered pass: see the module
    docstring.  A call that is not on `stream=` fails its own check here; a producer that is over before the last enqueue
    fails the test as inconclusive."""
    k = W[i]
    bt = Batch(H, 40 + i, MASKS[i], extra=(k["host"], k["base"][:k["n"]].cpu().numpy(), k["w"]))
    mv = Moves(40 + i, 64 if i == 2 else 1024)
    cases = _cases(H, k, bt, mv)
    words = _status(2 * len(cases))
    s, other = _streams(2)
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    H.device_copy(producer[0][:4096], producer[1][:4096], stream=s)          # (the streams' first launches are not timed)
    H.device_copy(producer[0][:4096], producer[1][:4096], stream=other)
    torch.cuda.synchronize()
    verdicts, short, slowest = [], [], 0.0
    for c, case in enumerate(cases):
        results, _pending, call_host = _enqueue_behind_producer(H, producer, None, case, words[2 * c:2 * c + 1], None, 0)
        torch.cuda.synchronize()
        slowest = max(slowest, call_host)
        for j, ((buf, want), r) in enumerate(zip(case.outs, results)):
            verdicts.append((f"{case.name} (serial): output {j} differs from the reference or its canaries are gone", _same(buf, want) & _same(r, want)))
        links = _links(producer, call_host)
        results, pending, _host = _enqueue_behind_producer(H, producer, s, case, words[2 * c + 1:2 * c + 2], s, links)
        s.synchronize()
        if not pending:
            short.append(f"{case.name} ({links} links for an enqueue of {call_host * 1e6:.0f} us)")
        for j, ((_buf, want), r) in enumerate(zip(case.outs, results)):
            verdicts.append((f"{case.name}: behind a producer on its stream, output {j} differs from the serial result "
                             "(the call did not run on stream=, or wrote behind its output)", _same(r, want)))
    # the control: the same enqueue with the call on another stream must NOT give the serial result
    control = cases[0]
    results, pending, _host = _enqueue_behind_producer(H, producer, s, control, None, other, _links(producer, slowest))
    torch.cuda.synchronize()
    control_differs = bool((~_same(results[0], control.outs[0][1])).item())
    print(f"slowest enqueue of a call with its feeds and copies: {slowest * 1e6:.0f} us")
    if not pending:
        short.append(f"the control ({control.name} on another stream)")
    assert not short, f"producer too short: it was over before the last enqueue of {len(short)} calls, which proves nothing: " + "; ".join(short[:8])
    assert control_differs, f"producer too short: the control ({control.name} enqueued on ANOTHER stream) gave the serial result"
    _words(verdicts, words, [0] * (2 * len(cases)), [f"{case.name}{tag}" for case in cases for tag in (" (serial)", "")])
    _fail_on(verdicts)
    assert H.status() == 0, "a launch reported into the fallback word"


# ---------------------------------------------------------------------------------------------------------------------
# 2. fan-out with status isolation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_filter_fan_out(H, W, fam):
    """split_<fam> into a guarded buffer, a copy of it, merge_<fam> of the copy in place, and the same through the batch forms
    over a dozen buffers, on each of eight streams at once.  Stream 1's batch has one unusable descriptor (width 3 / filter
    word 2 / a base pointer that is 8 mod 16): BAD_BATCH in its two words and in no other, that buffer's output keeps its
    canary, every other byte of every stream equals the serial result, nothing is written behind any buffer."""
    k8 = len(W)
    bts = [Batch(H, 10 + i, MASKS[i], bad=fam if i == 1 else None) for i in range(k8)]
    bufs = [dict(b=_blank(k["S"]), c=_blank(k["S"]), B=_blank(bt.total), C=_blank(bt.total)) for k, bt in zip(W, bts)]
    for bt, u in zip(bts, bufs):
        u["src"], u["pB"], u["pC"] = bt.ptrs(bt.src), bt.ptrs(u["B"]), bt.ptrs(u["C"])
    words = _status(4 * k8)

    def chain(i, s, word, sync):
        k, bt, u = W[i], bts[i], bufs[i]
        steps = [
            lambda: _single(H, fam, False, k, k["img"]["x"], u["b"], s),
            lambda: H.device_copy(u["b"], u["c"], stream=s),
            lambda: _single(H, fam, True, k, u["c"], u["c"], s),
            lambda: _batched(H, fam, False, bt, u["src"], u["pB"], s, word[0:1]),
            lambda: H.device_copy(u["B"], u["C"], stream=s),
            lambda: _batched(H, fam, True, bt, u["pC"], u["pC"], s, word[1:2]),
        ]
        for step in steps:
            step()
            if sync:
                torch.cuda.synchronize()

    def check(tag, against):
        v = []
        for i, (k, bt, u) in enumerate(zip(W, bts, bufs)):
            v += [(f"{_describe(i, 'split_' + fam)}{tag}: differs from {against} or wrote behind its n bytes", _same(u["b"], k["img"][fam])),
                  (f"{_describe(i, 'merge_' + fam + ' in place')}{tag}: differs from {against} or wrote behind its n bytes", _same(u["c"], k["img"]["x"])),
                  (f"stream {i}: split_{fam}_batch, {bt.describe()}{tag}: a buffer or a guard differs from {against}", _same(u["B"], bt.split[fam])),
                  (f"stream {i}: merge_{fam}_batch in place, {bt.describe()}{tag}: a buffer or a guard differs from {against}",
                   _same(u["C"], bt.merged))]
        return v

    verdicts = []
    for i in range(k8):
        chain(i, None, words[2 * i:2 * i + 2], True)
    verdicts += check(" (serial)", "the reference")
    for u in bufs:
        for name in ("b", "c", "B", "C"):
            u[name].fill_(CANARY)
    streams = _streams(k8)
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        chain(i, s, words[2 * (k8 + i):2 * (k8 + i) + 2], False)
    torch.cuda.synchronize()
    verdicts += check("", "the serial result")
    expected = [H.STATUS_BAD_BATCH if i == 1 else 0 for i in range(k8) for _ in range(2)] * 2
    _words(verdicts, words, expected, [f"stream {i % k8}: {name}_{fam}_batch{' (serial)' if i < k8 else ''}" for i in range(2 * k8)
                                       for name in ("split", "merge")])
    _fail_on(verdicts)
    assert H.status() == 0, f"{fam}: a launch reported into the fallback word"


def test_estimate_and_survey_fan_out(H, W):
    """estimate, survey_planes and survey_delta (a different widths mask per stream), single and batch forms, on each of eight
    streams at once, into rows with canaries behind them.  The rows a mask leaves out keep their canary.  Stream 1's batch has
    a buffer pointer that is 8 mod 16: BAD_BATCH in its three words and in no other, and that buffer's columns keep the canary."""
    k8 = len(W)
    bts = [Batch(H, 20 + i, MASKS[i], bad="ptr" if i == 1 else None) for i in range(k8)]
    names = ("e", "sp", "sd", "E", "SP", "SD")
    bufs = []
    for k, bt in zip(W, bts):
        wants = dict(e=k["est"], sp=k["sp"], sd=k["sd"], E=bt.est, SP=bt.sp, SD=bt.sd)
        bufs.append(dict(want=wants, src=bt.ptrs(bt.src), **{name: _blank(wants[name].numel()) for name in names}))
    words = _status(6 * k8)

    def chain(i, s, word, sync):
        k, bt, u = W[i], bts[i], bufs[i]
        x, n = k["img"]["x"], k["n"]
        steps = [
            lambda: H.estimate(x, n_bytes=n, d_est=_as_est(u["e"]), stream=s),
            lambda: H.survey_planes(x, d_est=_as_rows(u["sp"], k["stride"]), n_bytes=n, stream=s),
            lambda: H.survey_delta(x, d_est=_as_rows(u["sd"], k["stride"]), n_bytes=n, stream=s, widths=MASKS[i]),
            lambda: H.estimate_batch(u["src"], bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_est(u["E"]), stream=s, d_status=word[0:1]),
            lambda: H.survey_planes_batch(u["src"], bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_rows(u["SP"], bt.stride), stream=s,
                                          d_status=word[1:2]),
            lambda: H.survey_delta_batch(u["src"], bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_rows(u["SD"], bt.stride), stream=s,
                                         d_status=word[2:3], widths=MASKS[i]),
        ]
        for step in steps:
            step()
            if sync:
                torch.cuda.synchronize()

    calls = ("estimate", "survey_planes", "survey_delta", "estimate_batch", "survey_planes_batch", "survey_delta_batch")

    def check(tag, against):
        return [(f"{_describe(i, call)}{', ' + bts[i].describe() if call.endswith('batch') else ''}, widths {MASKS[i]}{tag}: "
                 f"differs from {against}, or a canary behind a row or in a row or column that is left alone is gone", _same(u[name], u["want"][name]))
                for i, u in enumerate(bufs) for name, call in zip(names, calls)]

    verdicts = []
    for i in range(k8):
        chain(i, None, words[3 * i:3 * i + 3], True)
    verdicts += check(" (serial)", "the reference")
    for u in bufs:
        for name in names:
            u[name].fill_(CANARY)
    streams = _streams(k8)
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        chain(i, s, words[3 * (k8 + i):3 * (k8 + i) + 3], False)
    torch.cuda.synchronize()
    verdicts += check("", "the serial result")
    expected = [H.STATUS_BAD_BATCH if i == 1 else 0 for i in range(k8) for _ in range(3)] * 2
    _words(verdicts, words, expected, [f"stream {i % k8}: {call}{' (serial)' if i < k8 else ''}" for i in range(2 * k8) for call in calls[3:]])
    _fail_on(verdicts)
    assert H.status() == 0, "the single-buffer forms report into the fallback word and had nothing to report"


def test_survey_xor_fan_out(H, W):
    """survey_xor and survey_xor_batch on each of eight streams at once, into est and scan rows with canaries behind them.  Stream i
    asks for both outputs, for the est rows alone or for the scan rows alone, by i mod 3: the output that was not asked for keeps
    every canary under contention too.  Stream 1's batch has a base pointer that is 8 mod 16: BAD_BATCH in its word and in no
    other, and that buffer's columns keep the canary in both outputs.  Buffers whose base pointer is 0 get the rows of their
    own bytes."""
    k8 = len(W)
    bts = [Batch(H, 20 + i, MASKS[i], bad="base_ptr" if i == 1 else None) for i in range(k8)]
    names = ("xe", "xs", "XE", "XS")
    asked = [(i % 3 != 2, i % 3 != 1) for i in range(k8)]                     # (est rows, scan rows)
    assert asked[:3] == [(True, True), (True, False), (False, True)]
    bufs = []
    for i, (k, bt) in enumerate(zip(W, bts)):
        wants = dict(xe=k["xe"], xs=k["xs"], XE=bt.xe, XS=bt.xs)
        for name in names:
            if not asked[i][name in ("xs", "XS")]:
                wants[name] = _blank(wants[name].numel())
        bufs.append(dict(want=wants, src=bt.ptrs(bt.src), xbase=bt.xbase_ptrs(bt.base), **{name: _blank(wants[name].numel()) for name in names}))
    words = _status(2 * k8)

    def chain(i, s, word, sync):
        k, bt, u = W[i], bts[i], bufs[i]
        est, scan = asked[i]
        steps = [
            lambda: H.survey_xor(k["img"]["x"], k["xbase"], d_est=_as_rows(u["xe"], k["stride"]) if est else False,
                                 d_scan=_as_rows(u["xs"], k["stride"]) if scan else False, n_bytes=k["n"], stream=s),
            lambda: H.survey_xor_batch(u["src"], bt.d_bytes, bt.d_fp, u["xbase"], bt.n, bt.npk, d_est=_as_rows(u["XE"], bt.stride) if est else False,
                                       d_scan=_as_rows(u["XS"], bt.stride) if scan else False, stream=s, d_status=word),
        ]
        for step in steps:
            step()
            if sync:
                torch.cuda.synchronize()

    def check(tag, against):
        return [(f"{_describe(i, call)}{', ' + bts[i].describe() if call.endswith('batch') else ''}, {what} rows "
                 f"({'asked for' if asked[i][what == 'scan'] else 'NOT asked for'}){tag}: differs from {against}, or a canary behind a row, in "
                 "a column that is left alone or in an output that was not asked for is gone", _same(u[name], u["want"][name]))
                for i, u in enumerate(bufs) for name, call, what in zip(names, ("survey_xor", "survey_xor", "survey_xor_batch", "survey_xor_batch"),
                                                                        ("est", "scan", "est", "scan"))]

    verdicts = []
    for i in range(k8):
        chain(i, None, words[i:i + 1], True)
    verdicts += check(" (serial)", "the reference")
    for u in bufs:
        for name in names:
            u[name].fill_(CANARY)
    streams = _streams(k8)
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        chain(i, s, words[k8 + i:k8 + i + 1], False)
    torch.cuda.synchronize()
    verdicts += check("", "the serial result")
    expected = [H.STATUS_BAD_BATCH if i == 1 else 0 for i in range(k8)] * 2
    _words(verdicts, words, expected, [f"stream {i % k8}: survey_xor_batch{' (serial)' if i < k8 else ''}" for i in range(2 * k8)])
    _fail_on(verdicts)
    assert H.status() == 0, "survey_xor reports into the fallback word and had nothing to report"


def _move_sets():
    return [Moves(30 + i, 64 if i < 4 else 1024, bad=i == 1) for i in range(8)]


def test_move_packets_fan_out(H):
    """move_packets on eight streams at once, each a shuffled set of regions of 1 .. 8192 bytes (64 or 1024 of them).  Stream 1
    has one region of 8193 bytes: BAD_BATCH in its word and in no other, that region is not written, every other region of
    every stream arrives byte-exact and nothing is written behind any of them."""
    sets = _move_sets()
    k8 = len(sets)
    words = _status(2 * k8)
    verdicts = []
    for i, mv in enumerate(sets):
        mv.run(H, None, words[i:i + 1])
        torch.cuda.synchronize()
        verdicts.append((f"stream {i}: {mv.describe()} (serial): a region or a guard differs from the reference", _same(mv.dst, mv.want)))
        mv.dst.fill_(CANARY)
    streams = _streams(k8)
    torch.cuda.synchronize()
    for i, (mv, s) in enumerate(zip(sets, streams)):
        mv.run(H, s, words[k8 + i:k8 + i + 1])
    torch.cuda.synchronize()
    for i, mv in enumerate(sets):
        verdicts.append((f"stream {i}: {mv.describe()}: a region or a guard differs from the serial result", _same(mv.dst, mv.want)))
    expected = [H.STATUS_BAD_BATCH if i == 1 else 0 for i in range(k8)] * 2
    _words(verdicts, words, expected, [f"stream {i % k8}: move_packets{' (serial)' if i < k8 else ''}" for i in range(2 * k8)])
    _fail_on(verdicts)
    assert H.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the fallback status word
# ---------------------------------------------------------------------------------------------------------------------
def test_fallback_word_of_the_batch_entry_points(H):
    """Each batch entry point that can report BAD_BATCH -- split_ and merge_planes_batch, _delta_batch and _xor_batch,
    estimate_batch, survey_planes_batch, survey_delta_batch, survey_xor_batch (a base pointer that is 8 mod 16), move_packets --
    with d_status=None and one unusable descriptor, on a non-blocking stream, one after another: status() returns BAD_BATCH after
    the call and 0 when asked again.  The XOR survey's rows are compared too: the columns of the buffer with the unusable base keep
    their canary in both outputs."""
    s = torch.cuda.Stream()
    calls = []
    for fam in FAMILIES:
        bt = Batch(H, 50, WIDTHS, bad=fam)
        out = _blank(bt.total)
        d_in, d_out = bt.ptrs(bt.src), bt.ptrs(out)
        for merge in (False, True):
            calls.append((("merge_" if merge else "split_") + fam + "_batch",
                          lambda fam=fam, merge=merge, bt=bt, d_in=d_in, d_out=d_out: _batched(H, fam, merge, bt, d_in, d_out, s, None)))
    bt = Batch(H, 51, WIDTHS, bad="ptr")
    est, rows = _blank(bt.est.numel()), _blank(bt.sp.numel())
    src = bt.ptrs(bt.src)
    calls += [
        ("estimate_batch", lambda: H.estimate_batch(src, bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_est(est), stream=s, d_status=None)),
        ("survey_planes_batch", lambda: H.survey_planes_batch(src, bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_rows(rows, bt.stride), stream=s,
                                                              d_status=None)),
        ("survey_delta_batch", lambda: H.survey_delta_batch(src, bt.d_bytes, bt.d_fp, bt.n, bt.npk, d_est=_as_rows(rows, bt.stride), stream=s,
                                                            d_status=None)),
    ]
    xt = Batch(H, 53, WIDTHS, bad="base_ptr")
    xe, xs = _blank(xt.xe.numel()), _blank(xt.xs.numel())
    xsrc, xbase = xt.ptrs(xt.src), xt.xbase_ptrs(xt.base)
    calls.append(("survey_xor_batch", lambda: H.survey_xor_batch(xsrc, xt.d_bytes, xt.d_fp, xbase, xt.n, xt.npk, d_est=_as_rows(xe, xt.stride),
                                                                d_scan=_as_rows(xs, xt.stride), stream=s, d_status=None)))
    mv = Moves(52, 16, bad=True)
    calls.append(("move_packets", lambda: mv.run(H, s, None)))
    torch.cuda.synchronize()
    assert H.status() == 0
    seen = []
    for name, call in calls:
        call()
        seen.append((name, H.status(), H.status()))
    wrong = [f"{name}: status() gave {first:#x}, then {second:#x}" for name, first, second in seen if (first, second) != (H.STATUS_BAD_BATCH, 0)]
    assert not wrong, f"the fallback word after a launch without a word of its own (want {H.STATUS_BAD_BATCH:#x}, then 0): " + "; ".join(wrong)
    _fail_on([(f"survey_xor_batch without a status word: the {what} rows differ from the reference, or buffer {BAD}'s columns lost their canary",
               _same(got, want)) for what, got, want in (("est", xe, xt.xe), ("scan", xs, xt.xs))])
    # and the other way round: the same launch with a word of its own reports there and leaves the fallback word alone
    word = _status(1)
    H.survey_xor_batch(xsrc, xt.d_bytes, xt.d_fp, xbase, xt.n, xt.npk, d_est=_as_rows(xe, xt.stride), d_scan=False, stream=s, d_status=word)
    assert (H.status(), int(word.item())) == (0, H.STATUS_BAD_BATCH), "survey_xor_batch with a status word of its own: the fallback word, the word"
    assert H.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. mixed co-residency
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["encoder_first", "encoder_last"])
def test_mixed_co_residency(H, oracle, W, order):
    """The LDS-heavy kernels next to the encoder and to each other: a throughput encode of 256 MiB on stream A, survey_delta of
    workload 7 on B, estimate_batch over all eight inputs on C (128 KiB of LDS per workgroup), split_xor of workload 6 on D,
    merge_delta in place of workload 5 on E, move_packets on F, crc32_batch over all eight inputs on G, survey_xor_batch over all
    eight inputs against their survey bases (workloads 0 and 2: base pointer 0) on H; the encoder enqueued first or last.  Every output equals its serial result (pinned: the slots against the reference encoder on 64-packet
    windows, the CRCs against zlib.crc32, the rest against the references of the fixture) and every status word is 0."""
    from test_gpu_concurrency import _slots_equal, _windows
    n = 256 * MiB + 5 * PACKET + 13
    npk = H.packet_count(n)
    d_in = H.generate("text", 640, n)
    word = _status(4)
    want_slots = H.encode(d_in, d_status=word[0:1], mode="throughput")
    torch.cuda.synchronize()
    for a, b in _windows(npk):
        rows = want_slots[a * SLOT:b * SLOT].view(b - a, SLOT).cpu().numpy()
        got = np.concatenate([row[:int(row[0]) | int(row[1]) << 8] for row in rows])
        want = oracle.encode_stream(d_in[a * PACKET:min(b * PACKET, n)].cpu().numpy())
        assert np.array_equal(got, want), f"encode throughput, text {n} bytes (serial): packets {a}..{b - 1} differ from the reference encoder"
    sizes = [k["n"] for k in W]
    fp, bpk = H.batch_packet_count(sizes)
    desc = torch.tensor([k["img"]["x"].data_ptr() for k in W] + sizes + fp, dtype=torch.int64, device="cuda")
    nb = len(W)
    d_ptrs, d_bytes, d_fp = desc[:nb], desc[nb:2 * nb], desc[2 * nb:]
    est_want = torch.cat([_as_est(k["est"])[:k["npk"]] for k in W])
    crc_host = np.array([zlib.crc32(k["host"][p * PACKET:(p + 1) * PACKET].tobytes()) for k in W for p in range(k["npk"])], dtype=np.uint32)
    crc_want = _dev(crc_host.view(np.int32))
    est_serial = H.estimate_batch(d_ptrs, d_bytes, d_fp, nb, bpk, d_status=word[1:2])
    crc_serial = H.crc32_batch(d_ptrs, d_bytes, d_fp, nb, bpk, d_status=word[2:3])
    mv = Moves(70, 1024)
    mv.run(H, None, word[3:4])
    # the XOR survey over the eight inputs: base pointer 0 for workloads 0 and 2, whose rows are those of their own bytes
    d_xbase = torch.tensor([0 if k["i"] in (0, 2) else k["xbase"].data_ptr() for k in W], dtype=torch.int64, device="cuda")
    x_want = []
    for k in W:
        if k["i"] in (0, 2):
            x_want.append(H.survey_xor_host(k["host"].tobytes(), bytes(k["n"])))
        else:
            x_want.append([[[v & 0xFFFFFFFF for v in row] for row in _as_rows(k[name], k["stride"])[:, :k["npk"]].cpu().tolist()] for name in ("xe", "xs")])
    xe_want, xs_want = (_rows_image([sum((x[which][j] for x in x_want), []) for j in range(4)], bpk) for which in (0, 1))
    x_stride = xe_want[1]
    xword = _status(2)
    xe_serial, xs_serial = _blank(xe_want[0].numel()), _blank(xs_want[0].numel())
    H.survey_xor_batch(d_ptrs, d_bytes, d_fp, d_xbase, nb, bpk, d_est=_as_rows(xe_serial, x_stride), d_scan=_as_rows(xs_serial, x_stride),
                       d_status=xword[0:1])
    torch.cuda.synchronize()
    verdicts = [("estimate_batch over the eight inputs (serial): differs from estimate_host", _same(est_serial[:bpk], est_want)),
                ("crc32_batch over the eight inputs (serial): differs from zlib.crc32", _same(crc_serial[:bpk], crc_want)),
                (f"{mv.describe()} (serial): differs from the reference", _same(mv.dst, mv.want)),
                ("survey_xor_batch over the eight inputs (serial): est rows differ from survey_xor_host", _same(xe_serial, xe_want[0])),
                ("survey_xor_batch over the eight inputs (serial): scan rows differ from survey_xor_host", _same(xs_serial, xs_want[0]))]
    _words(verdicts, word, [0] * 4, ["encode (serial)", "estimate_batch (serial)", "crc32_batch (serial)", "move_packets (serial)"])
    mv.dst.fill_(CANARY)

    k7, k6, k5 = W[7], W[6], W[5]
    slots = torch.full((npk * SLOT,), 0xEE, dtype=torch.uint8, device="cuda")
    rows = _blank(k7["sd"].numel())
    est = _blank(_r16(4 * (bpk + 2)))
    xored = _blank(k6["S"])
    merged = k5["img"]["delta"].clone()
    crc = _blank(_r16(4 * (bpk + 2)))
    words = _status(4)
    xe, xs = _blank(xe_want[0].numel()), _blank(xs_want[0].numel())
    sA, sB, sC, sD, sE, sF, sG, sH = _streams(8)
    launches = [
        lambda: H.survey_delta(k7["img"]["x"], d_est=_as_rows(rows, k7["stride"]), n_bytes=k7["n"], stream=sB, widths=MASKS[7]),
        lambda: H.estimate_batch(d_ptrs, d_bytes, d_fp, nb, bpk, d_est=_as_est(est), stream=sC, d_status=words[1:2]),
        lambda: H.split_xor(k6["img"]["x"], k6["base"], k6["w"], d_out=xored, n_bytes=k6["n"], stream=sD),
        lambda: H.merge_delta(merged, k5["w"], d_out=merged, n_bytes=k5["n"], stream=sE),
        lambda: mv.run(H, sF, words[2:3]),
        lambda: H.crc32_batch(d_ptrs, d_bytes, d_fp, nb, bpk, d_crc=_as_est(crc), stream=sG, d_status=words[3:4]),
        lambda: H.survey_xor_batch(d_ptrs, d_bytes, d_fp, d_xbase, nb, bpk, d_est=_as_rows(xe, x_stride), d_scan=_as_rows(xs, x_stride), stream=sH,
                                   d_status=xword[1:2]),
    ]
    encoder = lambda: H.encode(d_in, slots, stream=sA, d_status=words[0:1], mode="throughput")
    launches = [encoder] + launches if order == "encoder_first" else launches + [encoder]
    torch.cuda.synchronize()
    for launch in launches:
        launch()
    torch.cuda.synchronize()
    verdicts += [
        (f"{order}: stream A: encode throughput, text {n} bytes ({npk} packets): slots differ from the serial slots", _slots_equal(slots, want_slots, npk)),
        (f"{order}: stream B: survey_delta of workload 7: rows or canaries differ from the serial result", _same(rows, k7["sd"])),
        (f"{order}: stream C: estimate_batch over the eight inputs: differs from the serial result, or wrote behind its {bpk} estimates",
         _same(_as_est(est)[:bpk], est_serial[:bpk]) & _as_est(est)[bpk:].eq(CANARY32 - (1 << 32)).all()),
        (f"{order}: stream D: split_xor of workload 6: differs from the serial result or wrote behind its n bytes", _same(xored, k6["img"]["xor"])),
        (f"{order}: stream E: merge_delta in place of workload 5: differs from the serial result or wrote behind its n bytes",
         _same(merged, k5["img"]["x"])),
        (f"{order}: stream F: {mv.describe()}: differs from the serial result", _same(mv.dst, mv.want)),
        (f"{order}: stream G: crc32_batch over the eight inputs: differs from the serial result, or wrote behind its {bpk} CRCs",
         _same(_as_est(crc)[:bpk], crc_serial[:bpk]) & _as_est(crc)[bpk:].eq(CANARY32 - (1 << 32)).all()),
        (f"{order}: stream H: survey_xor_batch over the eight inputs: rows differ from the serial result, or a canary behind a row is gone",
         _same(xe, xe_serial) & _same(xs, xs_serial)),
    ]
    _words(verdicts, xword, [0] * 2, ["survey_xor_batch (serial)", f"{order}: stream H: survey_xor_batch"])
    _words(verdicts, words, [0] * 4, [f"{order}: stream {s}: {f}" for s, f in (("A", "encode"), ("C", "estimate_batch"), ("F", "move_packets"),
                                                                              ("G", "crc32_batch"))])
    _fail_on(verdicts)
    assert H.status() == 0, "survey_delta, split_xor and merge_delta report into the fallback word and had nothing to report"


# ---------------------------------------------------------------------------------------------------------------------
# 5. the batch API from threads
# ---------------------------------------------------------------------------------------------------------------------
def _cut(a, n_bytes):
    """the first n_bytes bytes of a host array, as bytes"""
    return D.raw_bytes(a)[:n_bytes].copy()


def _thread_families():
    """Seven keyword families of batch.compress, each with its inputs as host arrays of their own type: [(name, arrays, bases or
    None, keywords)].  Every batch has an empty tensor, a one-byte tensor, PACKET and PACKET + 1 bytes, tensors from the tables
    of DESIGN.md 4.9 / 4.10 for which "auto" and "survey" decide each way (TABLE_DELTA_WINS, TABLE_BASE_WINS and the others),
    and one tensor of about 16 MiB."""
    tbl = {name: a for name, (a, _w) in D.table_inputs(1 << 16).items()}
    prs = X.table_pairs(1 << 17)
    big = P.typed_input("bf16", 16 * MiB + 2 * PACKET + 6, seed=7)
    big_base = big.copy()
    big_base[::64] ^= 1
    edge = P.typed_input("fp32", PACKET + 8, seed=8)
    small = [np.empty(0, dtype=np.float32), edge[:1].copy(), edge[:PACKET].copy(), edge[:PACKET + 1].copy()]
    bf16 = P.typed_input("bf16", 5 * PACKET + 334, seed=9).view(np.uint16)
    fp32 = P.typed_input("fp32", 9 * PACKET + 44, seed=10).view(np.float32)
    fams = []
    fams.append(("planes=auto, checksum", small + [bf16, fp32, tbl["csr_offsets"], tbl["int16_walk"], big.view(np.uint16)], None,
                 dict(planes="auto", checksum=True)))
    arrays = small + [_cut(tbl[name], 1 << 20) for name in ("csr_offsets", "fp32", "uniform", "int16_walk")] + [big]
    fams.append(("planes=[...], delta=[mixed], stored=auto", arrays, None,
                 dict(planes=[4, 2, 1, 8, 8, 4, 2, 2, 2], delta=[False, True, True, False, True, False, False, True, False], stored="auto")))
    arrays = small + [_cut(tbl[name], 1 << 20) for name in ("position_ids", "unordered_int64", "uint8_walk", "uniform", "timestamps")] + [big]
    fams.append(("planes=survey, delta=survey, checksum", arrays, None, dict(planes="survey", delta="survey", checksum=True)))
    names = ("step_1e-3", "one_percent", "unrelated", "uniform")
    arrays = small + [prs[name][0] for name in names] + [big]
    bases = [np.empty(0, dtype=np.float32), edge[1:2].copy(), None, edge[7:PACKET + 8].copy()] + [prs[name][1] for name in names] + [big_base]
    fams.append(("base=[...], base_auto, planes=2, checksum, stored=auto", arrays, bases,
                 dict(base_auto=True, planes=2, checksum=True, stored="auto")))
    arrays = small + [tbl[name] for name in ("csr_offsets", "timestamps", "unordered_int64")] + [_cut(tbl["fp32"], 1 << 18), big]
    fams.append(("planes=8, delta=auto", arrays, None, dict(planes=8, delta="auto")))
    arrays = small + [tbl["sorted_indices"], tbl["fp32"], big]
    sizes = [D.raw_bytes(a).size for a in arrays]
    mask = []
    for b, n in enumerate(sizes):
        mask += [b >= 5 and p % 3 == 1 for p in range((n + PACKET - 1) // PACKET)]       # (buffers 0-4 keep every packet coded)
    fams.append(("planes=4, stored=a fixed mask", arrays, None, dict(planes=4, stored=mask)))
    # width and base chosen together, raw and sparse packets counted: the inputs and bases of the base_auto family, and the big tensor
    # against a base from which every 64th byte differs by a bit: the host rule gives widths 2, 1, 2, 1 and 8 behind the four small
    # tensors, keeps three bases of five and drops two, and keeps 1793 of the big tensor's 2051 packets as sparse records
    arrays = small + [prs[name][0] for name in names] + [big]
    fams.append(("base=[...], base_auto=survey, planes=survey, stored=auto, sparse=auto", arrays, list(bases),
                 dict(base_auto="survey", planes="survey", stored="auto", sparse="auto")))
    return fams


def _tensor(a):
    """a host array on the device, as a tensor of its own type (uint16: the bits as bfloat16)"""
    if a.dtype == np.uint16:
        return _dev(a.view(np.int16)).view(torch.bfloat16)
    return _dev(a)


def _bytes_view(t):
    return t.view(torch.uint8).reshape(-1) if t.numel() else torch.empty(0, dtype=torch.uint8, device=t.device)


def _total(H, coded):
    return sum(H.estimate_host(coded.tobytes()))


def _kinds_of(H, coded, stored_on, sparse_on):
    """(kind, bytes it is kept in) of every packet of the bytes `coded`: hip.sparse_rule on the host estimate and the host scan word
    (without sparse: hip.stored_rule on the estimate) -- a sparse packet its record, a raw one its bytes, a coded one its estimate"""
    raw = coded.tobytes()
    est = H.estimate_host(raw)
    scan = H.sparse_scan_host(raw) if sparse_on else [None] * len(est)
    out = []
    for p, (e, s) in enumerate(zip(est, scan)):
        n = min(PACKET, coded.size - p * PACKET)
        kind = H.sparse_rule(s, e, n, stored_on) if sparse_on else int(stored_on and H.stored_rule(e, n))
        out.append((kind, H.sparse_len(s >> 8) if kind == H.KIND_SPARSE else n if kind == H.KIND_RAW else e))
    return out


def _host_rule(H, hosts, bases, kw, elem_sizes):
    """What the host rules make of a batch: (widths, filter flags or None, based or None, the bytes that are coded per buffer, the
    stored flags per packet or None -- with sparse="auto": the kinds) -- hip.choose_planes / choose_filter on the host surveys, the
    `+ n_packets` tie rule of delta="auto" and base_auto on host estimates, hip.stored_rule on the host estimate of the coded bytes;
    planes="survey" with base_auto="survey": hip.choose_filter on the totals of the numpy splits of the bytes as they are and
    XORed, every packet counted as hip.sparse_rule keeps it (a buffer without a base or without packets: hip.choose_planes of the
    first)."""
    n = len(hosts)
    npk = [H.packet_count(h.size) for h in hosts]
    planes, delta = kw.get("planes"), kw.get("delta")
    stored_on, sparse_on = kw.get("stored") == "auto", kw.get("sparse") == "auto"
    flags = based = None
    if planes == "survey" and kw.get("base_auto") == "survey":
        kept = lambda coded: sum(size for _kind, size in _kinds_of(H, coded, stored_on, sparse_on))
        widths, based = [], []
        for h, q, p in zip(hosts, bases, npk):
            plain = [kept(P.numpy_split(h, w)) for w in WIDTHS]
            if q is None or p == 0:
                choice = (H.choose_planes(plain, p), False)
            else:
                choice = H.choose_filter(plain, [kept(X.numpy_split_xor(h, q, w)) for w in WIDTHS], p)
            widths.append(choice[0])
            based.append(choice[1])
    elif planes == "survey" and delta == "survey":
        choice = [H.choose_filter(totals_of(H.survey_planes_host(h.tobytes()), h.size), totals_of(H.survey_delta_host(h.tobytes()), h.size), p)
                  for h, p in zip(hosts, npk)]
        widths, flags = [c[0] for c in choice], [c[1] for c in choice]
    elif planes == "auto":
        widths = [e if e in (2, 4, 8) else 1 for e in elem_sizes]
    else:
        widths = [planes] * n if isinstance(planes, int) else list(planes)
    if delta == "auto":
        flags = [p > 0 and _total(H, D.numpy_split_delta(h, w)) + p <= _total(H, P.numpy_split(h, w)) for h, w, p in zip(hosts, widths, npk)]
    elif isinstance(delta, list):
        flags = delta
    if bases is not None and based is None:
        based = [q is not None and p > 0 and _total(H, X.numpy_split_xor(h, q, w)) + p <= _total(H, P.numpy_split(h, w))
                 for h, q, w, p in zip(hosts, bases, widths, npk)]
    coded = []
    for b, (h, w) in enumerate(zip(hosts, widths)):
        if based is not None and based[b]:
            coded.append(X.numpy_split_xor(h, bases[b], w))
        elif flags is not None and flags[b]:
            coded.append(D.numpy_split_delta(h, w))
        else:
            coded.append(P.numpy_split(h, w))
    stored = kw.get("stored")
    if sparse_on:
        stored = [kind for c in coded for kind, _size in _kinds_of(H, c, stored_on, True)]
    elif isinstance(stored, str):
        stored = [H.stored_rule(e, min(PACKET, c.size - p * PACKET)) for c in coded for p, e in enumerate(H.estimate_host(c.tobytes()))]
    return widths, flags, based, coded, stored


def _same_or_none(a, b):
    if a is None or b is None:
        return torch.tensor(a is None and b is None, device="cuda")
    return _same(a, b)


def test_thread_batch_compress_families(H, oracle):
    """batch.compress(..., stream=s) then batch.decompress(c, stream=s) from seven threads at once, each with its own stream and
    one keyword family: the paths that allocate and free temporaries (the split copy, both halves of base_auto, the slots)
    between launches on a side stream while other threads do the same.  The serial pass pins every family: widths, filter
    flags, kept bases and the stored mask against the host rules, the first 64 packets of every buffer without a stored packet
    against the reference encoder on the host composition of the references, the CRCs against zlib.crc32 of the original
    bytes.  The concurrent pass reproduces stream, offsets, crc32, stored, raw, raw_offsets, sparse, sparse_offsets and the three
    host lists exactly,
    and every buffer round-trips."""
    from gpuar_amd import batch
    fams = _thread_families()
    runs = []
    for name, arrays, bases, kw in fams:
        tensors = [_tensor(a) for a in arrays]
        d_bases = None if bases is None else [None if q is None else _tensor(q) for q in bases]
        hosts = [D.raw_bytes(a) for a in arrays]
        host_bases = None if bases is None else [None if q is None else D.raw_bytes(q) for q in bases]
        runs.append(dict(name=name, tensors=tensors, bases=d_bases, hosts=hosts, host_bases=host_bases, kw=kw,
                         elem=[a.dtype.itemsize for a in arrays]))
    torch.cuda.synchronize()

    def compress(r, stream):
        kw = dict(r["kw"], base=r["bases"]) if r["bases"] is not None else r["kw"]
        return batch.compress(r["tensors"], stream=stream, **kw)

    for t, r in enumerate(runs):
        c = compress(r, None)
        torch.cuda.synchronize()
        tag = f"thread {t} (serial): batch.compress {r['name']}"
        widths, flags, based, coded, stored = _host_rule(H, r["hosts"], r["host_bases"], r["kw"], r["elem"])
        assert c.planes == widths, f"{tag}: widths {c.planes}, the host rule gives {widths}"
        assert c.delta == flags, f"{tag}: filter flags {c.delta}, the host rule gives {flags}"
        assert c.based == based, f"{tag}: kept bases {c.based}, the host rule gives {based}"
        if flags is not None and isinstance(r["kw"].get("delta"), str):
            assert True in flags[4:] and False in flags[4:], f"{tag}: the rule decides one way only: {flags}"
        if based is not None:
            assert True in based[4:] and False in based[4:], f"{tag}: the rule decides one way only: {based}"
        if r["kw"].get("sparse") == "auto":                    # the kinds themselves: 0 coded, 1 raw, 2 sparse
            assert c.stored.cpu().tolist() == stored, f"{tag}: the kinds differ from the host rule"
            assert set(stored) == {H.KIND_CODED, H.KIND_RAW, H.KIND_SPARSE}, f"{tag}: the rule never keeps a packet as {sorted({0, 1, 2} - set(stored))}"
            assert len(set(widths[4:])) > 1, f"{tag}: one width throughout: {widths}"
        got_stored = None if c.stored is None else [bool(v) for v in c.stored.cpu().tolist()]
        assert got_stored == (None if stored is None else [bool(v) for v in stored]), f"{tag}: the stored mask differs from the host rule"
        if stored is not None:
            assert True in stored and False in stored, f"{tag}: every packet is {'stored' if stored[0] else 'coded'}"
        off = c.offsets.cpu().tolist()
        for b, h in enumerate(r["hosts"]):
            lo, hi = c.first_packet[b], c.first_packet[b + 1]
            if h.size == 0 or (stored is not None and any(stored[lo:hi])):
                continue
            lo, hi = c._coded_range(b)
            hi = min(hi, lo + 64)
            got = c.stream[off[lo]:off[hi]].cpu().numpy()
            want = oracle.encode_stream(coded[b][:(hi - lo) * PACKET])
            assert np.array_equal(got, want), f"{tag}: buffer {b} ({h.size} bytes, width {widths[b]}) differs from the reference encoder"
        if r["kw"].get("checksum"):
            want = [zlib.crc32(h[p * PACKET:(p + 1) * PACKET].tobytes()) for h in r["hosts"] for p in range(H.packet_count(h.size))]
            assert [v & 0xFFFFFFFF for v in c.crc32.cpu().tolist()] == want, f"{tag}: the CRCs are not those of the original bytes"
        else:
            assert c.crc32 is None
        r["serial"] = c
    assert H.status() == 0

    k = len(runs)
    streams = _streams(k)
    start = threading.Barrier(k)
    torch.cuda.synchronize()

    def run(t):
        r, s = runs[t], streams[t]
        start.wait()
        c = compress(r, s)
        return c, batch.decompress(c, stream=s, base=r["bases"])

    with ThreadPoolExecutor(k) as pool:
        results = [f.result() for f in [pool.submit(run, t) for t in range(k)]]
    torch.cuda.synchronize()
    verdicts = []
    for t, ((c, outs), r) in enumerate(zip(results, runs)):
        want = r["serial"]
        tag = f"thread {t}: batch.compress {r['name']}, {c.n_buffers} buffers, {sum(c.sizes)} bytes ({c.n_packets} packets)"
        assert (c.planes, c.delta, c.based) == (want.planes, want.delta, want.based), \
            f"{tag}: planes / delta / based {(c.planes, c.delta, c.based)}, the serial run chose {(want.planes, want.delta, want.based)}"
        assert (c.first_packet, c.sizes) == (want.first_packet, want.sizes), tag
        for field in ("stream", "offsets", "crc32", "stored", "raw", "raw_offsets", "sparse", "sparse_offsets"):
            verdicts.append((f"{tag}: {field} differs from the serial run's", _same_or_none(getattr(c, field), getattr(want, field))))
        for b, (o, v) in enumerate(zip(outs, r["tensors"])):
            verdicts.append((f"{tag}: batch.decompress buffer {b} ({o.numel()} bytes) does not round-trip", _same(o, _bytes_view(v))))
    _fail_on(verdicts)
    assert H.status() == 0, "a launch of the module reported into the fallback word"
