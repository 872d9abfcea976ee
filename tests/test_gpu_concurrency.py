"""The kernels under concurrent streams and host threads (include/gpuar_hip.h: every call takes an explicit stream; a
launch ORs its flags into its own status word and no other; compaction may run concurrently on different streams; the
library is usable from one host thread per GPU; the per-device state it keeps -- the fallback status word, the encoder's
per-CU arrival counters, the clock-sample table -- affects no result).

This module covers the coders and what was built with them: encode (throughput, latency, table, auto), decode, decode_stream,
compact, crc32 / verify_crc32, generate, encode_batch / decode_batch / decode_stream_batch / crc32_batch,
batch.compress(checksum=True) / decompress, the executors' thread-local last error and the fallback status word.  The entry
points added since -- split_ / merge_planes, _delta and _xor, estimate, survey_planes, survey_delta, their batch forms,
move_packets, and batch.compress with planes=, delta=, stored=, base= -- are covered in the same way by
tests/test_gpu_filter_concurrency.py.  The verdict helpers both modules use are in tests/concurrency_checks.py.

Every test works the same way: the serial result of each workload comes first (one launch at a time, synchronised) and is
pinned against the reference (oracle.encode_stream on 64-packet windows, the oracle's decoder, zlib.crc32); then the same
workloads run concurrently, and the concurrent result must be byte-equal to the serial one, with every status word
exactly what its own launch should report.  Comparisons run on the device; only the verdicts are copied back.

1. Stream fan-out, one kernel family at a time: eight non-blocking streams, each with its own seeded input, outputs and
   zeroed status word, launched back to back and synchronised once at the end.  Sizes: one packet, one ragged wavefront,
   both sides of the auto switch (32768 / 32769 packets), 512 MiB - 1 GiB inputs; uniform, zipf, text and zeros.  The
   encoder's own status word is exercised with the 1024-byte slot build, where random input overflows its slots.
   encode_kernel and encode_kernel_t16 (the table walk), which deal their roles by the same per-CU ticket counters, run
   beside each other on two streams.
2. Mixed co-residency: a >= 1 GiB throughput encode next to decode_slots, decode_stream, compaction and crc32_batch of
   other inputs, the encoder launched first and last, three seeds each.
3. Host threads: whole chains from eight threads at once; batch.compress / decompress from several threads; the
   thread-local last error.
4. The fallback status word: every flag is reported by exactly one gpuar_hip_status call while another thread launches.
Fixed seeds throughout.
"""
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import packet_families as PF
from concurrency_checks import _fail_on, _same, _status, _streams, _words
from gpuar_amd import synth
from test_gpu_parity import small_slot_lib  # noqa: F401  (the 1024-byte slot build, a module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
MiB = 1 << 20
CANARY = 0xA5
CHUNK = 16384                        # packets per step of a masked slot comparison (bounds its temporaries)

# (kind, seed, bytes): stream / thread i runs workload i
WORKLOADS = [
    ("text", 11, 5000),                              # one packet
    ("zipf", 12, 63 * PACKET + 4321),                # one wavefront, its last lane short
    ("uniform", 13, 32768 * PACKET),                 # the largest input auto sends to the latency kernel
    ("text", 14, 32768 * PACKET + 77),               # 32769 packets: the smallest it sends to the table-walk kernel
    ("zeros", 0, 1024 * MiB),
    ("uniform", 15, 768 * MiB + 3 * PACKET + 17),
    ("zipf", 16, 512 * MiB + 999),
    ("text", 17, 1024 * MiB - 5 * PACKET + 3),
]
SMALL = 1                                            # the workload whose packets the status checks damage
DAMAGED_PACKET = 17


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


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _describe(i, family, mode=None):
    kind, seed, n = WORKLOADS[i]
    m = f" {mode}" if mode else ""
    return f"stream {i}: {family}{m}, {kind} seed {seed}, {n} bytes ({(n + PACKET - 1) // PACKET} packets)"


def _clens(slots, npk):
    v = slots[:npk * SLOT].view(npk, SLOT)
    return v[:, 0].long() | (v[:, 1].long() << 8)


def _slots_equal(got, want, npk):
    """Device verdict: the npk slots of `got` equal `want` on want's clen bytes (a slot's bytes behind clen are undefined)."""
    g, w = got[:npk * SLOT].view(npk, SLOT), want[:npk * SLOT].view(npk, SLOT)
    cols = torch.arange(SLOT, device=got.device)[None, :]
    ok = torch.ones((), dtype=torch.bool, device=got.device)
    for a in range(0, npk, CHUNK):
        b = min(a + CHUNK, npk)
        clen = w[a:b, 0].long() | (w[a:b, 1].long() << 8)
        ok &= ((g[a:b] == w[a:b]) | (cols >= clen[:, None])).all()
    return ok


def _decoded(out, d_in, npk, hole=None):
    """Device verdict: `out` holds d_in and the canary behind it up to npk * 8192; `hole` (a packet index): that packet's
    8192 bytes are left unwritten (canary) instead."""
    n = d_in.numel()
    if hole is None:
        return out[:n].eq(d_in).all() & out[n:npk * PACKET].eq(CANARY).all()
    a, b = hole * PACKET, (hole + 1) * PACKET
    return (out[:a].eq(d_in[:a]).all() & out[a:b].eq(CANARY).all() & out[b:n].eq(d_in[b:]).all()
            & out[n:npk * PACKET].eq(CANARY).all())


def _windows(npk):
    return [(a, min(a + 64, npk)) for a in sorted({0, (npk // 2) & ~63, max(npk - 64, 0)})]


@pytest.fixture(scope="module")
def serial(H, oracle):
    """Each workload's input (device-generated), slots (throughput kernel), compacted stream, offsets and CRCs, one launch
    at a time, each synchronised, and pinned: the generator against numpy, 64-packet windows of the stream against the
    reference encoder and decoder, the offsets against the slots' clens, both decoders against the input, CRCs of
    packets against zlib.crc32."""
    ws = []
    verdicts = []
    assert H.status() == 0
    for i, (kind, seed, n) in enumerate(WORKLOADS):
        npk = H.packet_count(n)
        d_in = H.generate(kind, seed, n)
        torch.cuda.synchronize()
        if kind != "zeros":
            head = min(n, 65536)
            mid = (n // 2) & ~7
            assert np.array_equal(d_in[:head].cpu().numpy(), synth.generate(kind, seed, head)), _describe(i, "generate")
            assert np.array_equal(d_in[mid:mid + 4096].cpu().numpy(), synth.generate(kind, seed, min(4096, n - mid), offset=mid)), \
                _describe(i, "generate")
        word = _status(3)
        slots = H.encode(d_in, d_status=word[0:1], mode="throughput")
        torch.cuda.synchronize()
        d_stream, offs = H.compact(slots, npk)
        torch.cuda.synchronize()
        total = int(offs[-1].item())
        d_stream = d_stream[:total].clone()
        want_offs = torch.zeros(npk + 1, dtype=torch.int64, device="cuda")
        want_offs[1:] = torch.cumsum(_clens(slots, npk), 0)
        verdicts.append((f"{_describe(i, 'compact')}: offsets are not the clens' exclusive sum", offs.eq(want_offs).all()))
        offs_host = offs.cpu().numpy()
        for a, b in _windows(npk):
            lo, hi = a * PACKET, min(b * PACKET, n)
            got = d_stream[int(offs_host[a]):int(offs_host[b])].cpu().numpy()
            want = oracle.encode_stream(d_in[lo:hi].cpu().numpy())
            assert np.array_equal(got, want), f"{_describe(i, 'encode throughput')}: packets {a}..{b - 1} differ from the reference encoder"
            back = oracle.decode_stream(got, hi - lo)
            assert np.array_equal(back[:hi - lo], d_in[lo:hi].cpu().numpy()), f"{_describe(i, 'encode')}: the reference decoder " \
                f"does not restore packets {a}..{b - 1}"
        crc = H.crc32(d_in)
        torch.cuda.synchronize()
        crc_host = crc.cpu().numpy().view(np.uint32)
        for p in {0, npk // 2, npk - 1}:
            want = zlib.crc32(d_in[p * PACKET:min((p + 1) * PACKET, n)].cpu().numpy().tobytes())
            assert int(crc_host[p]) == want, f"{_describe(i, 'crc32')}: packet {p}"
        out = torch.full((npk * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
        H.decode(slots, npk, out, d_status=word[1:2])
        torch.cuda.synchronize()
        verdicts.append((f"{_describe(i, 'decode')} (serial)", _decoded(out, d_in, npk)))
        out.fill_(CANARY)
        H.decode_stream(d_stream, offs, npk, out, d_status=word[2:3])
        torch.cuda.synchronize()
        verdicts.append((f"{_describe(i, 'decode_stream')} (serial)", _decoded(out, d_in, npk)))
        del out
        _words(verdicts, word, [0, 0, 0], [_describe(i, f) for f in ("encode", "decode", "decode_stream")])
        ws.append(dict(d_in=d_in, n=n, npk=npk, slots=slots, stream=d_stream, offs=offs, offs_host=offs_host, crc=crc))
    _fail_on(verdicts)
    assert H.status() == 0
    return ws


# ---------------------------------------------------------------------------------------------------------------------
# 1. stream fan-out, one kernel family at a time
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["throughput", "latency", "auto", "table"])
def test_encode_fan_out(H, serial, mode):
    """encode_mode on eight streams at once.  Serial pass first: each workload alone in this mode must equal the pinned
    slots on their clen bytes.  Concurrent pass into the same buffers (refilled): equal again, so equal to the serial
    pass.  Several throughput or table-walk grids (in auto: latency grids beside table-walk ones) share the chip, which
    changes the order in which workgroups draw their per-CU tickets; the slots must not depend on it."""
    k = len(serial)
    bufs = [torch.full((w["npk"] * SLOT,), 0xEE, dtype=torch.uint8, device="cuda") for w in serial]
    words = _status(2 * k)
    verdicts = []
    for i, w in enumerate(serial):
        H.encode(w["d_in"], bufs[i], d_status=words[i:i + 1], mode=mode)
        torch.cuda.synchronize()
        verdicts.append((f"{_describe(i, 'encode', mode)}: the serial slots differ from the pinned slots",
                         _slots_equal(bufs[i], w["slots"], w["npk"])))
    for b in bufs:
        b.fill_(0xEE)
    streams = _streams(k)
    torch.cuda.synchronize()
    for i, (w, s) in enumerate(zip(serial, streams)):
        H.encode(w["d_in"], bufs[i], stream=s, d_status=words[k + i:k + i + 1], mode=mode)
    torch.cuda.synchronize()
    for i, w in enumerate(serial):
        verdicts.append((f"{_describe(i, 'encode', mode)}: the concurrent slots differ from the serial slots",
                         _slots_equal(bufs[i], w["slots"], w["npk"])))
    _words(verdicts, words, [0] * (2 * k), [_describe(i, "encode", mode) + " (serial)" for i in range(k)] +
           [_describe(i, "encode", mode) for i in range(k)])
    _fail_on(verdicts)
    assert H.status() == 0, f"encode {mode}: a launch reported into the fallback word"


TWO_KERNEL_N = 130 * PACKET + 4097                   # two full groups and a third of three lanes, the last one short


def test_table_and_throughput_kernels_side_by_side(H, oracle):
    """encode_kernel_t16 (the table walk) on one stream while encode_kernel runs on the other, then swapped: the only place
    where workgroups of the two kernels draw tickets from the same per-CU arrival counters at once (each kernel deals its
    wavefronts' roles by SIMD after its ticket, four resident workgroups holding four consecutive ones -- with two kernels
    on a CU they no longer do).  130 packets + 4097 bytes each of zipf and of the parity suite's keep-carrying packets; every
    launch's slots equal the same kernel's serial slots and the reference encoder's, both status words are 0 and nothing
    goes to the fallback word."""
    inputs = {"zipf": torch.from_numpy(synth.zipf(61, TWO_KERNEL_N)).cuda(),
              "carry": torch.from_numpy(np.ascontiguousarray(PF.keep_carrying(131)[:TWO_KERNEL_N])).cuda()}
    npk = H.packet_count(TWO_KERNEL_N)
    assert npk == 131 and H.status() == 0
    verdicts = []
    want, serial_slots = {}, {}
    for name, d_in in inputs.items():
        host = d_in.cpu().numpy()
        stream = oracle.encode_stream(host)
        ref = np.zeros((npk, SLOT), dtype=np.uint8)
        at = 0
        for p in range(npk):
            c = int(stream[at]) | (int(stream[at + 1]) << 8)
            ref[p, :c] = stream[at:at + c]
            at += c
        assert at == stream.size
        want[name] = torch.from_numpy(ref).cuda().view(-1)
        for mode in ("table", "throughput"):
            word = _status()
            serial_slots[name, mode] = H.encode(d_in, d_status=word, mode=mode)
            torch.cuda.synchronize()
            verdicts.append((f"encode {mode}, {name} {TWO_KERNEL_N} bytes (serial): slots differ from the reference encoder",
                             _slots_equal(serial_slots[name, mode], want[name], npk)))
            _words(verdicts, word, [0], [f"encode {mode}, {name} (serial)"])
    sA, sB = _streams(2)
    pairs = [(("zipf", "table"), ("carry", "throughput")), (("zipf", "throughput"), ("carry", "table")),
             (("carry", "table"), ("zipf", "throughput")), (("carry", "throughput"), ("zipf", "table"))]
    words = _status(2 * len(pairs))
    what, expected = [], []
    for r, pair in enumerate(pairs):
        bufs = [torch.full((npk * SLOT,), 0xEE, dtype=torch.uint8, device="cuda") for _ in pair]
        torch.cuda.synchronize()
        for j, ((name, mode), s) in enumerate(zip(pair, (sA, sB))):
            H.encode(inputs[name], bufs[j], stream=s, d_status=words[2 * r + j:2 * r + j + 1], mode=mode)
        torch.cuda.synchronize()
        for j, (name, mode) in enumerate(pair):
            other = pair[1 - j]
            tag = f"round {r}, stream {'AB'[j]}: encode {mode}, {name}, beside encode {other[1]}, {other[0]}"
            verdicts.append((f"{tag}: slots differ from the same kernel's serial slots", _slots_equal(bufs[j], serial_slots[name, mode], npk)))
            verdicts.append((f"{tag}: slots differ from the reference encoder", _slots_equal(bufs[j], want[name], npk)))
            what.append(tag)
            expected.append(0)
    _words(verdicts, words, expected, what)
    _fail_on(verdicts)
    assert H.status() == 0, "a launch reported into the fallback word"


SMALL_SLOT = 1024
SMALL_SLOT_PACKETS = 2048


def _small_slots_defined(got, want, npk):
    """Device verdict for 1024-byte slots: equal on want's clen bytes, and for an overflowed slot (clen = 1024) on all but its
    last two dwords (what the coder had not yet flushed there is not part of the promise)."""
    g, w = got[:npk * SMALL_SLOT].view(npk, SMALL_SLOT), want[:npk * SMALL_SLOT].view(npk, SMALL_SLOT)
    clen = w[:, 0].long() | (w[:, 1].long() << 8)
    limit = torch.where(clen >= SMALL_SLOT, SMALL_SLOT - 8, clen)
    cols = torch.arange(SMALL_SLOT, device=got.device)[None, :]
    return ((g == w) | (cols >= limit[:, None])).all()


@pytest.mark.parametrize("how", ["streams", "threads"])
def test_encode_status_isolation_with_small_slots(H, oracle, small_slot_lib, how):
    """The encoder's own status word, which the shipped 8704-byte slots never give it a reason to touch: with the 1024-byte
    slot build of tests/test_gpu_parity.py, random bytes overflow every slot and zeros fit.  Eight encodes of 2048
    packets, alternately overflowing and fitting, the throughput, latency and table-walk kernels in turn, on eight streams launched
    back to back or from eight host threads: SLOT_OVERFLOW lands in exactly the overflowing launches' words, the others
    stay 0, and the slots equal the serial run's (pinned against the reference encoder) on their defined bytes."""
    k = 8
    n = SMALL_SLOT_PACKETS * PACKET
    guard = 4096
    inputs = [H.generate("uniform", 300 + i, n) if i % 2 == 0 else torch.zeros(n, dtype=torch.uint8, device="cuda")
              for i in range(k)]
    modes = [(1, 2, 3)[(i // 2 + i % 2) % 3] for i in range(k)]       # GPUAR_MODE_THROUGHPUT / LATENCY / TABLE, each on both kinds
    slots = [torch.full((SMALL_SLOT_PACKETS * SMALL_SLOT + guard,), CANARY, dtype=torch.uint8, device="cuda") for _ in range(k)]
    words = _status(2 * k)
    expected = [H.STATUS_SLOT_OVERFLOW if i % 2 == 0 else 0 for i in range(k)]

    def what(i):
        return (f"{'thread' if how == 'threads' else 'stream'} {i}: encode_mode {('throughput', 'latency', 'table')[modes[i] - 1]} with "
                f"1024-byte slots, {('uniform', 'zeros')[i % 2]} {n} bytes ({SMALL_SLOT_PACKETS} packets)")

    def launch(i, stream, word):
        handle = None if stream is None else stream.cuda_stream
        return small_slot_lib.gpuar_hip_encode_mode(inputs[i].data_ptr(), n, slots[i].data_ptr(), word.data_ptr(), handle, modes[i])

    rcs = []
    for i in range(k):
        rcs.append(launch(i, None, words[i]))
        torch.cuda.synchronize()
    serial = [s.clone() for s in slots]
    zero_pkt = np.frombuffer(oracle.encode_packet(bytes(PACKET)), dtype=np.uint8)
    for i in range(k):
        got = serial[i][:8 * SMALL_SLOT].view(8, SMALL_SLOT).cpu().numpy()
        for p in (0, 7):
            if i % 2:
                assert np.array_equal(got[p, :zero_pkt.size], zero_pkt), f"{what(i)} (serial): packet {p} differs from the reference encoder"
            else:
                want = np.frombuffer(oracle.encode_packet(inputs[i][p * PACKET:(p + 1) * PACKET].cpu().numpy().tobytes()), dtype=np.uint8)
                assert int(got[p, 0]) | (int(got[p, 1]) << 8) == SMALL_SLOT, f"{what(i)} (serial): packet {p} is not marked overflowed"
                assert np.array_equal(got[p, 4:SMALL_SLOT - 8], want[4:SMALL_SLOT - 8]), \
                    f"{what(i)} (serial): packet {p}'s prefix differs from the reference encoder"
    for s in slots:
        s.fill_(CANARY)
    streams = _streams(k)
    torch.cuda.synchronize()
    if how == "streams":
        for i, s in enumerate(streams):
            rcs.append(launch(i, s, words[k + i]))
    else:
        start = threading.Barrier(k)

        def run(i):
            start.wait()
            return launch(i, streams[i], words[k + i])

        with ThreadPoolExecutor(k) as pool:
            rcs += [f.result() for f in [pool.submit(run, i) for i in range(k)]]
    torch.cuda.synchronize()
    assert rcs == [0] * (2 * k), rcs
    verdicts = []
    for i in range(k):
        verdicts.append((f"{what(i)}: slots differ from the serial slots", _small_slots_defined(slots[i], serial[i], SMALL_SLOT_PACKETS)))
        verdicts.append((f"{what(i)}: written past the last slot", slots[i][SMALL_SLOT_PACKETS * SMALL_SLOT:].eq(CANARY).all()))
    _words(verdicts, words, expected * 2, [what(i) + " (serial)" for i in range(k)] + [what(i) for i in range(k)])
    _fail_on(verdicts)
    assert H.status() == 0


def _skewed(d_stream, skew):
    """A copy of d_stream at an address that is `skew` mod 16 (its own allocation, 64 bytes of slack): (allocation, view)."""
    raw = torch.zeros(d_stream.numel() + 64, dtype=torch.uint8, device="cuda")
    base = (-raw.data_ptr()) % 16 + skew
    view = raw[base:base + d_stream.numel()]
    view.copy_(d_stream)
    assert view.data_ptr() % 16 == skew
    return raw, view


def _damage_ulen(buf, at):
    """An impossible ulen (0xFFFF > 8192) in the packet header at byte `at` of a slot buffer or a packet stream."""
    buf[at + 2:at + 4] = 0xFF


@pytest.mark.parametrize("via", ["slots", "stream"])
def test_decode_fan_out(H, serial, via):
    """decode (slots) or decode_stream on eight streams at once; decode_stream reads every other stream's packets at
    pointer skew 4.  Stream 1's packet 17 carries an impossible ulen: BAD_PACKET in stream 1's word and in no other, that
    packet's output left unwritten, every other byte of every output equal to the serial run (= the input)."""
    k = len(serial)
    srcs, keep = [], []
    for i, w in enumerate(serial):
        if via == "slots":
            src = w["slots"]
            if i == SMALL:
                src = src.clone()
                _damage_ulen(src, DAMAGED_PACKET * SLOT)
        else:
            src = w["stream"]
            if i == SMALL:
                src = src.clone()
                _damage_ulen(src, int(w["offs_host"][DAMAGED_PACKET]))
            if i % 2:
                raw, src = _skewed(src, 4)
                keep.append(raw)
        srcs.append(src)
    outs = [torch.full((w["npk"] * PACKET,), CANARY, dtype=torch.uint8, device="cuda") for w in serial]
    words = _status(2 * k)
    family = "decode" if via == "slots" else "decode_stream"

    def launch(i, w, stream, word):
        if via == "slots":
            H.decode(srcs[i], w["npk"], outs[i], stream=stream, d_status=word)
        else:
            H.decode_stream(srcs[i], w["offs"], w["npk"], outs[i], stream=stream, d_status=word)

    def mode(i):
        return None if via == "slots" else f"skew {4 * (i % 2)}"

    verdicts = []
    for i, w in enumerate(serial):
        launch(i, w, None, words[i:i + 1])
        torch.cuda.synchronize()
        verdicts.append((f"{_describe(i, family, mode(i))} (serial): output", _decoded(outs[i], w["d_in"], w["npk"],
                                                                                   DAMAGED_PACKET if i == SMALL else None)))
    for o in outs:
        o.fill_(CANARY)
    streams = _streams(k)
    torch.cuda.synchronize()
    for i, (w, s) in enumerate(zip(serial, streams)):
        launch(i, w, s, words[k + i:k + i + 1])
    torch.cuda.synchronize()
    for i, w in enumerate(serial):
        verdicts.append((f"{_describe(i, family, mode(i))}: the concurrent output differs from the serial output",
                         _decoded(outs[i], w["d_in"], w["npk"], DAMAGED_PACKET if i == SMALL else None)))
    expected = [H.STATUS_BAD_PACKET if i == SMALL else 0 for i in range(k)]
    _words(verdicts, words, expected * 2, [_describe(i, family, mode(i)) + " (serial)" for i in range(k)] +
           [_describe(i, family, mode(i)) for i in range(k)])
    _fail_on(verdicts)
    assert H.status() == 0, f"{family}: a launch reported into the fallback word"


def test_compact_fan_out(H, serial):
    """compact on eight streams at once: its scan scratch lives in each caller's d_stream, so concurrent compactions share
    nothing.  Offsets and stream equal the serial (pinned) ones, and nothing is written behind offsets[n]."""
    k = len(serial)
    outs = [torch.full((w["npk"] * SLOT,), CANARY, dtype=torch.uint8, device="cuda") for w in serial]
    offs = [torch.full((w["npk"] + 2,), -7, dtype=torch.int64, device="cuda") for w in serial]

    def check(tag):
        v = []
        for i, w in enumerate(serial):
            total = w["stream"].numel()
            v.append((f"{_describe(i, 'compact')}{tag}: offsets differ", offs[i][:w["npk"] + 1].eq(w["offs"]).all()
                      & offs[i][w["npk"] + 1].eq(-7)))
            v.append((f"{_describe(i, 'compact')}{tag}: stream differs or written past offsets[n]",
                      outs[i][:total].eq(w["stream"]).all() & outs[i][total:].eq(CANARY).all()))
        return v

    verdicts = []
    for i, w in enumerate(serial):
        H.compact(w["slots"], w["npk"], outs[i], offs[i])
        torch.cuda.synchronize()
    verdicts += check(" (serial)")
    for o, f in zip(outs, offs):
        o.fill_(CANARY)
        f.fill_(-7)
    streams = _streams(k)
    torch.cuda.synchronize()
    for i, (w, s) in enumerate(zip(serial, streams)):
        H.compact(w["slots"], w["npk"], outs[i], offs[i], stream=s)
    torch.cuda.synchronize()
    verdicts += check("")
    _fail_on(verdicts)


def test_crc32_fan_out(H, serial):
    """crc32 then verify_crc32 on each of eight streams at once.  Stream 1 verifies against CRCs with packet 17's flipped:
    CHECKSUM and first_bad = 17 there and nowhere else; every other verify reports 0 and leaves first_bad at -1."""
    k = len(serial)
    crcs = [torch.full((w["npk"],), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for w in serial]
    refs = []
    for i, w in enumerate(serial):
        r = w["crc"]
        if i == SMALL:
            r = r.clone()
            r[DAMAGED_PACKET] ^= 1
        refs.append(r)
    words = _status(2 * k)
    first_bad = torch.full((2 * k,), -1, dtype=torch.int64, device="cuda")

    def launch(i, w, stream, j):
        H.crc32(w["d_in"], d_crc=crcs[i], stream=stream)
        H.verify_crc32(w["d_in"], refs[i], d_first_bad=first_bad[j:j + 1], d_status=words[j:j + 1], stream=stream)

    verdicts = []
    for i, w in enumerate(serial):
        launch(i, w, None, i)
        torch.cuda.synchronize()
        verdicts.append((f"{_describe(i, 'crc32')} (serial): CRCs differ from the pinned CRCs", crcs[i].eq(w["crc"]).all()))
    for c in crcs:
        c.fill_(0x5A5A5A5A)
    streams = _streams(k)
    torch.cuda.synchronize()
    for i, (w, s) in enumerate(zip(serial, streams)):
        launch(i, w, s, k + i)
    torch.cuda.synchronize()
    for i, w in enumerate(serial):
        verdicts.append((f"{_describe(i, 'crc32')}: the concurrent CRCs differ from the serial CRCs", crcs[i].eq(w["crc"]).all()))
    expected = [H.STATUS_CHECKSUM if i == SMALL else 0 for i in range(k)] * 2
    _words(verdicts, words, expected, [_describe(i, "verify_crc32") + " (serial)" for i in range(k)] +
           [_describe(i, "verify_crc32") for i in range(k)])
    for j in range(2 * k):
        want = DAMAGED_PACKET if j % k == SMALL else -1
        verdicts.append((f"{_describe(j % k, 'verify_crc32')}{' (serial)' if j < k else ''}: first_bad is not {want}",
                         first_bad[j].eq(want)))
    _fail_on(verdicts)
    assert H.status() == 0


def _batch_sizes(i):
    """Stream i's batch: empty and one-byte buffers, the packet boundaries, seeded small ones, and one large buffer --
    above the auto switch on stream 0."""
    rng = np.random.default_rng([29, i])
    big = 300 * MiB + 4321 if i == 0 else (8 + 7 * i) * MiB + 1001 * i
    return ([0, 1, PACKET - 1, PACKET, PACKET + 1, 0] + [int(x) for x in rng.integers(1, 3 * PACKET, 12)] + [big] +
            [int(x) for x in rng.integers(1, 200, 5)] + [0])


def test_batch_fan_out(H, oracle):
    """encode_batch -> compact -> decode_batch and decode_stream_batch, a whole chain on each of eight streams, each
    batch in a canary arena (tests/test_gpu_batch.py), the modes auto / throughput / latency in turn.  The serial chains
    are pinned: every buffer's stream against the reference encoder (whole, or its first 64 packets), the decoded arenas
    against the input arena, gaps and canaries included.  The concurrent slots, offsets, streams and output arenas equal
    the serial ones, and every one of the 24 status words is 0."""
    from test_gpu_batch import Arena, _desc
    kinds = ("text", "zipf", "uniform")
    modes = ("auto", "throughput", "latency")
    k = 8
    runs = []
    for i in range(k):
        sizes = _batch_sizes(i)
        a = Arena(sizes, fill=False)
        for b, (at, n) in enumerate(zip(a.starts, a.sizes)):
            if n:
                H.generate(kinds[(i + b) % 3], 1000 * i + b, n, out=a.mem[at:at + n])
        d_ptrs, d_bytes, d_fp, fp, npk = _desc(H, a.views())
        outs = [Arena(sizes, fill=False), Arena(sizes, fill=False)]
        d_optr = [_desc(H, o.views())[0] for o in outs]
        slots = torch.full((npk * SLOT,), 0xEE, dtype=torch.uint8, device="cuda")
        stream = torch.full((npk * SLOT,), CANARY, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(npk + 1, dtype=torch.int64, device="cuda")
        runs.append(dict(a=a, sizes=sizes, d_ptrs=d_ptrs, d_bytes=d_bytes, d_fp=d_fp, fp=fp, npk=npk, outs=outs, d_optr=d_optr,
                         slots=slots, stream=stream, offs=offs, mode=modes[i % 3]))
    words = _status(6 * k)

    def chain(i, r, s, w, sync):
        k_ = len(r["sizes"])
        steps = [
            lambda: H.encode_batch(r["d_ptrs"], r["d_bytes"], r["d_fp"], k_, r["npk"], d_slots=r["slots"], stream=s,
                                   d_status=w[0:1], mode=r["mode"]),
            lambda: H.compact(r["slots"], r["npk"], r["stream"], r["offs"], stream=s),
            lambda: H.decode_batch(r["slots"], r["d_fp"], k_, r["npk"], r["d_optr"][0], r["d_bytes"], stream=s, d_status=w[1:2]),
            lambda: H.decode_stream_batch(r["stream"], r["offs"], r["d_fp"], k_, r["npk"], r["d_optr"][1], r["d_bytes"],
                                          stream=s, d_status=w[2:3]),
        ]
        for step in steps:
            step()
            if sync:
                torch.cuda.synchronize()

    def what(i, r):
        return f"stream {i}: batch {r['mode']}, {len(r['sizes'])} buffers, {sum(r['sizes'])} bytes ({r['npk']} packets)"

    verdicts = []
    serial = []
    for i, r in enumerate(runs):
        chain(i, r, None, words[3 * i:3 * i + 3], True)
        offs_host = r["offs"].cpu().numpy()
        for b, (at, n) in enumerate(zip(r["a"].starts, r["a"].sizes)):
            if n == 0:
                continue
            p0 = r["fp"][b]
            p1 = min(r["fp"][b + 1], p0 + 64)
            got = r["stream"][int(offs_host[p0]):int(offs_host[p1])].cpu().numpy()
            want = oracle.encode_stream(r["a"].mem[at:at + min(n, (p1 - p0) * PACKET)].cpu().numpy())
            assert np.array_equal(got, want), f"{what(i, r)} (serial): buffer {b} ({n} bytes) differs from the reference encoder"
        for j, o in enumerate(r["outs"]):
            verdicts.append((f"{what(i, r)} (serial): the {('decode_batch', 'decode_stream_batch')[j]} arena differs from the input arena",
                             o.mem.eq(r["a"].mem).all()))
        total = int(offs_host[-1])
        serial.append(dict(slots=r["slots"].clone(), stream=r["stream"][:total].clone(), offs=r["offs"].clone(), total=total))
        r["slots"].fill_(0xEE)
        r["stream"].fill_(CANARY)
        r["offs"].zero_()
        for o in r["outs"]:
            o.mem.fill_(CANARY)
    streams = _streams(k)
    torch.cuda.synchronize()
    for i, (r, s) in enumerate(zip(runs, streams)):
        with torch.cuda.stream(s):
            chain(i, r, s, words[3 * (k + i):3 * (k + i) + 3], False)
    torch.cuda.synchronize()
    for i, (r, sr) in enumerate(zip(runs, serial)):
        verdicts.append((f"{what(i, r)}: encode_batch slots differ from the serial slots", _slots_equal(r["slots"], sr["slots"], r["npk"])))
        verdicts.append((f"{what(i, r)}: compact offsets / stream differ from the serial ones",
                         r["offs"].eq(sr["offs"]).all() & r["stream"][:sr["total"]].eq(sr["stream"]).all()
                         & r["stream"][sr["total"]:].eq(CANARY).all()))
        for j, o in enumerate(r["outs"]):
            verdicts.append((f"{what(i, r)}: the {('decode_batch', 'decode_stream_batch')[j]} arena differs from the serial arena "
                             "(= the input arena, gaps included)", o.mem.eq(r["a"].mem).all()))
    _words(verdicts, words, [0] * (6 * k), [f"{what(i % k, runs[i % k])}{' (serial)' if i < k else ''}: "
                                            f"{('encode_batch', 'decode_batch', 'decode_stream_batch')[j]}"
                                            for i in range(2 * k) for j in range(3)])
    _fail_on(verdicts)
    assert H.status() == 0


def test_generate_fan_out(H, serial):
    """generate on eight streams at once equals the serial (pinned) inputs."""
    k = len(serial)
    outs = [torch.full((w["n"],), CANARY, dtype=torch.uint8, device="cuda") for w in serial]
    streams = _streams(k)
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        kind, seed, n = WORKLOADS[i]
        with torch.cuda.stream(s):
            H.generate(kind, seed, n, out=outs[i], stream=s)
    torch.cuda.synchronize()
    _fail_on([(f"{_describe(i, 'generate')}: differs from the serial run", outs[i].eq(w["d_in"]).all()) for i, w in enumerate(serial)])


# ---------------------------------------------------------------------------------------------------------------------
# 2. mixed co-residency
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("order", ["encoder_first", "encoder_last"])
def test_mixed_co_residency(H, oracle, serial, order, seed):
    """Different kernels on the chip at the same moment: a throughput encode of >= 1 GiB on stream A; decode_slots of
    workload 6 on B, decode_stream of workload 5 on C, compaction of workload 7 on D, crc32_batch over all eight inputs
    on E; the encoder launched first or last.

    The throughput encoder gives each wavefront of a workgroup its role by SIMD, after a ticket from its CU's arrival
    counter, and falls back to roles by wavefront index when the four SIMD ids are not distinct.  Which branch a
    workgroup took cannot be observed here and is not looked for: what is checked is that the bytes do not depend on
    it.  The encoder's slots equal its serial slots (pinned against the reference encoder), and every other output
    equals its serial output."""
    kind = ("text", "zipf", "uniform")[seed - 1]
    n = 1024 * MiB + seed * 7 * PACKET + 13 * seed
    npk = H.packet_count(n)
    d_in = H.generate(kind, 500 + seed, n)
    word = _status(5)
    want_slots = H.encode(d_in, d_status=word[0:1], mode="throughput")
    torch.cuda.synchronize()
    clens = _clens(want_slots, npk)
    offs = torch.zeros(npk + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(clens, 0)
    offs_host = offs.cpu().numpy()
    slots_host = None
    for a, b in _windows(npk):
        slots_host = want_slots[a * SLOT:b * SLOT].view(b - a, SLOT).cpu().numpy()
        got = np.concatenate([slots_host[j, :int(offs_host[a + j + 1] - offs_host[a + j])] for j in range(b - a)])
        want = oracle.encode_stream(d_in[a * PACKET:min(b * PACKET, n)].cpu().numpy())
        assert np.array_equal(got, want), f"encode throughput, {kind} seed {500 + seed}, {n} bytes (serial): packets {a}..{b - 1} " \
                                          "differ from the reference encoder"
    assert int(word[0].item()) == 0
    del slots_host

    wd, ws, wc = serial[6], serial[5], serial[7]
    ptrs = [w["d_in"].data_ptr() for w in serial]
    sizes = [w["n"] for w in serial]
    fp, bpk = H.batch_packet_count(sizes)
    d = torch.tensor(ptrs + sizes + fp, dtype=torch.int64).cuda()
    nb = len(serial)
    d_ptrs, d_bytes, d_fp = d[:nb], d[nb:2 * nb], d[2 * nb:]
    crc_want = torch.cat([w["crc"] for w in serial])
    crc_serial = H.crc32_batch(d_ptrs, d_bytes, d_fp, nb, bpk, d_status=word[1:2])
    torch.cuda.synchronize()
    verdicts = [("crc32_batch of the eight inputs (serial): differs from their pinned CRCs", crc_serial[:bpk].eq(crc_want).all())]

    slots = torch.full((npk * SLOT,), 0xEE, dtype=torch.uint8, device="cuda")
    out_d = torch.full((wd["npk"] * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    out_s = torch.full((ws["npk"] * PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    c_stream = torch.full((wc["npk"] * SLOT,), CANARY, dtype=torch.uint8, device="cuda")
    c_offs = torch.zeros(wc["npk"] + 1, dtype=torch.int64, device="cuda")
    crc = torch.zeros(bpk, dtype=torch.int32, device="cuda")
    words = _status(4)
    sA, sB, sC, sD, sE = _streams(5)
    launches = [
        ("decode_slots", lambda: H.decode(wd["slots"], wd["npk"], out_d, stream=sB, d_status=words[1:2])),
        ("decode_stream", lambda: H.decode_stream(ws["stream"], ws["offs"], ws["npk"], out_s, stream=sC, d_status=words[2:3])),
        ("compact", lambda: H.compact(wc["slots"], wc["npk"], c_stream, c_offs, stream=sD)),
        ("crc32_batch", lambda: H.crc32_batch(d_ptrs, d_bytes, d_fp, nb, bpk, d_crc=crc, stream=sE, d_status=words[3:4])),
    ]
    encoder = ("encode", lambda: H.encode(d_in, slots, stream=sA, d_status=words[0:1], mode="throughput"))
    launches = [encoder] + launches if order == "encoder_first" else launches + [encoder]
    torch.cuda.synchronize()
    for _, launch in launches:
        launch()
    torch.cuda.synchronize()

    what = f"{order}, seed {seed}"
    verdicts += [
        (f"{what}: stream A: encode throughput, {kind} {n} bytes ({npk} packets): slots differ from the serial slots",
         _slots_equal(slots, want_slots, npk)),
        (f"{what}: stream B: decode_slots, workload 6 ({wd['n']} bytes): output differs from the serial output",
         _decoded(out_d, wd["d_in"], wd["npk"])),
        (f"{what}: stream C: decode_stream, workload 5 ({ws['n']} bytes): output differs from the serial output",
         _decoded(out_s, ws["d_in"], ws["npk"])),
        (f"{what}: stream D: compact, workload 7 ({wc['npk']} packets): offsets or stream differ from the serial ones",
         c_offs.eq(wc["offs"]).all() & c_stream[:wc["stream"].numel()].eq(wc["stream"]).all()),
        (f"{what}: stream E: crc32_batch, {bpk} packets: CRCs differ from the serial ones", crc.eq(crc_serial[:bpk]).all()),
    ]
    _words(verdicts, words, [0, 0, 0, 0], [f"{what}: stream {s}: {f}" for s, f in
                                            (("A", "encode"), ("B", "decode_slots"), ("C", "decode_stream"), ("E", "crc32_batch"))])
    _fail_on(verdicts)
    assert int(word[1].item()) == 0 and H.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. host threads
# ---------------------------------------------------------------------------------------------------------------------
def test_thread_chains(H, serial):
    """Eight host threads, each with its own stream and status words, each running encode -> compact -> decode_stream ->
    verify_crc32 on its own workload (ctypes releases the GIL during a call, so the launches interleave).  Thread 1's
    stream gets an impossible ulen in packet 17 after compaction: only its decode word reports BAD_PACKET, only its
    verify word CHECKSUM with first_bad = 17 (that packet's output is left unwritten); every other word is 0 and the
    fallback word stays 0.  Slots, offsets, streams and outputs equal the serial (pinned) results."""
    k = len(serial)
    bufs = []
    for w in serial:
        bufs.append(dict(slots=torch.full((w["npk"] * SLOT,), 0xEE, dtype=torch.uint8, device="cuda"),
                         stream=torch.full((w["npk"] * SLOT,), CANARY, dtype=torch.uint8, device="cuda"),
                         offs=torch.zeros(w["npk"] + 1, dtype=torch.int64, device="cuda"),
                         out=torch.full((w["npk"] * PACKET,), CANARY, dtype=torch.uint8, device="cuda")))
    words = _status(3 * k)
    first_bad = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    streams = _streams(k)
    torch.cuda.synchronize()
    start = threading.Barrier(k)

    def chain(i):
        w, b, s = serial[i], bufs[i], streams[i]
        start.wait()
        with torch.cuda.stream(s):
            H.encode(w["d_in"], b["slots"], stream=s, d_status=words[3 * i:3 * i + 1], mode="throughput")
            H.compact(b["slots"], w["npk"], b["stream"], b["offs"], stream=s)
            if i == SMALL:
                _damage_ulen(b["stream"], int(w["offs_host"][DAMAGED_PACKET]))
            H.decode_stream(b["stream"], b["offs"], w["npk"], b["out"], stream=s, d_status=words[3 * i + 1:3 * i + 2])
            H.verify_crc32(b["out"], w["crc"], n_bytes=w["n"], d_first_bad=first_bad[i:i + 1], d_status=words[3 * i + 2:3 * i + 3],
                           stream=s)

    with ThreadPoolExecutor(k) as pool:
        for f in [pool.submit(chain, i) for i in range(k)]:
            f.result()
    torch.cuda.synchronize()
    verdicts = []
    for i, (w, b) in enumerate(zip(serial, bufs)):
        tag = _describe(i, "chain").replace("stream", "thread", 1)
        total = w["stream"].numel()
        want_stream = w["stream"]
        if i == SMALL:
            want_stream = want_stream.clone()
            _damage_ulen(want_stream, int(w["offs_host"][DAMAGED_PACKET]))
        verdicts += [
            (f"{tag}: encode slots differ from the serial slots", _slots_equal(b["slots"], w["slots"], w["npk"])),
            (f"{tag}: compact offsets / stream differ from the serial ones",
             b["offs"].eq(w["offs"]).all() & b["stream"][:total].eq(want_stream).all()),
            (f"{tag}: decode_stream output differs from the serial output",
             _decoded(b["out"], w["d_in"], w["npk"], DAMAGED_PACKET if i == SMALL else None)),
            (f"{tag}: verify_crc32 first_bad", first_bad[i].eq(DAMAGED_PACKET if i == SMALL else -1)),
        ]
    expected = []
    for i in range(k):
        expected += [0, H.STATUS_BAD_PACKET, H.STATUS_CHECKSUM] if i == SMALL else [0, 0, 0]
    _words(verdicts, words, expected, [f"{_describe(i, f).replace('stream', 'thread', 1)}" for i in range(k)
                                       for f in ("encode", "decode_stream", "verify_crc32")])
    _fail_on(verdicts)
    assert H.status() == 0, "the fallback word was touched by launches that had words of their own"


def test_thread_batch_compress(H, oracle):
    """batch.compress(checksum=True) and batch.decompress from six threads at once, each on its own stream: the
    compressed streams, offsets and CRCs equal the serial ones (pinned against the reference encoder and zlib.crc32),
    and every buffer round-trips."""
    from test_gpu_batch import Arena
    from gpuar_amd import batch
    k = 6
    arenas = []
    for t in range(k):
        rng = np.random.default_rng([41, t])
        sizes = [0, 3, PACKET, PACKET + 1] + [int(x) for x in rng.integers(1, 4 * PACKET, 10)] + [(16 + 24 * t) * MiB + 5 * t]
        a = Arena(sizes, fill=False)
        for b, (at, n) in enumerate(zip(a.starts, a.sizes)):
            if n:
                H.generate(("zipf", "text", "uniform")[(t + b) % 3], 2000 * t + b, n, out=a.mem[at:at + n])
        arenas.append(a)
    torch.cuda.synchronize()
    serial = []
    for t, a in enumerate(arenas):
        c = batch.compress(a.views(), checksum=True)
        torch.cuda.synchronize()
        for b, v in enumerate(a.views()):
            if v.numel() == 0:
                continue
            head = v[:min(v.numel(), 64 * PACKET)]
            npk = H.packet_count(head.numel())
            fp0 = c.first_packet[b]
            off = c.offsets[fp0:fp0 + npk + 1].cpu().numpy()
            got = c.stream[int(off[0]):int(off[-1])].cpu().numpy()
            want = oracle.encode_stream(head.cpu().numpy())
            assert np.array_equal(got, want), f"thread {t} (serial): buffer {b} ({v.numel()} bytes) differs from the reference encoder"
            for j in {0, npk - 1}:
                pkt = v[j * PACKET:min((j + 1) * PACKET, v.numel())].cpu().numpy().tobytes()
                assert int(c.crc32[fp0 + j].item()) & 0xFFFFFFFF == zlib.crc32(pkt), f"thread {t} (serial): buffer {b} packet {j} CRC"
        serial.append(c)
    streams = _streams(k)
    start = threading.Barrier(k)

    def run(t):
        s = streams[t]
        start.wait()
        c = batch.compress(arenas[t].views(), stream=s, checksum=True)
        return c, batch.decompress(c, stream=s)

    with ThreadPoolExecutor(k) as pool:
        results = [f.result() for f in [pool.submit(run, t) for t in range(k)]]
    torch.cuda.synchronize()
    verdicts = []
    for t, ((c, outs), want) in enumerate(zip(results, serial)):
        tag = f"thread {t}: batch.compress checksum=True, {c.n_buffers} buffers, {sum(c.sizes)} bytes ({c.n_packets} packets)"
        verdicts.append((f"{tag}: stream / offsets / CRCs differ from the serial ones",
                         _same(c.stream, want.stream) & _same(c.offsets, want.offsets) & _same(c.crc32, want.crc32)))
        for b, (o, v) in enumerate(zip(outs, arenas[t].views())):
            verdicts.append((f"{tag}: batch.decompress buffer {b} ({v.numel()} bytes) does not round-trip", _same(o, v)))
    _fail_on(verdicts)
    assert H.status() == 0


def test_thread_local_last_error(H):
    """gpuar_hip_last_error() is per host thread: thread 0 makes executor calls the host refuses (misaligned pointers;
    nothing reaches the device) while the seven others make executor calls that are accepted.  After all have called,
    thread 0 reads GPUAR_ERR_ALIGNMENT (then 0: read-and-clear) and every other thread reads GPUAR_OK.  The accepted
    encodes give the serial slots."""
    lib = H.load()
    k = 8
    n = 3 * PACKET + 555
    d_in = H.generate("text", 77, n)
    npk = H.packet_count(n)
    want = H.encode(d_in, mode="latency")
    slots = [torch.full((npk * SLOT,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(k)]
    torch.cuda.synchronize()
    assert lib.gpuar_hip_last_error() == 0
    called = threading.Barrier(k)

    def run(t):
        if t == 0:
            lib.garCompressExecutor(d_in.data_ptr() + 1, n, slots[t].data_ptr(), 1)
            lib.garDecompressExecutor(want.data_ptr(), npk * SLOT, slots[t].data_ptr() + 4, 1)
        else:
            lib.garCompressExecutor(d_in.data_ptr(), n, slots[t].data_ptr(), 1)
        called.wait()
        return lib.gpuar_hip_last_error(), lib.gpuar_hip_last_error()

    with ThreadPoolExecutor(k) as pool:
        errors = [f.result() for f in [pool.submit(run, t) for t in range(k)]]
    torch.cuda.synchronize()
    want_errors = [(-1, 0)] + [(0, 0)] * (k - 1)
    assert errors == want_errors, f"last error per thread (first read, second read): {errors}, want {want_errors}"
    _fail_on([(f"thread {t}: garCompressExecutor, text {n} bytes: slots differ from the serial slots", _slots_equal(slots[t], want, npk))
              for t in range(1, k)] +
             [("thread 0: a refused call wrote its output", slots[0].eq(0xEE).all())])
    assert H.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. the fallback status word
# ---------------------------------------------------------------------------------------------------------------------
ROUNDS = 48


def test_fallback_status_is_reported_exactly_once(H):
    """gpuar_hip_status reads and clears the fallback word in one device atomic, so every flag ORed into it is reported by
    exactly one call.  A conservation check, round by round: in each round one thread makes exactly one launch that uses
    the fallback word -- garDecompressExecutor (NULL stream) and a native decode with d_status=None on a non-blocking
    stream in turn -- over a slot whose ulen is impossible (clean slots in every third round), while a second thread
    calls status() concurrently; after both have joined, status() is called once more.  In a damaged round BAD_PACKET is
    in exactly one of the two results (neither lost nor reported twice); in a clean round both are 0.

    This cannot force the race between a launch and the read-and-clear; the launch is started a different number of
    microseconds after the status() call in each round, over a bounded number of rounds: a regression guard, not a
    proof."""
    lib = H.load()
    good = H.encode(H.generate("text", 5, 700))
    bad = good.clone()
    _damage_ulen(bad, 0)
    out = torch.full((PACKET,), CANARY, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert H.status() == 0
    pair = threading.Barrier(2)

    def launch(kind, slots, delay):
        pair.wait()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < delay:
            pass
        if kind == "executor":
            lib.garDecompressExecutor(slots.data_ptr(), SLOT, out.data_ptr(), 1)
        else:
            H.decode(slots, 1, out, stream=s, d_status=None)

    def read():
        pair.wait()
        return H.status()

    results = []
    with ThreadPoolExecutor(2) as pool:
        for r in range(ROUNDS):
            kind = ("executor", "native")[r % 2]
            damaged = r % 3 != 2
            delay = (r * 37 % 240) * 1e-6
            fl = pool.submit(launch, kind, bad if damaged else good, delay)
            fr = pool.submit(read)
            fl.result()
            during = fr.result()
            after = H.status()
            results.append((r, kind, damaged, round(delay * 1e6), during, after))
    assert lib.gpuar_hip_last_error() == 0
    wrong = []
    for r, kind, damaged, us, during, after in results:
        if damaged:
            ok = sorted((during, after)) == [0, H.STATUS_BAD_PACKET]
        else:
            ok = during == 0 and after == 0
        if not ok:
            wrong.append(f"round {r}: {kind} decode, {'impossible ulen' if damaged else 'clean'}, launched {us} us after the "
                         f"status() call: status() during {during:#x}, after {after:#x}")
    assert not wrong, f"{len(wrong)} of {ROUNDS} rounds broke conservation: " + "; ".join(wrong[:10])
