"""Helpers of the batch-matrix tests (not a test module): a host model of gpuar_amd/batch.py -- compress, estimate and decompress
over every keyword, from batch.py's docstrings and DESIGN.md 4.6-4.12 -- the batch both matrix modules run, and the matrix itself.

The model needs numpy, the numpy definitions of the filters (planes_ref, delta_ref, xor_ref, sparse_ref), the trailers restated in
trailer_ref / delta_ref / xor_ref, zlib.crc32, the host library's estimate (hip.estimate_host) and the oracle's codec; no device and
no torch.  Where batch.py measures (planes="survey", delta="auto" / "survey", base_auto) the model decides by definition: it splits
with numpy, estimates the split bytes and applies the rule, restated here (choose_planes, choose_filter) and pinned against the C
functions by tests/test_batch_model_host.py.  base_auto="survey" is decided the same way, from the split bytes' estimates and
scan words and never from the XOR survey (hip.survey_xor_host), which is what batch.py decides from.

Everything that depends only on a layout -- (buffer, width, none | delta | base) -- is made once and shared by every combination
that uses it: the split bytes, the per-packet estimates and scan words and the oracle's packets."""
import zlib

import numpy as np

import delta_ref as D
import planes_ref as P
import sparse_ref as S
import trailer_ref as T
import xor_ref as X

PACKET = 8192
WIDTHS = (1, 2, 4, 8)
CODED, RAW, SPARSE = S.CODED, S.RAW, S.SPARSE
ELEMENT_BYTES = {"uint8": 1, "bfloat16": 2, "int32": 4, "float32": 4, "int64": 8}     # (none of them complex)


# ---- the rules the surveys apply, restated from DESIGN.md 4.8 and 4.11 ---------------------------------------------------

def choose_planes(totals, n_packets):
    """the smallest width whose total is at most the lowest total + n_packets"""
    low = min(totals)
    return next(w for w, t in zip(WIDTHS, totals) if t <= low + n_packets)


def choose_filter(plain, filtered, n_packets):
    """(width, filter): the filter at the width choose_planes picks from `filtered` iff that total + n_packets is at most the total
    of the width choose_planes picks from `plain` (a tie, and a buffer without packets: no filter), else that width without it"""
    wp, wd = choose_planes(plain, n_packets), choose_planes(filtered, n_packets)
    if n_packets and filtered[WIDTHS.index(wd)] + n_packets <= plain[WIDTHS.index(wp)]:
        return wd, True
    return wp, False


def filter_pays(est_filtered, est_plain, n_packets):
    """the rule of delta="auto", delta="survey" at a fixed width and base_auto: one byte per packet is the estimate's resolution, a
    tie goes to no filter, and so does a buffer without packets"""
    return bool(n_packets) and est_filtered + n_packets <= est_plain


# ---- layouts -------------------------------------------------------------------------------------------------------------

def packets_of(n):
    return (n + PACKET - 1) // PACKET


def cut(x):
    """the packets of a buffer's bytes"""
    return [x[at:at + PACKET] for at in range(0, len(x), PACKET)]


class Layout:
    """One buffer's bytes as they are coded, and what depends on them alone."""

    def __init__(self, data):
        from gpuar_amd import hip as H
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.lens = [p.size for p in cut(self.data)]
        self.est = H.estimate_host(self.data.tobytes())
        self.scan = [S.scan(p) for p in cut(self.data)]
        self._coded = None

    @property
    def coded(self):
        """the oracle's packet for every packet of the layout"""
        if self._coded is None:
            stream = codec().encode_stream(self.data).tobytes() if self.data.size else b""
            self._coded, at = [], 0
            for clen in P.packet_lengths(stream):
                self._coded.append(stream[at:at + clen])
                at += clen
            assert len(self._coded) == len(self.lens)
        return self._coded


_CODEC = None
_LAYOUTS = {}
_DECODED = {}


def codec():
    global _CODEC
    if _CODEC is None:
        from oracle import oracle as O
        _CODEC = O.require_best()
    return _CODEC


def layout(x, w, how="none", base=None):
    """The layout (x, w, how) -- how: "none" (split), "delta" (filtered and split) or "base" (XORed with `base` and split) -- made once
    per array object, width and filter."""
    key = (id(x), w, how, id(base) if how == "base" else None)
    if key not in _LAYOUTS:
        raw = _raw(x)
        data = P.numpy_split(raw, w) if how == "none" else D.numpy_split_delta(raw, w) if how == "delta" else X.numpy_split_xor(raw, _raw(base), w)
        _LAYOUTS[key] = (Layout(data), x, base)                 # (the arrays are held: their ids stay theirs)
    return _LAYOUTS[key][0]


def layouts_made():
    """every layout made so far"""
    return [entry[0] for entry in _LAYOUTS.values()]


def decode_packet(pkt):
    if pkt not in _DECODED:
        _DECODED[pkt] = codec().decode_packet(pkt)
    return _DECODED[pkt]


# ---- the model -----------------------------------------------------------------------------------------------------------

class Refused(Exception):
    """what batch.py refuses with GpuarError before any launch"""


class Model:
    """Every field of batch.Compressed as host data (bytes, lists, None as there), `gips` (per buffer its .gip file, or None for a
    buffer that has none) and `layouts`, what the model coded every buffer from."""


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _totals(ests, lens, replace):
    """a buffer's predicted bytes from its packets' estimates; `replace`: a packet that would be kept raw counts as its bytes"""
    return sum(n if replace and e >= 4 + n else e for e, n in zip(ests, lens))


def _kept_total(lay, replace, count_sparse):
    """a layout's predicted bytes with every packet counted as it would be kept: under sparse="auto" by sparse_ref.rule -- a sparse
    packet as its record, a raw one as its bytes --, under stored="auto" alone a packet whose estimate is not below 4 + its bytes as
    its bytes, else its estimate"""
    if not count_sparse:
        return _totals(lay.est, lay.lens, replace)
    total = 0
    for s, e, n in zip(lay.scan, lay.est, lay.lens):
        kind = S.rule(s, e, n, replace)
        total += S.sparse_len(s >> 8) if kind == SPARSE else n if kind == RAW else e
    return total


def survey_base_totals(arrays, base, b, replace=False, count_sparse=False):
    """(plain, xored) of buffer b for base_auto="survey" beside planes="survey": the four totals of its bytes split at widths 1, 2, 4
    and 8 as they are and XORed with its base (None without one), every packet counted as it would be kept (_kept_total)"""
    plain = [_kept_total(layout(arrays[b], w, "none"), replace, count_sparse) for w in WIDTHS]
    if base is None or base[b] is None or not _raw(arrays[b]).size:
        return plain, None
    return plain, [_kept_total(layout(arrays[b], w, "base", base[b]), replace, count_sparse) for w in WIDTHS]


def _resolve(arrays, dtypes, planes, delta, base, base_auto, stored, sparse):
    """(the buffers' bytes, their packet counts, widths or None, flags or None, based or None, the layout every buffer is coded from,
    the kind of every batch packet or None) -- every choice batch.py measures for, made by definition"""
    arrays = list(arrays)
    xs = [_raw(a) for a in arrays]
    n = len(xs)
    counts = [packets_of(x.size) for x in xs]
    n_packets = sum(counts)
    if base is None and base_auto:
        raise Refused("base_auto without base")
    if isinstance(base_auto, str) and base_auto != "survey":
        raise Refused("base_auto is a string other than \"survey\"")
    if base is not None and delta is not None:
        raise Refused("base with delta")
    if stored is not None and not isinstance(stored, str) and len(stored) != n_packets:
        raise Refused("stored of another length")
    if sparse is not None and stored is not None and not isinstance(stored, str):
        raise Refused("sparse beside a list of stored packets")
    replace = isinstance(stored, str) and stored == "auto"

    def total(b, w, how):
        lay = layout(arrays[b], w, how)
        return _totals(lay.est, lay.lens, False), _totals(lay.est, lay.lens, replace)

    flags = based = None
    if isinstance(planes, str) and planes == "survey" and base is not None and isinstance(base_auto, str):
        # width and base together: choose_filter with the base in the filter's place, on totals that count raw and sparse packets
        both = [survey_base_totals(arrays, base, b, replace, sparse is not None) for b in range(n)]
        choice = [(choose_planes(plain, counts[b]), False) if xored is None else choose_filter(plain, xored, counts[b])
                  for b, (plain, xored) in enumerate(both)]
        widths, based = [w for w, _k in choice], [k for _w, k in choice]
    elif isinstance(planes, str) and planes == "survey":
        plain = [[total(b, w, "none")[1] for w in WIDTHS] for b in range(n)]
        if isinstance(delta, str) and delta == "survey":
            filtered = [[total(b, w, "delta")[1] for w in WIDTHS] for b in range(n)]
            choice = [choose_filter(plain[b], filtered[b], counts[b]) for b in range(n)]
            widths, flags = [w for w, _f in choice], [f for _w, f in choice]
        else:
            widths = [choose_planes(plain[b], counts[b]) for b in range(n)]
    elif planes is None:
        widths = None
    elif isinstance(planes, str):
        assert planes == "auto"
        widths = [ELEMENT_BYTES[d] if ELEMENT_BYTES[d] in (2, 4, 8) else 1 for d in dtypes]
    else:
        widths = [planes] * n if isinstance(planes, int) else list(planes)
    if widths is None and (delta is not None or base is not None):
        widths = [1] * n                                        # a filter without `planes` works on bytes
    if flags is None and delta is not None:
        if isinstance(delta, str):
            assert delta in ("auto", "survey")
            flags = [filter_pays(total(b, widths[b], "delta")[0], total(b, widths[b], "none")[0], counts[b]) for b in range(n)]
        else:
            flags = [bool(delta)] * n if isinstance(delta, (bool, int)) else [bool(f) for f in delta]
    if base is not None and based is None:
        based = [q is not None and xs[b].size > 0 for b, q in enumerate(base)]
        if base_auto:                                           # (True and "survey" at fixed widths: one rule, on coded estimates)
            based = [based[b] and filter_pays(sum(layout(arrays[b], widths[b], "base", base[b]).est), total(b, widths[b], "none")[0], counts[b])
                     for b in range(n)]
    lays = []
    for b in range(n):
        w = widths[b] if widths is not None else 1
        if based is not None and based[b]:
            lays.append(layout(arrays[b], w, "base", base[b]))
        elif flags is not None and flags[b]:
            lays.append(layout(arrays[b], w, "delta"))
        else:
            lays.append(layout(arrays[b], w, "none"))
    kinds = None
    if sparse is not None:
        assert sparse == "auto"
        kinds = [S.rule(s, e, m, replace) for lay in lays for s, e, m in zip(lay.scan, lay.est, lay.lens)]
    elif replace:
        kinds = [RAW if e >= 4 + m else CODED for lay in lays for e, m in zip(lay.est, lay.lens)]
    elif stored is not None:
        kinds = [RAW if f else CODED for f in stored]
    return xs, counts, widths, flags, based, lays, kinds


def model_compress(arrays, dtypes, planes=None, delta=None, base=None, base_auto=False, stored=None, sparse=None, checksum=False):
    """What batch.compress(tensors, checksum=, planes=, stored=, delta=, base=, base_auto=, sparse=) returns for tensors that hold
    `arrays` (numpy arrays; `dtypes`: their tensors' types by name; `base`: None or one uint8 array or None per array)."""
    xs, counts, widths, flags, based, lays, kinds = _resolve(arrays, dtypes, planes, delta, base, base_auto, stored, sparse)
    m = Model()
    m.sizes = [x.size for x in xs]
    m.first_packet = [0]
    for c in counts:
        m.first_packet.append(m.first_packet[-1] + c)
    m.planes, m.delta, m.based, m.layouts = widths, flags, based, lays
    m.stored = kinds
    per_packet = [(lay, j) for lay in lays for j in range(len(lay.lens))]
    coded = [lay.coded[j] for p, (lay, j) in enumerate(per_packet) if kinds is None or kinds[p] == CODED]
    m.stream = b"".join(coded)
    m.offsets = [0]
    for pkt in coded:
        m.offsets.append(m.offsets[-1] + len(pkt))
    m.raw = m.raw_offsets = m.sparse = m.sparse_offsets = None
    if kinds is not None:
        m.raw, m.raw_offsets = b"", [0]
        for p, (lay, j) in enumerate(per_packet):
            if kinds[p] == RAW:
                data = lay.data[j * PACKET:(j + 1) * PACKET].tobytes()
                m.raw += data + bytes(-len(data) % 16)
                m.raw_offsets.append(len(m.raw))
    if sparse is not None:
        m.sparse, m.sparse_offsets = b"", [0]
        for p, (lay, j) in enumerate(per_packet):
            if kinds[p] == SPARSE:
                m.sparse += S.pack(lay.data[j * PACKET:(j + 1) * PACKET])
                m.sparse_offsets.append(len(m.sparse))
    m.crc32 = [zlib.crc32(p.tobytes()) for x in xs for p in cut(x)] if checksum else None
    m.nbytes = len(m.stream) + len(m.raw or b"") + len(m.sparse or b"")
    m.gips = [_gip(m, b) for b in range(len(xs))]
    return m


def _gip(m, b):
    """buffer b as `gpuar c` writes it, or None where it has no .gip form: a buffer with a raw or a sparse packet, and a buffer that
    was XORed with a base without the CRCs"""
    from oracle import oracle as O
    lo, hi = m.first_packet[b], m.first_packet[b + 1]
    if m.stored is not None and any(m.stored[lo:hi]):
        return None
    xored = m.based is not None and m.based[b]
    if xored and m.crc32 is None:
        return None
    packets = m.layouts[b].coded
    stream = b"".join(packets)
    out = O.gip_header(m.sizes[b], len(stream)) + stream
    w = m.planes[b] if m.planes is not None else 1
    filtered = m.delta is not None and m.delta[b]
    clens = [len(p) for p in packets]
    crcs = m.crc32[lo:hi] if m.crc32 is not None else None
    if xored:
        return out + X.trailer_v5(clens, w, crcs)
    if filtered:
        return out + D.trailer_v4(clens, w, crcs)
    if w > 1 or crcs is not None:
        return out + T.write(clens, w, crcs)
    return out


def model_estimate(arrays, dtypes, planes=None, delta=None, base=None, base_auto=False, stored=None, sparse=None):
    """What batch.estimate returns: per tensor the sum of its packets' estimates, a packet that would be kept sparse counting as its
    record's bytes and one that would be kept raw as its own."""
    assert stored is None or stored == "auto"
    _xs, _counts, _widths, _flags, _based, lays, kinds = _resolve(arrays, dtypes, planes, delta, base, base_auto, stored, sparse)
    out, p = [], 0
    for lay in lays:
        total = 0
        for s, e, n in zip(lay.scan, lay.est, lay.lens):
            kind = kinds[p] if kinds is not None else CODED
            total += S.sparse_len(s >> 8) if kind == SPARSE else n if kind == RAW else e
            p += 1
        out.append(total)
    return out


def model_decompress(m, bases=None):
    """The bytes of every buffer from the model's (or a Compressed's, brought to the host) stream, raw packets and records: the
    oracle's decoder, sparse_ref.unpack and the numpy merges.  A record that is not valid raises ValueError."""
    out, rank = [], [0, 0, 0]
    for b, size in enumerate(m.sizes):
        parts = []
        for p in range(m.first_packet[b], m.first_packet[b + 1]):
            n = min(PACKET, size - (p - m.first_packet[b]) * PACKET)
            kind = m.stored[p] if m.stored is not None else CODED
            r = rank[kind]
            rank[kind] += 1
            if kind == CODED:
                data = np.frombuffer(decode_packet(bytes(m.stream[m.offsets[r]:m.offsets[r + 1]])), dtype=np.uint8)
                assert data.size == n
            elif kind == RAW:
                data = np.frombuffer(bytes(m.raw[m.raw_offsets[r]:m.raw_offsets[r] + n]), dtype=np.uint8)
            else:
                lo, hi = m.sparse_offsets[r], m.sparse_offsets[r + 1]
                data = S.unpack(m.sparse[lo:hi], hi - lo, n)
                if data is None:
                    raise ValueError(f"the record of batch packet {p} is not valid")
            parts.append(data)
        coded = np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)
        w = m.planes[b] if m.planes is not None else 1
        if m.based is not None and m.based[b]:
            out.append(X.numpy_merge_xor(coded, _raw(bases[b]), w))
        elif m.delta is not None and m.delta[b]:
            out.append(D.numpy_merge_delta(coded, w))
        else:
            out.append(P.numpy_merge(coded, w))
    return out


def first_wrong_packet(m, got):
    """(buffer, packet) of the first packet of `got` (what model_decompress returned) whose CRC-32 is not m.crc32's, or None"""
    for b, x in enumerate(got):
        for j, p in enumerate(cut(x)):
            if zlib.crc32(p.tobytes()) != m.crc32[m.first_packet[b] + j]:
                return b, j
    return None


# ---- the batch under test ------------------------------------------------------------------------------------------------

def _bf16_weights(rng, elements):
    return X.bf16(rng.standard_normal(elements).astype(np.float32) * np.float32(0.02))


def _make_batch():
    from gpuar_amd import synth
    rng = np.random.default_rng(20)
    near_base = _bf16_weights(rng, (6 * PACKET + 100) // 2)
    near = near_base.copy()
    where = rng.choice(near.size, max(near.size // 1000, 1), replace=False)
    near[where] = _bf16_weights(rng, where.size)
    same = _bf16_weights(rng, (2 * PACKET + 100) // 2)
    far, far_base = _bf16_weights(rng, 3 * PACKET // 2), _bf16_weights(rng, 3 * PACKET // 2)
    fp32 = (rng.standard_normal(PACKET + 1).astype(np.float32) * np.float32(0.02)).view(np.uint8)[:4 * PACKET + 3].copy()
    walk = (np.cumsum(rng.normal(0, 2, PACKET + 1)).astype(np.int64) % 256).astype(np.uint8)
    batch = [                                                               # (array, its tensor's type, base)
        (np.cumsum(rng.integers(0, 64, (11 * PACKET + 4104) // 8)).astype(np.int64), "int64", None),
        ((np.arange((5 * PACKET + 2052) // 4) % 4096).astype(np.int32), "int32", None),
        (near, "bfloat16", near_base.view(np.uint8)),
        (same, "bfloat16", same.copy().view(np.uint8)),
        (far, "bfloat16", far_base.view(np.uint8)),
        (rng.integers(0, 256, 3 * PACKET + 1, dtype=np.uint8), "uint8", None),
        (synth.text(6, 20000), "uint8", None),
        (fp32, "uint8", None),
        (np.zeros(2 * PACKET + 100, dtype=np.uint8), "uint8", None),
        (np.empty(0, dtype=np.float32), "float32", None),
        (np.full(1, 9, dtype=np.uint8), "uint8", None),
        (np.full(2, 9, dtype=np.uint8), "uint8", None),
        (np.full(3, 9, dtype=np.uint8), "uint8", None),
        (walk, "uint8", None),
    ]
    for a, _d, _b in batch:
        a.setflags(write=False)
    return batch


_BATCH = _make_batch()
ARRAYS = [a for a, _d, _b in _BATCH]
DTYPES = [d for _a, d, _b in _BATCH]
BASES = [b for _a, _d, b in _BATCH]
SIZES = [_raw(a).size for a in ARRAYS]
N_PACKETS = sum(packets_of(n) for n in SIZES)
assert SIZES == [11 * PACKET + 4104, 5 * PACKET + 2052, 6 * PACKET + 100, 2 * PACKET + 100, 3 * PACKET, 3 * PACKET + 1, 20000, 4 * PACKET + 3,
                 2 * PACKET + 100, 0, 1, 2, 3, PACKET + 1]

# ---- the matrix ----------------------------------------------------------------------------------------------------------

PLANES_AXIS = {"none": None, "auto": "auto", "2": 2, "list": [8, 4, 2, 1, 2, 1, 1, 4, 2, 4, 1, 2, 8, 1], "survey": "survey"}
DELTA_LIST = [True, True, False, False, True, False, False, True, False, True, True, False, True, True]
FILTER_AXIS = {                                                     # the keywords delta, base and base_auto
    "none": {},
    "delta": {"delta": True},
    "delta_list": {"delta": DELTA_LIST},
    "delta_auto": {"delta": "auto"},
    "delta_survey": {"delta": "survey"},
    "base": {"base": BASES},
    "base_auto": {"base": BASES, "base_auto": True},
    "base_survey": {"base": BASES, "base_auto": "survey"},
}
STORED_AXIS = {"none": None, "auto": "auto", "list": [p % 3 == 0 for p in range(N_PACKETS)]}
SPARSE_AXIS = {"none": None, "auto": "auto"}
assert sorted(set(PLANES_AXIS["list"])) == [1, 2, 4, 8] and len(set(DELTA_LIST)) == 2


def combinations():
    """every (planes, filter, stored, sparse) by name, 240 of them"""
    return [(p, f, s, q) for p in PLANES_AXIS for f in FILTER_AXIS for s in STORED_AXIS for q in SPARSE_AXIS]


def is_refused(combo):
    """sparse="auto" beside a list of stored packets: the only refusal inside the matrix"""
    _p, _f, s, q = combo
    return s == "list" and q == "auto"


# Tensors 5 and 10-12 are raw under stored="auto" in every combination (that is what they are there for), so over the whole batch
# the raw kind is never empty under stored="auto", the coded kind never at all and the sparse kind never under sparse="auto".  Three
# parts of the batch fill that in, under the combinations of SUBSET_COMBOS: "calm" (text, zeros, nothing) has no packet that is kept
# raw; "still" (the tensor equal to its base, zeros, nothing) has under `base` only sparse packets with sparse="auto" and only coded
# ones without; "rough" (uniform bytes, text, one byte) has no sparse packet.
SUBSETS = {"calm": [6, 8, 9], "still": [3, 8, 9], "rough": [5, 6, 10]}
SUBSET_COMBOS = [("auto", f, s, q) for f in ("delta", "base", "base_survey") for s in ("none", "auto") for q in ("none", "auto")]


def keywords(combo, subset=None):
    """the keywords of model_compress / batch.compress for a combination (the bases as host arrays); `subset`: for that part of the
    batch (every per-tensor list cut down to it; a list of stored packets has no such part)"""
    p, f, s, q = combo
    kw = dict(FILTER_AXIS[f], planes=PLANES_AXIS[p], stored=STORED_AXIS[s], sparse=SPARSE_AXIS[q])
    if subset is not None:
        assert s != "list"
        for name in ("planes", "delta", "base"):
            if isinstance(kw.get(name), list):
                kw[name] = [kw[name][b] for b in SUBSETS[subset]]
    return kw


_MODELS = {}


def model(combo, checksum, subset=None):
    """model_compress of the batch (or of a part of it) for a combination, made once"""
    key = (combo, checksum, subset)
    if key not in _MODELS:
        which = range(len(ARRAYS)) if subset is None else SUBSETS[subset]
        _MODELS[key] = model_compress([ARRAYS[b] for b in which], [DTYPES[b] for b in which], checksum=checksum, **keywords(combo, subset))
    return _MODELS[key]
