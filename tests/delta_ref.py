"""Helpers of the delta-filter tests (not a test module): an independent numpy restatement of delta / undelta per group and tail
(gpuar_amd/csrc/delta.h), the definition read off index by index, split_delta / merge_delta composed with planes_ref, the .gip
trailer version 4 restated in Python, and the seeded inputs of DESIGN.md 4.9's table."""
import struct

import numpy as np

import planes_ref as P

PACKET = 8192
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
WIDTHS = (1, 2, 4, 8)
KINDS = ("uniform", "ones", "ramp")


def _pieces(n, w):
    """(start, elements) of every full group and of the tail's whole elements"""
    G = w * PACKET
    out = [(B, PACKET) for B in range(0, n // G * G, G)]
    e = n % G // w
    if e:
        out.append((n - n % G, e))
    return out


def numpy_delta(x, w):
    """d[0] = v[0], d[i] = v[i] - v[i - 1] mod 2^(8 w) inside every group and inside the tail's whole elements; the rest stays."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.uint8).reshape(-1))
    out = x.copy()
    for B, e in _pieces(x.size, w):
        v = x[B:B + e * w].view("<u%d" % w).astype(UINT[w])
        d = v.copy()
        d[1:] = v[1:] - v[:-1]                                   # unsigned: wraps
        out[B:B + e * w] = d.astype("<u%d" % w).view(np.uint8)
    return out


def numpy_undelta(x, w):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.uint8).reshape(-1))
    out = x.copy()
    for B, e in _pieces(x.size, w):
        d = x[B:B + e * w].view("<u%d" % w).astype(UINT[w])
        out[B:B + e * w] = np.cumsum(d, dtype=UINT[w]).astype("<u%d" % w).view(np.uint8)
    return out


def delta_by_definition(x, w):
    """The definition read off literally with Python integers (slow: for short inputs)."""
    x = bytes(x)
    n, G = len(x), w * PACKET
    out = bytearray(x)
    for B in range(0, n, G):
        e = min(G, n - B) // w
        prev = 0
        for i in range(e):
            v = int.from_bytes(x[B + i * w:B + i * w + w], "little")
            out[B + i * w:B + i * w + w] = ((v - prev) % (1 << 8 * w)).to_bytes(w, "little")
            prev = v
    return bytes(out)


def numpy_split_delta(x, w):
    return P.numpy_split(numpy_delta(x, w), w)


def numpy_merge_delta(x, w):
    return numpy_undelta(P.numpy_merge(x, w), w)


def lengths_for(w):
    G = w * PACKET
    return [0, 1, w - 1, w, 15, 16 * w + 1, 8191, 8192, G - 1, G, G + 1, 3 * G + 4097]


def bytes_of(kind, n, w, seed=0):
    """The three kinds of bytes of the grid: seeded uniform bytes (every difference wraps), all 0xFF (every prefix sum carries
    through every byte), and elements v[i] = i * 0x0101...01 truncated to w bytes (carries across byte planes)."""
    if kind == "uniform":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if kind == "ones":
        return np.full(n, 0xFF, dtype=np.uint8)
    if kind == "ramp":
        m = (n + w - 1) // w
        step = int.from_bytes(b"\x01" * w, "little")
        v = (np.arange(m, dtype=np.uint64) * np.uint64(step)).astype(UINT[w])
        return v.astype("<u%d" % w).view(np.uint8)[:n].copy()
    raise ValueError(kind)


def trailer_v4(clens, elem_bytes, crcs=None):
    """"GIPX" u32 4 u64 n | u32 elem_bytes | u32 flags (bit 0: CRCs, bit 1: delta, always set) | u16 clen[n] | pad to 4 |
    u32 crc32[n] if flags & 1 | pad to 8 | u64 trailer_bytes "XPIG"; pads are zeros, counted from "GIPX"."""
    n = len(clens)
    t = b"GIPX" + struct.pack("<I", 4) + struct.pack("<Q", n) + struct.pack("<I", elem_bytes) + struct.pack("<I", 2 | (1 if crcs is not None else 0))
    t += b"".join(struct.pack("<H", c) for c in clens)
    t += b"\0" * (-len(t) % 4)
    if crcs is not None:
        t += b"".join(struct.pack("<I", c) for c in crcs)
    t += b"\0" * (-len(t) % 8)
    return t + struct.pack("<Q", len(t) + 12) + b"XPIG"


TABLE = ("csr_offsets", "timestamps", "position_ids", "sorted_indices", "int16_walk", "uint8_walk", "unordered_int64", "fp32", "uniform")
TABLE_DELTA_WINS = TABLE[:6]


def table_inputs(n=1 << 18):
    """The nine inputs of the table in DESIGN.md 4.9, n elements each, from ONE np.random.default_rng(1) drawn in this order:
    {name: (array of its own type, element width)}."""
    rng = np.random.default_rng(1)
    out = {}
    out["csr_offsets"] = (np.cumsum(rng.integers(0, 64, n)).astype(np.int64), 8)
    out["timestamps"] = (np.cumsum(rng.normal(1e6, 2e3, n).astype(np.int64)), 8)
    out["position_ids"] = ((np.arange(n) % 4096).astype(np.int32), 4)
    out["sorted_indices"] = (np.sort(rng.choice(1 << 28, n, replace=False)).astype(np.int32), 4)
    out["int16_walk"] = (np.cumsum(rng.normal(0, 40, n)).astype(np.int64).astype(np.int16), 2)
    out["uint8_walk"] = ((np.cumsum(rng.normal(0, 2, n)).astype(np.int64) % 256).astype(np.uint8), 1)
    out["unordered_int64"] = (rng.integers(0, 50000, n).astype(np.int64), 8)
    out["fp32"] = ((rng.standard_normal(n) * 0.02).astype(np.float32), 4)
    out["uniform"] = (rng.integers(0, 256, 2 * n, dtype=np.uint8).view(np.uint16), 2)
    return out


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)
