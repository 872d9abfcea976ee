"""Helpers of the byte-plane tests (not a test module): an independent numpy restatement of the split / merge maps of
include/gpuar_hip.h, the .gip trailer version 3 restated in Python, and the seeded typed inputs the ratio tests code."""
import struct

import numpy as np

PACKET = 8192


def numpy_split(x, w):
    """Split: every full group of w * 8192 bytes is a (8192, w) array of bytes transposed to (w, 8192); the tail's e = r // w whole
    elements are an (e, w) array transposed to (w, e); the last r % w bytes stay."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.uint8).reshape(-1))
    out = x.copy()
    if w == 1:
        return out
    G = w * PACKET
    full = x.size // G * G
    if full:
        out[:full] = x[:full].reshape(-1, PACKET, w).transpose(0, 2, 1).reshape(-1)
    e = (x.size - full) // w
    if e:
        out[full:full + e * w] = x[full:full + e * w].reshape(e, w).T.reshape(-1)
    return out


def numpy_merge(x, w):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.uint8).reshape(-1))
    out = x.copy()
    if w == 1:
        return out
    G = w * PACKET
    full = x.size // G * G
    if full:
        out[:full] = x[:full].reshape(-1, w, PACKET).transpose(0, 2, 1).reshape(-1)
    e = (x.size - full) // w
    if e:
        out[full:full + e * w] = x[full:full + e * w].reshape(w, e).T.reshape(-1)
    return out


def split_by_definition(x, w):
    """The definition read off literally, index by index (slow: for short inputs)."""
    x = bytes(x)
    n, G = len(x), w * PACKET
    out = bytearray(x)
    for B in range(0, n, G):
        r = min(G, n - B)
        e = r // w
        for k in range(w):
            for i in range(e):
                out[B + k * e + i] = x[B + i * w + k]
    return bytes(out)


def trailer_v3(clens, elem_bytes, crcs=None):
    """"GIPX" u32 3 u64 n | u32 elem_bytes | u32 flags | u16 clen[n] | pad to 4 | u32 crc32[n] if flags & 1 | pad to 8 |
    u64 trailer_bytes "XPIG"; pads are zeros, counted from "GIPX"."""
    n = len(clens)
    t = b"GIPX" + struct.pack("<I", 3) + struct.pack("<Q", n) + struct.pack("<I", elem_bytes) + struct.pack("<I", 1 if crcs is not None else 0)
    t += b"".join(struct.pack("<H", c) for c in clens)
    t += b"\0" * (-len(t) % 4)
    if crcs is not None:
        t += b"".join(struct.pack("<I", c) for c in crcs)
    t += b"\0" * (-len(t) % 8)
    return t + struct.pack("<Q", len(t) + 12) + b"XPIG"


def packet_lengths(stream):
    """The u16 clen of every packet of a back-to-back packet stream."""
    stream = bytes(stream)
    out, at = [], 0
    while at < len(stream):
        c = stream[at] | stream[at + 1] << 8
        assert c >= 4 and at + c <= len(stream)
        out.append(c)
        at += c
    return out


def typed_input(kind, n_bytes, seed=1):
    """Seeded inputs of n_bytes bytes: normal x 0.02 as bf16 (fp32 rounded to nearest even on its upper 16 bits) or fp32, or
    uniform bytes."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 256, n_bytes, dtype=np.uint8)
    if kind == "fp32":
        return (rng.standard_normal(n_bytes // 4).astype(np.float32) * np.float32(0.02)).view(np.uint8)
    if kind == "bf16":
        bits = (rng.standard_normal(n_bytes // 2).astype(np.float32) * np.float32(0.02)).view(np.uint32)
        bits = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
        return bits.astype(np.uint16).view(np.uint8)
    raise ValueError(kind)
