"""Helpers of the XOR-base tests (not a test module): the numpy oracle of split_xor / merge_xor, the lengths every width is
tested at, the .gip trailer version 5 restated in Python, and the seeded checkpoint pairs of the gain table."""
import struct

import numpy as np

import planes_ref as R

PACKET = 8192
WIDTHS = (1, 2, 4, 8)


def lengths_for(w):
    G = w * PACKET
    return sorted({0, 1, 7, 8, 9, 15, 16, 17, 8191, 8192, 8193, G - 1, G, G + 1, 65537, 3 * G + 24653})


def pair(n, seed):
    """(buffer, base): two seeded arrays of n uniform bytes"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)


def numpy_split_xor(x, b, w):
    return R.numpy_split(np.asarray(x, dtype=np.uint8) ^ np.asarray(b, dtype=np.uint8), w)


def numpy_merge_xor(s, b, w):
    return R.numpy_merge(s, w) ^ np.asarray(b, dtype=np.uint8)


def trailer_v5(clens, elem_bytes, crcs):
    """"GIPX" u32 5 u64 n | u32 elem_bytes | u32 flags = 5 (CRCs, base) | u16 clen[n] | pad to 4 | u32 crc32[n] | pad to 8 |
    u64 trailer_bytes "XPIG"; pads are zeros, counted from "GIPX"."""
    n = len(clens)
    t = b"GIPX" + struct.pack("<IQII", 5, n, elem_bytes, 5)
    t += b"".join(struct.pack("<H", c) for c in clens)
    t += b"\0" * (-len(t) % 4)
    t += b"".join(struct.pack("<I", c) for c in crcs)
    t += b"\0" * (-len(t) % 8)
    return t + struct.pack("<Q", len(t) + 12) + b"XPIG"


def bf16(a):
    """fp32 -> bf16 bits, round to nearest even"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


TABLE_BASE_WINS = ("step_1e-3", "step_1e-4", "step_1e-5", "one_percent")
TABLE_BASE_LOSES = ("unrelated", "uniform")


def table_pairs(elements=1 << 19, seed=1):
    """{name: (tensor bytes, base bytes, w)}: bf16 weights normal x 0.02 as the base; the tensor is the base moved by a normal step of
    1e-3, 1e-4 or 1e-5 (in fp32, then rounded to bf16), the base with 1 % of its elements replaced, or an unrelated tensor; and
    uniform bytes against uniform bytes."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(elements).astype(np.float32) * np.float32(0.02)
    out = {}
    for name, step in (("step_1e-3", 1e-3), ("step_1e-4", 1e-4), ("step_1e-5", 1e-5)):
        out[name] = base + rng.standard_normal(elements).astype(np.float32) * np.float32(step)
    fresh = rng.standard_normal(elements).astype(np.float32) * np.float32(0.02)
    changed = base.copy()
    where = rng.choice(elements, elements // 100, replace=False)
    changed[where] = fresh[where]
    out["one_percent"] = changed
    out["unrelated"] = rng.standard_normal(elements).astype(np.float32) * np.float32(0.02)
    pairs = {name: (bf16(a).view(np.uint8), bf16(base).view(np.uint8), 2) for name, a in out.items()}
    pairs["uniform"] = (rng.integers(0, 256, 2 * elements, dtype=np.uint8), rng.integers(0, 256, 2 * elements, dtype=np.uint8), 2)
    return pairs
