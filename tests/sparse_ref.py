"""Helpers of the sparse-packet tests (not a test module): the definitions of gpuar_amd/csrc/sparse.h restated in numpy (scan,
record, validity, rule), the packets every implementation is tested on, the damaged records, one class each, and the rule's table."""
import struct

import numpy as np

import xor_ref as X

PACKET = 8192
NONE = 0xFFFFFFFF
CODED, RAW, SPARSE = 0, 1, 2
LENGTHS = (1, 2, 3, 15, 16, 17, 127, 128, 129, 4097, 8191, 8192)
FILLS = (0x00, 0x80, 0xFF)


def sparse_len(k):
    return (4 + 3 * k + 3) & ~3


def scan(x):
    """(k << 8) | f for the packet's majority byte f (2 count(f) > n) and its k exceptions, else NONE"""
    x = np.asarray(x, dtype=np.uint8)
    h = np.bincount(x, minlength=256)
    f = int(h.argmax())
    return ((x.size - int(h[f])) << 8) | f if 2 * int(h[f]) > x.size else NONE


def pack(x):
    """the packet's record, or None for a packet without a majority byte"""
    x = np.asarray(x, dtype=np.uint8)
    s = scan(x)
    if s == NONE:
        return None
    fill, k = s & 255, s >> 8
    where = np.flatnonzero(x != fill)
    assert where.size == k
    rec = struct.pack("<BBH", fill, 0, k) + where.astype("<u2").tobytes() + x[where].tobytes()
    return rec + bytes(sparse_len(k) - len(rec))


def unpack(rec, rec_bytes, n):
    """the packet of n bytes from the first rec_bytes bytes of rec, or None for a record that is not valid"""
    rec = bytes(rec)[:rec_bytes]
    if rec_bytes < 4 or len(rec) < 4:
        return None
    fill, reserved, k = struct.unpack("<BBH", rec[:4])
    if reserved != 0 or not 2 * k < n or sparse_len(k) > rec_bytes:
        return None
    pos = np.frombuffer(rec, dtype="<u2", count=k, offset=4).astype(np.int64)
    val = np.frombuffer(rec, dtype=np.uint8, count=k, offset=4 + 2 * k)
    if (pos >= n).any() or (np.diff(pos) <= 0).any() or (val == fill).any():
        return None
    out = np.full(n, fill, dtype=np.uint8)
    out[pos] = val
    return out


def rule(scan_word, est, n, stored_on):
    raw_ok = bool(stored_on) and est >= 4 + n
    s = sparse_len(scan_word >> 8) if scan_word != NONE else float("inf")
    if s + 1 < est and (not raw_ok or s < n):
        return SPARSE
    return RAW if raw_ok else CODED


def _packet(n, fill, where, values=None):
    x = np.full(n, fill, dtype=np.uint8)
    where = np.asarray(where, dtype=np.int64)
    x[where] = (fill + 1 + np.arange(where.size) % 255) % 256 if values is None else values      # never the fill
    return x


def cases():
    """[(name, packet)]: every length with no exception, with count(f) exactly n/2 (not sparse) and n/2 + 1 (sparse) and with
    exceptions at the packet's ends and at a lane boundary (127 | 128); 128 consecutive exceptions in one lane; one exception in
    each of the 64 lanes; every fill with exception values covering all other byte values.  The fills rotate over the cases."""
    out, turn = [], 0

    def add(name, n, where, values=None, fill=None):
        nonlocal turn
        f = FILLS[turn % 3] if fill is None else fill
        turn += 1
        if all(have != f"{name}_n{n}_f{f:02x}" for have, _x in out):         # (the rotation may have made it already)
            out.append((f"{name}_n{n}_f{f:02x}", _packet(n, f, where, values)))

    for n in LENGTHS:
        add("k0", n, [])
        add("half", n, np.arange(n - n // 2) * 2)                            # count(f) = n / 2 rounded down: f is no majority
        if n // 2 + 1 <= n:
            add("half_plus_1", n, np.arange(n - (n // 2 + 1)) * 2 + 1)       # count(f) = n / 2 + 1: the most exceptions a packet has
        ends = sorted({p for p in (0, n - 1, 127, 128) if p < n})
        if 2 * len(ends) < n:
            add("ends", n, ends)
    for n in (4097, 8191, 8192):
        add("one_lane", n, np.arange(128) + 3 * 128)
        lanes = np.arange((n + 127) // 128)
        at = lanes * 128 + (lanes * 37) % 128
        add("every_lane", n, at[at < n])
    for f in FILLS:
        others = np.array([v for v in range(256) if v != f], dtype=np.uint8)
        add("all_values", PACKET, (np.arange(255) * 32 + 5), others, fill=f)
    # the three fills at the full length, at either side of the majority
    for f in FILLS:
        add("k0", PACKET, [], fill=f)
        add("half", PACKET, np.arange(PACKET // 2) * 2, fill=f)
        add("half_plus_1", PACKET, np.arange(PACKET // 2 - 1) * 2 + 1, fill=f)
    return out


GOOD_N = 300
GOOD = _packet(GOOD_N, 7, [5, 130, 131, 299], np.array([1, 2, 3, 4], dtype=np.uint8))       # record: 16 bytes, k = 4


def _patched(rec, at, data):
    rec = bytearray(rec)
    rec[at:at + len(data)] = data
    return bytes(rec)


def damaged():
    """[(name, record bytes, rec_bytes, n)]: records that are not valid, one class at a time (every other rule holds)"""
    good = pack(GOOD)
    assert len(good) == 16 and unpack(good, 16, GOOD_N) is not None
    small = pack(_packet(9, 7, [0, 1, 2, 3]))                                # valid for n = 9 (k = 4), not for n = 8
    return [
        ("k_too_large_for_n", small, len(small), 8),
        ("record_longer_than_rec_bytes", good, 12, GOOD_N),
        ("rec_bytes_3", good, 3, GOOD_N),
        ("rec_bytes_0", good, 0, GOOD_N),
        ("pos_equals_n", _patched(good, 4 + 6, struct.pack("<H", GOOD_N)), 16, GOOD_N),
        ("pos_far_beyond_n", _patched(good, 4 + 6, struct.pack("<H", 0xFFFF)), 16, GOOD_N),
        ("descending_positions", _patched(good, 4 + 2, struct.pack("<HH", 131, 130)), 16, GOOD_N),
        ("duplicate_position", _patched(good, 4 + 4, struct.pack("<H", 130)), 16, GOOD_N),
        ("reserved_byte", _patched(good, 1, b"\x01"), 16, GOOD_N),
        ("value_equals_fill", _patched(good, 4 + 8 + 2, b"\x07"), 16, GOOD_N),
    ]


# (scan, est, n, stored_on, kind): worked out by hand from the rule's text
RULE_TABLE = [
    (0x07, 5, 1, True, RAW),                     # one byte: est 5 >= 4 + 1, and the record (4) is no smaller than the byte
    (0x07, 5, 1, False, CODED),                  # ... 4 + 1 < 5 is false
    (0x07, 8, 4, True, RAW),                     # a tie with raw (record 4 bytes, packet 4 bytes) goes to raw
    (0x07, 8, 4, False, SPARSE),
    (0x07, 9, 5, True, SPARSE),                  # the record is smaller than the packet
    (0x07, 6, 5, True, SPARSE),                  # est < 4 + n: raw is not in question, and 4 + 1 < 6
    (0x07, 5, 5, False, CODED),                  # 4 + 1 < 5 is false
    (0x00, 210, 8192, True, SPARSE),             # 8192 equal bytes
    (0x00, 210, 8192, False, SPARSE),
    ((68 << 8) | 0x80, 210, 8192, False, SPARSE),        # 208 + 1 < 210
    ((69 << 8) | 0x80, 210, 8192, False, CODED),         # 212
    ((69 << 8) | 0x80, 213, 8192, True, CODED),          # 212 + 1 < 213 is false: the estimate's resolution
    ((69 << 8) | 0x80, 214, 8192, True, SPARSE),
    (NONE, 9000, 8192, True, RAW),
    (NONE, 9000, 8192, False, CODED),
    (NONE, 100, 8192, True, CODED),
    ((7 << 8) | 0xFF, 25, 16, True, RAW),        # record 28: not under the estimate
    ((7 << 8) | 0xFF, 40, 16, True, RAW),        # under the estimate, but not under the packet's 16 bytes
    ((7 << 8) | 0xFF, 40, 16, False, SPARSE),
    ((4095 << 8) | 0x00, 8300, 8192, True, RAW), # the longest record, 12292 bytes
    ((4095 << 8) | 0x00, 12294, 8192, False, SPARSE),
]


def xor_base_cases(elements=1 << 19, seed=1):
    """{name: (tensor bytes, base bytes, w)}: the XOR-base cases whose sizes README.md and DESIGN.md 4.12 quote.  One generator,
    drawn from in this order: the base (bf16 weights, normal x 0.02), a fresh tensor of the same kind, then for "replaced_0.1%" and
    for "replaced_1%" in turn the elements to replace (rng.choice without replacement), which take the fresh tensor's values;
    "equal" is the base itself."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(elements).astype(np.float32) * np.float32(0.02)
    fresh = rng.standard_normal(elements).astype(np.float32) * np.float32(0.02)
    out = {"equal": base}
    for name, share in (("replaced_0.1%", 0.001), ("replaced_1%", 0.01)):
        changed = base.copy()
        where = rng.choice(elements, int(elements * share), replace=False)
        changed[where] = fresh[where]
        out[name] = changed
    return {name: (X.bf16(a).view(np.uint8), X.bf16(base).view(np.uint8), 2) for name, a in out.items()}
