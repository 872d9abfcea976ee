"""Helpers of the raw / sparse packet tests (not a test module): the stream form of gpuar_amd/csrc/kinds.h, the rule that picks a
packet's kind and the version-6 trailer of INTEGRATION.md section 4.1, restated in numpy / Python, and `file()`, which assembles a
whole .gip from them -- the coded packets from the oracle, the filter transforms from planes_ref / delta_ref / xor_ref.

    every packet: u16 clen (these 4 bytes included) | u16 ulen, then
        kind 0 coded   the bitstream                         kind 1 raw   the ulen bytes, clen = 4 + ulen
        kind 2 sparse  the record of sparse_ref.pack, clen = 4 + sparse_len(k)
    kind = sparse_ref.rule(scan, est, ulen, stored_on) with scan = NONE where sparse is off
    trailer: "GIPX" u32 6 u64 n | u32 elem_bytes | u32 flags (1 CRCs, 2 delta, 4 base, 8 kinds: always) | u16 clen[n] | pad to 4 |
             u32 crc32[n] if bit 0 | u8 kind[n] | pad to 8 | u64 trailer_bytes "XPIG"
"""
import struct
import zlib

import numpy as np

import delta_ref as D
import planes_ref as R
import sparse_ref as S
import xor_ref as X

PACKET = 8192
SLOT = 8704
HEADER = 20
CODED, RAW, SPARSE = 0, 1, 2
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 127, 128, 129, 4095, 4096, 8191, 8192)
MAX_EST = 8281           # 8192 bytes that hold each value 32 times


def _lg16(k):
    """floor(2^16 log2 k), exactly (integers only)"""
    e = k.bit_length() - 1
    r, m = e, k << (62 - e)
    for _ in range(16):
        m = (m * m) >> 62
        r <<= 1
        if m >> 63:
            m >>= 1
            r |= 1
    return r


_LF = [0, 0]
for _c in range(2, PACKET + 256):
    _LF.append(_LF[-1] + _lg16(_c))


def estimate(x):
    """est_clen of estimate.h: 4 + ceil(cost16 / 2^19) from the histogram alone"""
    x = np.asarray(x, dtype=np.uint8)
    h = np.bincount(x, minlength=256)
    cost = _LF[x.size + 255] - _LF[255] - sum(_LF[int(c)] for c in h)
    return 4 + ((cost + (1 << 19) - 1) >> 19)


def kind_of(x, stored, sparse):
    x = np.asarray(x, dtype=np.uint8)
    return S.rule(S.scan(x) if sparse else S.NONE, estimate(x), x.size, stored)


def store(x, stored, sparse):
    """(kind, packet bytes): the packet in its stream form; b"" for a coded one (the encoder's)"""
    x = np.asarray(x, dtype=np.uint8)
    kind = kind_of(x, stored, sparse)
    if kind == RAW:
        return kind, struct.pack("<HH", 4 + x.size, x.size) + x.tobytes()
    if kind == SPARSE:
        rec = S.pack(x)
        return kind, struct.pack("<HH", 4 + len(rec), x.size) + rec
    return kind, b""


def expand(pkt, kind, n):
    """the n bytes of the raw or sparse packet, or None for a packet that is not valid (and for any other kind)"""
    pkt = bytes(pkt)
    if kind not in (RAW, SPARSE) or len(pkt) < 4 or not 1 <= n <= PACKET:
        return None
    clen, ulen = struct.unpack("<HH", pkt[:4])
    if clen != len(pkt) or ulen != n:
        return None
    if kind == RAW:
        return np.frombuffer(pkt[4:], dtype=np.uint8).copy() if clen == 4 + ulen else None
    return S.unpack(pkt[4:], len(pkt) - 4, n)


def trailer_v6(clens, kinds, elem_bytes=1, crcs=None, delta=False, base=False):
    n = len(clens)
    assert len(kinds) == n and not (base and (delta or crcs is None))
    t = b"GIPX" + struct.pack("<IQII", 6, n, elem_bytes, (1 if crcs is not None else 0) | (2 if delta else 0) | (4 if base else 0) | 8)
    t += b"".join(struct.pack("<H", c) for c in clens)
    t += b"\0" * (-len(t) % 4)
    if crcs is not None:
        t += b"".join(struct.pack("<I", c) for c in crcs)
    t += bytes(kinds)
    t += b"\0" * (-len(t) % 8)
    return t + struct.pack("<Q", len(t) + 12) + b"XPIG"


def transformed(data, planes=1, delta=False, base=None):
    """the bytes that are coded: the input XORed with its base or delta-filtered, then split into planes"""
    x = np.asarray(data, dtype=np.uint8)
    if base is not None:
        return X.numpy_split_xor(x, np.asarray(base, dtype=np.uint8), planes)
    if delta:
        return D.numpy_split_delta(x, planes)
    return R.numpy_split(x, planes) if planes > 1 else x


def file(data, oracle, stored=False, sparse=False, planes=1, delta=False, base=None, checksum=False):
    """(the whole .gip `gpuar c --stored=auto / --sparse=auto ...` writes for `data`, the kind of every packet)"""
    x = np.asarray(data, dtype=np.uint8)
    assert stored or sparse
    coded = transformed(x, planes, delta, base)
    packets, kinds = [], []
    for at in range(0, x.size, PACKET):
        part = coded[at:at + PACKET]
        kind, pkt = store(part, stored, sparse)
        packets.append(pkt if kind != CODED else oracle.encode_packet(part))
        kinds.append(kind)
    stream = b"".join(packets)
    crcs = [zlib.crc32(x[at:at + PACKET].tobytes()) for at in range(0, x.size, PACKET)] if (checksum or base is not None) else None
    head = bytearray(HEADER)
    head[0:3] = bytes([0, 1, 0])
    head[4:12] = int(x.size).to_bytes(8, "little")
    head[12:20] = int(HEADER + len(stream)).to_bytes(8, "little")
    return bytes(head) + stream + trailer_v6([len(p) for p in packets], kinds, planes, crcs, delta, base is not None), kinds


# ---- packets ----------------------------------------------------------------------------------------------------------

TEXT = (b"It is a truth universally acknowledged, that a single man in possession of a good fortune, must be in want of a wife. "
        b"However little known the feelings or views of such a man may be on his first entering a neighbourhood, ") * 40


def _with_exceptions(n, fill, where):
    x = np.full(n, fill, dtype=np.uint8)
    where = np.asarray(where, dtype=np.int64)
    x[where] = (fill + 1 + np.arange(where.size) % 255) % 256
    return x


def packets():
    """[(name, packet)]: every length as zeros, uniform bytes and text; the fills 0x00 / 0x80 / 0xFF with k = 0, 1, 63, 64, 65, 127,
    128 exceptions spread over the packet; exceptions at position 0, at n - 1 and on either side of a 128-byte lane boundary; 128
    exceptions in one lane."""
    rng = np.random.default_rng(20)
    out = []
    for n in LENGTHS:
        out.append((f"zeros_n{n}", np.zeros(n, dtype=np.uint8)))
        out.append((f"uniform_n{n}", rng.integers(0, 256, n, dtype=np.uint8)))
        out.append((f"text_n{n}", np.frombuffer(TEXT[:n], dtype=np.uint8).copy()))
    for n in (4096, 8191, 8192):
        for fill in S.FILLS:
            for k in (0, 1, 63, 64, 65, 127, 128):
                out.append((f"fill{fill:02x}_k{k}_n{n}", _with_exceptions(n, fill, (np.arange(k) * (n // 129) + 7) if k else [])))
        out.append((f"ends_n{n}", _with_exceptions(n, 0x80, [0, 127, 128, n - 1])))
        out.append((f"one_lane_n{n}", _with_exceptions(n, 0xFF, np.arange(128) + 5 * 128)))
    for n in (129, 4095):
        out.append((f"ends_n{n}", _with_exceptions(n, 0x00, [0, 127, 128, n - 1])))
    return out


GOOD_N = S.GOOD_N


def damaged():
    """[(name, packet bytes, kind, n)]: packets that are not valid, one class at a time"""
    raw = struct.pack("<HH", 4 + 100, 100) + bytes(range(100))
    good = struct.pack("<HH", 4 + 16, GOOD_N) + S.pack(S.GOOD)
    assert expand(raw, RAW, 100) is not None and expand(good, SPARSE, GOOD_N) is not None
    out = [
        ("kind_3", raw, 3, 100),
        ("kind_0", raw, 0, 100),
        ("raw_clen_short", struct.pack("<HH", 4 + 99, 100) + bytes(range(100)), RAW, 100),
        ("raw_clen_long", struct.pack("<HH", 4 + 101, 100) + bytes(range(100)), RAW, 100),
        ("raw_clen_not_4_plus_ulen", struct.pack("<HH", 4 + 101, 100) + bytes(101), RAW, 100),
        ("raw_ulen_other_than_n", raw, RAW, 99),
        ("raw_ulen_0", struct.pack("<HH", 4, 0), RAW, 1),
        ("raw_ulen_above_8192", struct.pack("<HH", 4 + 8193, 8193) + bytes(8193), RAW, 8192),
        ("raw_clen_above_8704", struct.pack("<HH", 8705, 8192) + bytes(8701), RAW, 8192),
        ("raw_3_bytes", raw[:3], RAW, 100),
        ("sparse_clen_other_than_the_packet", struct.pack("<HH", 4 + 12, GOOD_N) + S.pack(S.GOOD), SPARSE, GOOD_N),
        ("sparse_ulen_other_than_n", good, SPARSE, GOOD_N - 1),
        ("sparse_header_only", struct.pack("<HH", 4, GOOD_N), SPARSE, GOOD_N),
    ]
    for name, rec, rec_bytes, n in S.damaged():
        held = rec[:rec_bytes]
        out.append((f"sparse_{name}", struct.pack("<HH", 4 + len(held), n) + held, SPARSE, n))
    return out


# ---- the files of the CLI tests ------------------------------------------------------------------------------------------

CLI_SIZES = (8 * PACKET + 5, 20 * PACKET + 4097)
CLI_CONTENTS = ("zeros", "uniform", "text", "bf16", "bf16_base_equal", "bf16_base_0.1%", "sorted_int32")
CLI_OPTIONS = ((True, False), (False, True), (True, True))       # (stored, sparse)


def cli_input(content, n):
    """(input bytes, base bytes or None, CLI flags, the same as keywords of file()) of one content at n bytes"""
    rng = np.random.default_rng(CLI_CONTENTS.index(content) * 1000 + n % 997)
    if content == "zeros":
        return np.zeros(n, dtype=np.uint8), None, [], {}
    if content == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8), None, [], {}
    if content == "text":
        return np.frombuffer((TEXT * (n // len(TEXT) + 1))[:n], dtype=np.uint8).copy(), None, [], {}
    if content.startswith("bf16"):
        weights = rng.standard_normal(n // 2 + 1).astype(np.float32) * np.float32(0.02)
        x = X.bf16(weights).view(np.uint8)[:n].copy()
        if content == "bf16":
            return x, None, ["--planes=2"], {"planes": 2}
        base = x.copy()
        if content == "bf16_base_0.1%":
            elements = base[:n // 2 * 2].view(np.uint16)
            where = rng.choice(elements.size, max(1, elements.size // 1000), replace=False)
            elements[where] = X.bf16(rng.standard_normal(where.size).astype(np.float32) * np.float32(0.02))
        return x, base, ["--planes=2"], {"planes": 2}
    assert content == "sorted_int32"
    values = np.sort(rng.integers(0, 1 << 30, n // 4 + 1, dtype=np.int64)).astype("<i4")
    return values.view(np.uint8)[:n].copy(), None, ["--planes=4", "--delta"], {"planes": 4, "delta": True}


def cli_flags(stored, sparse):
    return (["--stored=auto"] if stored else []) + (["--sparse=auto"] if sparse else [])
