"""Helpers of the .gip reader tests (not a test module): the files `gpuar-host c` writes under every option that leaves a trace in
a file, what a reader must find in each -- restated from the inputs, the flags and the trailer writers of trailer_ref / delta_ref /
kinds_ref, never from the reader under test --, and the damaged files the reader must refuse."""
import os
import struct
import subprocess
import zlib

import numpy as np

import client_build as B
import delta_ref as D
import kinds_ref as K
import trailer_ref as T

PACKET, SLOT, HEADER = 8192, 8704, 20
SIZES = (0, 1, PACKET, PACKET + 1, 3 * PACKET + 4097)
FAMILIES = ("zeros", "text", "uniform", "sparse")

# (name, CLI flags, what they say: version, elem_bytes, crcs, delta, base, stored, sparse)
FLAG_SETS = [
    ("plain", [], dict(version=0)),
    ("index", ["--index"], dict(version=1)),
    ("checksum", ["--checksum"], dict(version=2, crcs=True)),
    ("planes2", ["--planes=2"], dict(version=3, elem=2)),
    ("planes4", ["--planes=4"], dict(version=3, elem=4)),
    ("planes8", ["--planes=8"], dict(version=3, elem=8)),
    ("delta_planes2", ["--delta", "--planes=2"], dict(version=4, elem=2, delta=True)),
    ("delta_planes4", ["--delta", "--planes=4"], dict(version=4, elem=4, delta=True)),
    ("base_planes2", ["--planes=2"], dict(version=5, elem=2, crcs=True, base=True)),
    ("stored", ["--stored=auto"], dict(version=6, stored=True)),
    ("sparse", ["--sparse=auto"], dict(version=6, sparse=True)),
    ("stored_sparse", ["--stored=auto", "--sparse=auto"], dict(version=6, stored=True, sparse=True)),
    ("stored_checksum", ["--stored=auto", "--checksum"], dict(version=6, stored=True, crcs=True)),
    ("sparse_checksum", ["--sparse=auto", "--checksum"], dict(version=6, sparse=True, crcs=True)),
    ("stored_sparse_checksum", ["--stored=auto", "--sparse=auto", "--checksum"], dict(version=6, stored=True, sparse=True, crcs=True)),
]


def family(name, n, seed=0):
    """n bytes of one family: zeros, text, uniform bytes, or one value with a few exceptions (the families of sparse_ref / kinds_ref)"""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + n % 997 + seed)
    if name == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if name == "text":
        return np.frombuffer((K.TEXT * (n // len(K.TEXT) + 1))[:n], dtype=np.uint8).copy()
    if name == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    x = np.full(n, 0x80, dtype=np.uint8)
    where = rng.choice(n, n // 300, replace=False) if n else np.zeros(0, dtype=np.int64)
    x[where] = rng.integers(0, 0x80, where.size, dtype=np.uint8)
    return x


def base_of(x):
    """a base for x: x itself with one element in a thousand changed"""
    base = x.copy()
    base[::977] ^= 0x11
    return base


def write(tmp, data, flags, base=None):
    """the file `gpuar-host c --host` writes for `data` (a uint8 array) with `flags` (and --base=, where `base` is given)"""
    B.ensure_products()
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.gip")
    np.asarray(data, dtype=np.uint8).tofile(src)
    extra = []
    if base is not None:
        np.asarray(base, dtype=np.uint8).tofile(os.path.join(str(tmp), "base.bin"))
        extra = ["--base=" + os.path.join(str(tmp), "base.bin")]
    r = subprocess.run([B.CLI_HOST, "c", "--host", "--nointeractive", f"--in={src}", f"--out={dst}", *flags, *extra], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (flags, r.stderr)
    with open(dst, "rb") as f:
        return f.read()


def walk(blob):
    """(clens, ulens, where the stream ends) from the packet headers alone: `off += clen` from byte 20 to the header's size"""
    end = struct.unpack("<I", blob[12:16])[0]
    at, clens, ulens = HEADER, [], []
    while at < end:
        clen, ulen = struct.unpack("<HH", blob[at:at + 4])
        assert 4 <= clen <= end - at
        clens.append(clen)
        ulens.append(ulen)
        at += clen
    return clens, ulens, end


def trailer_v5(clens, elem_bytes, crcs):
    """"GIPX" u32 5 u64 n | u32 elem_bytes | u32 flags = 5 (CRCs, base) | u16 clen[n] | pad to 4 | u32 crc32[n] | pad to 8 |
    u64 trailer_bytes "XPIG"; pads are zeros, counted from "GIPX"."""
    t = b"GIPX" + struct.pack("<IQII", 5, len(clens), elem_bytes, 5)
    t += b"".join(struct.pack("<H", c) for c in clens)
    t += b"\0" * (-len(t) % 4)
    t += b"".join(struct.pack("<I", c) for c in crcs)
    t += b"\0" * (-len(t) % 8)
    return t + struct.pack("<Q", len(t) + 12) + b"XPIG"


def expected(blob, data, says, base=None):
    """What a reader must find in `blob`, the file of `data` written with the options `says` (a FLAG_SETS entry): a dict of
    uncompressed, stream_begin, stream_end, version, elem_bytes, flags, clens, crcs, kinds -- and the assertion that the file's
    trailer is, byte for byte, what the restated writers make of them."""
    x = np.asarray(data, dtype=np.uint8)
    clens, ulens, end = walk(blob)
    n = (x.size + PACKET - 1) // PACKET
    assert len(clens) == n and ulens == [min(PACKET, x.size - p * PACKET) for p in range(n)]
    version, elem = says["version"], says.get("elem", 1)
    crcs = [zlib.crc32(x[p * PACKET:(p + 1) * PACKET].tobytes()) for p in range(n)] if says.get("crcs") else None
    delta, based = bool(says.get("delta")), bool(says.get("base"))
    kinds = None
    if version == 6:
        coded = K.transformed(x, elem, delta, base if based else None)
        kinds = [K.kind_of(coded[p * PACKET:(p + 1) * PACKET], bool(says.get("stored")), bool(says.get("sparse"))) for p in range(n)]
        tail = K.trailer_v6(clens, kinds, elem, crcs, delta, based)
    elif version == 5:
        tail = trailer_v5(clens, elem, crcs)
    elif version == 4:
        tail = D.trailer_v4(clens, elem, crcs)
    elif version == 0:
        tail = b""
    else:
        tail = T.write(clens, elem, crcs)
    assert blob[end:] == tail, (says, len(blob) - end, len(tail))
    flags = 0 if version < 2 else (1 if crcs is not None else 0) | (2 if delta else 0) | (4 if based else 0) | (8 if version == 6 else 0)
    return dict(uncompressed=x.size, stream_begin=HEADER, stream_end=end, version=version, elem_bytes=elem, flags=flags, clens=clens,
                crcs=crcs, kinds=kinds)


def fields(g):
    """the same dict from a batch.GipFile"""
    return dict(uncompressed=g.uncompressed, stream_begin=g.stream_begin, stream_end=g.stream_end, version=g.version, elem_bytes=g.elem_bytes,
                flags=g.flags, clens=g.clens.tolist(), crcs=None if g.crcs is None else g.crcs.tolist(),
                kinds=None if g.kinds is None else g.kinds.tolist())


def garbage_header(blob):
    """the file with header bytes 3, 8 .. 11 and 16 .. 19 overwritten, as a reference-written file has them (uninitialised)"""
    d = bytearray(blob)
    d[3] = 0xA5
    d[8:12] = b"\xDE\xAD\xBE\xEF"
    d[16:20] = b"\xFE\xED\xFA\xCE"
    return bytes(d)


def patched(blob, at, data):
    d = bytearray(blob)
    d[at:at + len(data)] = data
    return bytes(d)
