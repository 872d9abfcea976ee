"""Helpers of the file-pipeline tests (not a test module): one input whose 64-packet segments are the chunks of `--batch=64`, the
flag sets and pipeline shapes it is sent through, a runner that starts nothing after a child ended badly, files spliced from several
`--host` files (short packets in the middle of a stream) and the damaged files of the matrix.  What a file must hold is restated by
gip_files.expected; what a spliced file decodes to is the concatenation of its parts."""
import os
import struct
import zlib

import numpy as np

import client_build as B
import gip_files as G
import kinds_ref as K
import trailer_ref as T

PACKET, HEADER = 8192, 20
CHUNK = 64                      # packets of a `--batch=64` chunk

# gip_files.FLAG_SETS and six more: (name, CLI flags, what they say); `base=True`: --base=FILE goes with them
FLAG_SETS = G.FLAG_SETS + [
    ("delta", ["--delta"], dict(version=4, elem=1, delta=True)),
    ("base", [], dict(version=5, elem=1, crcs=True, base=True)),
    ("delta_planes8_checksum_index", ["--planes=8", "--delta", "--checksum", "--index"], dict(version=4, elem=8, delta=True, crcs=True)),
    ("delta_planes4_stored_sparse_checksum", ["--planes=4", "--delta", "--stored=auto", "--sparse=auto", "--checksum"],
     dict(version=6, elem=4, delta=True, stored=True, sparse=True, crcs=True)),
    ("base_planes2_stored_sparse", ["--planes=2", "--stored=auto", "--sparse=auto"],
     dict(version=6, elem=2, base=True, crcs=True, stored=True, sparse=True)),
    ("base_sparse", ["--sparse=auto"], dict(version=6, elem=1, base=True, crcs=True, sparse=True)),
]
FLAGS = {name: (flags, says) for name, flags, says in FLAG_SETS}

# (name, argv tail, environment): how the pipeline cuts the file and deals the chunks.  By default a file is cut so that each of the
# three lanes gets a chunk (whole multiples of 64 packets): one chunk -- and the encoder's own choice of kernel -- up to 64 packets.
OVERSUBSCRIBE = {"GPUAR_OVERSUBSCRIBE_DEVICES": "1"}
SHAPES = [
    ("default", [], {}),
    ("batch64", ["--batch=64"], {}),
    ("batch100", ["--batch=100"], {}),                       # rounds down to 64
    ("gpus2_batch64", ["--gpus=2", "--batch=64"], OVERSUBSCRIBE),
    ("gpus3", ["--gpus=3"], OVERSUBSCRIBE),
    ("batch128_no_mmap", ["--batch=128"], {"GPUAR_NO_MMAP": "1"}),
]
SHAPE = {name: (argv, env) for name, argv, env in SHAPES}


# ---- the input ----------------------------------------------------------------------------------------------------------

def _sorted_int32(n, seed):
    values = np.sort(np.random.default_rng(seed).integers(0, 1 << 30, n // 4 + 1, dtype=np.int64)).astype("<i4")
    return values.view(np.uint8)[:n].copy()


def matrix_input():
    """(input, base): 6 segments of 64 packets and a ragged tail --
        0 uniform bytes | 1 zeros | 2 text | 3 32 packets uniform, 32 of gip_files.family("sparse") |
        4 zeros / uniform / text / sparse, packet by packet | 5 sorted little-endian int32 | 17 packets of text and 4097 bytes.
    The base is the input with every 977th byte XORed with 0x11, except where the input is uniform bytes (segment 0, the first half of
    segment 3, every fourth packet of segment 4): there the base is independent uniform bytes, so those packets stay incompressible
    after the XOR.  (Over segment 0 alone, every other packet of a --base file would be sparse: no coded packet, no chunk of two
    kinds.)"""
    seg = CHUNK * PACKET
    cycle = ("zeros", "uniform", "text", "sparse")
    parts = [G.family("uniform", seg, 1), G.family("zeros", seg), G.family("text", seg),
             np.concatenate([G.family("uniform", seg // 2, 2), G.family("sparse", seg // 2, 3)]),
             np.concatenate([G.family(cycle[p % 4], PACKET, 10 + p) for p in range(CHUNK)]),
             _sorted_int32(seg, 5), G.family("text", 17 * PACKET + 4097, 6)]
    x = np.concatenate(parts)
    base = G.base_of(x)
    other = np.random.default_rng(99).integers(0, 256, x.size, dtype=np.uint8)
    uniform = [(0, seg), (3 * seg, 3 * seg + seg // 2)] + [(4 * seg + p * PACKET, 4 * seg + (p + 1) * PACKET) for p in range(1, CHUNK, 4)]
    for begin, end in uniform:
        base[begin:end] = other[begin:end]
    return x, base


def kinds_of(x, base, says):
    """the kind of every packet of `x` under a flag set, from kinds_ref alone"""
    coded = K.transformed(x, says.get("elem", 1), bool(says.get("delta")), base if says.get("base") else None)
    return [K.kind_of(coded[at:at + PACKET], bool(says.get("stored")), bool(says.get("sparse"))) for at in range(0, x.size, PACKET)]


# ---- children -----------------------------------------------------------------------------------------------------------

_children = B.Children()        # one for the process: after a child that ended badly nothing more is started, in any module


def run_cli(exe, mode, src, dst, args=(), env=None, timeout=120):
    """`exe c|d --in=src --out=dst args` under a time limit of its own.  A child that ends on a signal, with status 134 or 139 or
    at its limit fails the test -- and every later run_cli of the process fails at once, without starting a child."""
    B.ensure_products()
    return _children.run([exe, mode, "--nointeractive", f"--in={src}", f"--out={dst}", *args], timeout,
                         env=dict(os.environ, **env) if env else None)


def host(mode, src, dst, args=(), timeout=300):
    return run_cli(B.CLI_HOST, mode, src, dst, ["--host", "--threads=0", *args], timeout=timeout)


def gpu(mode, src, dst, shape="default", args=(), timeout=120, env=None):
    argv, shape_env = SHAPE[shape]
    r = run_cli(B.CLI, mode, src, dst, [*argv, *args], env=dict(shape_env, **(env or {})), timeout=timeout)
    assert "Attention" not in r.stdout, "the host path ran"
    return r


# ---- spliced files ------------------------------------------------------------------------------------------------------

def header(uncompressed, stream_bytes):
    """the 20 bytes of file_header.hpp: 0, 1, 0, a spare byte, u64 uncompressed size, u64 offset of the stream's end"""
    return bytes([0, 1, 0, 0]) + struct.pack("<QQ", uncompressed, HEADER + stream_bytes)


def spliced(tmp, parts, trailer=None):
    """(blob, data): one .gip of the packet streams of the `--host` files of `parts` (uint8 arrays) back to back, behind a header with
    the summed sizes, and the concatenated input.  `trailer`: None, "index" (version 1), "crcs" (version 2, the true CRC-32 of what
    every packet holds) or "planes" (version 3, W = 2)."""
    stream, clens, crcs = b"", [], []
    for x in parts:
        blob = G.write(tmp, x, [])
        part_clens, ulens, end = G.walk(blob)
        assert end == len(blob) and sum(ulens) == x.size
        stream += blob[HEADER:]
        clens += part_clens
        at = 0
        for u in ulens:
            crcs.append(zlib.crc32(x[at:at + u].tobytes()))
            at += u
    data = np.concatenate(parts)
    tail = {None: b"", "index": T.write(clens, 1, None), "crcs": T.write(clens, 1, crcs), "planes": T.write(clens, 2, None)}[trailer]
    return header(data.size, len(stream)) + stream + tail, data.tobytes()


SPLICE_SIZES = (63 * PACKET + 100, 1, PACKET + 4097, 1, 64 * PACKET, 30 * PACKET + 7, 5)
SPLICE_TRAILERS = (None, "index", "crcs", "planes")


def splice_parts():
    return [G.family(G.FAMILIES[i % 4], n, seed=20 + i) for i, n in enumerate(SPLICE_SIZES)]


def splice_ulens(sizes=SPLICE_SIZES):
    """what every packet of the spliced file holds, and the assertion that the short ones sit where the pipeline's paths part"""
    ulens = [u for n in sizes for u in [PACKET] * (n // PACKET) + ([n % PACKET] if n % PACKET else [])]
    short = [p for p, u in enumerate(ulens[:-1]) if u < PACKET]
    n_chunks = (len(ulens) + CHUNK - 1) // CHUNK
    assert any(p % CHUNK == CHUNK - 1 and p // CHUNK < n_chunks - 1 and all(u == PACKET for u in ulens[p - CHUNK + 1:p]) for p in short), \
        "a short packet that ends a chunk of otherwise full ones, not the last chunk"
    assert any(0 < p % CHUNK < CHUNK - 1 for p in short), "a short packet in the middle of a chunk"
    assert any(p % CHUNK == 0 for p in short), "a short packet that begins a chunk"
    assert any(ulens[p] == 1 for p in short), "a packet of one byte"
    assert any(p + 1 in short and p // CHUNK == (p + 1) // CHUNK for p in short), "two short packets side by side in one chunk"
    return ulens, short


def splice_verdicts(tmp, splices):
    """{trailer: (exit status, stderr class, output or None)} of `gpuar-host d --host`: what the GPU test expects of `gpuar d`"""
    out = {}
    for trailer, (blob, _data) in splices.items():
        (tmp / "s.gip").write_bytes(blob)
        r = host("d", tmp / "s.gip", tmp / "s.out")
        out[trailer] = (r.returncode, T.stderr_class(r.returncode, r.stderr), (tmp / "s.out").read_bytes() if r.returncode == 0 else None)
    return out


# ---- damaged files ------------------------------------------------------------------------------------------------------

def packet_offsets(blob):
    clens, _ulens, _end = G.walk(blob)
    return [HEADER + sum(clens[:p]) for p in range(len(clens))] + [HEADER + sum(clens)]


def damaged(blob, kinds, chunk=3):
    """[(what, blob, file offsets of the chunk's first byte and of the one behind its last)]: `blob` with one packet of `--batch=64`
    chunk `chunk` damaged -- a coded packet that says it holds more than it does, a raw packet with another payload byte, a sparse
    record with another count -- as far as `kinds` (or None: all coded) has such packets in that chunk."""
    at = packet_offsets(blob)
    kinds = kinds if kinds is not None else [K.CODED] * (len(at) - 1)
    out, begin, end = [], at[chunk * CHUNK], at[(chunk + 1) * CHUNK]
    for what, kind in (("coded_ulen", K.CODED), ("raw_byte", K.RAW), ("sparse_count", K.SPARSE)):
        where = [p for p in range(chunk * CHUNK + 1, (chunk + 1) * CHUNK - 1) if kinds[p] == kind]
        if not where:
            continue
        p = where[len(where) // 2]
        if kind == K.CODED:
            assert struct.unpack_from("<H", blob, at[p] + 2)[0] == PACKET
            out.append((what, G.patched(blob, at[p] + 2, struct.pack("<H", 0xFFFF)), begin, end))
        elif kind == K.RAW:
            out.append((what, G.patched(blob, at[p] + 4 + 100, bytes([blob[at[p] + 4 + 100] ^ 1])), begin, end))
        else:
            k = struct.unpack_from("<H", blob, at[p] + 6)[0]
            out.append((what, G.patched(blob, at[p] + 6, struct.pack("<H", k + 1)), begin, end))
    return out


def message_class(returncode, stderr):
    """trailer_ref.stderr_class, and for the messages it does not know what they begin with: the two paths word the place of a
    malformed packet differently (its number on the host, its chunk's file offsets on the GPU)"""
    cls = T.stderr_class(returncode, stderr)
    if cls != stderr:
        return cls
    for known in ("Incorrect file format", "Invalid file length"):
        if known in stderr:
            return known
    return stderr
