"""Helpers of the trailer tests (not a test module): the .gip trailer versions 1, 2 and 3 and the rules by which a reader takes or
refuses what it finds behind the packet stream, restated in Python from the layout comment of gpuar_amd/csrc/host/packet_index.hpp
and INTEGRATION.md section 4.1 -- and the damaged files both trailer tests decode.

Layout, little-endian, pads are zeros counted from "GIPX":
    version 1   "GIPX" u32 1 u64 n | u16 clen[n] | pad to 8 | u64 trailer_bytes "XPIG"
    version 2   "GIPX" u32 2 u64 n | u16 clen[n] | pad to 4 | u32 crc32[n] | pad to 8 | u64 trailer_bytes "XPIG"
    version 3   "GIPX" u32 3 u64 n | u32 elem_bytes | u32 flags (bit 0: crc32[] present) | u16 clen[n] | pad to 4 |
                u32 crc32[n] if flagged | pad to 8 | u64 trailer_bytes "XPIG"
What a reader makes of the bytes between the end of the stream and the end of the file:
    "GIPX", 3 in the first 8 bytes         ok, or `unusable` (an error): width not 2, 4 or 8, unknown flag bits, a length, the tail or
                                           the sum of the clens that does not fit
    a complete, valid version 1            ok; anything wrong with it: none, silently
    "GIPX", 2 with 16 bytes there          ok, or `malformed` (a warning, nothing verified) for any such misfit
    anything else, unknown versions too    none
Pad bytes are not looked at."""
import struct
import zlib

import numpy as np

import planes_ref

PACKET = 8192
HEADER = 20


def write(clens, elem_bytes=1, crcs=None):
    """The trailer `gpuar c` appends: version 3 for elem_bytes > 1, version 2 when only crcs are given, else version 1."""
    n = len(clens)
    if elem_bytes > 1:
        t = b"GIPX" + struct.pack("<IQII", 3, n, elem_bytes, 0 if crcs is None else 1)
    else:
        t = b"GIPX" + struct.pack("<IQ", 1 if crcs is None else 2, n)
    for c in clens:
        t += struct.pack("<H", c)
    if crcs is not None:
        assert len(crcs) == n
        t += b"\0" * (-len(t) % 4)
        for c in crcs:
            t += struct.pack("<I", c)
    t += b"\0" * (-len(t) % 8)
    return t + struct.pack("<Q", len(t) + 12) + b"XPIG"


def stream_end(blob):
    """Where the packets end: the header's compressed-size field when it is sane, else the end of the file."""
    claimed = struct.unpack("<Q", blob[12:20])[0]
    return claimed if HEADER <= claimed <= len(blob) else len(blob)


def classify(blob):
    """(status, version, clens, crcs, elem_bytes) of the file `blob`: status "none", "ok", "malformed" or "unusable"; version 0,
    clens [] and elem_bytes 1 unless ok; crcs None unless the trailer carries them."""
    end = stream_end(blob)
    t = blob[end:]
    nothing = (0, [], None, 1)
    if len(t) < 8 or t[:4] != b"GIPX":
        return ("none",) + nothing
    version = struct.unpack("<I", t[4:8])[0]
    if version == 3:
        bad, fixed = "unusable", 24
    elif version == 2 and len(t) >= 16:
        bad, fixed = "malformed", 16
    elif version == 1:
        bad, fixed = "none", 16
    else:
        return ("none",) + nothing
    if len(t) < fixed + 12:
        return (bad,) + nothing
    n = struct.unpack("<Q", t[8:16])[0]
    width, flags = struct.unpack("<II", t[16:24]) if version == 3 else (1, 1 if version == 2 else 0)
    if version == 3 and (width not in (2, 4, 8) or flags & ~1):
        return (bad,) + nothing
    if n > len(t) // 2:
        return (bad,) + nothing
    crc_at = fixed + 2 * n
    crc_at += -crc_at % 4 if flags else 0
    body = crc_at + (4 * n if flags else 0)
    body += -body % 8
    if body + 12 != len(t) or t[-4:] != b"XPIG" or struct.unpack("<Q", t[-12:-4])[0] != len(t):
        return (bad,) + nothing
    clens = list(struct.unpack(f"<{n}H", t[fixed:fixed + 2 * n]))
    if sum(clens) != end - HEADER:
        return (bad,) + nothing
    crcs = list(struct.unpack(f"<{n}I", t[crc_at:crc_at + 4 * n])) if flags else None
    return "ok", version, clens, crcs, width


# ---- the files of the damage sweep ------------------------------------------------------------------------------------

FLAGS = (["--index"], ["--checksum"], ["--planes=2"], ["--planes=2", "--checksum"])
TRAILER_BYTES = (36, 52, 44, 60)
N_INPUT = 2 * PACKET + 77          # 3 packets: a first, a middle and a partial last one, and one planes group with a tail


def sweep_input():
    from gpuar_amd import synth
    return synth.text(3, N_INPUT).tobytes()


def damaged(good):
    """(what was done, blob) for the undamaged file, every cut from the end of the stream to one byte short, and every trailer
    byte with its lowest bit or all of its bits flipped."""
    end = stream_end(good)
    yield "undamaged", good
    for n in range(end, len(good)):
        yield f"cut to {n - end} trailer bytes", good[:n]
    for mask in (0x01, 0xFF):
        for at in range(end, len(good)):
            d = bytearray(good)
            d[at] ^= mask
            yield f"trailer byte {at - end} ^ {mask:#04x}", bytes(d)


def expected(blob, x, split):
    """What `gpuar d` does with `blob`, a damaged file of input `x` (`split`: its packets hold the byte planes of width 2):
    (exit status, stderr class, output bytes or None where nothing is said about them) -- from classify(blob) alone."""
    status, version, clens, crcs, elem_bytes = classify(blob)
    stream = planes_ref.numpy_split(np.frombuffer(x, np.uint8), 2).tobytes() if split else x
    if status == "unusable":
        return 1, "planes", None
    if status == "malformed":
        return 0, "warning", stream
    out = planes_ref.numpy_merge(np.frombuffer(stream, np.uint8), elem_bytes).tobytes()
    if crcs is not None:
        for p, crc in enumerate(crcs):
            if crc != zlib.crc32(x[p * PACKET:(p + 1) * PACKET]):
                return 1, f"checksum {p}", None
    return 0, "quiet", out


def stderr_class(returncode, stderr):
    """The class of a run's stderr, in the words of expected(); anything else comes back as it is and equals no class."""
    lines = [line for line in stderr.splitlines() if line.strip()]
    if not lines:
        return "quiet"
    if returncode == 0 and len(lines) == 1 and "malformed checksum trailer: nothing was verified" in lines[0]:
        return "warning"
    if returncode == 1 and "byte planes (version 3)" in stderr:
        return "planes"
    if returncode == 1 and "Checksum mismatch: packet " in stderr:
        return "checksum " + stderr.split("Checksum mismatch: packet ")[1].split()[0]
    return stderr


def cross_cases(x, goods):
    """Twelve of the sweep's files for a second decoder: (what it is, blob, expected(blob)) -- every file undamaged, and the first
    file of every other (planes or not, status, stderr class) the sweep produces."""
    taken, cases = set(), []
    for i, good in enumerate(goods):
        for what, blob in damaged(good):
            want = expected(blob, x, split=i >= 2)
            key = (i >= 2, classify(blob)[0], want[1].split()[0])
            if key[1:] == ("ok", "quiet"):
                key = (i,)
            if key not in taken:
                taken.add(key)
                cases.append((f"{' '.join(FLAGS[i])}: {what}", blob, want))
    return cases
