"""PacketPlan (gpuar_amd/csrc/host/compressor.hpp), the one description of what a job's packets go through, against the trailer it is
read from (no GPU needed): for every trailer Trailer::load accepts, versions 1 to 6, `transforms()` is `Trailer::merging()` and the
fields are what the trailer's own bytes say.  The files are trailer_ref's -- its four trailers undamaged, cut at every length and
with every byte flipped -- and the same sweep over versions 4, 5 and 6 at every width and flag set, written here from the layout
comment of packet_index.hpp; tests/packet_plan_test.cpp, built with the address and undefined-behaviour sanitizers, reads them."""
import os
import struct
import subprocess

import trailer_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLENS = [70, 4, 30]
CRC, DELTA, BASE, KINDS = 1, 2, 4, 8


def wide(version, elem, flags, kinds=(0, 1, 2)):
    """a trailer of version 3 to 6 as packet_index.hpp lays it out, whether or not a reader takes it"""
    n = len(CLENS)
    t = b"GIPX" + struct.pack("<IQII", version, n, elem, flags) + struct.pack(f"<{n}H", *CLENS)
    if flags & CRC or version == 6:
        t += b"\0" * (-len(t) % 4)
    if flags & CRC:
        t += struct.pack(f"<{n}I", *range(1000, 1000 + n))
    if version == 6:
        t += bytes(kinds)
    t += b"\0" * (-len(t) % 8)
    return t + struct.pack("<Q", len(t) + 12) + b"XPIG"


def gip(trailer):
    stream = sum(CLENS)
    return bytes([0, 1, 0, 0]) + struct.pack("<QQ", 3 * T.PACKET, T.HEADER + stream) + bytes(stream) + trailer


# (version, width, flags) of trailers a reader takes ...
TAKEN = [(3, w, f) for w in (2, 4, 8) for f in (0, CRC)] + \
        [(4, w, DELTA | f) for w in (1, 2, 4, 8) for f in (0, CRC)] + \
        [(5, w, BASE | CRC) for w in (1, 2, 4, 8)] + \
        [(6, w, KINDS | f) for w in (1, 2, 4, 8) for f in (0, CRC, DELTA, DELTA | CRC, BASE | CRC)]
# ... and of some it refuses: a width that is none, a version without its flag, a base without CRCs or with delta, an unknown flag
REFUSED = [(3, 1, 0), (3, 3, 0), (4, 2, 0), (4, 2, CRC), (5, 2, BASE), (5, 2, BASE | CRC | DELTA), (6, 2, 0), (6, 2, KINDS | BASE),
           (6, 2, KINDS | BASE | CRC | DELTA), (6, 16, KINDS), (6, 2, KINDS | 16)]


def test_the_plan_of_every_trailer_a_reader_takes(tmp_path):
    goods = [gip(T.write(CLENS)), gip(T.write(CLENS, crcs=[1, 2, 3])), gip(T.write(CLENS, 2)), gip(T.write(CLENS, 4, [1, 2, 3]))]
    goods += [gip(wide(*case)) for case in TAKEN]
    for i, case in enumerate(TAKEN):
        if case[0] == 3:
            assert goods[4 + i] == gip(T.write(CLENS, case[1], list(range(1000, 1003)) if case[2] else None)), "the two writers of this test"
    files = [blob for good in goods for _what, blob in T.damaged(good)] + [gip(wide(*case)) for case in REFUSED] + \
            [gip(wide(6, 2, KINDS, kinds=(0, 3, 0)))]
    (tmp_path / "cases").write_bytes(b"".join(struct.pack("<Q", len(blob)) + blob for blob in files))

    exe = str(tmp_path / "packet_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{ROOT}/include", "-I", os.path.join(ROOT, "gpuar_amd", "csrc", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "packet_plan_test.cpp")])
    r = subprocess.run([exe, str(tmp_path / "cases")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(files)

    taken = {}
    for blob, line in zip(files, lines):
        said, plan = (tuple(int(w) for w in part.split()) for part in line.split("|"))
        status, version, merging = said
        elem, delta, based, crcs, stored, sparse, kinds, transforms = plan
        if status != 1:
            assert version == 0 and plan == (1, 0, 0, 0, 0, 0, 0, 0), line       # nothing a reader may use: the plan of no trailer
            continue
        assert transforms == merging, line
        # the fields, from the file's own bytes (the trailer begins where the header says the stream ends)
        t = blob[T.stream_end(blob):]
        assert version == struct.unpack("<I", t[4:8])[0]
        width, flags = struct.unpack("<II", t[16:24]) if version >= 3 else (1, CRC if version == 2 else 0)
        assert (elem, delta, based, crcs, kinds) == (width, int(flags & DELTA != 0), int(flags & BASE != 0), int(flags & CRC != 0), int(version == 6)), line
        assert (stored, sparse) == (0, 0) and transforms == int(width > 1 or delta or based), line
        taken.setdefault(version, set()).add((elem, delta, based, crcs, kinds, transforms))
    assert sorted(taken) == [1, 2, 3, 4, 5, 6]
    assert {v: len(taken[v]) for v in taken} == {1: 1, 2: 1, 3: 6, 4: 8, 5: 4, 6: 20}, "every width and flag set of TAKEN was taken"
    # the refused ones were refused, whatever the sweep's damage made of the others
    for line in lines[-len(REFUSED) - 1:]:
        assert int(line.split()[0]) != 1, line
    # a version-6 file of width 1 with nothing but kinds is the one trailer of versions 3 to 6 that merges nothing
    assert (1, 0, 0, 0, 1, 0) in taken[6] and all(p[5] == 1 for v in (3, 4, 5) for p in taken[v])
