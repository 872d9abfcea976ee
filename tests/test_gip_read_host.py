"""batch.read_gip -- the CLI's own reader behind gpuar_hip_gip_read_host / gpuar_hip_gip_tables_host (include/gpuar_hip.h; DESIGN.md
4.14) -- on the CPU, no device: every file `gpuar-host c` writes under every option that leaves a trace in a file is read back and
every field held against the restatements of tests/gip_files.py; damaged files are refused with a message that says what and where;
and the same files go through tests/gip_read_client.cpp, a stand-alone program built with -fsanitize=address,undefined."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import client_build as B
import gip_files as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batch():
    B.ensure_products()
    from gpuar_amd import batch
    return batch


def inputs():
    return [(fam, n, G.family(fam, n)) for n in G.SIZES for fam in G.FAMILIES]


@pytest.mark.parametrize("name,flags,says", G.FLAG_SETS, ids=[s[0] for s in G.FLAG_SETS])
def test_read_gip_finds_what_the_cli_wrote(batch, tmp_path, name, flags, says):
    for fam, n, x in inputs():
        base = G.base_of(x) if says.get("base") else None
        blob = G.write(tmp_path, x, flags, base)
        want = G.expected(blob, x, says, base)
        got = batch.read_gip(blob)
        assert G.fields(got) == want, (name, fam, n)
        assert got.n_packets == len(want["clens"]) and got.delta == bool(says.get("delta")) and got.based == bool(says.get("base"))
        assert got.stream.tobytes() == blob[want["stream_begin"]:want["stream_end"]]
        # as a reference-written file has its header: garbage where the reference leaves bytes uninitialised
        assert G.fields(batch.read_gip(G.garbage_header(blob))) == want, (name, fam, n, "garbage header bytes")
        # every accepted container of the bytes
        if n == G.SIZES[-1]:
            for held in (bytearray(blob), memoryview(blob), np.frombuffer(blob, dtype=np.uint8)):
                assert G.fields(batch.read_gip(held)) == want
        if name == "plain":                              # the walk finds the lengths the trailer lists
            indexed = batch.read_gip(G.write(tmp_path, x, ["--index"]))
            assert indexed.version == 1 and indexed.clens.tolist() == got.clens.tolist() == G.walk(blob)[0]


def test_read_gip_takes_a_cpu_tensor_and_refuses_other_shapes(batch, tmp_path):
    import torch
    from gpuar_amd.hip import GpuarError
    x = G.family("text", G.PACKET + 1)
    blob = G.write(tmp_path, x, ["--checksum"])
    want = G.expected(blob, x, dict(version=2, crcs=True))
    assert G.fields(batch.read_gip(torch.frombuffer(bytearray(blob), dtype=torch.uint8))) == want
    with pytest.raises(GpuarError, match="contiguous one-dimensional array of uint8"):
        batch.read_gip(np.frombuffer(blob, dtype=np.uint8)[::2])


# ---- damaged files ----------------------------------------------------------------------------------------------------------

def kinds_at(blob, end):
    """where the kinds of a version-6 trailer stand in the file"""
    n, _elem, flags = struct.unpack("<QII", blob[end + 8:end + 24])
    at = end + 24 + 2 * n
    at += -(at - end) % 4
    return at + (4 * n if flags & 1 else 0)


def damaged_files(tmp):
    """[(what, blob, what the message must say)]"""
    text = G.family("text", 3 * G.PACKET + 4097)
    whole = G.family("text", 2 * G.PACKET)
    mixed = np.concatenate([G.family("zeros", G.PACKET), G.family("uniform", G.PACKET), G.family("text", G.PACKET + 4097)])
    plain = G.write(tmp, text, [])
    clens, _ulens, end = G.walk(plain)
    second, last = G.HEADER + clens[0], end - clens[-1]
    out = [
        ("19 bytes", plain[:19], r"19 bytes are fewer than the 20"),
        ("no bytes", b"", r"0 bytes are fewer than the 20"),
        ("version 1.1.0", G.patched(plain, 0, b"\x01"), r"not the version 0\.1\.0"),
        ("compressed size one beyond the file", G.patched(plain, 12, struct.pack("<Q", len(plain) + 1)), r"compressed size .* beyond the file's \d+ bytes"),
        ("compressed size 19", G.patched(plain, 12, struct.pack("<Q", 19)), r"compressed size .* below 20"),
        ("walk: clen 3", G.patched(plain, G.HEADER, struct.pack("<H", 3)), r"packet 0 at offset 20: a clen below 4 or above 8704"),
        ("walk: clen 8705", G.patched(plain, second, struct.pack("<H", 8705)), rf"packet 1 at offset {second}: a clen below 4 or above 8704"),
        ("walk: ulen 8191", G.patched(plain, second + 2, struct.pack("<H", 8191)), rf"packet 1 at offset {second}: ulen is not"),
        ("walk: the last ulen one more", G.patched(plain, last + 2, struct.pack("<H", 4098)), rf"packet 3 at offset {last}: ulen is not"),
        ("walk: the last packet longer than the stream", G.patched(plain, last, struct.pack("<H", clens[-1] + 5)),
         rf"stream ends inside packet 3 at offset {last}"),
        ("walk: the stream ends inside a header", G.patched(plain, 12, struct.pack("<Q", last + 2))[:last + 2], rf"stream ends inside packet 3 at offset {last}"),
    ]
    # a packet count that does not fit the uncompressed size: one packet more needed than there are, with and without a trailer
    for flags in ([], ["--index"]):
        good = G.write(tmp, whole, flags)
        out.append((f"{flags}: 2 packets for 3 * 8192 bytes", G.patched(good, 4, struct.pack("<Q", 3 * G.PACKET)), r"2 packets .* not what the header's uncompressed size needs"))
    out.append(("walk: 4 packets for 8192 bytes", G.patched(plain, 4, struct.pack("<Q", G.PACKET)), r"1 packets .* not what the header's uncompressed size needs"))
    # a trailer of version 3 .. 6 that cannot be used: a width of 3
    base = G.base_of(text)
    for version, flags, b in ((3, ["--planes=2"], None), (4, ["--delta", "--planes=2"], None), (5, ["--planes=2"], base), (6, ["--stored=auto"], None)):
        good = G.write(tmp, text, flags, b)
        t = G.walk(good)[2]
        assert struct.unpack("<I", good[t + 4:t + 8])[0] == version
        out.append((f"version {version}: width 3", G.patched(good, t + 16, struct.pack("<I", 3)), rf"trailer at offset {t} says version {version} but cannot be used"))
        out.append((f"version {version}: cut by one byte", good[:-1], rf"trailer at offset {t} says version {version} but cannot be used"))
    # a trailer whose lengths sum to the stream and differ from the headers
    good = G.write(tmp, text, ["--index"])
    t = G.walk(good)[2]
    out.append(("trailer: clen[0] + 1, clen[1] - 1", G.patched(good, t + 16, struct.pack("<HH", clens[0] + 1, clens[1] - 1)),
                r"packet 0 at offset 20: the header's clen is not the trailer's"))
    # version 6: packet 0 sparse (zeros), packet 1 raw (uniform), packets 2 and 3 coded (text)
    good = G.write(tmp, mixed, ["--stored=auto", "--sparse=auto"])
    c6, _u6, t = G.walk(good)
    k = kinds_at(good, t)
    assert list(good[k:k + 4]) == [2, 1, 0, 0]
    third = G.HEADER + c6[0] + c6[1]
    out += [
        ("version 6: kind 3", G.patched(good, k + 2, b"\x03"), rf"trailer at offset {t} says version 6 but cannot be used.*packet kind"),
        ("version 6: a coded packet called raw", G.patched(good, k + 2, b"\x01"), rf"packet 2 at offset {third}: a raw packet whose clen is not 4 \+ ulen"),
        ("version 6: a coded packet called sparse", G.patched(good, k + 3, b"\x02"), rf"packet 3 at offset {third + c6[2]}: a sparse packet whose record head"),
        ("version 6: a sparse head with byte 1 set", G.patched(good, G.HEADER + 5, b"\x01"), r"packet 0 at offset 20: a sparse packet whose record head"),
        ("version 6: a sparse head with a count that does not fit", G.patched(good, G.HEADER + 6, struct.pack("<H", 1)), r"packet 0 at offset 20: a sparse packet whose record head"),
    ]
    return out


def test_read_gip_refuses_damaged_files_and_says_what_and_where(batch, tmp_path):
    from gpuar_amd.hip import GpuarError
    for what, blob, says in damaged_files(tmp_path):
        with pytest.raises(GpuarError) as e:
            batch.read_gip(blob, "files[7]")
        assert re.search(says, str(e.value), re.S) and str(e.value).startswith("files[7]: "), (what, str(e.value))


def test_a_trailer_the_cli_ignores_is_ignored(batch, tmp_path):
    """An unusable version 1 is no trailer, a malformed version 2 neither (the CLI warns that nothing is verified), and a trailer of
    an unknown version is none: the lengths then come from the walk."""
    x = G.family("text", 3 * G.PACKET + 4097)
    for flags, at, data in ((["--index"], 8, struct.pack("<Q", 5)), (["--checksum"], 8, struct.pack("<Q", 5)), (["--index"], 4, struct.pack("<I", 9))):
        good = G.write(tmp_path, x, flags)
        t = G.walk(good)[2]
        got = batch.read_gip(G.patched(good, t + at, data))
        assert got.version == 0 and got.crcs is None and got.kinds is None and got.clens.tolist() == G.walk(good)[0], (flags, at)


# ---- the same files under the sanitizers --------------------------------------------------------------------------------------

def library_line(blob):
    """what tests/gip_read_client.cpp prints for `blob`, from the library through ctypes"""
    import ctypes as C
    from gpuar_amd import hip as H
    lib = H.load()
    info = (C.c_uint64 * H.GIP_INFO_WORDS)()
    held = C.create_string_buffer(bytes(blob), max(len(blob), 1))
    code = lib.gpuar_hip_gip_read_host(C.addressof(held), len(blob), info)
    line = f"{code} | " + " ".join(str(v) for v in info)
    if code == 0:
        n = info[4]
        clen, crc, kind = (C.c_uint16 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_uint8 * max(n, 1))()
        has_crcs, has_kinds = bool(info[6] & 1), info[3] == 6
        assert lib.gpuar_hip_gip_tables_host(C.addressof(held), len(blob), clen, crc if has_crcs else None, kind if has_kinds else None, n) == 0
        rows = [list(clen)[:n], list(crc)[:n] if has_crcs else ["-"], list(kind)[:n] if has_kinds else ["-"]]
        line += "".join(" |" + "".join(f" {v}" for v in row) for row in rows)
    return line


def test_the_reader_is_clean_under_address_and_undefined_sanitizers(batch, tmp_path):
    """tests/gip_read_client.cpp + gpuar_amd/csrc/host/gip_read.cpp, built with -fsanitize=address,undefined into tests/_build/: every
    file is read into a heap block of exactly its size, so a read past either end is a report.  The program must end with status 0,
    say nothing on stderr, and print for every file what the library gives."""
    csrc = os.path.join(ROOT, "gpuar_amd", "csrc")
    source = os.path.join(B.HOST, "gip_read.cpp")
    exe = B._make("gip_read_client", [os.path.join(ROOT, "tests", "gip_read_client.cpp"), source],
                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{csrc}"], [],
                  [os.path.join(csrc, h) for h in ("kinds.h", "sparse.h", "estimate.h")])
    blobs = []
    for _name, flags, says in G.FLAG_SETS:
        for fam, n in (("zeros", 0), ("uniform", 1), ("sparse", G.PACKET), ("text", G.PACKET + 1), ("uniform", 3 * G.PACKET + 4097), ("sparse", 3 * G.PACKET + 4097)):
            x = G.family(fam, n)
            blob = G.write(tmp_path, x, flags, G.base_of(x) if says.get("base") else None)
            blobs += [blob, G.garbage_header(blob)]
    blobs += [blob for _what, blob, _says in damaged_files(tmp_path)]
    paths = []
    for i, blob in enumerate(blobs):
        paths.append(str(tmp_path / f"file{i}.gip"))
        with open(paths[-1], "wb") as f:
            f.write(blob)
    r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(blobs)
    for i, (line, blob) in enumerate(zip(lines, blobs)):
        assert line == library_line(blob), i
    assert {int(line.split()[0]) for line in lines} >= set(range(0, 13)) - {10}      # every defect a file can carry past Trailer::load
