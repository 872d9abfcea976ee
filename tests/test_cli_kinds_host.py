"""`gpuar-host c --host --stored=auto --sparse=auto` and `d --host` (no GPU needed): the file against its restatement
(tests/kinds_ref.py) byte for byte over contents, sizes, option pairs, --checksum and --threads; the round trip with no flag but
--base; the count of packets of every kind per case; files written without the two flags unchanged; bad flag values; and damaged
version-6 files -- the trailer, a kind byte, a raw packet's clen, a sparse record -- each refused with exit 1, an empty output and a
message that names the cause."""
import collections
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import delta_ref as D
import kinds_ref as K
import planes_ref as R
import trailer_ref as T
import xor_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gpuar_amd", "bin")
PACKET = 8192


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(os.path.join(BIN, "gpuar-host")):
        import __graft_entry__ as g
        g.build()
    return os.path.join(BIN, "gpuar-host")


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O.best()


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=600)


def kinds_of_file(blob):
    """(version, flags, the kind bytes) of a version-6 file's trailer"""
    end = struct.unpack("<Q", blob[12:20])[0]
    version, n, _w, flags = struct.unpack_from("<IQII", blob, end + 4)
    at = end + 24 + 2 * n
    at += -(at - end) % 4 + (4 * n if flags & 1 else 0)
    return version, flags, list(blob[at:at + n])


# what every case is there for: {(content, stored, sparse): kind -> share of the packets, at least}
MUST_HOLD = {
    ("zeros", False, True): {K.SPARSE: 1.0}, ("zeros", True, True): {K.SPARSE: 1.0},
    ("uniform", True, False): {K.RAW: 1.0}, ("uniform", True, True): {K.RAW: 1.0}, ("uniform", False, True): {K.CODED: 1.0},
    ("text", False, True): {K.CODED: 1.0}, ("text", True, True): {K.CODED: 0.85},
    ("bf16", True, False): {K.RAW: 0.4, K.CODED: 0.4}, ("bf16", True, True): {K.RAW: 0.4, K.CODED: 0.4},
    ("bf16_base_equal", False, True): {K.SPARSE: 1.0}, ("bf16_base_equal", True, True): {K.SPARSE: 1.0},
    ("bf16_base_0.1%", True, True): {K.SPARSE: 1.0},
    ("sorted_int32", True, True): {K.RAW: 0.2, K.CODED: 0.2, K.SPARSE: 0.2},
}


@pytest.mark.parametrize("n", K.CLI_SIZES)
@pytest.mark.parametrize("content", K.CLI_CONTENTS)
def test_the_file_is_its_restatement_and_decodes(cli, oracle, tmp_path, content, n):
    x, base, flags, how = K.cli_input(content, n)
    src, base_path = tmp_path / "in", tmp_path / "base"
    x.tofile(src)
    if base is not None:
        base.tofile(base_path)
        flags = flags + [f"--base={base_path}"]
    n_packets = (n + PACKET - 1) // PACKET
    seen = collections.Counter()
    for stored, sparse in K.CLI_OPTIONS:
        for checksum in (False, True):
            want, kinds = K.file(x, oracle, stored, sparse, base=base, checksum=checksum, **how)
            gip, back = tmp_path / "a.gip", tmp_path / "back"
            extra = K.cli_flags(stored, sparse) + (["--checksum"] if checksum else [])
            r = run(cli, "c", "--host", "--threads=1", *flags, *extra, f"--in={src}", f"--out={gip}")
            assert r.returncode == 0, r.stderr
            got = gip.read_bytes()
            assert got == want, (content, n, stored, sparse, checksum)
            version, trailer_flags, file_kinds = kinds_of_file(got)
            assert version == 6 and trailer_flags & 8 and file_kinds == kinds and len(kinds) == n_packets
            count = collections.Counter(kinds)
            print(content, n, stored, sparse, dict(count), len(got))
            for kind, share in MUST_HOLD.get((content, stored, sparse), {}).items():
                assert count[kind] >= share * n_packets - 1e-9, (content, n, stored, sparse, dict(count))
            seen.update(kinds)
            every = tmp_path / "t.gip"
            assert run(cli, "c", "--host", "--threads=0", *flags, *extra, f"--in={src}", f"--out={every}").returncode == 0
            assert every.read_bytes() == got, "the file does not depend on --threads"
            r = run(cli, "d", "--host", f"--threads={0 if checksum else 1}", *([f"--base={base_path}"] if base is not None else []), f"--in={gip}", f"--out={back}")
            assert r.returncode == 0, r.stderr
            assert back.read_bytes() == x.tobytes(), (content, n, stored, sparse, checksum)
    if content == "sorted_int32":
        assert set(seen) == {K.CODED, K.RAW, K.SPARSE}


def test_a_file_equal_to_its_base_is_8_bytes_a_packet(cli, tmp_path):
    x, base, flags, _how = K.cli_input("bf16_base_equal", K.CLI_SIZES[1])
    x.tofile(tmp_path / "in")
    base.tofile(tmp_path / "base")
    sizes = {}
    for name, extra in (("with", ["--stored=auto", "--sparse=auto"]), ("without", [])):
        assert run(cli, "c", "--host", *flags, f"--base={tmp_path / 'base'}", *extra, f"--in={tmp_path / 'in'}", f"--out={tmp_path / name}").returncode == 0
        sizes[name] = struct.unpack("<Q", (tmp_path / name).read_bytes()[12:20])[0] - 20
    assert sizes["with"] == 8 * 21 and sizes["without"] > 200 * 20, sizes


@pytest.mark.parametrize("content", K.CLI_CONTENTS)
def test_without_the_flags_the_file_is_what_it_was(cli, port_oracle, tmp_path, content):
    """Byte for byte what was written before the two flags existed (and with them off): the coded stream of the transformed input
    behind the header, and the trailer of versions 1 to 5 as the earlier restatements give it."""
    from gpuar_amd import hip
    n = K.CLI_SIZES[0]
    x, base, flags, how = K.cli_input(content, n)
    x.tofile(tmp_path / "in")
    if base is not None:
        base.tofile(tmp_path / "base")
        flags = flags + [f"--base={tmp_path / 'base'}"]
    stream = port_oracle.encode_stream(K.transformed(x, how.get("planes", 1), how.get("delta", False), base)).tobytes()
    clens = R.packet_lengths(stream)
    crcs = [zlib.crc32(x[p * PACKET:(p + 1) * PACKET].tobytes()) for p in range(len(clens))]
    for extra, with_crcs in (([], False), (["--checksum"], True), (["--index"], False)):
        with_crcs = with_crcs or base is not None
        if base is not None:
            trailer = X.trailer_v5(clens, how["planes"], crcs)
        elif how.get("delta"):
            trailer = D.trailer_v4(clens, how["planes"], crcs if with_crcs else None)
        elif how.get("planes", 1) > 1 or extra:
            trailer = T.write(clens, how.get("planes", 1), crcs if with_crcs else None)
        else:
            trailer = b""
        want = hip.gip_header(n, len(stream)) + stream + trailer
        for off in ([], ["--stored=off", "--sparse=off"]):
            a = tmp_path / "a.gip"
            assert run(cli, "c", "--host", *flags, *extra, *off, f"--in={tmp_path / 'in'}", f"--out={a}").returncode == 0
            assert a.read_bytes() == want, (content, extra, off)


def test_bad_values_of_the_flags_exit_2(cli, tmp_path):
    (tmp_path / "in").write_bytes(bytes(100))
    for flag in ("--stored=on", "--stored=1", "--sparse=yes", "--sparse=", "--stored=AUTO"):
        out = tmp_path / "never.gip"
        r = run(cli, "c", "--host", flag, f"--in={tmp_path / 'in'}", f"--out={out}")
        assert r.returncode == 2 and flag.split("=")[0] in r.stderr and not out.exists(), (flag, r.returncode, r.stderr)
    for flags in (["--stored"], ["--sparse"], ["--stored=auto", "--sparse=off"]):
        assert run(cli, "c", "--host", *flags, f"--in={tmp_path / 'in'}", f"--out={tmp_path / 'ok.gip'}").returncode == 0
        assert kinds_of_file((tmp_path / "ok.gip").read_bytes())[0] == 6
    assert "--stored" in run(cli, "--help").stdout and "--sparse" in run(cli, "--help").stdout


@pytest.fixture(scope="module")
def mixed_file(cli, tmp_path_factory):
    """(file bytes, input bytes, kinds, packet offsets): sorted int32 with --planes=4 --delta and both flags: all three kinds"""
    d = tmp_path_factory.mktemp("kinds_damage")
    x, _base, flags, _how = K.cli_input("sorted_int32", K.CLI_SIZES[0])
    x.tofile(d / "in")
    assert run(cli, "c", "--host", *flags, "--stored=auto", "--sparse=auto", f"--in={d / 'in'}", f"--out={d / 'a.gip'}").returncode == 0
    blob = (d / "a.gip").read_bytes()
    _version, _flags, kinds = kinds_of_file(blob)
    offsets, at = [], K.HEADER
    for _k in kinds:
        offsets.append(at)
        at += struct.unpack_from("<H", blob, at)[0]
    assert at == struct.unpack("<Q", blob[12:20])[0] and set(kinds) == {0, 1, 2}
    return blob, x.tobytes(), kinds, offsets


def _damaged_files(blob, kinds, offsets):
    end = struct.unpack("<Q", blob[12:20])[0]
    n = len(kinds)
    kinds_at = end + 24 + 2 * n + (-(24 + 2 * n) % 4)

    def patched(at, data):
        b = bytearray(blob)
        b[at:at + len(data)] = data
        return bytes(b)

    raw = offsets[kinds.index(K.RAW)]
    sparse = max((at for at, kind in zip(offsets, kinds) if kind == K.SPARSE), key=lambda at: struct.unpack_from("<H", blob, at + 6)[0])
    raw_clen = struct.unpack_from("<H", blob, raw)[0]
    k = struct.unpack_from("<H", blob, sparse + 6)[0]          # the sparse packet with the most exceptions
    assert blob[kinds_at:kinds_at + n] == bytes(kinds)
    beyond = ("sparse_position_beyond_the_packet", patched(sparse + 8, struct.pack("<H", 0xFFFF)), "malformed") if k else \
             ("sparse_more_exceptions_than_the_record_holds", patched(sparse + 6, struct.pack("<H", 1)), "malformed")
    return [
        ("trailer_flag", patched(end + 20, struct.pack("<I", 2 | 8 | 32)), "version 6"),
        ("trailer_cut", blob[:-1], "version 6"),
        ("kind_3", patched(kinds_at + kinds.index(K.RAW), b"\x03"), "version 6"),
        ("raw_clen", patched(raw, struct.pack("<H", raw_clen - 1)), "malformed"),
        ("sparse_reserved_byte", patched(sparse + 5, b"\x01"), "malformed"),
        beyond,
        ("sparse_called_raw", patched(kinds_at + kinds.index(K.SPARSE), b"\x01"), "malformed"),
    ]


def test_damaged_version_6_files_are_refused(cli, mixed_file, tmp_path):
    blob, x, kinds, offsets = mixed_file
    good, out = tmp_path / "good.gip", tmp_path / "out"
    good.write_bytes(blob)
    assert run(cli, "d", "--host", f"--in={good}", f"--out={out}").returncode == 0 and out.read_bytes() == x
    for name, bad, says in _damaged_files(blob, kinds, offsets):
        path = tmp_path / f"{name}.gip"
        path.write_bytes(bad)
        out.write_bytes(b"left over")
        r = run(cli, "d", "--host", f"--in={path}", f"--out={out}")
        assert r.returncode == 1 and says in r.stderr, (name, r.returncode, r.stderr)
        assert out.read_bytes() == b"", name
