"""`gpuar-host c --host --base=FILE` and `d --host --base=FILE` (no GPU needed): round trips at every width setting, a file that
does not depend on --threads, the refusals -- no base for a version-5 file, a base for any other file, a base of another length,
--base with --delta -- a wrong base reported as the checksum mismatch it is, and files written without --base unchanged."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import planes_ref as R
import trailer_ref as T
import xor_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gpuar_amd", "bin")
PACKET = 8192
N = 3 * 2 * PACKET + 24653             # three groups of w = 2 and a tail (six groups of w = 1 and a tail)


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(os.path.join(BIN, "gpuar-host")):
        import __graft_entry__ as g
        g.build()
    return os.path.join(BIN, "gpuar-host")


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(input path, base path, input bytes, base bytes): bf16 weights and the same weights a small step on"""
    d = tmp_path_factory.mktemp("cli_base")
    rng = np.random.default_rng(11)
    weights = rng.standard_normal(N // 2 + 1).astype(np.float32) * np.float32(0.02)
    b = X.bf16(weights).view(np.uint8)[:N].copy()
    x = X.bf16(weights + rng.standard_normal(weights.size).astype(np.float32) * np.float32(1e-4)).view(np.uint8)[:N].copy()
    x.tofile(d / "in")
    b.tofile(d / "base")
    return d / "in", d / "base", x, b


@pytest.mark.parametrize("planes", ["1", "2", "auto"])
def test_round_trip_and_threads_do_not_change_the_file(cli, files, tmp_path, planes):
    src, base, x, b = files
    gip, back = tmp_path / "a.gip", tmp_path / "back"
    r = run(cli, "c", "--host", f"--base={base}", f"--planes={planes}", f"--in={src}", f"--out={gip}")
    assert r.returncode == 0, r.stderr
    data = gip.read_bytes()
    size = struct.unpack("<Q", data[12:20])[0]
    version, n_packets, w, flags = struct.unpack_from("<IQII", data, size + 4)
    assert (version, n_packets, flags) == (5, (N + PACKET - 1) // PACKET, 5) and w in (1, 2, 4, 8)
    if planes != "auto":
        assert w == int(planes)
    assert len(data) < N // 2, "against a close base the file is well under half the input"
    threaded = tmp_path / "t.gip"
    assert run(cli, "c", "--host", "--threads=4", f"--base={base}", f"--planes={planes}", f"--in={src}", f"--out={threaded}").returncode == 0
    assert threaded.read_bytes() == data
    r = run(cli, "d", "--host", "--threads=3", f"--base={base}", f"--in={gip}", f"--out={back}")
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == x.tobytes()


@pytest.fixture(scope="module")
def based_files(cli, files, tmp_path_factory):
    """{w: path} of the input compressed against the base at widths 1 and 2"""
    src, base, _x, _b = files
    d = tmp_path_factory.mktemp("cli_based")
    out = {}
    for w in (1, 2):
        out[w] = d / f"w{w}.gip"
        assert run(cli, "c", "--host", f"--base={base}", f"--planes={w}", f"--in={src}", f"--out={out[w]}").returncode == 0
    return out


def test_decompress_without_the_base_names_the_flag(cli, based_files, tmp_path):
    out = tmp_path / "out"
    out.write_bytes(b"left over")
    r = run(cli, "d", "--host", f"--in={based_files[2]}", f"--out={out}")
    assert r.returncode == 1 and "--base" in r.stderr, (r.returncode, r.stderr)
    assert out.read_bytes() == b""


@pytest.mark.parametrize("w,packet", [(1, 5), (2, 4), (2, 5)])
def test_a_wrong_base_is_the_checksum_mismatch(cli, files, based_files, tmp_path, w, packet):
    """One byte of the base differs inside `packet`: merge_xor hands back that one byte wrong, in that packet of the ORIGINAL bytes,
    which is the packet the CRCs (those of the original bytes) name -- for a group's first packet (5 at w = 1, 4 at w = 2) and for
    its second (5 at w = 2) alike."""
    _src, _base, _x, b = files
    wrong = b.copy()
    wrong[packet * PACKET + 1234] ^= 0x40
    other, out = tmp_path / "other", tmp_path / "out"
    wrong.tofile(other)
    r = run(cli, "d", "--host", f"--base={other}", f"--in={based_files[w]}", f"--out={out}")
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert f"Checksum mismatch: packet {packet} (uncompressed bytes {packet * PACKET} .. {(packet + 1) * PACKET})" in r.stderr, r.stderr


def test_a_base_for_a_plain_file_is_refused(cli, files, tmp_path):
    src, base, _x, _b = files
    for flags in ([], ["--planes=2"], ["--checksum"], ["--delta", "--planes=2"]):
        gip, out = tmp_path / "p.gip", tmp_path / "out"
        assert run(cli, "c", "--host", *flags, f"--in={src}", f"--out={gip}").returncode == 0
        out.write_bytes(b"left over")
        r = run(cli, "d", "--host", f"--base={base}", f"--in={gip}", f"--out={out}")
        assert r.returncode == 1 and "--base" in r.stderr, (flags, r.returncode, r.stderr)
        assert out.read_bytes() == b"", flags


def test_a_base_of_another_length_is_refused(cli, files, based_files, tmp_path):
    src, _base, _x, b = files
    for other in (b[:-1], np.concatenate([b, b[:1]]), b[:0]):
        short, gip, out = tmp_path / "short", tmp_path / "s.gip", tmp_path / "out"
        other.tofile(short)
        r = run(cli, "c", "--host", f"--base={short}", f"--in={src}", f"--out={gip}")
        assert r.returncode == 1 and "base" in r.stderr, (r.returncode, r.stderr)
        assert (gip.read_bytes() if gip.exists() else b"") == b"", "nothing was written"
        out.write_bytes(b"left over")
        r = run(cli, "d", "--host", f"--base={short}", f"--in={based_files[2]}", f"--out={out}")
        assert r.returncode == 1 and "base" in r.stderr, (r.returncode, r.stderr)
        assert out.read_bytes() == b""
    r = run(cli, "c", "--host", f"--base={tmp_path / 'missing'}", f"--in={src}", f"--out={tmp_path / 'm.gip'}")
    assert r.returncode == 1 and "base" in r.stderr


def test_base_with_delta_exits_2(cli, files, tmp_path):
    src, base, _x, _b = files
    gip = tmp_path / "never.gip"
    for mode in ("c", "d"):
        r = run(cli, mode, "--host", "--delta", f"--base={base}", f"--in={src}", f"--out={gip}")
        assert r.returncode == 2 and "--base" in r.stderr and "--delta" in r.stderr, (r.returncode, r.stderr)
        assert not gip.exists()
    assert run(cli, "c", "--host", "--base=", f"--in={src}", f"--out={gip}").returncode == 2


def test_without_the_flag_the_file_is_what_it_was(cli, files, port_oracle, tmp_path):
    """Byte for byte what was written before --base existed: the packet stream of the (split) input and the trailer of
    trailer_ref.write, versions 1 to 3."""
    from gpuar_amd import hip
    src, _base, x, _b = files
    for w in (1, 2, 4, 8):
        stream = port_oracle.encode_stream(R.numpy_split(x, w)).tobytes()
        clens = R.packet_lengths(stream)
        crcs = [zlib.crc32(x[p * PACKET:(p + 1) * PACKET].tobytes()) for p in range(len(clens))]
        for extra, with_crcs in (([], False), (["--checksum"], True), (["--index"], False)):
            a = tmp_path / "a.gip"
            assert run(cli, "c", "--host", f"--planes={w}", *extra, f"--in={src}", f"--out={a}").returncode == 0
            trailer = T.write(clens, w, crcs if with_crcs else None) if (w > 1 or extra) else b""
            assert a.read_bytes() == hip.gip_header(N, len(stream)) + stream + trailer, (w, extra)
