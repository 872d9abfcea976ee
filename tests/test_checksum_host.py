"""Per-packet CRC-32 checks on the CPU: the compile-time tables of gpuar_amd/csrc/crc32.h against zlib, the .gip trailer
version 2 that `gpuar c --checksum` writes (layout, CRCs, the untouched prefix, the v1 / v2 choice), verification by
`gpuar d --host` on damaged files, and the host-side argument checks of the four new C calls (no GPU needed)."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from gpuar_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gpuar_amd", "bin")
LIB = os.path.join(ROOT, "gpuar_amd", "lib", "libgpuar_hip.so")
POLY = 0xEDB88320


@pytest.fixture(scope="module")
def clis():
    if not all(os.path.exists(os.path.join(BIN, b)) for b in ("gpuar", "gpuar-host")):
        import __graft_entry__ as g
        g.build()
    return [os.path.join(BIN, "gpuar"), os.path.join(BIN, "gpuar-host")]


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=600)


# ---- the tables -------------------------------------------------------------------------------------------------------

def raw(state, data):
    """A raw CRC state (initial value `state`, no final xor) after `data`, by zlib."""
    return zlib.crc32(bytes(data), state ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def mulmod(a, b):
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """Every table of crc32.h as the host compiler builds it, plus crc32_update over a test vector."""
    d = tmp_path_factory.mktemp("crc")
    src, exe = d / "dump.cpp", d / "dump"
    src.write_text("""
#include <cstdio>
#include "crc32.h"
static const gpuar::CrcTables t;
static const gpuar::CrcShiftTable k;
static const gpuar::CrcLaneColumns c;
int main() {
    for (int j = 0; j < 4; ++j) for (int i = 0; i < 256; ++i) std::printf("%u\\n", t.t[j][i]);
    for (int i = 0; i <= 8192; ++i) std::printf("%u\\n", k.k[i]);
    for (int i = 0; i < 32; ++i) for (int l = 0; l < 64; ++l) std::printf("%u\\n", c.c[i][l]);
    static unsigned char buf[20000];
    for (int i = 0; i < 20000; ++i) buf[i] = static_cast<unsigned char>(i * 131u + (i >> 7));
    for (int n = 0; n <= 20000; n += 997) std::printf("%u\\n", gpuar::crc32_update(0, buf, n));
    std::printf("%u\\n", gpuar::crc32_update(gpuar::crc32_update(0, buf, 5), buf + 5, 9));
}
""")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fconstexpr-ops-limit=100000000", "-fconstexpr-loop-limit=1000000",
                           "-I", os.path.join(ROOT, "gpuar_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    v = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    t = [v[j * 256:(j + 1) * 256] for j in range(4)]
    k = v[1024:1024 + 8193]
    cols = v[1024 + 8193:1024 + 8193 + 2048]
    return t, k, cols, v[1024 + 8193 + 2048:]


def test_byte_tables_match_zlib(tables):
    t, _, _, _ = tables
    for j in range(4):
        for i in range(256):
            assert t[j][i] == raw(0, [i] + [0] * j), (j, i)


def test_shift_constants_match_zlib_at_every_length(tables):
    """k[d] = x^(8 d) mod P: multiplying a state by it is what d zero bytes do to it, for every d in 0..8192."""
    _, k, _, _ = tables
    rng = np.random.default_rng(5)
    states = [int(s) for s in rng.integers(1, 1 << 32, size=8193)]
    for d in range(8193):
        assert mulmod(states[d], k[d]) == raw(states[d], bytes(d)), d


def test_lane_columns_shift_each_lane_over_the_bytes_behind_it(tables):
    _, _, cols, _ = tables
    for lane in range(64):
        behind = bytes(8192 - 128 * (lane + 1))
        for i in range(32):
            assert cols[i * 64 + lane] == raw(1 << i, behind), (lane, i)


def test_host_crc_equals_zlib(tables):
    _, _, _, got = tables
    buf = bytes((i * 131 + (i >> 7)) & 255 for i in range(20000))
    assert got[:-1] == [zlib.crc32(buf[:n]) for n in range(0, 20001, 997)]
    assert got[-1] == zlib.crc32(buf[:14]) and zlib.crc32(b"123456789") == 0xCBF43926


# ---- the trailer ------------------------------------------------------------------------------------------------------

def parse_trailer(blob):
    """(version, clens, crcs or None) of the trailer behind the stream of a .gip, checking every length and pad on the way."""
    end = int.from_bytes(blob[12:20], "little")
    t = blob[end:]
    assert t[:4] == b"GIPX" and t[-4:] == b"XPIG"
    version, n = struct.unpack_from("<IQ", t, 4)
    assert struct.unpack_from("<Q", t, len(t) - 12)[0] == len(t)
    clens = list(struct.unpack_from(f"<{n}H", t, 16))
    at = 16 + 2 * n
    crcs = None
    if version == 2:
        assert t[at:at + (-at % 4)] == bytes(-at % 4)
        at += -at % 4
        crcs = list(struct.unpack_from(f"<{n}I", t, at))
        at += 4 * n
    else:
        assert version == 1
    assert t[at:len(t) - 12] == bytes(-at % 8) and (len(t) - 12) % 8 == 0
    assert sum(clens) == end - 20
    return version, clens, crcs


SIZES = [0, 1, 5, 8191, 8192, 8193, 3 * 8192 + 77, 100000]


@pytest.mark.parametrize("n", SIZES)
def test_checksum_trailer_layout_and_crcs(clis, tmp_path, n):
    data = synth.generate("text", 3, n).tobytes() if n else b""
    src = tmp_path / "in.dat"
    src.write_bytes(data)
    outs = {}
    for flags in ((), ("--index",), ("--checksum",), ("--index", "--checksum")):
        gip = tmp_path / ("out" + "".join(flags) + ".gip")
        r = run(clis[1], "c", "--host", f"--in={src}", f"--out={gip}", *flags)
        assert r.returncode == 0, r.stderr
        outs[flags] = gip.read_bytes()
    plain = outs[()]
    end = int.from_bytes(plain[12:20], "little")
    assert len(plain) == end
    for flags, blob in outs.items():
        assert blob[:end] == plain, flags                  # the prefix up to the header's size: byte for byte the plain file
        if not flags:
            continue
        version, clens, crcs = parse_trailer(blob)
        assert len(clens) == (n + 8191) // 8192
        assert version == (2 if "--checksum" in flags else 1), flags
        if crcs is not None:
            assert crcs == [zlib.crc32(data[p * 8192:(p + 1) * 8192]) for p in range(len(clens))]
    assert outs[("--checksum",)] == outs[("--index", "--checksum")]
    # --index alone is the version-1 trailer: 16 + 2n padded to 8 + 12
    npk = (n + 8191) // 8192
    assert len(outs[("--index",)]) - end == 16 + 2 * npk + (-2 * npk % 8) + 12


def test_checksummed_files_round_trip_through_both_host_clis(clis, tmp_path):
    data = synth.generate("zipf", 8, 5 * 8192 + 1234).tobytes()
    src, gip = tmp_path / "in.dat", tmp_path / "out.gip"
    src.write_bytes(data)
    assert run(clis[1], "c", "--host", "--checksum", f"--in={src}", f"--out={gip}").returncode == 0
    for cli in clis:
        for extra in ((), ("--threads", "0")):
            back = tmp_path / "back.dat"
            r = run(cli, "d", "--host", *extra, f"--in={gip}", f"--out={back}")
            assert r.returncode == 0 and "Warning" not in r.stderr, r.stderr
            assert back.read_bytes() == data


def silent_flip(cli, tmp_path, data, gip_blob, packet):
    """A bit of `packet`'s body whose flip decodes WITHOUT complaint (exit 0) to wrong bytes when the file has no trailer:
    (flipped file with the trailer, bit offset)."""
    end = int.from_bytes(gip_blob[12:20], "little")
    _, clens, _ = parse_trailer(gip_blob)
    start = 20 + sum(clens[:packet])
    for at in range(start + 4 + 8, start + clens[packet] - 8, 37):     # inside the arithmetic-coded body
        bad = bytearray(gip_blob)
        bad[at] ^= 0x10
        plain = tmp_path / "plain.gip"
        plain.write_bytes(bytes(bad[:end]))
        back = tmp_path / "plain.dat"
        r = run(cli, "d", "--host", f"--in={plain}", f"--out={back}")
        if r.returncode == 0 and back.read_bytes() != data:
            return bytes(bad), at
    raise AssertionError("no flip in the packet's body decodes silently")


def test_damaged_body_decodes_silently_without_and_fails_with_the_trailer(clis, tmp_path):
    data = synth.generate("text", 11, 4 * 8192 + 999).tobytes()
    src, gip = tmp_path / "in.dat", tmp_path / "out.gip"
    src.write_bytes(data)
    assert run(clis[1], "c", "--host", "--checksum", f"--in={src}", f"--out={gip}").returncode == 0
    blob = gip.read_bytes()
    for packet in (0, 2, 4):
        bad, _ = silent_flip(clis[1], tmp_path, data, blob, packet)
        damaged = tmp_path / "damaged.gip"
        damaged.write_bytes(bad)
        for cli in clis:
            r = run(cli, "d", "--host", f"--in={damaged}", f"--out={tmp_path / 'back.dat'}")
            assert r.returncode == 1, (cli, r.stdout, r.stderr)
            hi = min((packet + 1) * 8192, len(data))
            assert f"Checksum mismatch: packet {packet} (uncompressed bytes {packet * 8192} .. " in r.stderr, r.stderr
            if packet == 4:
                assert f".. {hi})" in r.stderr, r.stderr


def zero_last_ulen(blob):
    """The file with its last packet's ulen 8192 turned into 0 by ONE bit flip (bit 5 of header byte 3)."""
    _, clens, _ = parse_trailer(blob)
    at = 20 + sum(clens[:-1]) + 3
    assert blob[at - 1] == 0x00 and blob[at] == 0x20, "the last packet must hold 8192 bytes"
    bad = bytearray(blob)
    bad[at] ^= 0x20
    return bytes(bad)


def test_last_packet_ulen_flipped_to_zero_is_caught(clis, tmp_path):
    """A size that is a multiple of 8192: one flip makes the last packet decode to nothing.  Without the trailer that is a
    silently short file; with it, exit 1 naming the packet."""
    data = synth.generate("text", 4, 3 * 8192).tobytes()
    src, gip = tmp_path / "in.dat", tmp_path / "out.gip"
    src.write_bytes(data)
    assert run(clis[1], "c", "--host", "--checksum", f"--in={src}", f"--out={gip}").returncode == 0
    blob = gip.read_bytes()
    bad = zero_last_ulen(blob)
    end = int.from_bytes(blob[12:20], "little")
    plain, damaged, back = tmp_path / "plain.gip", tmp_path / "damaged.gip", tmp_path / "back.dat"
    plain.write_bytes(bad[:end])
    damaged.write_bytes(bad)
    r = run(clis[1], "d", "--host", f"--in={plain}", f"--out={back}")
    assert r.returncode == 0 and back.read_bytes() == data[:2 * 8192]
    for cli in clis:
        r = run(cli, "d", "--host", f"--in={damaged}", f"--out={back}")
        assert r.returncode == 1 and "Checksum mismatch: packet 2 (uncompressed bytes 16384 .. 16384)" in r.stderr, (cli, r.stderr)


def test_trailer_with_bad_lengths_decodes_with_a_warning(clis, tmp_path):
    data = synth.generate("uniform", 2, 2 * 8192 + 5).tobytes()
    src, gip = tmp_path / "in.dat", tmp_path / "out.gip"
    src.write_bytes(data)
    assert run(clis[1], "c", "--host", "--checksum", f"--in={src}", f"--out={gip}").returncode == 0
    blob = gip.read_bytes()
    end = int.from_bytes(blob[12:20], "little")
    for where in (end + 8, len(blob) - 12, end + 16):       # the packet count, the trailer's length, a clen
        bad = bytearray(blob)
        bad[where] ^= 1
        damaged = tmp_path / "bad.gip"
        damaged.write_bytes(bytes(bad))
        for cli in clis:
            back = tmp_path / "back.dat"
            r = run(cli, "d", "--host", f"--in={damaged}", f"--out={back}")
            assert r.returncode == 0, r.stderr
            assert "malformed checksum trailer: nothing was verified" in r.stderr
            assert len([l for l in r.stderr.splitlines() if l.strip()]) == 1
            assert back.read_bytes() == data


def test_version_one_trailer_is_unchanged_and_silent(clis, tmp_path):
    data = synth.generate("zipf", 1, 3 * 8192).tobytes()
    src, gip = tmp_path / "in.dat", tmp_path / "out.gip"
    src.write_bytes(data)
    assert run(clis[1], "c", "--host", "--index", f"--in={src}", f"--out={gip}").returncode == 0
    r = run(clis[1], "d", "--host", f"--in={gip}", f"--out={tmp_path / 'back.dat'}")
    assert r.returncode == 0 and r.stderr == ""
    assert (tmp_path / "back.dat").read_bytes() == data


def test_help_names_the_flag(clis):
    for cli in clis:
        assert "--checksum" in run(cli, "--help").stdout


# ---- host-side checks of the C calls ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("libgpuar_hip.so not built")
    from gpuar_amd import hip as H
    return H.load()


A16, A8, A4, ODD = 0x10000, 0x10008, 0x10004, 0x10001
OK, ALIGN, ARG = 0, -1, -2


def test_crc32_host_checks(lib):
    f = lib.gpuar_hip_crc32
    assert f(None, 0, None, None) == OK                     # nothing to do: nothing launched, nothing checked
    assert f(None, 5, A16, None) == ARG
    assert f(A16, 5, None, None) == ARG
    assert f(A16, (1 << 32) * 8192, A16, None) == ARG       # more packets than a launch indexes
    assert f(A8, 5, A16, None) == ALIGN                     # data: 16 bytes
    assert f(A16, 5, A16 + 2, None) == ALIGN                # crc: 4 bytes


def test_verify_crc32_host_checks(lib):
    f = lib.gpuar_hip_verify_crc32
    assert f(None, 0, None, None, None, None) == OK
    assert f(None, 5, A16, None, None, None) == ARG
    assert f(A16, 5, None, None, None, None) == ARG
    assert f(A8, 5, A16, None, None, None) == ALIGN
    assert f(A16, 5, ODD, None, None, None) == ALIGN
    assert f(A16, 5, A16, A4, None, None) == ALIGN          # first_bad: 8 bytes
    assert f(A16, 5, A16, None, A16 + 2, None) == ALIGN     # status: 4 bytes


def test_crc32_batch_host_checks(lib):
    f = lib.gpuar_hip_crc32_batch
    assert f(None, None, None, 0, 0, None, None, None) == OK
    assert f(None, A16, A16, 1, 1, A16, None, None) == ARG
    assert f(A16, None, A16, 1, 1, A16, None, None) == ARG
    assert f(A16, A16, None, 1, 1, A16, None, None) == ARG
    assert f(A16, A16, A16, 1, 1, None, None, None) == ARG
    assert f(A16, A16, A16, 1, 1 << 32, A16, None, None) == ARG
    assert f(A16, A16, A16, 1 << 32, 1, A16, None, None) == ARG
    assert f(A4, A16, A16, 1, 1, A16, None, None) == ALIGN  # descriptor arrays: 8 bytes
    assert f(A16, A4, A16, 1, 1, A16, None, None) == ALIGN
    assert f(A16, A16, A4, 1, 1, A16, None, None) == ALIGN
    assert f(A16, A16, A16, 1, 1, ODD, None, None) == ALIGN
    assert f(A16, A16, A16, 1, 1, A16, A16 + 2, None) == ALIGN


def test_verify_crc32_batch_host_checks(lib):
    f = lib.gpuar_hip_verify_crc32_batch
    assert f(None, None, None, 0, 0, None, None, None, None) == OK
    assert f(None, A16, A16, 1, 1, A16, None, None, None) == ARG
    assert f(A16, A16, A16, 1, 1, None, None, None, None) == ARG
    assert f(A16, A16, A16, 1, 1 << 32, A16, None, None, None) == ARG
    assert f(A4, A16, A16, 1, 1, A16, None, None, None) == ALIGN
    assert f(A16, A16, A4, 1, 1, A16, None, None, None) == ALIGN
    assert f(A16, A16, A16, 1, 1, ODD, None, None, None) == ALIGN
    assert f(A16, A16, A16, 1, 1, A16, A4, None, None) == ALIGN
    assert f(A16, A16, A16, 1, 1, A16, None, A16 + 2, None) == ALIGN


def test_crc_kernels_keep_the_code_object_rules():
    """No scratch, no spills, no buffer_ / scratch_ / MFMA instructions: the rules of test_codeobj_contract.py, for the two
    instantiations of crc32_kernel by their mangled names (that file's parser merges them)."""
    import re
    from test_codeobj_contract import TOOLS, _need_tools
    _need_tools()
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fat, elf = os.path.join(d, "fat.bin"), os.path.join(d, "g.elf")
        subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fat}", LIB, os.path.join(d, "unused.so")])
        targets = subprocess.check_output([TOOLS["clang-offload-bundler"], "--list", "--type=o", f"--input={fat}"], text=True).split()
        gfx = [t for t in targets if t.endswith("gfx950")][0]
        subprocess.check_call([TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fat}", f"--targets={gfx}", f"--output={elf}"])
        notes = subprocess.check_output([TOOLS["llvm-readelf"], "--notes", elf], text=True)
        dis = subprocess.check_output([TOOLS["llvm-objdump"], "-d", "--no-show-raw-insn", elf], text=True)
    records = re.findall(r"\.name:\s+(_ZN5gpuar12crc32_kernelILb[01]\S*)", notes)
    assert len(records) == 2, records
    for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert re.findall(rf"\.{field}:\s+(\d+)", notes) and all(v == "0" for v in re.findall(rf"\.{field}:\s+(\d+)", notes)), field
    body = re.findall(r"<_ZN5gpuar12crc32_kernelILb[01][^>]*>:\n(.*?)(?=\n\n|\Z)", dis, re.S)
    assert len(body) == 2
    for text in body:
        ops = {line.split()[0] for line in text.splitlines() if line.strip()}
        assert not [o for o in ops if o.startswith(("v_mfma", "v_smfmac", "scratch_", "buffer_"))]
        assert "global_load_dwordx4" in ops and "ds_read_b32" in ops
