"""The XOR-against-a-base filter on the CPU (no GPU needed): the host definitions of gpuar_amd/csrc/xorbase.h against numpy at
every width and length, the argument checks of the new calls, what the filter buys in compressed size (the table of DESIGN.md
4.10, pinned as the inequalities of base_auto's rule), a sanitized stand-alone program over the header, and the .gip trailer
version 5 that `gpuar c --base` writes and `gpuar d` needs."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import planes_ref as R
import xor_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gpuar_amd", "bin")
PACKET = 8192
GUARD = 64


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as g
    from gpuar_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        g.build()
    hip.load()
    return hip


@pytest.fixture(scope="module")
def host_cli():
    if not os.path.exists(os.path.join(BIN, "gpuar-host")):
        import __graft_entry__ as g
        g.build()
    return os.path.join(BIN, "gpuar-host")


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=600)


def _ptr(a, at=0):
    return C.c_void_p(a.ctypes.data + at)


def host_call(fn, x, b, n, w, in_place=False):
    """fn (split or merge, host) over the first n bytes of guarded copies of x and b; returns the n bytes and checks the guards."""
    src = np.full(n + GUARD, 0xA5, dtype=np.uint8)
    src[:n] = x[:n]
    base = np.full(n + GUARD, 0x3C, dtype=np.uint8)
    base[:n] = b[:n]
    dst = src if in_place else np.full(n + GUARD, 0x5A, dtype=np.uint8)
    assert fn(_ptr(src), _ptr(base), n, w, _ptr(dst)) == 0
    assert (dst[n:] == (0xA5 if in_place else 0x5A)).all(), "bytes behind n were written"
    assert (base[:n] == b[:n]).all() and (base[n:] == 0x3C).all(), "the base was modified"
    if not in_place:
        assert (src[:n] == x[:n]).all() and (src[n:] == 0xA5).all(), "the input was modified"
    return dst[:n].copy()


# ---- the definition ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", X.WIDTHS)
def test_host_definitions_against_numpy(H, w):
    lib = H.load()
    for n in X.lengths_for(w):
        x, b = X.pair(n, seed=31 * w + n % 997)
        want = X.numpy_split_xor(x, b, w)
        assert (host_call(lib.gpuar_hip_split_xor_host, x, b, n, w) == want).all(), (w, n)
        assert (host_call(lib.gpuar_hip_split_xor_host, x, b, n, w, in_place=True) == want).all(), (w, n)
        assert (host_call(lib.gpuar_hip_merge_xor_host, want, b, n, w) == x).all(), (w, n)
        assert (host_call(lib.gpuar_hip_merge_xor_host, want, b, n, w, in_place=True) == x).all(), (w, n)
        assert (X.numpy_merge_xor(want, b, w) == x).all(), (w, n)
        assert H.merge_xor_host(H.split_xor_host(x.tobytes(), b.tobytes(), w), b.tobytes(), w) == x.tobytes(), (w, n)
        # a zero base gives the byte planes alone
        assert H.split_xor_host(x.tobytes(), bytes(n), w) == H.split_planes_host(x.tobytes(), w), (w, n)
        assert H.merge_xor_host(want.tobytes(), bytes(n), w) == H.merge_planes_host(want.tobytes(), w), (w, n)


def test_width_one_is_work_and_the_tails_last_bytes_are_xored(H):
    x, b = X.pair(100, seed=5)
    assert H.split_xor_host(x.tobytes(), b.tobytes(), 1) == (x ^ b).tobytes()
    x, b = X.pair(8 * PACKET + 8 * 13 + 7, seed=6)                  # w = 8: the last 7 bytes belong to no element
    got = np.frombuffer(H.split_xor_host(x.tobytes(), b.tobytes(), 8), dtype=np.uint8)
    assert (got[-7:] == (x ^ b)[-7:]).all() and (b[-7:] != 0).any()


def test_argument_checks_match_the_planes_calls(H):
    lib = H.load()
    x = np.arange(100, dtype=np.uint8)
    b = np.arange(100, dtype=np.uint8) * 7
    out = np.zeros(100, dtype=np.uint8)
    for fn, planes_fn in ((lib.gpuar_hip_split_xor_host, lib.gpuar_hip_split_planes_host), (lib.gpuar_hip_merge_xor_host, lib.gpuar_hip_merge_planes_host)):
        for w in (0, 3, 5, 16):
            assert fn(_ptr(x), _ptr(b), 100, w, _ptr(out)) == planes_fn(_ptr(x), 100, w, _ptr(out)) == -2, w       # GPUAR_ERR_ARGUMENT
        assert fn(None, _ptr(b), 100, 2, _ptr(out)) == -2 and fn(_ptr(x), _ptr(b), 100, 2, None) == -2
        assert fn(_ptr(x), None, 100, 2, _ptr(out)) == -2                                # a null base
        assert fn(None, None, 0, 2, None) == 0
        assert fn(None, None, 0, 3, None) == -2                                          # the width comes first, as for planes
        assert fn(_ptr(x), _ptr(b), 50, 2, _ptr(x, 10)) == -2                            # in and out overlap without being equal
        assert fn(_ptr(x), _ptr(out, 10), 50, 2, _ptr(out)) == -2                        # the base overlaps the output
        assert fn(_ptr(x), _ptr(x), 50, 2, _ptr(x)) == -2                                # ... in place too
    assert (out == 0).all()
    a = 1 << 20                                                                          # the device calls: host-side checks come first
    far = a + (1 << 16)
    for fn, planes_fn in ((lib.gpuar_hip_split_xor, lib.gpuar_hip_split_planes), (lib.gpuar_hip_merge_xor, lib.gpuar_hip_merge_planes)):
        assert fn(a, far, 4096, 3, a + 8192, None) == planes_fn(a, 4096, 3, a + 8192, None) == -2
        assert fn(a, far, 0, 2, a, None) == 0 and fn(None, None, 0, 8, None, None) == 0
        assert fn(None, far, 4096, 2, a, None) == -2 and fn(a, far, 4096, 2, None, None) == -2
        assert fn(a, None, 4096, 2, a + 8192, None) == -2                                # a null base
        assert fn(a + 4, far, 4096, 2, a + 8192, None) == planes_fn(a + 4, 4096, 2, a + 8192, None) == -1      # GPUAR_ERR_ALIGNMENT
        assert fn(a, far + 4, 4096, 2, a + 8192, None) == -1                             # a misaligned base
        assert fn(None, far + 4, 4096, 2, a, None) == -2                                 # null pointers before alignment
        assert fn(a, far, 8192, 1, a + 4096, None) == -2                                 # partial overlap of in and out
        assert fn(a, a + 8192 + 4096, 8192, 1, a + 8192, None) == -2                     # the base overlaps the output
        assert fn(a, a, 8192, 1, a, None) == -2                                          # ... in place too
    for fn in (lib.gpuar_hip_split_xor_batch, lib.gpuar_hip_merge_xor_batch):
        assert fn(a, a, a, a, a, 1, 0, a, None, None) == 0                               # no packets: nothing to do
        assert fn(a, a, a, a, None, 1, 1, a, None, None) == -2                           # no base array
        assert fn(a, a, a, a, a + 4, 1, 1, a, None, None) == -1
    assert H.load().gpuar_hip_abi_version() == 2
    with pytest.raises(H.GpuarError):
        H.split_xor_host(b"abcd", b"abc", 1)


def test_sanitized_program_over_the_host_definitions(tmp_path):
    """A stand-alone program (own main) drives xorbase.h's host definitions and its block form over the grid's lengths, built with
    AddressSanitizer and UBSan and run directly."""
    src, exe = tmp_path / "xor_check.cpp", tmp_path / "xor_check"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xorbase.h"
static uint32_t state = 4321u;
static uint8_t next() { state = state * 1664525u + 1013904223u; return static_cast<uint8_t>(state >> 24); }
template <int W> static int block() {
    uint32_t mixed[4 * W], base[4 * W], want[4 * W];
    for (int d = 0; d < 4 * W; ++d) mixed[d] = next() * 0x01010101u + d, base[d] = next() * 0x00010203u, want[d] = mixed[d] ^ base[d];
    gpuar::xor_block<W>(mixed, base);
    return memcmp(mixed, want, sizeof want) != 0;
}
int main() {
    int bad = 0;
    for (uint32_t w = 1; w <= 8; w *= 2) {
        const size_t G = size_t(w) * gpuar::kPlanePacket;
        const size_t lengths[] = {0, 1, 7, 8, 9, 15, 16, 17, 8191, 8192, 8193, G - 1, G, G + 1, 65537, 3 * G + 24653};
        for (size_t n : lengths) {
            // exact-size heap blocks: one byte read or written beyond n is a report
            std::vector<uint8_t> x(n), b(n), split(n), back(n), zero(n, 0), planes(n);
            for (auto &v : x) v = next();
            for (auto &v : b) v = next();
            gpuar::split_xor_host(x.data(), b.data(), n, w, split.data());
            gpuar::merge_xor_host(split.data(), b.data(), n, w, back.data());
            bad += x != back;
            std::vector<uint8_t> place(x);
            gpuar::split_xor_host(place.data(), b.data(), n, w, place.data());
            bad += place != split;
            gpuar::merge_xor_host(place.data(), b.data(), n, w, place.data());
            bad += place != x;
            gpuar::split_xor_host(x.data(), zero.data(), n, w, split.data());
            gpuar::planes_host<false>(x.data(), n, w, planes.data());
            bad += split != planes;
        }
    }
    bad += block<1>() + block<2>() + block<4>() + block<8>();
    std::printf("%d\n", bad);
    return 0;
}
""")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gpuar_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["0"], (r.returncode, r.stdout, r.stderr[-2000:])


# ---- what it buys -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table_estimates(H):
    """{name: (estimate of split_planes, estimate of split_xor, packets)} on the six pairs, computed once"""
    out = {}
    for name, (x, b, w) in X.table_pairs().items():
        plain = sum(H.estimate_host(H.split_planes_host(x.tobytes(), w)))
        xored = sum(H.estimate_host(H.split_xor_host(x.tobytes(), b.tobytes(), w)))
        out[name] = (plain, xored, (x.size + PACKET - 1) // PACKET)
    return out


def test_the_gain_table_as_the_rule_of_base_auto(table_estimates):
    """A base is kept iff est_xor + n_packets <= est_plain.  Measured on the CPU (bytes of 1 048 576): the three steps give 0.72,
    0.41 and 0.16 of the plain size, 1 % replaced 0.06, an unrelated base 1.04, uniform bytes against uniform bytes 1.00 (a gain of
    40 bytes, under the 128 of the rule's resolution)."""
    for name, (plain, xored, n_packets) in table_estimates.items():
        print(f"{name}: plain {plain}, xor {xored}, ratio {xored / plain:.3f}, {n_packets} packets")
    assert set(table_estimates) == set(X.TABLE_BASE_WINS + X.TABLE_BASE_LOSES)
    for name in X.TABLE_BASE_WINS:
        plain, xored, n_packets = table_estimates[name]
        assert xored + n_packets <= plain, (name, plain, xored)
    for name in X.TABLE_BASE_LOSES:
        plain, xored, n_packets = table_estimates[name]
        assert xored + n_packets > plain, (name, plain, xored)


# ---- the container ----------------------------------------------------------------------------------------------------

def cli_pair(n, seed=3):
    """a bf16-like buffer and a base close to it"""
    rng = np.random.default_rng(seed + n)
    b = R.typed_input("bf16", n + 2, seed=seed)[:n].copy()
    x = b.copy()
    x[rng.integers(0, max(n, 1), n // 50)] ^= 1
    return x, b


def base_args(w, base):
    return [f"--base={base}"] + ([f"--planes={w}"] if w > 1 else [])


@pytest.mark.parametrize("w", X.WIDTHS)
def test_base_file_round_trips_and_its_trailer_is_version_5(H, host_cli, port_oracle, tmp_path, w):
    from gpuar_amd import batch
    for n in (0, 1, w - 1, 8191, w * PACKET, w * PACKET + 1, 70 * PACKET + 13):
        x, b = cli_pair(n)
        src, base, gip, back = tmp_path / "in", tmp_path / "base", tmp_path / "out.gip", tmp_path / "back"
        x.tofile(src)
        b.tofile(base)
        r = run(host_cli, "c", "--host", *base_args(w, base), f"--in={src}", f"--out={gip}")       # (--base implies --checksum)
        assert r.returncode == 0, r.stderr
        data = gip.read_bytes()
        stream = port_oracle.encode_stream(X.numpy_split_xor(x, b, w)).tobytes() if n else b""
        size = struct.unpack("<Q", data[12:20])[0]
        assert struct.unpack("<Q", data[4:12])[0] == n and size == 20 + len(stream), (w, n)
        assert data[20:size] == stream, (w, n)
        clens = R.packet_lengths(stream)
        crcs = [zlib.crc32(x[p * PACKET:(p + 1) * PACKET].tobytes()) for p in range(len(clens))]      # of the ORIGINAL bytes
        trailer = data[size:]
        assert trailer == X.trailer_v5(clens, w, crcs) == batch.trailer(clens, w, crcs, base=True), (w, n)
        assert trailer[:4] == b"GIPX" and struct.unpack("<IQII", trailer[4:24]) == (5, len(clens), w, 5)
        assert trailer[-4:] == b"XPIG" and struct.unpack("<Q", trailer[-12:-4])[0] == len(trailer)
        r = run(host_cli, "d", "--host", f"--base={base}", f"--in={gip}", f"--out={back}")
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == x.tobytes(), (w, n)
    with_flag = tmp_path / "c.gip"                              # saying --checksum as well changes nothing
    assert run(host_cli, "c", "--host", "--checksum", *base_args(w, base), f"--in={src}", f"--out={with_flag}").returncode == 0
    assert with_flag.read_bytes() == data


def test_the_python_trailer_refuses_what_version_5_cannot_say():
    from gpuar_amd import batch
    with pytest.raises(batch.GpuarError):
        batch.trailer([10], 2, None, base=True)                 # no CRCs
    with pytest.raises(batch.GpuarError):
        batch.trailer([10], 2, [1], delta=True, base=True)


def _refused(host_cli, tmp_path, data, base):
    bad, out = tmp_path / "bad.gip", tmp_path / "bad.out"
    bad.write_bytes(bytes(data))
    out.write_bytes(b"left over")
    r = run(host_cli, "d", "--host", f"--base={base}", f"--in={bad}", f"--out={out}")
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert out.read_bytes() == b"", "a refused file leaves an empty output behind"
    assert "version 5" in r.stderr and "version 3" not in r.stderr and "version 4" not in r.stderr, r.stderr


def test_unusable_version_5_trailers_are_errors(host_cli, tmp_path):
    x, b = cli_pair(5 * PACKET + 100)
    src, base, gip = tmp_path / "in", tmp_path / "base", tmp_path / "good.gip"
    x.tofile(src)
    b.tofile(base)
    assert run(host_cli, "c", "--host", *base_args(2, base), f"--in={src}", f"--out={gip}").returncode == 0
    good = bytearray(gip.read_bytes())
    size = struct.unpack("<Q", good[12:20])[0]
    assert struct.unpack_from("<III", good, size + 4) == (5, 6, 0) and struct.unpack_from("<II", good, size + 16) == (2, 5)
    for at, value in ((size + 16, 3),                       # the width field says 3
                      (size + 20, 4),                       # bit 0, the CRCs, clear
                      (size + 20, 1),                       # bit 2, the base, clear
                      (size + 20, 7),                       # bit 1 (delta) set as well
                      (size + 20, 5 | 8)):                  # an unknown flag bit
        d = bytearray(good)
        d[at:at + 4] = struct.pack("<I", value)
        _refused(host_cli, tmp_path, d, base)
    d = bytearray(good)                                     # one clen off by one: the lengths no longer add up to the stream
    d[size + 24:size + 26] = struct.pack("<H", struct.unpack("<H", d[size + 24:size + 26])[0] + 1)
    _refused(host_cli, tmp_path, d, base)
    d = bytearray(good[:-8])                                # cut short
    _refused(host_cli, tmp_path, d, base)
    ok = tmp_path / "ok.out"
    assert run(host_cli, "d", "--host", f"--base={base}", f"--in={gip}", f"--out={ok}").returncode == 0 and ok.read_bytes() == x.tobytes()
