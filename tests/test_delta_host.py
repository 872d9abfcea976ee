"""The delta filter on the CPU (no GPU needed): the host transform of gpuar_amd/csrc/delta.h against two independent restatements
of its definition, the register block transforms the kernels run, what the filter buys in compressed size, the rule of
delta="auto", and the .gip trailer version 4 that `gpuar c --delta` writes and `gpuar d` needs."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import delta_ref as D
import planes_ref as R

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


def host_call(fn, x, n, w, in_place=False):
    """fn (split or merge, host) over the first n bytes of a guarded copy of x; returns the n bytes and checks the guard."""
    src = np.full(n + GUARD, 0xA5, dtype=np.uint8)
    src[:n] = x[:n]
    dst = src if in_place else np.full(n + GUARD, 0x5A, dtype=np.uint8)
    assert fn(_ptr(src), n, w, _ptr(dst)) == 0
    assert (dst[n:] == (0xA5 if in_place else 0x5A)).all(), "bytes behind n were written"
    if not in_place:
        assert (src[:n] == x[:n]).all() and (src[n:] == 0xA5).all(), "the input was modified"
    return dst[:n].copy()


# ---- the definition ---------------------------------------------------------------------------------------------------

def test_the_numpy_restatement_is_the_definition():
    for w in D.WIDTHS:
        for kind in D.KINDS:
            for n in (0, 1, w - 1, w, 15, 16 * w + 1, 8191, w * PACKET + w + 1):
                x = D.bytes_of(kind, n, w, seed=n)
                d = D.numpy_delta(x, w)
                assert d.tobytes() == D.delta_by_definition(x.tobytes(), w), (w, kind, n)
                assert (D.numpy_undelta(d, w) == x).all(), (w, kind, n)


@pytest.mark.parametrize("w", D.WIDTHS)
def test_host_transform_against_both_restatements(H, w):
    lib = H.load()
    for kind in D.KINDS:
        for n in D.lengths_for(w):
            x = D.bytes_of(kind, n, w, seed=17 * w + n % 991)
            want = D.numpy_split_delta(x, w)
            if n <= w * PACKET + 1:
                assert want.tobytes() == R.split_by_definition(D.delta_by_definition(x.tobytes(), w), w), (w, kind, n)
            assert (host_call(lib.gpuar_hip_split_delta_host, x, n, w) == want).all(), (w, kind, n)
            assert (host_call(lib.gpuar_hip_split_delta_host, x, n, w, in_place=True) == want).all(), (w, kind, n)
            assert (host_call(lib.gpuar_hip_merge_delta_host, want, n, w) == x).all(), (w, kind, n)
            assert (host_call(lib.gpuar_hip_merge_delta_host, want, n, w, in_place=True) == x).all(), (w, kind, n)
            assert (D.numpy_merge_delta(want, w) == x).all(), (w, kind, n)
            assert H.split_delta_host(x.tobytes(), w) == want.tobytes() and H.merge_delta_host(want.tobytes(), w) == x.tobytes()


def test_host_width_one_is_work_and_argument_checks(H):
    lib = H.load()
    x = np.arange(100, dtype=np.uint8) * 3
    got = host_call(lib.gpuar_hip_split_delta_host, x, 100, 1, in_place=True)
    assert (got == np.array([0] + [3] * 99, dtype=np.uint8)).all()
    out = np.zeros(100, dtype=np.uint8)
    for fn in (lib.gpuar_hip_split_delta_host, lib.gpuar_hip_merge_delta_host):
        for w in (0, 3, 5, 16):
            assert fn(_ptr(x), 100, w, _ptr(out)) == -2, w                     # GPUAR_ERR_ARGUMENT
        assert fn(None, 100, 2, _ptr(out)) == -2 and fn(_ptr(x), 100, 2, None) == -2
        assert fn(None, 0, 2, None) == 0
        assert fn(_ptr(x), 50, 2, _ptr(x, 10)) == -2                           # overlapping without being equal
    assert (out == 0).all()
    a = 1 << 20                                                                # the device calls: host-side checks come first
    for fn in (lib.gpuar_hip_split_delta, lib.gpuar_hip_merge_delta):
        assert fn(a, 4096, 3, a + 8192, None) == -2
        assert fn(a, 0, 2, a, None) == 0 and fn(None, 0, 8, None, None) == 0
        assert fn(None, 4096, 2, a, None) == -2 and fn(a, 4096, 2, None, None) == -2
        assert fn(a + 4, 4096, 2, a + 8192, None) == -1                        # GPUAR_ERR_ALIGNMENT
        assert fn(a, 8192, 1, a + 4096, None) == -2                            # partial overlap
    for fn in (lib.gpuar_hip_split_delta_batch, lib.gpuar_hip_merge_delta_batch):
        assert fn(a, a, a, a, a, 1, 0, a, None, None) == 0                     # no packets: nothing to do
        assert fn(a, a, a, a, None, 1, 1, a, None, None) == -2                 # no filter array
        assert fn(a, a, a, a, a + 4, 1, 1, a, None, None) == -1
    assert H.load().gpuar_hip_abi_version() == 2


# ---- the register transform of one block ------------------------------------------------------------------------------

@pytest.mark.parametrize("w", D.WIDTHS)
def test_block_transforms_against_the_definition(H, w):
    """delta_block / undelta_block as the kernels compose them: two consecutive blocks, the second with the first's last element
    as pred and the first's total as offset; on the three kinds of bytes and many seeds."""
    dt = D.UINT[w]
    for kind, seeds in (("uniform", range(40)), ("ones", [0]), ("ramp", [0])):
        for seed in seeds:
            x = D.bytes_of(kind, 32 * w, w, seed=seed)
            v = x.view("<u%d" % w).astype(dt)
            if kind == "ramp":
                v = v + dt(0xF0)                                               # carries out of the low byte inside the block
            want = D.numpy_delta(v.astype("<u%d" % w).view(np.uint8), w).view(np.uint32)
            dwords = v.astype("<u%d" % w).view(np.uint32).tolist()
            b0, _ = H.delta_block_host(dwords[:4 * w], w, False, 0)
            b1, _ = H.delta_block_host(dwords[4 * w:], w, False, int(v[15]) | (0xABCD << 8 * w if w < 8 else 0))      # (pred's upper bytes do not count)
            assert b0 + b1 == want.tolist(), (w, kind, seed)
            u0, t0 = H.delta_block_host(b0, w, True, 0)
            assert t0 % (1 << 8 * w) == int(v[15]), (w, kind, seed)
            u1, t1 = H.delta_block_host(b1, w, True, t0)
            assert u0 + u1 == dwords, (w, kind, seed)
            assert (t0 + t1) % (1 << 8 * w) == int(v[31]), (w, kind, seed)


def test_sanitized_program_over_the_host_definitions(tmp_path):
    """A stand-alone program (own main) drives delta.h's host definitions and block transforms over the grid's lengths, built with
    AddressSanitizer and UBSan and run directly."""
    src, exe = tmp_path / "delta_check.cpp", tmp_path / "delta_check"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "delta.h"
static uint32_t state = 12345u;
static uint8_t next() { state = state * 1664525u + 1013904223u; return static_cast<uint8_t>(state >> 24); }
template <int W> static int blocks() {
    uint8_t bytes[32 * W], back[32 * W];
    for (auto &b : bytes) b = next();
    uint32_t d[2][4 * W];
    memcpy(d, bytes, sizeof bytes);
    const uint64_t last = gpuar::delta_load(bytes + 15 * W, W);
    gpuar::delta_block<W>(d[0], 0), gpuar::delta_block<W>(d[1], last);
    std::vector<uint8_t> want(sizeof bytes);
    gpuar::delta_host<false>(bytes, sizeof bytes, W, want.data());
    int bad = memcmp(d, want.data(), sizeof bytes) != 0;
    const uint64_t t0 = gpuar::undelta_block<W>(d[0], 0);
    gpuar::undelta_block<W>(d[1], t0);
    memcpy(back, d, sizeof back);
    return bad + (memcmp(back, bytes, sizeof bytes) != 0);
}
int main() {
    int bad = 0;
    for (uint32_t w = 1; w <= 8; w *= 2) {
        const size_t G = size_t(w) * gpuar::kPlanePacket;
        const size_t lengths[] = {0, 1, w - 1, w, 15, 16 * w + 1, 8191, 8192, G - 1, G, G + 1, 3 * G + 4097};
        for (size_t n : lengths)
            for (int kind = 0; kind < 2; ++kind) {
                // exact-size heap blocks: one byte read or written beyond n is a report
                std::vector<uint8_t> x(n), split(n), back(n);
                for (auto &b : x) b = kind ? 0xFF : next();
                gpuar::split_delta_host(x.data(), n, w, split.data());
                gpuar::merge_delta_host(split.data(), n, w, back.data());
                bad += x != back;
                std::vector<uint8_t> place(x);
                gpuar::split_delta_host(place.data(), n, w, place.data());
                bad += place != split;
                gpuar::merge_delta_host(place.data(), n, w, place.data());
                bad += place != x;
            }
    }
    for (int t = 0; t < 100; ++t) bad += blocks<1>() + blocks<2>() + blocks<4>() + blocks<8>();
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
    """{name: (bytes, w, estimate of split_planes, estimate of split_delta, packets)} on the nine inputs, computed once"""
    out = {}
    for name, (a, w) in D.table_inputs().items():
        x = D.raw_bytes(a).tobytes()
        planes = sum(H.estimate_host(H.split_planes_host(x, w)))
        delta = sum(H.estimate_host(H.split_delta_host(x, w)))
        out[name] = (x, w, planes, delta, (len(x) + PACKET - 1) // PACKET)
    return out


def test_sizes_of_the_table_inputs(table_estimates):
    """delta + planes against planes alone, by the codec's size estimate.  The bounds are those of the issue: the numpy formula
    gave 0.07 - 0.52 for the four ordered integer inputs and the uint8 walk, 0.71 for the int16 walk, and >= 1.0 for unordered
    int64, fp32 and uniform bytes."""
    for name, (x, w, planes, delta, _np) in table_estimates.items():
        ratio = delta / planes
        print(f"{name}: w {w}, planes {planes / len(x):.3f}, delta + planes {delta / len(x):.3f}, delta / planes {ratio:.3f}")
    for name, (x, w, planes, delta, _np) in table_estimates.items():
        ratio = delta / planes
        if name in ("csr_offsets", "timestamps", "position_ids", "sorted_indices", "uint8_walk"):
            assert ratio <= 0.6, (name, ratio)
        elif name == "int16_walk":
            assert ratio <= 0.8, (name, ratio)
        else:
            assert ratio >= 1.0, (name, ratio)


def test_the_estimate_is_the_codecs_size_on_filtered_bytes(H, port_oracle, table_estimates):
    x, w, _planes, delta, n_packets = table_estimates["csr_offsets"]
    filtered = np.frombuffer(H.split_delta_host(x, w), dtype=np.uint8)
    assert (filtered == D.numpy_split_delta(np.frombuffer(x, dtype=np.uint8), w)).all()
    coded = port_oracle.encode_stream(filtered).size
    print(f"csr_offsets: estimate {delta}, codec {coded}, {n_packets} packets")
    assert abs(coded - delta) <= n_packets


def test_the_rule_of_auto_on_host_estimates(table_estimates):
    """delta iff est_delta + n_packets <= est_plain (plain: the split without the filter)."""
    for name, (_x, _w, planes, delta, n_packets) in table_estimates.items():
        assert (delta + n_packets <= planes) == (name in D.TABLE_DELTA_WINS), (name, planes, delta, n_packets)


# ---- the container ----------------------------------------------------------------------------------------------------

def cli_input(n, w):
    """sorted-ish integers of width w: what the filter is for"""
    rng = np.random.default_rng(n + w)
    m = n // w + 1
    v = np.cumsum(rng.integers(0, 50, m)).astype(np.uint64).astype(D.UINT[w])
    return v.astype("<u%d" % w).view(np.uint8)[:n].copy()


def delta_args(w):
    return ["--delta"] + ([f"--planes={w}"] if w > 1 else [])


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("w", D.WIDTHS)
def test_delta_file_round_trips_and_its_trailer_is_version_4(H, host_cli, port_oracle, tmp_path, w, checksum):
    from gpuar_amd import batch
    for n in (0, 1, w - 1, 8191, w * PACKET, w * PACKET + 1, 70 * PACKET + 13):
        x = cli_input(n, w)
        src, gip, back = tmp_path / "in", tmp_path / "out.gip", tmp_path / "back"
        x.tofile(src)
        r = run(host_cli, "c", "--host", *delta_args(w), *(["--checksum"] if checksum else []), f"--in={src}", f"--out={gip}")
        assert r.returncode == 0, r.stderr
        data = gip.read_bytes()
        stream = port_oracle.encode_stream(D.numpy_split_delta(x, w)).tobytes() if n else b""
        size = struct.unpack("<Q", data[12:20])[0]
        assert struct.unpack("<Q", data[4:12])[0] == n and size == 20 + len(stream), (w, n)
        assert data[20:size] == stream, (w, n)
        clens = R.packet_lengths(stream)
        crcs = [zlib.crc32(x[p * PACKET:(p + 1) * PACKET].tobytes()) for p in range(len(clens))] if checksum else None      # of the ORIGINAL bytes
        trailer = data[size:]
        assert trailer == D.trailer_v4(clens, w, crcs) == batch.trailer(clens, w, crcs, delta=True), (w, n)
        assert trailer[:4] == b"GIPX" and struct.unpack("<IQII", trailer[4:24]) == (4, len(clens), w, 3 if checksum else 2)
        assert trailer[-4:] == b"XPIG" and struct.unpack("<Q", trailer[-12:-4])[0] == len(trailer)
        r = run(host_cli, "d", "--host", "--delta", f"--in={gip}", f"--out={back}")      # (on d the flag is accepted and means nothing)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == x.tobytes(), (w, n)
    # the file does not depend on --threads
    a = tmp_path / "t4.gip"
    assert run(host_cli, "c", "--host", "--threads=4", *delta_args(w), *(["--checksum"] if checksum else []), f"--in={src}", f"--out={a}").returncode == 0
    assert a.read_bytes() == data


def test_without_the_flag_the_file_is_what_it_was(host_cli, tmp_path):
    x = cli_input(5 * PACKET + 17, 4)
    src = tmp_path / "in"
    x.tofile(src)
    for w in (1, 2, 4, 8):
        for extra in ([], ["--checksum"], ["--index"]):
            a = tmp_path / "a.gip"
            assert run(host_cli, "c", "--host", f"--planes={w}", *extra, f"--in={src}", f"--out={a}").returncode == 0
            data = a.read_bytes()
            size = struct.unpack("<Q", data[12:20])[0]
            stream = data[20:size]
            clens = R.packet_lengths(stream)
            crcs = [zlib.crc32(x[p * PACKET:(p + 1) * PACKET].tobytes()) for p in range(len(clens))] if extra == ["--checksum"] else None
            from gpuar_amd import batch
            want = batch.trailer(clens, w, crcs) if (w > 1 or extra) else b""
            assert data[size:] == want, (w, extra)
            if w > 1:
                assert data[size:] == R.trailer_v3(clens, w, crcs)
            if data[size:]:
                assert struct.unpack_from("<I", data, size + 4)[0] in (1, 2, 3)


def _good_file(host_cli, tmp_path, w, checksum, n=5 * PACKET + 100):
    x = cli_input(n, w)
    src, gip = tmp_path / "in", tmp_path / "good.gip"
    x.tofile(src)
    assert run(host_cli, "c", "--host", *delta_args(w), *(["--checksum"] if checksum else []), f"--in={src}", f"--out={gip}").returncode == 0
    data = bytearray(gip.read_bytes())
    return x, data, struct.unpack("<Q", data[12:20])[0]


def _refused(host_cli, tmp_path, data):
    bad, out = tmp_path / "bad.gip", tmp_path / "bad.out"
    bad.write_bytes(bytes(data))
    r = run(host_cli, "d", "--host", f"--in={bad}", f"--out={out}")
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert (out.read_bytes() if out.exists() else b"") == b"", "a refused file leaves no output behind"
    assert "version 4" in r.stderr and "byte planes (version 3)" not in r.stderr and "version 3" not in r.stderr, r.stderr


@pytest.mark.parametrize("checksum", [False, True])
def test_unusable_version_4_trailers_are_errors(host_cli, tmp_path, checksum):
    x, good, size = _good_file(host_cli, tmp_path, 2, checksum)
    flags = 3 if checksum else 2
    assert struct.unpack_from("<II", good, size + 4 + 12) == (2, flags)
    for at, value in ((size + 16, 3),                       # the width field says 3
                      (size + 20, flags | 4),               # flag bit 2 set
                      (size + 20, flags & 1)):              # bit 1, delta, clear
        d = bytearray(good)
        d[at:at + 4] = struct.pack("<I", value)
        _refused(host_cli, tmp_path, d)
    d = bytearray(good)                                     # one clen off by one: the lengths no longer add up to the stream
    d[size + 24:size + 26] = struct.pack("<H", struct.unpack("<H", d[size + 24:size + 26])[0] + 1)
    _refused(host_cli, tmp_path, d)
    (tmp_path / "same.gip").write_bytes(bytes(good))
    ok = tmp_path / "ok.out"
    assert run(host_cli, "d", "--host", f"--in={tmp_path / 'same.gip'}", f"--out={ok}").returncode == 0 and ok.read_bytes() == x.tobytes()
