"""Sparse packets on the CPU (no GPU needed): the host definitions of gpuar_amd/csrc/sparse.h -- scan, record, validity, rule --
against their numpy restatement (tests/sparse_ref.py) on the packets every implementation is tested on, the damaged records one
class at a time, the argument checks of the new calls, and a sanitized stand-alone program over the header."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import sparse_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
def cases():
    return S.cases()


def _ptr(a, at=0):
    return C.c_void_p(a.ctypes.data + at)


def test_the_case_list_holds_what_it_promises(cases):
    names = [name for name, _x in cases]
    assert len(names) == len(set(names)) and len(cases) < 80
    scans = {name: S.scan(x) for name, x in cases}
    for n in S.LENGTHS:
        assert any(x.size == n and scans[name] != S.NONE and scans[name] >> 8 == 0 for name, x in cases), n
        assert any(x.size == n and name.startswith("half_plus_1") and scans[name] >> 8 == n - (n // 2 + 1) for name, x in cases), n
        if n > 1:
            assert any(x.size == n and name.startswith("half_n") and scans[name] == S.NONE for name, x in cases), n
    fills = {scans[name] & 255 for name, _x in cases if scans[name] != S.NONE and name.startswith(("k0", "all_values", "half_plus_1"))}
    assert fills >= set(S.FILLS)
    for name, x in cases:
        if name.startswith("all_values"):
            f = scans[name] & 255
            assert set(x.tolist()) == set(range(256)) and scans[name] >> 8 == 255 and f in S.FILLS
        if name.startswith("one_lane"):
            assert (x[384:512] != x[0]).all() and scans[name] >> 8 == 128
        if name.startswith("every_lane_n8192"):
            assert all((x[128 * l:128 * l + 128] != (scans[name] & 255)).sum() == 1 for l in range(64))
        if name.startswith("ends_n8192") or name.startswith("ends_n4097"):
            f = scans[name] & 255
            assert x[0] != f and x[-1] != f and x[127] != f and x[128] != f


def test_scan_pack_and_unpack_against_the_restatement(H, cases):
    lib = H.load()
    for name, x in cases:
        n = x.size
        want_scan, want_rec = S.scan(x), S.pack(x)
        assert H.sparse_scan_host(x.tobytes()) == [want_scan], name
        rec = np.full(S.sparse_len(PACKET // 2) + GUARD, 0x5A, dtype=np.uint8)
        length = C.c_size_t(12345)
        if want_rec is None:
            assert lib.gpuar_hip_sparse_pack_host(_ptr(x), n, _ptr(rec), rec.size, C.byref(length)) == -2, name
            assert (rec == 0x5A).all() and length.value == 12345, name
            continue
        k = want_scan >> 8
        assert len(want_rec) == S.sparse_len(k) == H.sparse_len(k) and 2 * k < n
        assert lib.gpuar_hip_sparse_pack_host(_ptr(x), n, _ptr(rec), len(want_rec), C.byref(length)) == 0, name       # exactly the room it needs
        assert length.value == len(want_rec) and rec[:length.value].tobytes() == want_rec, name                       # the pads included
        assert (rec[length.value:] == 0x5A).all(), (name, "wrote behind the record")
        assert lib.gpuar_hip_sparse_pack_host(_ptr(x), n, _ptr(rec), len(want_rec) - 1, C.byref(length)) == -2, name   # one byte short
        out = np.full(n + GUARD, 0x5A, dtype=np.uint8)
        assert lib.gpuar_hip_sparse_unpack_host(_ptr(rec), len(want_rec), _ptr(out), n) == 0, name
        assert (out[:n] == x).all() and (out[n:] == 0x5A).all(), name
        assert (S.unpack(want_rec, len(want_rec), n) == x).all(), name
        assert H.sparse_unpack_host(H.sparse_pack_host(x.tobytes()), n) == x.tobytes(), name
        # a record with room behind it is the same record
        assert lib.gpuar_hip_sparse_unpack_host(_ptr(rec), len(want_rec) + GUARD, _ptr(out), n) == 0 and (out[:n] == x).all(), name


def test_scan_of_a_buffer_is_the_scan_of_its_packets(H, cases):
    parts = [x for _name, x in cases if x.size == PACKET][:5] + [cases[3][1]]       # full packets and a short last one
    data = np.concatenate(parts)
    assert H.sparse_scan_host(data.tobytes()) == [S.scan(x) for x in parts]
    assert H.sparse_scan_host(b"") == []


def test_sparse_len_and_the_rule_match_the_table(H):
    for k in (0, 1, 2, 3, 4, 5, 82, 128, 4095):
        assert H.sparse_len(k) == S.sparse_len(k) == -(-(4 + 3 * k) // 4) * 4
    assert [H.sparse_len(k) for k in (0, 1, 8, 16, 32, 64, 82, 128)] == [4, 8, 28, 52, 100, 196, 252, 388]
    for scan, est, n, on, want in S.RULE_TABLE:
        assert S.rule(scan, est, n, on) == want, (scan, est, n, on)
        assert H.sparse_rule(scan, est, n, on) == want, (scan, est, n, on)
    rng = np.random.default_rng(5)
    for _ in range(3000):                                   # and the restatement everywhere else
        n = int(rng.choice([1, 2, 3, 4, 5, 8, 9, 16, 17, 300, 8191, 8192]))
        scan = S.NONE if rng.random() < 0.2 else (int(rng.integers(0, (n + 1) // 2)) << 8) | int(rng.integers(0, 256))
        est = int(rng.choice([4, 5, 6, 8, 9, 12, n + 3, n + 4, n + 5, int(rng.integers(4, 9000))]))
        for on in (False, True):
            assert H.sparse_rule(scan, est, n, on) == S.rule(scan, est, n, on), (scan, est, n, on)
    assert H.SPARSE_NONE == S.NONE and (H.KIND_CODED, H.KIND_RAW, H.KIND_SPARSE) == (S.CODED, S.RAW, S.SPARSE)


def test_the_size_table_of_the_design(H):
    """k distinct exception values in 8192 bytes (the worst case for the coder): the estimate against the record."""
    coded, sparse = [], []
    for k in (0, 1, 8, 16, 32, 64, 82, 128):
        x = np.zeros(PACKET, dtype=np.uint8)
        x[np.arange(k) * 61 + 3] = np.arange(k) + 1
        coded.append(H.estimate_host(x.tobytes())[0])
        sparse.append(len(H.sparse_pack_host(x.tobytes())))
        assert H.sparse_rule(H.sparse_scan_host(x.tobytes())[0], coded[-1], PACKET, True) == S.SPARSE
    print("coded", coded, "sparse", sparse)
    assert coded == [210, 212, 223, 236, 262, 314, 343, 418] and sparse == [4, 8, 28, 52, 100, 196, 252, 388]
    assert all(s < c for s, c in zip(sparse, coded))


def test_the_sizes_of_the_xor_base_cases(H):
    """What README.md and DESIGN.md 4.12 quote: 1 MiB of bf16 against its base, w = 2, by the host functions alone -- planes alone,
    XORed with stored="auto", and XORed with stored="auto" and sparse="auto" (the rule applied per packet)."""
    import planes_ref as R
    import xor_ref as X
    got = {}
    for name, (x, b, w) in S.xor_base_cases().items():
        planes = sum(H.estimate_host(R.numpy_split(x, w).tobytes()))
        split = X.numpy_split_xor(x, b, w).tobytes()
        est, scan = H.estimate_host(split), H.sparse_scan_host(split)
        assert len(est) == 128
        stored = sum(PACKET if H.stored_rule(e, PACKET) else e for e in est)
        kinds = [H.sparse_rule(s, e, PACKET, True) for s, e in zip(scan, est)]
        sparse = sum(S.sparse_len(s >> 8) if k == S.SPARSE else PACKET if k == S.RAW else e for k, s, e in zip(kinds, scan, est))
        got[name] = (planes, stored, sparse, kinds.count(S.SPARSE), max(s >> 8 for s in scan))
        print(name, got[name])
    assert got == {"equal": (714820, 26880, 512, 128, 0), "replaced_0.1%": (714811, 28405, 3544, 128, 13),
                   "replaced_1%": (714793, 40914, 28852, 128, 100)}


@pytest.mark.parametrize("name,rec,rec_bytes,n", S.damaged(), ids=[d[0] for d in S.damaged()])
def test_damaged_records_are_refused(H, name, rec, rec_bytes, n):
    lib = H.load()
    assert S.unpack(rec, rec_bytes, n) is None                                  # the restatement refuses it too
    held = np.frombuffer(rec, dtype=np.uint8).copy()
    out = np.full(n + GUARD, 0x5A, dtype=np.uint8)
    assert lib.gpuar_hip_sparse_unpack_host(_ptr(held), rec_bytes, _ptr(out), n) == -2
    assert (out[n:] == 0x5A).all(), "wrote outside the packet"
    with pytest.raises(H.GpuarError):
        H.sparse_unpack_host(rec[:rec_bytes], n)


def test_the_undamaged_record_is_taken(H):
    good = S.pack(S.GOOD)
    assert H.sparse_unpack_host(good, S.GOOD_N) == S.GOOD.tobytes()


def test_argument_checks(H):
    lib = H.load()
    x = np.zeros(100, dtype=np.uint8)
    rec = np.zeros(64, dtype=np.uint8)
    length = C.c_size_t(0)
    assert lib.gpuar_hip_sparse_pack_host(None, 100, _ptr(rec), 64, C.byref(length)) == -2
    assert lib.gpuar_hip_sparse_pack_host(_ptr(x), 100, None, 64, C.byref(length)) == -2
    assert lib.gpuar_hip_sparse_pack_host(_ptr(x), 100, _ptr(rec), 64, None) == -2
    assert lib.gpuar_hip_sparse_pack_host(_ptr(x), 0, _ptr(rec), 64, C.byref(length)) == -2
    assert lib.gpuar_hip_sparse_pack_host(_ptr(x), PACKET + 1, _ptr(rec), 64, C.byref(length)) == -2
    assert lib.gpuar_hip_sparse_pack_host(_ptr(x), 100, _ptr(rec), 3, C.byref(length)) == -2
    assert lib.gpuar_hip_sparse_pack_host(_ptr(x), 100, _ptr(rec), 4, C.byref(length)) == 0 and length.value == 4
    assert lib.gpuar_hip_sparse_unpack_host(None, 4, _ptr(x), 100) == -2 and lib.gpuar_hip_sparse_unpack_host(_ptr(rec), 4, None, 100) == -2
    assert lib.gpuar_hip_sparse_unpack_host(_ptr(rec), 4, _ptr(x), 0) == -2 and lib.gpuar_hip_sparse_unpack_host(_ptr(rec), 4, _ptr(x), PACKET + 1) == -2
    assert lib.gpuar_hip_sparse_scan_host(None, 0, None) == 0
    assert lib.gpuar_hip_sparse_scan_host(None, 10, _ptr(rec)) == -2 and lib.gpuar_hip_sparse_scan_host(_ptr(x), 10, None) == -2
    a = 1 << 20                                             # the device calls: host-side checks come first, as for the estimate calls
    for fn, twin in ((lib.gpuar_hip_sparse_scan, lib.gpuar_hip_estimate),):
        assert fn(None, 0, None, None) == twin(None, 0, None, None) == 0
        assert fn(None, 100, a, None) == twin(None, 100, a, None) == -2 and fn(a, 100, None, None) == twin(a, 100, None, None) == -2
        assert fn(a + 8, 100, a, None) == twin(a + 8, 100, a, None) == -1 and fn(a, 100, a + 2, None) == twin(a, 100, a + 2, None) == -1
    for fn, twin in ((lib.gpuar_hip_sparse_scan_batch, lib.gpuar_hip_estimate_batch),):
        assert fn(a, a, a, 1, 0, a, None, None) == twin(a, a, a, 1, 0, a, None, None) == 0
        assert fn(None, a, a, 1, 1, a, None, None) == twin(None, a, a, 1, 1, a, None, None) == -2
        assert fn(a, a, a, 1, 1, None, None, None) == twin(a, a, a, 1, 1, None, None, None) == -2
        assert fn(a, a, a, 1, 1, a + 2, None, None) == twin(a, a, a, 1, 1, a + 2, None, None) == -1
        assert fn(a + 4, a, a, 1, 1, a, None, None) == twin(a + 4, a, a, 1, 1, a, None, None) == -1
    assert lib.gpuar_hip_sparse_pack(None, None, None, None, 0, None, None) == 0
    assert lib.gpuar_hip_sparse_unpack(None, None, None, None, 0, None, None) == 0
    for missing in range(4):
        args = [a, a, a, a]
        args[missing] = None
        assert lib.gpuar_hip_sparse_pack(*args, 1, None, None) == -2 and lib.gpuar_hip_sparse_unpack(*args, 1, None, None) == -2, missing
    for off in range(4):
        args = [a, a, a, a]
        args[off] = a + (2 if off == 2 else 4)              # (d_scan, pack's third array, is 32-bit: 4-byte aligned)
        assert lib.gpuar_hip_sparse_pack(*args, 1, None, None) == -1, off
        args[off] = a + 4
        assert lib.gpuar_hip_sparse_unpack(*args, 1, None, None) == -1, off
    assert lib.gpuar_hip_sparse_pack(a, a, a, a, 1, a + 2, None) == -1 and lib.gpuar_hip_sparse_unpack(a, a, a, a, 1, a + 2, None) == -1
    assert lib.gpuar_hip_abi_version() == 2


def test_sanitized_program_over_the_host_definitions(tmp_path, cases):
    """A stand-alone program (own main) drives sparse.h's host definitions over the packets of the case list and the damaged
    records, each in a heap block of exactly its size, built with AddressSanitizer and UBSan and run directly."""
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _name, x in cases:
            f.write(struct.pack("<I", x.size) + x.tobytes())
        bad = S.damaged()
        f.write(struct.pack("<I", len(bad)))
        for _name, rec, rec_bytes, n in bad:
            held = rec[:rec_bytes]                          # what a reader may touch
            f.write(struct.pack("<III", n, rec_bytes, len(held)) + held)
    src, exe = tmp_path / "sparse_check.cpp", tmp_path / "sparse_check"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sparse.h"
static uint32_t word(FILE *f) { uint32_t v = 0; if (fread(&v, 4, 1, f) != 1) std::abort(); return v; }
static std::vector<uint8_t> block(FILE *f, size_t n) { std::vector<uint8_t> v(n); if (n && fread(v.data(), 1, n, f) != n) std::abort(); return v; }
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int bad = 0, sparse = 0;
    for (uint32_t c = word(f); c > 0; --c) {
        const uint32_t n = word(f);
        const std::vector<uint8_t> x = block(f, n);          // exact-size heap blocks: one byte beyond is a report
        const uint32_t scan = gpuar::sparse_scan_packet(x.data(), n);
        uint32_t many = 0;
        gpuar::sparse_scan_host(x.data(), n, &many);
        bad += many != scan;
        size_t len = 777;
        if (scan == gpuar::kSparseNone) {
            std::vector<uint8_t> none(1);
            bad += gpuar::sparse_pack_host(x.data(), n, none.data(), 0, &len) || len != 777;
            continue;
        }
        ++sparse;
        const uint32_t k = scan >> 8;
        std::vector<uint8_t> rec(gpuar::sparse_len(k)), back(n), small(gpuar::sparse_len(k) - 1);
        bad += !gpuar::sparse_pack_host(x.data(), n, rec.data(), rec.size(), &len) || len != rec.size();
        bad += gpuar::sparse_pack_host(x.data(), n, small.data(), small.size(), &len);
        bad += !gpuar::sparse_unpack_host(rec.data(), rec.size(), back.data(), n) || back != x;
        bad += gpuar::sparse_kind(scan, 0xFFFFFFFFu, n, false) != gpuar::kSparseSparse;
    }
    int refused = 0;
    for (uint32_t c = word(f); c > 0; --c) {
        const uint32_t n = word(f), rec_bytes = word(f), held = word(f);
        const std::vector<uint8_t> rec = block(f, held);
        std::vector<uint8_t> out(n);
        refused += !gpuar::sparse_unpack_host(rec.data(), rec_bytes, out.data(), n);
    }
    fclose(f);
    std::printf("%d %d %d\n", bad, sparse, refused);
    return 0;
}
""")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gpuar_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    n_sparse = sum(S.scan(x) != S.NONE for _name, x in cases)
    assert r.returncode == 0 and r.stdout.split() == ["0", str(n_sparse), str(len(S.damaged()))], (r.returncode, r.stdout, r.stderr[-2000:])
