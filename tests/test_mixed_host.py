"""The mixed filter on the CPU (no GPU needed): the host definitions of gpuar_amd/csrc/mixed.h -- split_mixed / merge_mixed against
the three filters they are composed of, the refusal of invalid modes, choose_modes against the rules written out in Python and
the bound on its totals --, the header's table (include/gpuar_hip_mixed.h, hip.MIXED_SIGNATURES) and a sanitized stand-alone
program over the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mixed_ref as M
from test_capi_symbols import declared_arity, declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "gpuar_hip_mixed.h"
ERR_ARGUMENT = -2


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as g
    from gpuar_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        g.build()
    hip.load()
    return hip


@pytest.fixture(scope="module")
def built(H):
    """the constructed buffer with its three surveys, made once"""
    x, b, where = M.constructed()
    return x, b, where, M.surveys(H, x, b)


def _ptr(a, at=0):
    return C.c_void_p(a.ctypes.data + at)


# ---- the header and its table -----------------------------------------------------------------------------------------

def test_the_header_declares_exactly_the_fourth_table(H):
    lib = H.load()
    names = declared_symbols(HEADER)
    assert set(names) == set(H.MIXED_SIGNATURES) and len(names) == 12, (names, list(H.MIXED_SIGNATURES))
    for other in (set(H.EXPORTS), set(H.GIP_SIGNATURES), set(H.XSURVEY_SIGNATURES), set(declared_symbols())):
        assert not set(names) & other
    for name, arity in declared_arity(HEADER).items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity == len(H.MIXED_SIGNATURES[name][1]), (name, arity, fn.argtypes)
    assert lib.gpuar_hip_abi_version() == 2


def test_mode_counts(H):
    lib = H.load()
    for n, want in ((0, 0), (1, 1), (65535, 1), (65536, 1), (65537, 2), (3 * 65536, 3)):
        assert lib.gpuar_hip_mode_count(n) == want == H.mode_count(n) == M.mode_count(n)
    first, total = H.batch_mode_count([0, 1, 65536, 65537, 0, 200000])
    assert first == [0, 0, 1, 2, 4, 4, 8] and total == 8
    assert [H.mode_parts(m) for m in (0, 3, 5, 10)] == [(1, False, False), (8, False, False), (2, True, False), (4, False, True)]
    with pytest.raises(H.GpuarError):
        H.mode_parts(12)


# ---- split and merge --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", M.MODES)
def test_uniform_modes_equal_the_existing_filters(H, mode):
    for n in M.LENGTHS:
        x, b = M.pair(n, seed=100 * mode + n % 991)
        want = M.dedicated(H, x.tobytes(), b.tobytes(), mode)
        got = H.split_mixed_host(x.tobytes(), M.uniform(mode, n), b.tobytes())
        assert got == want, (mode, n)
        assert H.merge_mixed_host(got, M.uniform(mode, n), b.tobytes()) == x.tobytes(), (mode, n)
        if mode < 8:                                      # no base is asked for: none is needed
            assert H.split_mixed_host(x.tobytes(), M.uniform(mode, n)) == want, (mode, n)


def _in_place(fn, data, modes, base):
    buf = np.frombuffer(bytearray(data) + b"\xA5" * 64, dtype=np.uint8)
    m = np.frombuffer(modes + b"\0", dtype=np.uint8)
    bs = np.frombuffer(base + b"\0", dtype=np.uint8)
    assert fn(_ptr(buf), _ptr(bs), len(data), _ptr(m), _ptr(buf)) == 0
    assert (buf[len(data):] == 0xA5).all(), "bytes behind n were written"
    return buf[:len(data)].tobytes()


def test_round_trips_with_cyclic_and_random_modes_also_in_place(H):
    lib = H.load()
    for n in M.LENGTHS:
        x, b = M.pair(n, seed=7 + n % 313)
        x, b = x.tobytes(), b.tobytes()
        for modes in (M.cyclic(n), M.cyclic(n, 5), M.random_modes(n, n % 89), M.random_modes(n, 1 + n % 97)):
            split = H.split_mixed_host(x, modes, b)
            assert split == M.by_supergroup(H, x, b, modes), (n, modes)
            assert H.merge_mixed_host(split, modes, b) == x, (n, modes)
            assert _in_place(lib.gpuar_hip_split_mixed_host, x, modes, b) == split, (n, modes)
            assert _in_place(lib.gpuar_hip_merge_mixed_host, split, modes, b) == x, (n, modes)


def test_supergroups_are_independent(H):
    """changing one supergroup's mode changes that supergroup's bytes alone"""
    n = 3 * M.SUPER + 5 * M.PACKET + 7
    x, b = (a.tobytes() for a in M.pair(n, seed=3))
    one = H.split_mixed_host(x, bytes([1, 6, 11, 3]), b)
    two = H.split_mixed_host(x, bytes([1, 2, 11, 3]), b)
    assert one[:M.SUPER] == two[:M.SUPER] and one[2 * M.SUPER:] == two[2 * M.SUPER:] and one[M.SUPER:2 * M.SUPER] != two[M.SUPER:2 * M.SUPER]


@pytest.mark.parametrize("bad", M.INVALID)
def test_invalid_modes_are_refused_and_nothing_is_written(H, bad):
    lib = H.load()
    n = 2 * M.SUPER + 100
    x, b = M.pair(n, seed=bad)
    for at in range(3):
        modes = np.array([1, 5, 9], dtype=np.uint8)
        modes[at] = bad
        for fn in (lib.gpuar_hip_split_mixed_host, lib.gpuar_hip_merge_mixed_host):
            out = np.full(n, 0x5A, dtype=np.uint8)
            assert fn(_ptr(x), _ptr(b), n, _ptr(modes), _ptr(out)) == ERR_ARGUMENT, (bad, at)
            assert (out == 0x5A).all(), (bad, at)
    with pytest.raises(H.GpuarError):
        H.split_mixed_host(x.tobytes(), bytes([1, bad, 0]), b.tobytes())


def test_the_other_argument_checks(H):
    lib = H.load()
    n = M.SUPER + 10
    x, b = M.pair(n, seed=1)
    out = np.full(n, 0x5A, dtype=np.uint8)
    modes = np.array([2, 9], dtype=np.uint8)
    for fn in (lib.gpuar_hip_split_mixed_host, lib.gpuar_hip_merge_mixed_host):
        assert fn(_ptr(x), None, n, _ptr(modes), _ptr(out)) == ERR_ARGUMENT          # a base mode and no base
        assert fn(None, _ptr(b), n, _ptr(modes), _ptr(out)) == ERR_ARGUMENT
        assert fn(_ptr(x), _ptr(b), n, None, _ptr(out)) == ERR_ARGUMENT
        assert fn(_ptr(x), _ptr(b), n, _ptr(modes), None) == ERR_ARGUMENT
        assert fn(_ptr(x), _ptr(b), 100, _ptr(modes), _ptr(x, 10)) == ERR_ARGUMENT   # in and out overlap without being equal
        assert fn(_ptr(x), _ptr(out, 10), 100, _ptr(modes), _ptr(out)) == ERR_ARGUMENT      # the base overlaps the output
        assert fn(None, None, 0, None, None) == 0
    assert (out == 0x5A).all()
    with pytest.raises(H.GpuarError):
        H.split_mixed_host(x.tobytes(), bytes([2]), b.tobytes())                     # one mode for two supergroups
    # the device calls: the host-side checks come before any device work
    a = 1 << 20
    far = a + (1 << 20)
    for fn in (lib.gpuar_hip_split_mixed, lib.gpuar_hip_merge_mixed):
        assert fn(None, None, 0, None, None, None, None) == 0
        assert fn(None, None, 4096, far, a, None, None) == ERR_ARGUMENT
        assert fn(a + 4, None, 4096, far, a + 8192, None, None) == -1                # GPUAR_ERR_ALIGNMENT
        assert fn(a, a + 8192 + 4, 4096, far, a + 16384, None, None) == -1           # a misaligned base
        assert fn(a, None, 8192, far, a + 4096, None, None) == ERR_ARGUMENT          # partial overlap
        assert fn(a, a + 8192, 8192, far, a + 8192, None, None) == ERR_ARGUMENT      # the base is the output
        assert fn(a, None, 4096, None, a, None, None) == ERR_ARGUMENT                # no modes
    for fn in (lib.gpuar_hip_split_mixed_batch, lib.gpuar_hip_merge_mixed_batch):
        assert fn(None, None, None, None, None, None, 0, 0, None, None, None) == 0
        assert fn(a, a, a, a, None, a, 1, 1, a, None, None) == ERR_ARGUMENT          # no modes
        assert fn(a, a, a, None, a, a, 1, 1, a, None, None) == ERR_ARGUMENT          # no first_mode
        assert fn(a, a, a, a, a, None, 1, 1, a, None, None) == ERR_ARGUMENT          # no base pointers (zeros say "no base")
        assert fn(a, a, a, a + 4, a, a, 1, 1, a, None, None) == -1
        assert fn(a, a, a, a, a, a + 4, 1, 1, a, None, None) == -1
    assert lib.gpuar_hip_choose_modes(None, None, None, 0, 0, None, None, None, None) == 0
    assert lib.gpuar_hip_choose_modes(a, None, None, 1, 8192, None, None, None, None) == ERR_ARGUMENT
    assert lib.gpuar_hip_choose_modes(a, None, None, 1, 8193, a, None, None, None) == ERR_ARGUMENT      # stride < packets
    assert lib.gpuar_hip_choose_modes(a + 2, None, None, 1, 8192, a, None, None, None) == -1
    assert lib.gpuar_hip_choose_modes_batch(a, None, None, 4, a, a, a, 1, 4, 0, a, None, None, None) == 0
    assert lib.gpuar_hip_choose_modes_batch(a, None, None, 3, a, a, a, 1, 4, 1, a, None, None, None) == ERR_ARGUMENT
    assert lib.gpuar_hip_choose_modes_batch(a, None, None, 4, a, a, a + 4, 1, 4, 1, a, None, None, None) == -1


# ---- the choice -------------------------------------------------------------------------------------------------------

def test_choose_mode_composes_the_existing_rules(H):
    flat = [8000, 8000, 8000, 8000]
    assert H.choose_mode(flat, None, None, 8) == (0, 8000)                            # a tie goes to the smallest width ...
    assert H.choose_mode(flat, [7993, 9000, 9000, 9000], None, 8) == (0, 8000)        # ... to no filter (7 < 8 packets) ...
    assert H.choose_mode(flat, [7992, 9000, 9000, 9000], None, 8) == (4, 7992)
    assert H.choose_mode(flat, None, [9000, 7993, 9000, 9000], 8) == (0, 8000)        # ... and to no base
    assert H.choose_mode(flat, None, [9000, 7992, 9000, 9000], 8) == (9, 7992)
    assert H.choose_mode(flat, [7000, 9000, 9000, 9000], [9000, 9000, 6993, 9000], 8) == (4, 7000)      # the base against what was chosen so far
    assert H.choose_mode(flat, [7000, 9000, 9000, 9000], [9000, 9000, 6992, 9000], 8) == (10, 6992)
    assert H.choose_mode([9, 9, 9, 5], [0, 0, 0, 0], [0, 0, 0, 0], 0) == (3, 5)       # no packets: no filter, no base
    with pytest.raises(H.GpuarError):
        H.choose_mode([1, 2, 3], None, None, 1)


def test_the_constructed_buffer_gets_a_mode_per_part(H, built):
    x, b, where, (plain, delta, xored) = built
    assert x.size == M.TOTAL == 1060921
    modes, totals = H.choose_modes_host(plain, delta, xored, x.size)
    kinds = {kind: set(modes[first:first + count]) for kind, first, count in where}
    assert kinds["bf16"] <= {8, 9, 10, 11} and kinds["int64"] == {7} and kinds["fp32"] == {2}, kinds
    assert all(m < 12 for m in kinds["bytes"]), kinds          # (uniform bytes: every candidate ties within the estimate's noise)
    # what the finer choice buys here: under the best single choice by more than a third
    assert 3 * sum(totals) < 2 * M.best_single_total(plain, delta, xored), (sum(totals), M.best_single_total(plain, delta, xored))


@pytest.mark.parametrize("with_delta", (False, True))
@pytest.mark.parametrize("with_base", (False, True))
def test_choose_modes_is_the_rules_per_supergroup_and_keeps_its_bound(H, built, with_delta, with_base):
    x, _b, _where, (plain, delta, xored) = built
    delta, xored = delta if with_delta else None, xored if with_base else None
    modes, totals = H.choose_modes_host(plain, delta, xored, x.size)
    assert (modes, totals) == M.python_choice(H, plain, delta, xored, x.size)
    assert all(m < (12 if with_base else 8) and (with_delta or m >> 2 != 1) for m in modes)
    n_packets = H.packet_count(x.size)
    assert sum(totals) <= M.best_single_total(plain, delta, xored) + 2 * n_packets
    # the totals are those of the rows the modes name
    rows = {0: plain, 1: delta, 2: xored}
    for s, (m, t) in enumerate(zip(modes, totals)):
        assert t == M.supergroup_totals(rows[m >> 2], x.size)[s][m & 3], (s, m)


def test_every_prefix_length_of_a_short_buffer(H):
    """the last, short supergroup sums 1 .. 8 packets and never reads beyond them"""
    x, b, _where = M.constructed(seed=5)
    for n in (1, 8192, 8193, 3 * 8192 + 5, 65536, 65537, 65536 + 7 * 8192 + 1):
        plain, delta, xored = M.surveys(H, x[:n], b[:n])
        assert H.choose_modes_host(plain, delta, xored, n) == M.python_choice(H, plain, delta, xored, n), n


def test_homogeneous_bf16_gets_its_whole_buffer_width_in_every_full_supergroup(H):
    x = M._bf16(np.random.default_rng(11), (4 * M.SUPER + 3 * M.PACKET) // 2).view(np.uint8)
    plain = H.survey_planes_host(x.tobytes())
    w = H.choose_planes([sum(row) for row in plain], H.packet_count(x.size))
    modes, _totals = H.choose_modes_host(plain, None, None, x.size)
    assert w == 2 and set(modes[:4]) == {H.SURVEY_WIDTHS.index(w)}, (w, modes)


# ---- a compiled caller under the sanitizers ---------------------------------------------------------------------------

def test_sanitized_program_over_the_host_definitions(tmp_path):
    """A stand-alone program (own main) drives mixed.h's host definitions over the lengths above, every output an allocation of
    exactly its bytes (one byte too many is a report), built with AddressSanitizer and UBSan and run directly."""
    src, exe = tmp_path / "mixed_check.cpp", tmp_path / "mixed_check"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "mixed.h"

int main() {
    const size_t S = 65536, lengths[] = {0, 1, 8191, 8192, 65535, 65536, 65537, 2 * S + 8 * 8192 - 1, 3 * S + 5 * 8192 + 7};
    int bad = 0;
    for (size_t n : lengths) {
        const size_t n_modes = gpuar::mode_count(n);
        std::unique_ptr<uint8_t[]> x(new uint8_t[n]), b(new uint8_t[n]), split(new uint8_t[n]), back(new uint8_t[n]), modes(new uint8_t[n_modes]);
        uint32_t v = 12345u + static_cast<uint32_t>(n);
        for (size_t i = 0; i < n; ++i) {
            v = v * 1664525u + 1013904223u;
            x[i] = static_cast<uint8_t>(v >> 24), b[i] = static_cast<uint8_t>(v >> 16) & 0xF0u;
        }
        for (uint32_t start = 0; start < 12u; ++start) {
            for (size_t s = 0; s < n_modes; ++s) modes[s] = static_cast<uint8_t>((start + s) % 12u);
            if (!gpuar::mixed_modes_ok(modes.get(), n, true)) ++bad;
            gpuar::split_mixed_host(x.get(), b.get(), n, modes.get(), split.get());
            gpuar::merge_mixed_host(split.get(), b.get(), n, modes.get(), back.get());
            if (memcmp(back.get(), x.get(), n) != 0) ++bad;
            memcpy(back.get(), x.get(), n);
            gpuar::split_mixed_host(back.get(), b.get(), n, modes.get(), back.get());              // in place
            if (memcmp(back.get(), split.get(), n) != 0) ++bad;
            gpuar::merge_mixed_host(back.get(), b.get(), n, modes.get(), back.get());
            if (memcmp(back.get(), x.get(), n) != 0) ++bad;
        }
        // the choice over rows of exactly the buffer's packets
        const size_t npk = (n + 8191) / 8192;
        std::unique_ptr<uint32_t[]> plain(new uint32_t[4 * npk]), delta(new uint32_t[4 * npk]), xored(new uint32_t[4 * npk]), totals(new uint32_t[n_modes]);
        gpuar::survey_host(x.get(), n, plain.get(), npk);
        gpuar::delta_survey_host(x.get(), n, gpuar::kSurveyAllWidths, delta.get(), npk);
        gpuar::xor_survey_host(x.get(), b.get(), n, xored.get(), nullptr, npk);
        gpuar::choose_modes_host(plain.get(), delta.get(), xored.get(), npk, n, modes.get(), totals.get());
        if (!gpuar::mixed_modes_ok(modes.get(), n, true)) ++bad;
        gpuar::choose_modes_host(plain.get(), nullptr, nullptr, npk, n, modes.get(), nullptr);
        if (!gpuar::mixed_modes_ok(modes.get(), n, false)) ++bad;
    }
    const uint8_t invalid[] = {12, 13, 14, 15, 16, 255};
    for (uint8_t m : invalid)
        if (gpuar::mixed_modes_ok(&m, 1, true)) ++bad;
    const uint8_t based = 9;
    if (gpuar::mixed_modes_ok(&based, 1, false) || !gpuar::mixed_modes_ok(&based, 1, true)) ++bad;
    std::printf("%d\n", bad);
    return 0;
}
""")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fconstexpr-ops-limit=100000000", "-fconstexpr-loop-limit=1000000",
                           "-I", os.path.join(ROOT, "gpuar_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["0"], (r.returncode, r.stdout, r.stderr[-2000:])
