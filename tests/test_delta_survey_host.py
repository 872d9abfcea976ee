"""The delta survey on the CPU (gpuar_amd/csrc/delta_survey.h through gpuar_hip_survey_delta_host and gpuar_hip_choose_filter) and
`gpuar-host c --host --delta=auto`.

The oracle is the composition that already ships and is pinned elsewhere: row j of the delta survey of x is, by definition,
estimate_host(split_delta_host(x, w_j)).  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import delta_ref as D
from test_survey_host import KINDS, LENGTHS, MIB, PACKET, SG, WIDTHS, data_of, one_mib, totals_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")
CUT = 3 * SG + 24653
GROUP_LENGTHS = sorted({w * PACKET + d for w in WIDTHS for d in (-1, 0, 1)})
ALL_LENGTHS = sorted(set(LENGTHS) | set(GROUP_LENGTHS))
# what choose_filter gives on the nine inputs of DESIGN.md 4.9's table and on 1 MiB of bf16, fp32, text and zeros
CHOICES = {"csr_offsets": (8, True), "timestamps": (8, True), "position_ids": (4, True), "sorted_indices": (4, True), "int16_walk": (2, True),
           "uint8_walk": (1, True), "unordered_int64": (8, False), "fp32": (4, False), "uniform": (1, False)}
MORE_CHOICES = {"bf16": (2, False), "fp32": (4, False), "text": (1, False), "zeros": (1, False)}


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as g
    from gpuar_amd import hip
    if not (os.path.exists(hip.LIB_PATH) and os.path.exists(HOST_CLI)):
        g.build()
    hip.load()
    return hip


def oracle(H, x, widths=WIDTHS):
    raw = bytes(x)
    return [H.estimate_host(H.split_delta_host(raw, w)) if w in widths else None for w in WIDTHS]


@pytest.fixture(scope="module")
def table():
    """{name: the input's bytes} for the nine inputs of the table (2^18 elements each)"""
    return {name: D.raw_bytes(a) for name, (a, _w) in D.table_inputs().items()}


def more_input(name):
    return np.zeros(MIB, dtype=np.uint8) if name == "zeros" else one_mib(name)


@pytest.mark.parametrize("kind", KINDS)
def test_every_row_is_the_estimate_of_the_filtered_split_at_every_length(H, kind):
    for n in ALL_LENGTHS:
        x = data_of(kind, n)
        assert x.size == n
        assert H.survey_delta_host(x.tobytes()) == oracle(H, x), (kind, n)


@pytest.mark.parametrize("kind", ["ramp", "ones"])
def test_borrows_through_every_byte_and_across_planes(H, kind):
    for w in WIDTHS:
        for n in ALL_LENGTHS:
            x = D.bytes_of(kind, n, w)
            assert H.survey_delta_host(x.tobytes()) == oracle(H, x), (kind, w, n)


def test_the_table_inputs_cut_to_an_odd_length(H, table):
    for name, x in table.items():
        assert H.survey_delta_host(x[:CUT].tobytes()) == oracle(H, x[:CUT]), name


def test_rows_that_were_not_asked_for_keep_their_canary(H):
    import ctypes as C
    lib = H.load()
    x = data_of("int64", SG + 3 * PACKET + 77).tobytes()
    npk = H.packet_count(len(x))
    want = oracle(H, x)
    for mask in range(1, 16):
        est = (C.c_uint32 * (4 * npk))(*([0x5A5A5A5A] * (4 * npk)))
        assert lib.gpuar_hip_survey_delta_host(x, len(x), mask, est, npk) == 0
        for j in range(4):
            assert list(est[j * npk:(j + 1) * npk]) == (want[j] if mask >> j & 1 else [0x5A5A5A5A] * npk), (mask, j)
    for w in WIDTHS:
        assert H.survey_delta_host(x, widths=(w,)) == oracle(H, x, (w,))
    for bad in ((), (3,), (1, 16)):
        with pytest.raises(H.GpuarError):
            H.survey_delta_host(x, widths=bad)


def test_the_stride_and_the_argument_checks(H):
    import ctypes as C
    lib = H.load()
    x = data_of("int64", SG + 100).tobytes()
    npk = H.packet_count(len(x))
    stride = npk + 3
    est = (C.c_uint32 * (4 * stride))(*([0x5A5A5A5A] * (4 * stride)))
    assert lib.gpuar_hip_survey_delta_host(x, len(x), 15, est, stride) == 0
    want = oracle(H, x)
    for j in range(4):
        assert list(est[j * stride:j * stride + npk]) == want[j]
        assert list(est[j * stride + npk:(j + 1) * stride]) == [0x5A5A5A5A] * 3
    canary = (C.c_uint32 * (4 * stride))(*([0x5A5A5A5A] * (4 * stride)))
    assert lib.gpuar_hip_survey_delta_host(None, 0, 0, None, 0) == 0                       # nothing to do comes first
    assert lib.gpuar_hip_survey_delta_host(None, len(x), 15, canary, stride) == -2
    assert lib.gpuar_hip_survey_delta_host(x, len(x), 15, None, stride) == -2
    assert lib.gpuar_hip_survey_delta_host(x, len(x), 15, canary, npk - 1) == -2
    assert lib.gpuar_hip_survey_delta_host(x, len(x), 0, canary, stride) == -2             # no width asked for
    assert lib.gpuar_hip_survey_delta_host(x, len(x), 16, canary, stride) == -2            # a bit above 3
    assert lib.gpuar_hip_survey_delta_host(x, len(x), 0x1F, canary, stride) == -2
    assert list(canary) == [0x5A5A5A5A] * (4 * stride)
    assert H.load().gpuar_hip_abi_version() == 2


def both_totals(H, x):
    raw = bytes(x)
    return totals_of(H.survey_planes_host(raw), len(raw)), totals_of(H.survey_delta_host(raw), len(raw))


def test_the_choice_on_the_table_inputs(H, table):
    for name, x in table.items():
        plain, filtered = both_totals(H, x)
        print(name, plain, filtered)
        assert H.choose_filter(plain, filtered, x.size // PACKET) == CHOICES[name], (name, plain, filtered)


@pytest.mark.parametrize("name", sorted(MORE_CHOICES))
def test_the_choice_on_floats_text_and_zeros(H, name):
    x = more_input(name)
    assert x.size == MIB
    plain, filtered = both_totals(H, x)
    print(name, plain, filtered)
    assert H.choose_filter(plain, filtered, MIB // PACKET) == MORE_CHOICES[name], (name, plain, filtered)


def test_the_choice_rule(H):
    n = 37
    plain = [5000, 4000, 3000, 3000]                                                       # choose_planes: 4
    assert H.choose_filter(plain, [9000, 9000, 3000 - n, 9000], n) == (4, True)            # exactly n_packets below: the filter
    assert H.choose_filter(plain, [9000, 9000, 3000 - n + 1, 9000], n) == (4, False)       # one byte less of a gain: a tie goes to no filter
    assert H.choose_filter(plain, [9000, 9000, 3000, 9000], n) == (4, False)
    assert H.choose_filter(plain, [100, 9000, 9000, 100], n) == (1, True)                  # the filter's own width, the smallest in a tie
    assert H.choose_filter(plain, [9000, 100 + n + 1, 9000, 100], n) == (8, True)
    assert H.choose_filter([0, 0, 0, 0], [0, 0, 0, 0], 0) == (1, False)                    # empty totals
    assert H.choose_filter([0, 0, 0, 0], [0, 0, 0, 0], 5) == (1, False)
    assert H.choose_filter([1 << 40] * 4, [(1 << 40) - 5, 1 << 41, 1 << 41, 1 << 41], 5) == (1, True)       # totals beyond 32 bits
    assert H.load().gpuar_hip_choose_filter(None, None, 3, None) == 0
    with pytest.raises(H.GpuarError):
        H.choose_filter([1, 2, 3], [1, 2, 3, 4], 1)


def test_position_ids_the_plane_survey_alone_picks_the_wrong_width(H, table):
    x = table["position_ids"]
    plain, filtered = both_totals(H, x)
    assert H.choose_planes(plain, MIB // PACKET) == 8
    assert H.choose_filter(plain, filtered, MIB // PACKET) == (4, True)
    assert plain == [553280, 531328, 415872, 384800] and filtered == [810240, 869824, 27136, 27488]


# ---- the command line -------------------------------------------------------------------------------------------------

def run(*args, ok=True):
    r = subprocess.run([HOST_CLI, *args], capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def compress(tmp_path, src, tag, *flags):
    out = str(tmp_path / f"{tag}.gip")
    r = run("c", "--host", *flags, f"--in={src}", f"--out={out}")
    return open(out, "rb").read(), r.stdout


def round_trip(tmp_path, tag, x):
    back = str(tmp_path / f"{tag}.back")
    run("d", "--host", f"--in={tmp_path / (tag + '.gip')}", f"--out={back}")
    assert open(back, "rb").read() == x.tobytes(), tag


def test_the_cli_chooses_width_and_filter_together(H, tmp_path, table):
    x = table["position_ids"]
    src = str(tmp_path / "position_ids.bin")
    x.tofile(src)
    auto, out = compress(tmp_path, src, "auto", "--delta=auto", "--planes=auto")
    assert "delta=auto: filter on, width 4 " in out, out
    for total in (553280, 531328, 415872, 384800, 810240, 869824, 27136, 27488):
        assert str(total) in out, out
    fixed, _ = compress(tmp_path, src, "fixed", "--delta", "--planes=4")
    assert auto == fixed
    assert compress(tmp_path, src, "on", "--delta=on", "--planes=4")[0] == fixed
    round_trip(tmp_path, "auto", x)


def test_the_cli_leaves_the_filter_off_where_it_would_grow_the_file(H, tmp_path, table):
    """Before --delta=auto existed the value was ignored: the filter was applied and the file grew."""
    x = table["unordered_int64"]
    src = str(tmp_path / "unordered.bin")
    x.tofile(src)
    auto, out = compress(tmp_path, src, "auto", "--delta=auto", "--planes=8")
    assert "delta=auto: filter off, width 8 " in out, out
    plain, _ = compress(tmp_path, src, "plain", "--planes=8")
    filtered, _ = compress(tmp_path, src, "filtered", "--delta", "--planes=8")
    assert auto == plain and len(filtered) > len(plain)
    round_trip(tmp_path, "auto", x)
    joint, out = compress(tmp_path, src, "joint", "--delta=auto", "--planes=auto")
    assert "delta=auto: filter off, width 8 " in out and joint == plain


def test_the_cli_with_a_fixed_width_uses_the_rule_of_auto_at_that_width(H, tmp_path, table):
    x = table["csr_offsets"][:5 * PACKET + 100]
    src = str(tmp_path / "csr.bin")
    x.tofile(src)
    for flags, w in ((["--planes=8"], 8), (["--planes=2"], 2), ([], 1)):
        plain, filtered = both_totals(H, x)
        j = WIDTHS.index(w)
        on = filtered[j] + H.packet_count(x.size) <= plain[j]
        auto, out = compress(tmp_path, src, f"auto{w}", "--delta=auto", *flags)
        assert f"delta=auto: filter {'on' if on else 'off'}, width {w} " in out, out
        want, _ = compress(tmp_path, src, f"want{w}", *(["--delta"] if on else []), *flags)
        assert auto == want, (w, on)
        round_trip(tmp_path, f"auto{w}", x)


def test_the_values_of_the_flag(H, tmp_path, table):
    x = table["int16_walk"][:3 * PACKET + 5]
    src = str(tmp_path / "walk.bin")
    x.tofile(src)
    none, _ = compress(tmp_path, src, "none")
    assert compress(tmp_path, src, "off", "--delta=off")[0] == none
    bare, _ = compress(tmp_path, src, "bare", "--delta")
    assert compress(tmp_path, src, "on", "--delta=on")[0] == bare and bare != none
    for bad in ("--delta=bogus", "--delta=", "--delta=AUTO"):
        r = run("c", "--host", bad, f"--in={src}", f"--out={tmp_path / 'bad.gip'}", ok=False)
        assert r.returncode == 2 and "--delta takes" in r.stderr, (bad, r.returncode, r.stderr)
    assert not os.path.exists(tmp_path / "bad.gip")
    r = run("c", "--host", "--delta=auto", f"--base={src}", f"--in={src}", f"--out={tmp_path / 'bad.gip'}", ok=False)
    assert r.returncode == 2 and "--base and --delta" in r.stderr
    assert "--delta=auto" in run("--help").stdout


def test_an_empty_file_takes_no_filter(H, tmp_path):
    src = str(tmp_path / "empty.bin")
    open(src, "wb").close()
    auto, out = compress(tmp_path, src, "auto", "--delta=auto", "--planes=auto")
    assert "delta=auto: filter off, width 1 " in out
    assert auto == compress(tmp_path, src, "none")[0]


# ---- the host definitions under sanitizers ----------------------------------------------------------------------------

def test_sanitized_program_over_the_host_definitions(tmp_path):
    """A stand-alone program (own main) drives delta_survey_host and choose_filter over the length grid against the composition
    estimate_host(split_delta_host), built with AddressSanitizer and UBSan and run directly."""
    src, exe = tmp_path / "delta_survey_check.cpp", tmp_path / "delta_survey_check"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "delta_survey.h"
static uint32_t state = 12345u;
static uint8_t next() { state = state * 1664525u + 1013904223u; return static_cast<uint8_t>(state >> 24); }
int main() {
    const size_t SG = gpuar::kSurveyBytes;
    const size_t lengths[] = {0, 1, 7, 8, 9, 15, 16, 17, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, 65535, 65536, 65537,
                              SG + 3 * 8192 + 77, 2 * SG, 3 * SG + 24653};
    int bad = 0;
    for (size_t n : lengths)
        for (int kind = 0; kind < 3; ++kind) {
            // exact-size heap blocks: one byte read or one entry written beyond them is a report
            const size_t npk = (n + 8191) / 8192;
            std::vector<uint8_t> x(n), split(n);
            uint64_t walk = 0;
            for (size_t i = 0; i < n; ++i) {
                if (i % 8 == 0) walk += next() & 63u;
                x[i] = kind == 0 ? next() : kind == 1 ? 0xFF : static_cast<uint8_t>(walk >> (8 * (i % 8)));
            }
            std::vector<uint32_t> all(4 * npk, 0xA5A5A5A5u), one(4 * npk), want(npk);
            gpuar::delta_survey_host(x.data(), n, gpuar::kSurveyAllWidths, all.data(), npk);
            uint64_t filtered[4] = {}, plain[4] = {};
            for (uint32_t j = 0; j < 4; ++j) {
                gpuar::split_delta_host(x.data(), n, 1u << j, split.data());
                gpuar::estimate_host(split.data(), n, want.data());
                one.assign(one.size(), 0x5A5A5A5Au);
                gpuar::delta_survey_host(x.data(), n, 1u << j, one.data(), npk);
                for (size_t p = 0; p < npk; ++p) {
                    bad += all[j * npk + p] != want[p] || one[j * npk + p] != want[p];
                    filtered[j] += want[p];
                }
                for (uint32_t i = 0; i < 4; ++i)
                    for (size_t p = 0; p < npk; ++p) bad += i != j && one[i * npk + p] != 0x5A5A5A5Au;
            }
            std::vector<uint32_t> rows(4 * npk);
            gpuar::survey_host(x.data(), n, rows.data(), npk);
            for (uint32_t j = 0; j < 4; ++j)
                for (size_t p = 0; p < npk; ++p) plain[j] += rows[j * npk + p];
            const gpuar::FilterChoice c = gpuar::choose_filter(plain, filtered, npk);
            const uint32_t wp = gpuar::choose_width(plain, npk), wd = gpuar::choose_width(filtered, npk);
            const bool on = npk != 0 && filtered[gpuar::survey_row(wd)] + npk <= plain[gpuar::survey_row(wp)];
            bad += c.filter != on || c.width != (on ? wd : wp) || (n == 0 && (c.filter || c.width != 1u));
            bad += kind == 2 && n >= 65536 && !(c.filter && c.width == 8u);      // a sorted int64 walk: what the filter is for
        }
    std::printf("%d\n", bad);
    return 0;
}
""")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fconstexpr-ops-limit=100000000", "-fconstexpr-loop-limit=1000000",
                           "-I", os.path.join(ROOT, "gpuar_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["0"], (r.returncode, r.stdout, r.stderr[-2000:])
