"""The XOR-base survey on the CPU (gpuar_amd/csrc/xor_survey.h through gpuar_hip_survey_xor_host; no device is touched).

Two oracles, both exact: the numpy restatement of tests/xor_survey_ref.py (XOR, planes_ref's split, integer estimate, majority
scan), and the identity that defines the survey -- survey_xor_host(x, b) is (survey_planes_host(x ^ b), sparse_scan_host of
split_planes_host(x ^ b, w)) supergroup by supergroup."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import xor_survey_ref as XS
from test_survey_host import KINDS, LENGTHS, MIB, PACKET, SG, WIDTHS, data_of, totals_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as g
    from gpuar_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        g.build()
    hip.load()
    return hip


def base_of(kind, n):
    return data_of("uniform" if kind in ("zeros", "ones") else kind, n, seed=7)


def by_identity(H, x, b):
    """(est, scan) from the calls that were there before: the plane survey and the scan of the plane splits of x ^ b, one supergroup
    at a time"""
    y = (np.frombuffer(bytes(x), dtype=np.uint8) ^ np.frombuffer(bytes(b), dtype=np.uint8)).tobytes()
    est, scan = [[] for _ in WIDTHS], [[] for _ in WIDTHS]
    for at in range(0, len(y), SG):
        rows = H.survey_planes_host(y[at:at + SG])
        for j, w in enumerate(WIDTHS):
            est[j] += rows[j]
            scan[j] += H.sparse_scan_host(H.split_planes_host(y[at:at + SG], w))
    return est, scan


@pytest.mark.parametrize("kind", KINDS)
def test_both_rows_are_the_restatement_and_the_identity_at_every_length(H, kind):
    for n in LENGTHS:
        x, b = data_of(kind, n), base_of(kind, n)
        got = H.survey_xor_host(x.tobytes(), b.tobytes())
        assert got == XS.survey_xor(x, b), (kind, n)
        assert got == by_identity(H, x, b), (kind, n)


def test_the_plane_survey_of_the_xor_is_the_est_rows_on_a_whole_buffer(H):
    x, b = XS.int64_pair()
    est, _ = H.survey_xor_host(x[:3 * SG + 24653].tobytes(), b[:3 * SG + 24653].tobytes())
    assert est == H.survey_planes_host((x ^ b)[:3 * SG + 24653].tobytes())


@pytest.mark.parametrize("w", WIDTHS)
def test_the_scan_edges(H, w):
    j = WIDTHS.index(w)
    for tag, x, b, packet, want in XS.scan_edges(w):
        est, scan = H.survey_xor_host(x.tobytes(), b.tobytes())
        assert (est, scan) == XS.survey_xor(x, b), (w, tag)
        if tag in ("equal to its base", "fill 0x5A everywhere"):
            for row in scan:                                # every packet of every width: k = 0 of the fill
                assert row == [want] * len(row), (w, tag)
        else:
            assert scan[j][packet] == want, (w, tag, hex(scan[j][packet]), hex(want))


def test_null_outputs_the_stride_and_the_argument_checks(H):
    lib = H.load()
    x, b = data_of("int64", SG + 3 * PACKET + 77).tobytes(), data_of("int64", SG + 3 * PACKET + 77, seed=3).tobytes()
    npk = H.packet_count(len(x))
    stride = npk + 3
    want_est, want_scan = XS.survey_xor(x, b)

    def rows():
        return (C.c_uint32 * (4 * stride))(*([CANARY] * (4 * stride)))

    def check(words, want):
        for j in range(4):
            assert list(words[j * stride:j * stride + npk]) == want[j]
            assert list(words[j * stride + npk:(j + 1) * stride]) == [CANARY] * 3

    est, scan = rows(), rows()
    assert lib.gpuar_hip_survey_xor_host(x, b, len(x), est, scan, stride) == 0
    check(est, want_est), check(scan, want_scan)
    est, scan = rows(), rows()
    assert lib.gpuar_hip_survey_xor_host(x, b, len(x), est, None, stride) == 0
    check(est, want_est)
    assert list(scan) == [CANARY] * (4 * stride)
    est, scan = rows(), rows()
    assert lib.gpuar_hip_survey_xor_host(x, b, len(x), None, scan, stride) == 0
    check(scan, want_scan)
    assert list(est) == [CANARY] * (4 * stride)
    assert H.survey_xor_host(x, b, scan=False) == (want_est, None) and H.survey_xor_host(x, b, est=False) == (None, want_scan)
    assert lib.gpuar_hip_survey_xor_host(None, None, 0, None, None, 0) == 0                # nothing to do comes first
    assert lib.gpuar_hip_survey_xor_host(None, b, len(x), est, scan, stride) == -2
    assert lib.gpuar_hip_survey_xor_host(x, None, len(x), est, scan, stride) == -2
    assert lib.gpuar_hip_survey_xor_host(x, b, len(x), None, None, stride) == -2
    assert lib.gpuar_hip_survey_xor_host(x, b, len(x), est, scan, npk - 1) == -2
    assert list(est) == [CANARY] * (4 * stride)
    with pytest.raises(H.GpuarError):
        H.survey_xor_host(x, b[:-1])
    with pytest.raises(H.GpuarError):
        H.survey_xor_host(x, b, est=False, scan=False)
    assert H.load().gpuar_hip_abi_version() == 2


def test_on_the_int64_input_the_plain_survey_picks_8_and_the_xor_survey_1(H):
    x, b = XS.int64_pair()
    assert x.size == MIB
    packets = MIB // PACKET
    plain = totals_of(H.survey_planes_host(x.tobytes()), MIB)
    est, scan = H.survey_xor_host(x.tobytes(), b.tobytes())
    xored = totals_of(est, MIB)
    print(plain, xored)
    assert H.choose_planes(plain, packets) == 8
    assert H.choose_planes(xored, packets) == 1
    assert abs(xored[0] - xored[3]) < packets
    assert H.choose_filter(plain, xored, packets) == (1, True)
    # counting sparse packets moves the totals, not the choice
    counted = [XS.kinds_total(est[j], scan[j], MIB, False, True) for j in range(4)]
    print(counted)
    assert all(c < t for c, t in zip(counted, xored)) and H.choose_planes(counted, packets) == 1


def test_the_base_is_kept_for_the_near_base_rows_of_the_table_and_dropped_for_the_others(H):
    import xor_ref as XR
    for name, (x, b) in XS.table_pairs().items():
        packets = H.packet_count(x.size)
        plain = totals_of(H.survey_planes_host(x.tobytes()), x.size)
        xored = totals_of(H.survey_xor_host(x.tobytes(), b.tobytes(), scan=False)[0], x.size)
        print(name, plain, xored)
        _, kept = H.choose_filter(plain, xored, packets)
        assert kept == (name in XR.TABLE_BASE_WINS), (name, plain, xored)
        assert (name in XR.TABLE_BASE_WINS) != (name in XR.TABLE_BASE_LOSES)
        assert (xored[1] + packets <= plain[1]) == kept, name                  # the fixed-width rule at the tensors' own width, 2


def test_sanitized_program_over_the_host_definitions(tmp_path):
    """A stand-alone program (own main) drives xor_survey_host over the length grid against the composition estimate_host /
    sparse_scan_host of split_xor_host, built with AddressSanitizer and UBSan and run directly."""
    src, exe = tmp_path / "xor_survey_check.cpp", tmp_path / "xor_survey_check"
    src.write_text(r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "xor_survey.h"
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
            std::vector<uint8_t> x(n), b(n), split(n);
            for (size_t i = 0; i < n; ++i) {
                b[i] = next();
                x[i] = kind == 0 ? next() : kind == 1 ? b[i] : static_cast<uint8_t>(b[i] ^ (next() < 100 ? 0x5A : 0x5B));
            }
            std::vector<uint32_t> est(4 * npk, 0xA5A5A5A5u), scan(4 * npk, 0xA5A5A5A5u), only(4 * npk, 0xA5A5A5A5u), want(npk);
            gpuar::xor_survey_host(x.data(), b.data(), n, est.data(), scan.data(), npk);
            gpuar::xor_survey_host(x.data(), b.data(), n, nullptr, only.data(), npk);
            for (size_t i = 0; i < 4 * npk; ++i) bad += only[i] != scan[i];
            gpuar::xor_survey_host(x.data(), b.data(), n, only.data(), nullptr, npk);
            for (size_t i = 0; i < 4 * npk; ++i) bad += only[i] != est[i];
            for (size_t at = 0, first = 0; at < n; at += SG, first += 8) {
                const size_t len = n - at < SG ? n - at : SG, pk = (len + 8191) / 8192;
                for (uint32_t j = 0; j < 4; ++j) {
                    gpuar::split_xor_host(x.data() + at, b.data() + at, len, 1u << j, split.data());
                    gpuar::estimate_host(split.data(), len, want.data());
                    for (size_t p = 0; p < pk; ++p) bad += est[j * npk + first + p] != want[p];
                    gpuar::sparse_scan_host(split.data(), len, want.data());
                    for (size_t p = 0; p < pk; ++p) bad += scan[j * npk + first + p] != want[p];
                    if (kind == 1)
                        for (size_t p = 0; p < pk; ++p) bad += scan[j * npk + first + p] != 0u;      // equal to its base: fill 0, k = 0
                }
            }
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
