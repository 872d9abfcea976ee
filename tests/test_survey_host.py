"""The plane-width survey on the CPU (gpuar_amd/csrc/survey.h through gpuar_hip_survey_planes_host and gpuar_hip_choose_planes) and
`gpuar-host c --host --planes=auto`.

The oracle is the composition that already ships and is pinned elsewhere: row j of the survey of x is, by definition,
estimate_host(split_planes_host(x, w_j)).  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import planes_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")
PACKET = 8192
SG = 8 * PACKET
WIDTHS = (1, 2, 4, 8)
MIB = 1 << 20
PREFIX = 16 * MIB
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 8191, 8192, 8193, 16383, 16384, 16385, 32768, 65535, 65536, 65537, SG + 3 * PACKET + 77, 2 * SG,
           3 * SG + 24653]
KINDS = ["uniform", "text", "zeros", "ones", "alternating", "last_differs", "period8", "by_eighth", "bf16", "fp32", "int64"]


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as g
    from gpuar_amd import hip
    if not (os.path.exists(hip.LIB_PATH) and os.path.exists(HOST_CLI)):
        g.build()
    hip.load()
    return hip


def data_of(kind, n, seed=0):
    """n bytes of a kind: the six of tests/test_gpu_estimate.py, two that show a wrong residue or group mapping, and typed data."""
    from gpuar_amd import synth
    if kind == "uniform":
        return np.random.default_rng(1000 + n + seed).integers(0, 256, n, dtype=np.uint8)
    if kind == "text":
        return synth.text(3 + seed, n)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "ones":
        return np.full(n, 0xFF, dtype=np.uint8)
    if kind == "alternating":
        return np.tile(np.array([0x41, 0xC2], dtype=np.uint8), n // 2 + 1)[:n]
    if kind == "last_differs":
        x = np.full(n, 0x10, dtype=np.uint8)
        x[PACKET - 1::PACKET] = 0xEF
        if n:
            x[-1] = 0xEF
        return x
    if kind == "period8":                                        # every residue histogram has one bin
        return (17 * (np.arange(n) % 8)).astype(np.uint8)
    if kind == "by_eighth":                                      # every eighth of a supergroup has one bin
        return (29 * ((np.arange(n) // PACKET) % 8)).astype(np.uint8)
    if kind in ("bf16", "fp32"):
        return np.ascontiguousarray(PR.typed_input(kind, (n + 7) // 8 * 8, seed=1 + seed)[:n])
    if kind == "int64":
        return np.random.default_rng(1 + seed).integers(0, 50000, n // 8 + 1, dtype=np.int64).view(np.uint8)[:n].copy()
    raise KeyError(kind)


def oracle(H, x):
    raw = bytes(x)
    return [H.estimate_host(H.split_planes_host(raw, w)) for w in WIDTHS]


def totals_of(rows, n, stored=False):
    """The four predicted totals; with the stored rule a packet whose estimate is not below 4 + its bytes counts as its bytes."""
    out = []
    for row in rows:
        t = 0
        for p, est in enumerate(row):
            ulen = min(PACKET, n - p * PACKET)
            t += ulen if stored and est >= 4 + ulen else est
        out.append(t)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_every_row_is_the_estimate_of_the_split_at_every_length(H, kind):
    for n in LENGTHS:
        x = data_of(kind, n)
        assert x.size == n
        assert H.survey_planes_host(x.tobytes()) == oracle(H, x), (kind, n)


def test_the_stride_and_the_argument_checks(H):
    import ctypes as C
    lib = H.load()
    x = data_of("bf16", SG + 100).tobytes()
    npk = H.packet_count(len(x))
    stride = npk + 3
    est = (C.c_uint32 * (4 * stride))(*([0x5A5A5A5A] * (4 * stride)))
    assert lib.gpuar_hip_survey_planes_host(x, len(x), est, stride) == 0
    want = oracle(H, x)
    for j in range(4):
        assert list(est[j * stride:j * stride + npk]) == want[j]
        assert list(est[j * stride + npk:(j + 1) * stride]) == [0x5A5A5A5A] * 3
    assert lib.gpuar_hip_survey_planes_host(None, 0, None, 0) == 0
    assert lib.gpuar_hip_survey_planes_host(None, len(x), est, stride) == -2
    assert lib.gpuar_hip_survey_planes_host(x, len(x), None, stride) == -2
    assert lib.gpuar_hip_survey_planes_host(x, len(x), est, npk - 1) == -2


def test_the_choice_rule(H):
    assert H.choose_planes([100, 100, 100, 100], 1) == 1                  # all equal
    assert H.choose_planes([0, 0, 0, 0], 0) == 1
    assert H.choose_planes([500, 400, 400, 400], 10) == 2                 # ties go to the smallest width
    assert H.choose_planes([500, 450, 400, 400], 10) == 4
    assert H.choose_planes([500, 450, 401, 400], 0) == 8                  # no packets, no margin
    n = 37
    assert H.choose_planes([1000 + n, 2000, 2000, 1000], n) == 1          # exactly n_packets above the minimum: wins
    assert H.choose_planes([1000 + n + 1, 2000, 2000, 1000], n) == 8      # one more: does not
    assert H.choose_planes([5000, 1000 + n + 1, 1000 + n, 1000], n) == 4
    assert H.choose_planes([1 << 40, (1 << 40) - 5, 1 << 41, 1 << 42], 5) == 1               # totals beyond 32 bits


def one_mib(name):
    rng = np.random.default_rng(1)
    if name in ("bf16", "fp32", "uniform"):
        return PR.typed_input(name, MIB)
    if name == "int64":
        return rng.integers(0, 50000, MIB // 8, dtype=np.int64).view(np.uint8)
    if name == "int32":
        return rng.integers(0, 50000, MIB // 4, dtype=np.int32).view(np.uint8)
    if name == "fp64":
        return (rng.standard_normal(MIB // 8) * 0.02).view(np.uint8)
    if name == "fp16":
        return (rng.standard_normal(MIB // 2).astype(np.float32) * np.float32(0.02)).astype(np.float16).view(np.uint8)
    if name == "text":
        from gpuar_amd import synth
        return synth.text(3, MIB)
    raise KeyError(name)


@pytest.mark.parametrize("name,width", [("bf16", 2), ("fp32", 4), ("uniform", 1), ("int64", 8), ("int32", 4), ("fp64", 8), ("fp16", 2),
                                        ("text", 1)])
def test_the_rule_picks_the_element_width_of_typed_data(H, name, width):
    x = one_mib(name)
    assert x.size == MIB
    rows = H.survey_planes_host(x.tobytes())
    assert rows == oracle(H, x)
    for stored in (False, True):
        totals = totals_of(rows, MIB, stored)
        print(name, "stored" if stored else "plain", totals)
        assert H.choose_planes(totals, MIB // PACKET) == width, (name, stored, totals)


def run(*args):
    return subprocess.run([HOST_CLI, *args], capture_output=True, text=True, check=True).stdout


def chosen_for(H, x):
    prefix = bytes(x[:PREFIX])
    return H.choose_planes(totals_of(H.survey_planes_host(prefix), len(prefix)), H.packet_count(len(prefix)))


def check_cli(H, tmp_path, x, tag):
    src, auto, fixed, back = (str(tmp_path / f"{tag}.{ext}") for ext in ("bin", "auto.gip", "fixed.gip", "back"))
    x.tofile(src)
    w = chosen_for(H, x)
    out = run("c", "--host", "--planes=auto", f"--in={src}", f"--out={auto}")
    assert f"planes=auto: width {w}" in out, out
    if w == 1:
        run("c", "--host", f"--in={src}", f"--out={fixed}")                           # the file without the flag: no trailer
    else:
        run("c", "--host", f"--planes={w}", f"--in={src}", f"--out={fixed}")
    assert open(auto, "rb").read() == open(fixed, "rb").read(), (tag, w)
    run("d", "--host", f"--in={auto}", f"--out={back}")
    assert open(back, "rb").read() == x.tobytes(), tag
    return w


@pytest.mark.parametrize("name,width", [("bf16", 2), ("fp32", 4), ("int64", 8), ("uniform", 1)])
def test_the_cli_writes_the_file_of_the_chosen_width(H, tmp_path, name, width):
    small = data_of(name, 5 * PACKET + 100)
    check_cli(H, tmp_path, small, name + "_small")
    assert check_cli(H, tmp_path, one_mib(name), name + "_mib") == width


def test_the_cli_chooses_from_the_first_16_mib(H, tmp_path):
    x = np.concatenate([PR.typed_input("bf16", PREFIX), PR.typed_input("uniform", 2 * MIB + 4321, seed=2)])
    assert check_cli(H, tmp_path, x, "prefix") == 2
