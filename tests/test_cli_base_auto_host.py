"""`gpuar-host c --host --base=FILE --base-auto [--planes=W|auto]`: the base is kept or dropped from a host survey of
the first 16 MiB of the input and of the base, the printed line says what was decided from which totals, and the file is byte for
byte that of the explicit flags -- `--base=FILE --planes=W` where the base was kept, `--planes=W` alone where it was dropped."""
import os
import subprocess

import numpy as np
import pytest

import xor_survey_ref as XS
from test_survey_host import PACKET, WIDTHS, totals_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as g
    from gpuar_amd import hip
    if not (os.path.exists(hip.LIB_PATH) and os.path.exists(HOST_CLI)):
        g.build()
    hip.load()
    return hip


def run(*args, ok=True):
    r = subprocess.run([HOST_CLI, *args], capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def compress(tmp_path, src, tag, *flags):
    out = str(tmp_path / f"{tag}.gip")
    r = run("c", "--host", *flags, f"--in={src}", f"--out={out}")
    return open(out, "rb").read(), r.stdout


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{name: (input path, base path, input bytes, base bytes)}: the int64 pair (the base pays, and the width moves from 8 to 1),
    bf16 against an unrelated tensor and uniform against uniform (the base does not pay), cut to an odd length"""
    d = tmp_path_factory.mktemp("base_auto")
    table = XS.table_pairs()
    cut = 5 * 65536 + 3 * PACKET + 4099
    pairs = {"int64": XS.int64_pair(), "unrelated": table["unrelated"], "uniform": tuple(a[:cut] for a in table["uniform"]),
             "one_percent": tuple(a[:cut] for a in table["one_percent"])}
    out = {}
    for name, (x, b) in pairs.items():
        src, base = str(d / f"{name}.bin"), str(d / f"{name}.base")
        x.tofile(src), b.tofile(base)
        out[name] = (src, base, x, b)
    return out


def totals(H, x, b):
    return totals_of(H.survey_planes_host(x.tobytes()), x.size), totals_of(H.survey_xor_host(x.tobytes(), b.tobytes(), scan=False)[0], x.size)


def line(kept, width, plain, xored):
    return (f"base-auto: base {'kept' if kept else 'dropped'}, width {width} (predicted bytes at widths 1, 2, 4, 8 without the base: "
            f"{', '.join(map(str, plain))}; against it: {', '.join(map(str, xored))})")


@pytest.mark.parametrize("name", ["int64", "one_percent", "unrelated", "uniform"])
@pytest.mark.parametrize("w", WIDTHS)
def test_a_fixed_width_keeps_the_base_by_the_rule_and_writes_the_file_of_the_explicit_flags(H, tmp_path, files, name, w):
    src, base, x, b = files[name]
    plain, xored = totals(H, x, b)
    j = WIDTHS.index(w)
    kept = xored[j] + H.packet_count(x.size) <= plain[j]
    assert kept == (name in ("int64", "one_percent"))
    extras = ([], ["--checksum"], ["--threads=3"], ["--checksum", "--threads=0", "--stored", "--sparse"]) if w == 2 else ([], ["--checksum", "--threads=3"])
    for extra in extras:
        auto, out = compress(tmp_path, src, "auto", f"--base={base}", "--base-auto", f"--planes={w}", *extra)
        assert line(kept, w, plain, xored) in out, out
        want, _ = compress(tmp_path, src, "want", *([f"--base={base}"] if kept else []), f"--planes={w}", *extra)
        assert auto == want, (name, w, extra)
    if kept:
        back = str(tmp_path / "back.bin")
        run("d", "--host", f"--base={base}", f"--in={tmp_path / 'auto.gip'}", f"--out={back}")
        assert open(back, "rb").read() == x.tobytes()
    else:                                                   # no base: no implied checksum, and decompress takes no --base
        plainest, _ = compress(tmp_path, src, "plainest", f"--base={base}", "--base-auto", f"--planes={w}")
        assert plainest == compress(tmp_path, src, "none", f"--planes={w}")[0]
        assert len(plainest) < len(compress(tmp_path, src, "crc", f"--planes={w}", "--checksum")[0])
        back = str(tmp_path / "back.bin")
        run("d", "--host", f"--in={tmp_path / 'plainest.gip'}", f"--out={back}")
        assert open(back, "rb").read() == x.tobytes()


def test_planes_auto_chooses_width_and_base_together_on_the_bytes_that_are_coded(H, tmp_path, files):
    src, base, x, b = files["int64"]
    plain, xored = totals(H, x, b)
    assert plain == [377469, 374427, 339439, 278520] and xored == [31062, 31063, 31045, 31021]
    assert H.choose_filter(plain, xored, x.size // PACKET) == (1, True)
    auto, out = compress(tmp_path, src, "auto", f"--base={base}", "--base-auto", "--planes=auto")
    assert line(True, 1, plain, xored) in out, out
    assert auto == compress(tmp_path, src, "want", f"--base={base}", "--planes=1")[0] == compress(tmp_path, src, "bare", f"--base={base}")[0]
    # without the flag nothing changes: --base=F --planes=auto keeps surveying the original bytes, which pick 8
    fixed, out = compress(tmp_path, src, "fixed", f"--base={base}", "--planes=auto")
    assert "planes=auto: width 8 " in out and "base-auto" not in out
    assert fixed == compress(tmp_path, src, "eight", f"--base={base}", "--planes=8")[0] and fixed != auto
    back = str(tmp_path / "back.bin")
    run("d", "--host", f"--base={base}", f"--in={tmp_path / 'auto.gip'}", f"--out={back}")
    assert open(back, "rb").read() == x.tobytes()
    for name, width in (("unrelated", 2), ("uniform", 1)):
        src, base, x, b = files[name]
        plain, xored = totals(H, x, b)
        assert H.choose_filter(plain, xored, H.packet_count(x.size)) == (width, False)
        auto, out = compress(tmp_path, src, name, f"--base={base}", "--base-auto", "--planes=auto", "--checksum")
        assert line(False, width, plain, xored) in out, out
        assert auto == compress(tmp_path, src, name + "_want", f"--planes={width}", "--checksum")[0]


def test_the_choice_is_made_from_the_first_16_mib(H, tmp_path):
    """An input that is its base for 16 MiB and unrelated to it behind: the base is kept, whatever follows."""
    rng = np.random.default_rng(3)
    b = rng.integers(0, 256, (16 << 20) + 3 * PACKET + 5, dtype=np.uint8)
    x = b.copy()
    x[16 << 20:] = rng.integers(0, 256, x.size - (16 << 20), dtype=np.uint8)
    src, base = str(tmp_path / "x.bin"), str(tmp_path / "b.bin")
    x.tofile(src), b.tofile(base)
    auto, out = compress(tmp_path, src, "auto", f"--base={base}", "--base-auto", "--threads=0")
    assert "base-auto: base kept, width 1 " in out and f"against it: {2048 * 210}, " in out, out       # 210 bytes for a packet of zeros
    assert auto == compress(tmp_path, src, "want", f"--base={base}", "--threads=0")[0]


def test_the_refused_forms_and_the_usage_text(H, tmp_path, files):
    src, base, x, _b = files["int64"]
    out = str(tmp_path / "bad.gip")
    r = run("c", "--host", "--base-auto", f"--in={src}", f"--out={out}", ok=False)
    assert r.returncode == 2 and "--base-auto goes with c and --base=FILE" in r.stderr
    good, _ = compress(tmp_path, src, "good", f"--base={base}")
    r = run("d", "--host", f"--base={base}", "--base-auto", f"--in={tmp_path / 'good.gip'}", f"--out={out}", ok=False)
    assert r.returncode == 2 and "--base-auto goes with c and --base=FILE" in r.stderr
    r = run("c", "--host", f"--base={base}", "--base-auto", "--delta=auto", f"--in={src}", f"--out={out}", ok=False)
    assert r.returncode == 2 and "--base and --delta" in r.stderr
    assert not os.path.exists(out)
    short = str(tmp_path / "short.base")
    x[:-1].tofile(short)
    r = run("c", "--host", f"--base={short}", "--base-auto", f"--in={src}", f"--out={out}", ok=False)
    assert r.returncode == 1 and "--base takes a file of exactly that length" in r.stderr
    assert "--base-auto" in run("--help").stdout


def test_an_empty_file_drops_its_base(H, tmp_path):
    src, base = str(tmp_path / "empty.bin"), str(tmp_path / "empty.base")
    open(src, "wb").close(), open(base, "wb").close()
    auto, out = compress(tmp_path, src, "auto", f"--base={base}", "--base-auto", "--planes=auto")
    assert line(False, 1, [0] * 4, [0] * 4) in out
    assert auto == compress(tmp_path, src, "none")[0]
