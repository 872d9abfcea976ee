"""`gpuar c --base=FILE --base-auto` on the MI355X writes the file `gpuar-host` writes: the choice is made on the host from a
constant prefix before the pipeline starts, so it does not depend on the chunking."""
import os
import subprocess

import pytest

import xor_survey_ref as XS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")
HOST_CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")


@pytest.mark.parametrize("name,planes,said", [("int64", "auto", "base kept, width 1 "), ("int64", "8", "base kept, width 8 "),
                                              ("unrelated", "auto", "base dropped, width 2 ")])
def test_the_cli_on_the_gpu_writes_the_hosts_file(tmp_path, name, planes, said):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    x, b = XS.int64_pair() if name == "int64" else XS.table_pairs()[name]
    src, base, host_gip = tmp_path / "in.dat", tmp_path / "base.dat", tmp_path / "host.gip"
    x.tofile(src), b.tofile(base)
    flags = [f"--base={base}", "--base-auto", f"--planes={planes}", f"--in={src}"]
    r = subprocess.run([HOST_CLI, "c", "--host", *flags, f"--out={host_gip}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "base-auto: " + said in r.stdout, (r.stdout, r.stderr)
    line = next(l for l in r.stdout.splitlines() if l.startswith("base-auto: "))
    for batch in (64, 128):
        gip = tmp_path / f"batch{batch}.gip"
        r = subprocess.run([CLI, "c", f"--batch={batch}", *flags, f"--out={gip}"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Attention" not in r.stdout and line in r.stdout.splitlines()
        assert gip.read_bytes() == host_gip.read_bytes(), (name, planes, batch)
    back = tmp_path / "back.dat"
    r = subprocess.run([CLI, "d", *([f"--base={base}"] if "kept" in said else []), f"--in={tmp_path / 'batch64.gip'}", f"--out={back}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == x.tobytes()
