"""host/pipeline_parts.hpp on the CPU: the concurrency core of the GPU file pipeline -- the writer thread in both of its modes, with a
failing pwrite and aborted with pieces queued, the chunks' turn at the output offset, the chunk map -- driven from several threads
by tests/pipeline_parts_test.cpp, once under the thread sanitizer and once under the address and undefined-behaviour sanitizers.
The header includes nothing of HIP: plain g++, no GPU, nothing preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizers", ["thread", "address,undefined"])
def test_the_pipeline_parts_under_sanitizers(tmp_path, sanitizers):
    exe = str(tmp_path / "pipeline_parts_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-fsanitize={sanitizers}", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gpuar_amd", "csrc", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "pipeline_parts_test.cpp"), "-lpthread"])
    r = subprocess.run([exe, str(tmp_path / "written.dat")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "pipeline parts ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)


def test_the_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "gpuar_amd", "csrc", "host", "pipeline_parts.hpp")).read()
    assert "#include <hip" not in text and "gpuar_hip" not in text
