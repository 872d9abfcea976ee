"""Builds the compiled test clients (tests/class_client.cpp, tests/executor_client.cpp) into tests/_build/ on demand and
runs them as children, one at a time.  Not a test module: test_class_api.py and test_executor_caller.py import it.

The compiler flags are the ones gpuar_amd/csrc/Makefile gives $(BIN)/gpuar and $(BIN)/gpuar-host."""
import os
import signal
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_build")
HOST = os.path.join(ROOT, "gpuar_amd", "csrc", "host")
LIB = os.path.join(ROOT, "gpuar_amd", "lib")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")
CLI_HOST = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")

CXXFLAGS = ["-O2", "-std=c++17", f"-I{ROOT}/include", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
            "-fconstexpr-ops-limit=100000000", "-fconstexpr-loop-limit=1000000"]
GPUFLAGS = ["-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include"]
GPULIBS = [f"-L{LIB}", "-lgpuar_hip", f"-L{ROCM}/lib", "-lamdhip64", "-lpthread", f"-Wl,-rpath,{LIB}", f"-Wl,-rpath,{ROCM}/lib"]


def _headers():
    csrc = os.path.dirname(HOST)
    return [os.path.join(HOST, f) for f in sorted(os.listdir(HOST)) if f.endswith(".hpp")] + \
           [os.path.join(csrc, "lane_codec.h"), os.path.join(csrc, "crc32.h"),
            os.path.join(ROOT, "include", "gpuar_hip.h"), os.path.join(ROOT, "include", "gpuar_host.h")]


def _make(name, sources, flags, libs, depends=()):
    """g++ sources -> tests/_build/name, again whenever a source, a header or `depends` is newer than the binary"""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    inputs = list(sources) + _headers() + list(depends)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in inputs):
        tmp = exe + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", *CXXFLAGS, *flags, f"-I{HOST}", "-o", tmp, *sources, *libs])
        os.replace(tmp, exe)
    return exe


def ensure_products():
    """the project's own libraries and CLIs (a clean checkout has none)"""
    if not all(os.path.exists(p) for p in (CLI, CLI_HOST, os.path.join(LIB, "libgpuar_hip.so"))):
        import __graft_entry__ as g
        g.build()


def class_client_host():
    """class_client with the CPU class only: needs neither libgpuar_hip.so nor a HIP runtime"""
    srcs = [os.path.join(HERE, "class_client.cpp"), os.path.join(HOST, "compressor.cpp"), os.path.join(HOST, "cpu_compressor.cpp")]
    return _make("class_client_host", srcs, ["-DGPUAR_HOST_ONLY"], ["-lpthread"])


def class_client_gpu():
    ensure_products()
    srcs = [os.path.join(HERE, "class_client.cpp")] + [os.path.join(HOST, f) for f in ("compressor.cpp", "cpu_compressor.cpp", "gpu_compressor.cpp")]
    return _make("class_client_gpu", srcs, GPUFLAGS, GPULIBS, [os.path.join(LIB, "libgpuar_hip.so")])


def executor_client():
    """plain g++ over <hip/hip_runtime_api.h> and gpuar_hip.h: no kernel of its own, no hipcc"""
    ensure_products()
    return _make("executor_client", [os.path.join(HERE, "executor_client.cpp")], GPUFLAGS, GPULIBS, [os.path.join(LIB, "libgpuar_hip.so")])


class Children:
    """Runs children one at a time, each under a time limit that kills it.  A child that ends by a signal, by exit code
    134 or 139, or by the time limit fails its test with what it printed -- and every later run() of the same Children
    (one per test module) fails at once WITHOUT starting anything: nothing goes on using a device after a fault, and
    nothing is retried."""

    def __init__(self):
        self.broken = None

    def run(self, argv, timeout, env=None, stdin_text=None):
        assert self.broken is None, f"not started: an earlier child of this module ended badly ({self.broken})"
        try:
            r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, env=env, input=stdin_text,
                               stdin=None if stdin_text is not None else subprocess.DEVNULL)
        except subprocess.TimeoutExpired as e:
            self.broken = f"{os.path.basename(argv[0])}: killed after {timeout} s"
            raise AssertionError(f"{self.broken}\nstdout: {_tail(e.stdout)}\nstderr: {_tail(e.stderr)}")
        if r.returncode < 0 or r.returncode in (134, 139):
            what = signal.Signals(-r.returncode).name if r.returncode < 0 else f"exit code {r.returncode}"
            self.broken = f"{os.path.basename(argv[0])}: {what}"
            raise AssertionError(f"{self.broken}\nstdout: {_tail(r.stdout)}\nstderr: {_tail(r.stderr)}")
        return r


def _tail(text, n=3000):
    if text is None:
        return ""
    if isinstance(text, bytes):
        text = text.decode(errors="replace")
    return text[-n:]


def parse_results(text):
    """the clients' result lines -> [{'status': 'ok'|'error', 'command': ..., 'what': ..., key: number ...}]"""
    out = []
    for line in text.splitlines():
        if line.startswith("ok "):
            words = line.split()
            rec = {"status": "ok", "command": words[1]}
            for w in words[2:]:
                k, v = w.split("=", 1)
                rec[k] = float(v) if any(c in v for c in ".einf") else int(v)
            out.append(rec)
        elif line.startswith("error "):
            command, _, what = line[6:].partition(": ")
            out.append({"status": "error", "command": command, "what": what})
    return out
