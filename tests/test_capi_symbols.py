"""The C-ABI library loads on a machine without a GPU and exports every symbol
include/gpuar_hip.h declares (no compute calls here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from gpuar_amd import hip as H
    if not os.path.exists(H.LIB_PATH):
        g.build()
    return H.load()


def declared_symbols(header="gpuar_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    return sorted(set(re.findall(r"\b(\w+)\s*\([^;{]*\)\s*;", text)))


def test_header_symbols_are_exported(lib):
    from gpuar_amd import hip as H
    names = declared_symbols()
    assert set(names) == set(H.EXPORTS), (names, H.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n


def declared_arity(header="gpuar_hip.h"):
    """name -> number of parameters, read off the header's prototypes"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^;{]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_bindings_pin_every_signature(lib):
    """A binding with a different number of arguments than the header's prototype is how a stream handle ends up
    where a status word is expected: the ctypes argtypes are checked against the header, and the
    library's ABI number against the header's."""
    from gpuar_amd import hip as H
    for name, arity in declared_arity().items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, (name, arity, fn.argtypes)
    header = open(os.path.join(ROOT, "include", "gpuar_hip.h")).read()
    abi = int(re.search(r"#define\s+GPUAR_HIP_ABI_VERSION\s+(\d+)", header).group(1))
    assert lib.gpuar_hip_abi_version() == abi == H.ABI_VERSION
    assert f"gpuar-hip 0.{abi} ".encode() in lib.gpuar_hip_version()


def test_library_reads_no_environment(lib):
    """The kernel choice is an argument of gpuar_hip_encode_mode; GPUAR_ENCODE_MODE is honoured by the Python shim only."""
    import subprocess
    from gpuar_amd import hip as H
    undefined = subprocess.run(["nm", "-D", "--undefined-only", H.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined, "libgpuar_hip.so imports getenv"
    assert lib.gpuar_hip_encode_mode(None, 8192, None, None, None, 7) == -2      # unknown mode: GPUAR_ERR_ARGUMENT, before anything else
    assert H._mode_id("latency", "GPUAR_ENCODE_MODE") == 2 and H._mode_id(None, "GPUAR_NO_SUCH_VARIABLE") == 0
    with pytest.raises(H.GpuarError):
        H._mode_id("fast", "GPUAR_ENCODE_MODE")


def test_host_codec_symbols_are_exported_by_both_libraries(lib):
    import ctypes
    from gpuar_amd import host as HC
    names = declared_symbols("gpuar_host.h")
    assert set(names) == set(HC.EXPORTS), (names, HC.EXPORTS)
    small = ctypes.CDLL(HC.LIB_PATH)
    for n in names:
        assert hasattr(small, n) and hasattr(lib, n), n


def test_host_only_calls(lib):
    assert lib.gpuar_hip_packet_count(0) == 0
    assert lib.gpuar_hip_packet_count(1) == 1
    assert lib.gpuar_hip_packet_count(8192) == 1
    assert lib.gpuar_hip_packet_count(8193) == 2
    assert b"gfx950" in lib.gpuar_hip_version()
    assert lib.gpuar_hip_error_string(0) == b"ok"
    assert b"align" in lib.gpuar_hip_error_string(-1)
    assert lib.gpuar_hip_last_error() == 0


def test_missing_library_fails_loudly(monkeypatch):
    from gpuar_amd import hip as H
    monkeypatch.setattr(H, "_lib", None)
    monkeypatch.setattr(H, "LIB_PATH", "/nonexistent/libgpuar_hip.so")
    with pytest.raises(H.GpuarError):
        H.load()


def test_header_layout_helper():
    from gpuar_amd import hip as H
    h = H.gip_header(65539, 66067)
    assert len(h) == 20 and h[0:3] == b"\x00\x01\x00"
    assert int.from_bytes(h[4:8], "little") == 65539
    assert int.from_bytes(h[12:16], "little") == 66087


def test_the_kernel_sources_hold_one_path_and_no_wrong_output_switch():
    """The product library can never be a wrong-output build, because no build can be one: the kernel source has no preprocessor
    conditional at all, the shared headers have only those of the host / device split and the tree-split parameters the tests
    build with, and none of the retired timing and A/B switch families is named anywhere in what builds or loads the library."""
    import ctypes as C
    lib = C.CDLL(os.path.join(ROOT, "gpuar_amd", "lib", "libgpuar_hip.so"))
    lib.gpuar_hip_version.restype = C.c_char_p
    assert lib.gpuar_hip_version() == b"gpuar-hip 0.2 gfx950"

    def text(*parts):
        return open(os.path.join(ROOT, *parts)).read()
    conditional = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)
    sources = {name: text("gpuar_amd", "csrc", name) for name in ("gpuar_kernels.hip", "lane_codec.h", "crc32.h", "planes.h", "Makefile")}
    sources["exp_build.sh"] = text("tools", "exp_build.sh")
    sources["hip.py"] = text("gpuar_amd", "hip.py")
    assert conditional.findall(sources["gpuar_kernels.hip"]) == []
    retired = ("GPUAR_EXP_", "GPUAR_EXPERIMENT_BUILD", "GPUAR_CARRY_NO_RARE", "GPUAR_STORE_POLICY", "GPUAR_CODER_OWED_BITS", "GPUAR_DEC_")
    found = [(name, token) for name, body in sources.items() for token in retired if token in body]
    assert found == []
    # every condition left in the headers names only these: a new switch has to be added HERE, in sight of a reviewer
    allowed = {
        "lane_codec.h": {"GPUAR_LANE_CODEC_H", "__HIP_DEVICE_COMPILE__", "__HIPCC__", "GPUAR_TOP_DEPTHS", "GPUAR_TOP_D1_REGS"},
        "crc32.h": {"GPUAR_CRC32_H", "__HIP_DEVICE_COMPILE__", "__HIPCC__"},
        "planes.h": {"GPUAR_PLANES_H", "__HIPCC__", "GPUAR_PLANE_GRID_CAP"},    # the cap: host launch code only (tests/test_grid_cap_host.py)
    }
    for name, names in allowed.items():
        conditions = conditional.findall(sources[name])
        assert conditions, name
        for condition in conditions:
            code = re.sub(r"//.*|/\*.*", "", condition)
            used = set(re.findall(r"[A-Za-z_]\w*", code)) - {"defined"}
            assert used and used <= names, (name, condition)
