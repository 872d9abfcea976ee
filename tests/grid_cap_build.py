"""Builds tests/_build/libgpuar_hip_gridcap3.so on demand: libgpuar_hip.so with -DGPUAR_PLANE_GRID_CAP=3u, the one host-side
constant behind the grids of the filter, move and sparse pack / unpack kernels (gpuar_kernels.hip: launch_filter, region_call).
Not a test module: test_grid_cap_host.py and test_gpu_grid_cap.py import it.

The cap is read by launch code only, so the variant holds the shipped kernels instruction for instruction (test_grid_cap_host.py
compares the code objects byte for byte) and runs them on grids of at most 3 workgroups: every workgroup then strides on over
kilobyte-sized inputs, which with the shipped cap of 2^22 takes 32 GiB.  The precedent is small_slot_lib in test_gpu_parity.py.

Three parts: the build and the swap (capped()); the pass arithmetic -- which workgroup or wavefront does which item on which
pass, in plain Python --; and the shapes of test_gpu_grid_cap.py, which stand here so that test_grid_cap_host.py can hold them to
that arithmetic without a device."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_build")
CSRC = os.path.join(ROOT, "gpuar_amd", "csrc")
SHIPPED = os.path.join(ROOT, "gpuar_amd", "lib", "libgpuar_hip.so")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")

# Why 3: odd, so it shares no factor with the group widths 1, 2, 4, 8 or with the 4 wavefronts of a sparse workgroup (with 2 or 4
# one workgroup would get every group of a w = 8 buffer); below every count the tests use; and the last pass is ragged for most.
CAP = 3
LIB = os.path.join(OUT, f"libgpuar_hip_gridcap{CAP}.so")
OBJECTS = [os.path.join(ROOT, "build", "host_codec.o"), os.path.join(ROOT, "build", "gip_read.o")]

PACKET, SLOT = 8192, 8704
SPARSE_WAVES = 4                         # kSparseWaves: wavefronts per workgroup of sparse_pack / sparse_unpack, a region each


# ---- the build and the swap -------------------------------------------------------------------------------------------

def _sources():
    headers = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")]
    include = os.path.join(ROOT, "include")
    return [os.path.join(CSRC, "gpuar_kernels.hip")] + headers + [os.path.join(include, f) for f in sorted(os.listdir(include)) if f.endswith(".h")]


def hipflags():
    """HIPFLAGS as gpuar_amd/csrc/Makefile has them (asked of make itself: the variant cannot drift from the shipped build)"""
    out = subprocess.check_output(["make", "-C", CSRC, "-s", "--no-print-directory", "--eval=print-hipflags: ; @echo $(HIPFLAGS)", "print-hipflags"],
                                  text=True)
    return out.split()


def build():
    """hipcc gpuar_kernels.hip -> tests/_build/libgpuar_hip_gridcap3.so, again whenever a source or a header is newer than it"""
    os.makedirs(OUT, exist_ok=True)
    if os.path.exists(LIB) and all(os.path.getmtime(s) <= os.path.getmtime(LIB) for s in _sources()):
        return LIB
    missing = [o for o in OBJECTS if not os.path.exists(o)]
    if missing:
        subprocess.check_call(["make", "-C", CSRC, *missing])
    tmp = LIB + f".{os.getpid()}.tmp"
    subprocess.check_call([HIPCC, *hipflags(), f"-DGPUAR_PLANE_GRID_CAP={CAP}u", "-shared", "-o", tmp, *OBJECTS, "gpuar_kernels.hip"], cwd=CSRC)
    os.replace(tmp, LIB)
    return LIB


_lib = None


def load():
    """The capped library with the prototypes gpuar_amd/hip.py gives the shipped one."""
    global _lib
    if _lib is None:
        from gpuar_amd import hip
        lib = C.CDLL(build())
        for name, (restype, argtypes) in (*hip.SIGNATURES.items(), *hip.GIP_SIGNATURES.items()):
            getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
        assert lib.gpuar_hip_abi_version() == hip.ABI_VERSION, (lib.gpuar_hip_abi_version(), hip.ABI_VERSION)
        _lib = lib
    return _lib


@contextlib.contextmanager
def capped():
    """Inside: every wrapper of gpuar_amd/hip.py, and so all of gpuar_amd/batch.py, calls the capped library; behind it, also
    when the body raises, the shipped one again.  Each library has a fallback status word of its own (hip.status() reads the
    one of the library in place), so every call under test passes its own d_status or reads status() inside the block."""
    from gpuar_amd import hip
    shipped = hip.load()
    hip._lib = load()
    try:
        yield hip
    finally:
        hip._lib = shipped


# ---- the pass arithmetic ----------------------------------------------------------------------------------------------

def grid(n, per=1):
    """capped_blocks(n, per, CAP): one workgroup for every `per` items, CAP at most"""
    return min((n + per - 1) // per, CAP)


def owner(i, n):
    """(workgroup, pass) of item i of n in a `for (x = blockIdx.x; x < n; x += gridDim.x)` loop: with n > CAP, i % CAP and i // CAP"""
    g = grid(n)
    return i % g, i // g


def wave_owner(r, n):
    """(wavefront of the grid, pass) of region r of n in a wave_item() / wave_items() loop: with n > 4 CAP, r % (4 CAP), r // (4 CAP)"""
    waves = SPARSE_WAVES * grid(n, SPARSE_WAVES)
    return r % waves, r // waves


def passes(n, workers, own, does_work=lambda i: True):
    """[[pass, ...] per worker]: the passes on which each of the `workers` workgroups (or wavefronts) has an item that does work"""
    out = [[] for _ in range(workers)]
    for i in range(n):
        if does_work(i):
            who, turn = own(i, n)
            out[who].append(turn)
    return out


def ragged(n, workers):
    """the last pass is not made by every worker"""
    return n > workers and n % workers != 0


def first_packets(sizes):
    fp = [0]
    for n in sizes:
        fp.append(fp[-1] + (n + PACKET - 1) // PACKET)
    return fp


def full_groups(sizes, widths, usable=None):
    """[(batch packet, buffer, group of the buffer)]: the leading packets of the full groups -- the items of a full-group filter
    kernel that do work, each done by the workgroup that owns that packet.  One buffer: sizes = [n], widths = [w]."""
    out, fp = [], first_packets(sizes)
    for b, (n, w) in enumerate(zip(sizes, widths)):
        if usable is None or usable[b]:
            out += [(fp[b] + g * w, b, g) for g in range(n // (w * PACKET))]
    return out


def group_passes(sizes, widths, usable=None):
    """[[(pass, buffer, group), ...] per workgroup] of a full-group filter kernel, in the order the workgroup meets them"""
    n_packets = first_packets(sizes)[-1]
    out = [[] for _ in range(grid(n_packets))]
    for packet, b, g in full_groups(sizes, widths, usable):
        who, turn = owner(packet, n_packets)
        out[who].append((turn, b, g))
    return out


# ---- the shapes of test_gpu_grid_cap.py -------------------------------------------------------------------------------

WIDTHS = (1, 2, 4, 8)
FILTERS = ("planes", "delta", "xor")
GUARD = 256

# (a) one buffer: n = k w 8192 + r
SINGLE_K = (2, 3, 4, 7, 11)


def single_r(w):
    return sorted({0, 1, w - 1, 4097})


def single_sizes(w):
    return [k * w * PACKET + r for k in SINGLE_K for r in single_r(w)]


# (b) a batch of 48 buffers: widths cycle through 1, 2, 4, 8; zero to six full groups; every tail at every width
N_BUFFERS = 48
BATCH_WIDTHS = [WIDTHS[b % 4] for b in range(N_BUFFERS)]
BATCH_GROUPS = [(3 * b + b // 4) % 7 for b in range(N_BUFFERS)]
BATCH_GROUPS[20] = BATCH_GROUPS[33] = BATCH_GROUPS[43] = 0


def batch_tail(b):
    w = BATCH_WIDTHS[b]
    return (0, 1, w - 1, 15, 16, 17, 8191, w * PACKET - 1)[(b // 4) % 8]


BATCH_SIZES = [BATCH_GROUPS[b] * BATCH_WIDTHS[b] * PACKET + batch_tail(b) for b in range(N_BUFFERS)]
# the optional part, mixed: the delta's filter word and whether the XOR has a base
BATCH_DELTA = [0 if b % 5 in (1, 3) else 1 for b in range(N_BUFFERS)]
BATCH_BASED = [b % 3 != 2 for b in range(N_BUFFERS)]
# (c) the buffer with the unusable descriptor: full groups and a tail, not among the first CAP buffers or packets
BAD_BUFFER = 25
DEFECTS = {"planes": ("width_3", "misaligned_output"), "delta": ("width_3", "misaligned_output", "filter_2"),
           "xor": ("width_3", "misaligned_output", "misaligned_base")}


def layout(sizes, guard=GUARD):
    """(offsets, total): the buffers one behind the other in one arena, each 16-byte aligned with at least `guard` bytes behind it"""
    at, offs = 0, []
    for n in sizes:
        offs.append(at)
        at += (n + guard + 15) // 16 * 16
    return offs, at


# (d) move_packets and move_bytes
MOVE_REGIONS = (1, 2, 3, 4, 5, 7, 100)
RAGGED_LENGTHS = [base + r for base in (0, 16, PACKET - 16) for r in range(1, 16)]      # tests/test_gpu_ragged_quads.py: LENGTHS
MOVE_PACKETS_LENGTHS = [(RAGGED_LENGTHS + [PACKET, 16, PACKET - 16, 4096])[(5 * r) % 49] for r in range(100)]
MOVE_BAD_REGION = 49                     # workgroup 1's, pass 16; 52, 55 ... come after it
MOVE_BYTES_ROUNDS = 3                    # launches of 100 regions: 300 regions hold every (src & 15, dst & 15) pair
MOVE_BYTES_BASES = (0, 16, 32, 240, 4096, 8176, 8688)


def move_bytes_regions(start=5):
    """(src offsets into the pool of test_gpu_gip_read.py, dst offsets, lengths) of 300 regions whose destinations stand back to
    back at byte grain from byte GUARD + start.  Region r is one byte longer, mod 16, than the region before, so the lengths take
    every residue and dst & 15 walks the triangular numbers: every residue, twice in 32 regions.  The j-th region at one dst & 15
    reads from src & 15 = j mod 16."""
    src, dst, lengths, seen, at = [], [], [], {}, 64 + start
    for r in range(100 * MOVE_BYTES_ROUNDS):
        res = (r + 1) % 16
        base = MOVE_BYTES_BASES[r % len(MOVE_BYTES_BASES)]
        n = base + res if base + res >= 1 else 16
        if n > SLOT:
            n -= 16
        j = seen.get(at % 16, 0)
        seen[at % 16] = j + 1
        src.append(((r * 37) % 3500) * 16 + j % 16)
        dst.append(at)
        lengths.append(n)
        at += n
    return src, dst, lengths


# (e) sparse_pack and sparse_unpack
SPARSE_REGIONS = (11, 12, 13, 24, 25, 113)
SPARSE_BAD_REGION = 37                   # of 113: wavefront 1's, pass 3; 49, 61 ... come after it
SPARSE_FIRST = ("k0_n8192_f00", "half_plus_1_n3_", "half_plus_1_n8192_", "k0_n1_", "ends_n4097_", "half_plus_1_n8191_", "ends_n17_", "k0_n129_")


def sparse_packets(n_regions):
    """[(name, packet)] of n_regions sparse packets out of sparse_ref.cases(): first no exception, one exception, the longest
    record (k = 4095 of 8192 bytes) and short last packets, then every other case that has a record, round and round"""
    import sparse_ref as S
    keep = [(name, x) for name, x in S.cases() if S.scan(x) != S.NONE]
    first = [next((name, x) for name, x in keep if name.startswith(p)) for p in SPARSE_FIRST]
    rest = [c for c in keep if all(c[0] != f[0] for f in first)]
    order = first + rest
    return [order[r % len(order)] for r in range(n_regions)]


def seeded(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
