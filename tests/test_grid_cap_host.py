"""The capped library of tests/grid_cap_build.py, on the CPU: it cross-compiles and exports what the shipped library exports; its
gfx950 code object is the shipped one's byte for byte (.text, .rodata, the metadata note), which is what makes
tests/test_gpu_grid_cap.py a test of the shipped kernels; and the shapes that module runs, held to the pass arithmetic: which
workgroup or wavefront strides on, where the ragged passes and the defective items fall, what the delta's `turn` sees, and how
much device memory the module asks for."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import grid_cap_build as G

LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = {t: os.path.join(LLVM, t) for t in ("clang-offload-bundler", "llvm-readelf", "llvm-objcopy")}
CAP = G.CAP


@pytest.fixture(scope="module")
def variant():
    if not os.path.exists(G.HIPCC):
        pytest.skip(f"{G.HIPCC} not installed")
    if not os.path.exists(G.SHIPPED):
        pytest.skip("gpuar_amd/lib/libgpuar_hip.so not built")
    return G.build()


def test_the_variant_cross_compiles_and_exports_every_name(variant):
    from gpuar_amd import hip
    lib = C.CDLL(variant)
    missing = [name for name in (*hip.EXPORTS, *hip.GIP_SIGNATURES) if not hasattr(lib, name)]
    assert not missing, missing
    lib.gpuar_hip_abi_version.restype = C.c_int
    assert lib.gpuar_hip_abi_version() == hip.ABI_VERSION
    assert os.path.dirname(variant) == os.path.join(G.HERE, "_build")          # a test artefact, never next to the shipped library


def code_object(lib, d):
    """(.text, .rodata, the metadata note without its file-name line) of the gfx950 code object inside `lib`"""
    os.makedirs(d)
    fat, elf = os.path.join(d, "fat.bin"), os.path.join(d, "gfx950.elf")
    subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "unused.so")])
    targets = subprocess.check_output([TOOLS["clang-offload-bundler"], "--list", "--type=o", f"--input={fat}"], text=True).split()
    gfx = [t for t in targets if t.endswith("gfx950")]
    assert len(gfx) == 1, targets
    subprocess.check_call([TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fat}", f"--targets={gfx[0]}", f"--output={elf}"])
    sections = []
    for name in (".text", ".rodata"):
        path = os.path.join(d, name[1:] + ".bin")
        subprocess.check_call([TOOLS["llvm-objcopy"], "--dump-section", f"{name}={path}", elf, os.path.join(d, "unused.elf")])
        sections.append(open(path, "rb").read())
    notes = subprocess.check_output([TOOLS["llvm-readelf"], "--notes", elf], text=True)
    return sections[0], sections[1], [line for line in notes.splitlines() if not line.startswith("File:")]


def test_the_variants_code_object_is_the_shipped_one(variant, tmp_path):
    missing = [p for p in TOOLS.values() if not os.path.exists(p)] + ([] if shutil.which("objcopy") else ["objcopy"])
    if missing:
        pytest.skip(f"ROCm LLVM tools not installed: {missing}")
    shipped, capped = code_object(G.SHIPPED, str(tmp_path / "shipped")), code_object(variant, str(tmp_path / "capped"))
    assert len(shipped[0]) > 100000 and len(shipped[1]) > 1000 and len(shipped[2]) > 1000       # the sections were really read
    assert capped[0] == shipped[0], "the kernels' .text differs: the cap has reached device code"
    assert capped[1] == shipped[1], ".rodata differs"
    assert capped[2] == shipped[2], "the metadata note differs"


# ---- the shapes of test_gpu_grid_cap.py ----------------------------------------------------------------------------------

def test_the_pass_arithmetic():
    assert [G.grid(n) for n in (1, 2, 3, 4, 100)] == [1, 2, 3, 3, 3]
    assert [G.grid(n, 4) for n in (1, 4, 5, 11, 12, 13, 113)] == [1, 1, 2, 3, 3, 3, 3]
    assert G.owner(7, 100) == (7 % CAP, 7 // CAP) and G.owner(1, 2) == (1, 0)
    assert G.wave_owner(37, 113) == (37 % (4 * CAP), 37 // (4 * CAP)) == (1, 3) and G.wave_owner(7, 8) == (7, 0)
    assert all(CAP % w for w in (2, 4, 8)) and CAP % 2 == 1


def all_stride_on(work, workers):
    """every worker makes at least two passes that do work"""
    return len(work) == workers and all(len(p) >= 2 for p in work)


def test_single_buffers_every_workgroup_strides_on():
    """(a): one buffer of k groups.  The workgroup of a group's leading packet does the group, and w shares no factor with CAP:
    from k = 2 CAP on every workgroup does two groups or more, and below that (k = 2, 3, 4: at, one under and one over the cap)
    some workgroup still makes a later pass over packets it does not lead -- a loop body that runs and leaves by `continue`."""
    most = 0
    for w in G.WIDTHS:
        sizes = G.single_sizes(w)
        assert len(sizes) == len(G.SINGLE_K) * len(G.single_r(w)) and max(sizes) < 1 << 20
        ragged_once = False
        for n in sizes:
            k, n_packets = n // (w * G.PACKET), (n + G.PACKET - 1) // G.PACKET
            work = G.group_passes([n], [w])
            assert sum(len(p) for p in work) == k
            if k >= 2 * CAP:
                assert G.grid(n_packets) == CAP and all_stride_on(work, CAP), (w, n)
            if n_packets > CAP:
                assert max(G.owner(i, n_packets)[1] for i in range(n_packets)) >= 1
            ragged_once |= G.ragged(n_packets, CAP)
            most = max(most, (n_packets + CAP - 1) // CAP)
        assert ragged_once, w
        assert any(all_stride_on(G.group_passes([n], [w]), CAP) for n in sizes)
    assert most == (11 * 8 + 1 + CAP - 1) // CAP == 30


def test_the_batch_has_every_width_tail_and_group_count():
    sizes, widths, groups = G.BATCH_SIZES, G.BATCH_WIDTHS, G.BATCH_GROUPS
    assert len(sizes) == G.N_BUFFERS == 48 and widths[:8] == [1, 2, 4, 8, 1, 2, 4, 8]
    assert set(groups) == set(range(7))
    for w in G.WIDTHS:
        tails = {n % (w * G.PACKET) for n, v in zip(sizes, widths) if v == w}
        assert tails >= {0, 1, w - 1, 15, 16, 17, 8191, w * G.PACKET - 1}, w
    assert sum(n == 0 for n in sizes) >= 2 and sum(0 < n < G.PACKET for n in sizes) >= 4
    assert max(sizes) < 1 << 20
    assert {(w, f) for w, f in zip(widths, G.BATCH_DELTA)} == {(w, f) for w in G.WIDTHS for f in (0, 1)}
    assert {(w, f) for w, f in zip(widths, G.BATCH_BASED)} == {(w, f) for w in G.WIDTHS for f in (False, True)}


def test_the_batch_every_workgroup_strides_on_and_the_tails_make_16_passes():
    """(b): the full-group kernels over the batch's packets, the tail kernels over its buffers"""
    sizes, widths = G.BATCH_SIZES, G.BATCH_WIDTHS
    n_packets = G.first_packets(sizes)[-1]
    work = G.group_passes(sizes, widths)
    assert G.grid(n_packets) == CAP and all_stride_on(work, CAP)
    assert all(len(p) >= 30 for p in work)                                     # dozens of groups per workgroup, not two
    assert G.ragged(n_packets, CAP), n_packets
    has_tail = lambda b: sizes[b] % (widths[b] * G.PACKET) != 0
    tails = G.passes(G.N_BUFFERS, CAP, G.owner, has_tail)
    assert all_stride_on(tails, CAP) and all(len(p) >= 10 for p in tails)
    assert max(G.owner(b, G.N_BUFFERS)[1] for b in range(G.N_BUFFERS)) == 15   # 16 passes through the same LDS
    # one launch per tail kernel that ends on a ragged pass: the batch of the defects' test stops one buffer short
    assert G.ragged(G.N_BUFFERS - 1, CAP) and not G.ragged(G.N_BUFFERS, CAP)


def test_the_delta_workgroups_alternate_their_lds_with_planes_groups_between():
    """each workgroup of the delta's full-group kernels meets three filtered groups or more (turn 0, 1, 0), with a planes-alone
    group -- which does not bump `turn` -- between two of them"""
    work = G.group_passes(G.BATCH_SIZES, G.BATCH_WIDTHS)
    for mine in work:
        kinds = [G.BATCH_DELTA[b] for _turn, b, _g in mine]
        assert sum(kinds) >= 3
        first, last = kinds.index(1), len(kinds) - 1 - kinds[::-1].index(1)
        assert 0 in kinds[first:last], kinds
        # ... and the same for the XOR's LDS: based groups wider than a byte on either side of a planes-alone one
        based = [G.BATCH_BASED[b] and G.BATCH_WIDTHS[b] > 1 for _turn, b, _g in mine]
        assert sum(based) >= 3 and False in based[based.index(True):len(based) - 1 - based[::-1].index(True)]
    # a single buffer is all filtered: k >= 3 CAP gives every workgroup turn 0, 1, 0
    for w in G.WIDTHS:
        assert all(len(p) >= 3 for p in G.group_passes([11 * w * G.PACKET], [w]))


def test_the_defective_buffer_is_met_on_a_later_pass_with_good_buffers_after_it():
    """(c)"""
    bad, sizes, widths = G.BAD_BUFFER, G.BATCH_SIZES, G.BATCH_WIDTHS
    fp = G.first_packets(sizes)
    n_packets = fp[-1]
    assert sizes[bad] // (widths[bad] * G.PACKET) >= 2 and sizes[bad] % (widths[bad] * G.PACKET) != 0 and sizes[bad] % G.PACKET != 0
    assert G.BATCH_DELTA[bad] == 1 and G.BATCH_BASED[bad] and widths[bad] > 1
    for packet in range(fp[bad], fp[bad + 1]):                                  # every packet of it is flagged by its own workgroup
        assert G.owner(packet, n_packets)[1] >= 1
    assert fp[bad + 1] - fp[bad] >= CAP                                         # ... so every workgroup meets it
    usable = [b != bad for b in range(G.N_BUFFERS)]
    after = G.group_passes(sizes, widths, usable)
    last_bad = (fp[bad + 1] - 1) // CAP
    assert all(any(turn > last_bad for turn, _b, _g in mine) for mine in after)
    # the tail kernel: its workgroup has made passes before it and has tails to do after it
    who, turn = G.owner(bad, G.N_BUFFERS - 1)
    assert turn >= 1
    later = [b for b in range(bad + 1, G.N_BUFFERS - 1) if G.owner(b, G.N_BUFFERS - 1)[0] == who and sizes[b] % (widths[b] * G.PACKET)]
    assert len(later) >= 2
    for name, defects in G.DEFECTS.items():
        assert {"width_3", "misaligned_output"} <= set(defects), name
    assert "filter_2" in G.DEFECTS["delta"] and "misaligned_base" in G.DEFECTS["xor"]


def test_the_moves_stride_on_and_their_defective_region_comes_late():
    """(d): n_regions below, at and above the cap, and 100.  From 2 CAP regions on every workgroup makes two passes or more; the
    counts below that are the cap's own edges (1, 2, 3: one pass; 4, 5: some workgroups stride on, some do not)."""
    assert G.MOVE_REGIONS == (1, 2, 3, 4, 5, 7, 100)
    for n in G.MOVE_REGIONS:
        work = G.passes(n, G.grid(n), G.owner)
        if n >= 2 * CAP:
            assert all_stride_on(work, CAP), n
    assert [n for n in G.MOVE_REGIONS if G.ragged(n, CAP)] == [4, 5, 7, 100]
    assert len(G.passes(100, CAP, G.owner)[0]) == 34                           # the most passes of a workgroup
    # move_packets: every residue of the length, full packets, and the defective region
    assert {n % 16 for n in G.MOVE_PACKETS_LENGTHS} == set(range(16)) and G.PACKET in G.MOVE_PACKETS_LENGTHS
    assert all(1 <= n <= G.PACKET for n in G.MOVE_PACKETS_LENGTHS)
    who, turn = G.owner(G.MOVE_BAD_REGION, 100)
    assert turn >= 1 and any(G.owner(r, 100)[0] == who for r in range(G.MOVE_BAD_REGION + 1, 100))
    # move_bytes: 300 regions, back to back, every pair of residues, every residue of the length, both ends of the length's range
    src, dst, lengths = G.move_bytes_regions()
    assert len(lengths) == 300 and all(1 <= n <= G.SLOT for n in lengths) and max(lengths) > G.PACKET and min(lengths) == 1
    assert all(d + n == d1 for d, n, d1 in zip(dst, lengths, dst[1:]))
    assert {(s % 16, d % 16) for s, d in zip(src, dst)} == {(s, d) for s in range(16) for d in range(16)}
    assert {n % 16 for n in lengths} == set(range(16))
    assert max(s + n for s, n in zip(src, lengths)) <= 65536 + G.SLOT + 16     # the pool of tests/test_gpu_gip_read.py


def test_the_sparse_waves_leave_on_different_passes_and_the_defective_region_comes_late():
    """(e): 11, 12, 13 regions are the edges of one pass of the 4 CAP wavefronts (one short, exact, one over: wavefront 0 alone
    strides on); from 24 on every wavefront makes two passes or more, and at 13, 25 and 113 the wavefronts of one workgroup leave
    the loop on different passes."""
    waves = G.SPARSE_WAVES * CAP
    assert G.SPARSE_REGIONS == (11, 12, 13, 24, 25, 113)
    for n in G.SPARSE_REGIONS:
        assert G.grid(n, G.SPARSE_WAVES) == CAP
        work = G.passes(n, waves, G.wave_owner)
        if n >= 2 * waves:
            assert all_stride_on(work, waves), n
        if n in (13, 25, 113):
            assert any(len({len(p) for p in work[g:g + G.SPARSE_WAVES]}) == 2 for g in range(0, waves, G.SPARSE_WAVES))      # inside one workgroup
    assert [n for n in G.SPARSE_REGIONS if G.ragged(n, waves)] == [13, 25, 113]
    assert len(G.passes(113, waves, G.wave_owner)[0]) == 10                     # the most passes of a wavefront
    who, turn = G.wave_owner(G.SPARSE_BAD_REGION, 113)
    assert turn >= 1 and G.wave_owner(G.SPARSE_BAD_REGION + waves, 113) == (who, turn + 1)
    import sparse_ref as S
    for n in G.SPARSE_REGIONS:
        packets = G.sparse_packets(n)
        ks = [S.scan(x) >> 8 for _name, x in packets]
        assert len(packets) == n and 0 in ks and 1 in ks and 4095 in ks         # no exception, one, the longest record
        assert sum(x.size < G.PACKET for _name, x in packets) >= 4
    after = G.sparse_packets(113)[G.SPARSE_BAD_REGION + waves][1]
    assert after.size > S.GOOD_N                                               # the next region of the wavefront covers what the bad one left in LDS


def test_every_gpu_test_stays_under_64_mib_of_device_memory():
    """what each test of the GPU module holds on the device at once (it measures the same, test by test); the largest single
    buffer stays under 1 MiB"""
    arena = G.layout(G.BATCH_SIZES)[1]
    footprint = {
        "single": 7 * (max(max(G.single_sizes(w)) for w in G.WIDTHS) + G.GUARD),       # input, base, four outputs, one clone in flight
        "batch": 6 * arena,                                                         # hosts, bases, split bytes, an output and two for the planes comparison
        "defects": 5 * arena,
        "move_packets": 2 * (G.layout(G.MOVE_PACKETS_LENGTHS, guard=0)[1] + G.PACKET + 256),
        "move_bytes": 65536 + G.SLOT + 16 + sum(G.move_bytes_regions()[2][:100]) + 2 * G.SLOT + 256,
        "sparse": 113 * (2 * G.PACKET + 2 * G.GUARD + 12304),                       # packets, destinations and the longest record each
        "batch.py": 16 << 20,                                                       # nine tensors of 0.2 MiB in all, their slots, streams and files
    }
    assert max(max(G.single_sizes(w)) for w in G.WIDTHS) < 1 << 20 and max(G.BATCH_SIZES) < 1 << 20
    assert arena < 5 << 20
    assert max(footprint.values()) < 64 << 20, footprint
