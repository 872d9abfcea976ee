"""The delta-filter kernels in the shipped gfx950 code object (read on the CPU, as tests/test_codeobj_planes.py reads the plane
kernels): present, without scratch, spills, flat_, buffer_ or scratch_ accesses; the full-group kernels move their data by
16-byte global loads and stores alone; the LDS bytes and barriers are the ones DESIGN.md 4.9 gives."""
import re
import subprocess

import pytest

import test_codeobj_contract as CC
from test_codeobj_planes import code_object, mnemonics      # noqa: F401  (the fixture)

FULL = ("split_delta_kernel", "merge_delta_kernel")
TAILS = ("delta_tail_kernel",)         # both instantiations (split, merge) are listed under the one name
TAIL_SYMBOLS = {"split": "_ZN5gpuar17delta_tail_kernelILb0EEEvNS_9DeltaArgsE", "merge": "_ZN5gpuar17delta_tail_kernelILb1EEEvNS_9DeltaArgsE"}


@pytest.fixture(scope="module")
def tail_records(code_object, tmp_path_factory):
    """the metadata records of the two tail kernels, by their symbols"""
    d = tmp_path_factory.mktemp("codeobj_delta")
    fat, elf = str(d / "fat.bin"), str(d / "gfx950.elf")
    subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fat}", CC.LIB, str(d / "unused.so")])
    targets = subprocess.check_output([CC.TOOLS["clang-offload-bundler"], "--list", "--type=o", f"--input={fat}"], text=True).split()
    gfx = [t for t in targets if t.endswith("gfx950")]
    subprocess.check_call([CC.TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fat}", f"--targets={gfx[0]}", f"--output={elf}"])
    notes = subprocess.check_output([CC.TOOLS["llvm-readelf"], "--notes", elf], text=True)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(CC, "demangled", lambda sym: sym)
        meta = CC.parse_metadata(notes)
    assert all(sym in meta for sym in TAIL_SYMBOLS.values()), sorted(k for k in meta if "delta" in k)
    return {kind: meta[sym] for kind, sym in TAIL_SYMBOLS.items()}


def _find(table, name):
    assert name in table, (name, sorted(table))
    return table[name]


def test_the_delta_kernels_are_in_the_code_object(code_object):
    meta, dis = code_object
    for name in FULL + TAILS:
        assert len(_find(dis, name)) > 20 and _find(meta, name), name


def test_no_scratch_no_spills_no_flat_or_buffer_accesses(code_object):
    meta, dis = code_object
    for name in FULL + TAILS:
        rec = _find(meta, name)
        assert rec["private_segment_fixed_size"] == 0, (name, rec["private_segment_fixed_size"])
        assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, name
        assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == 512, name
        ops = mnemonics(_find(dis, name))
        bad = sorted({o for o in ops if o.startswith(("flat_", "buffer_", "scratch_"))})
        assert not bad, (name, bad)


def test_full_groups_move_by_16_byte_global_accesses(code_object):
    meta, dis = code_object
    for name in FULL:
        rec, ops = _find(meta, name), mnemonics(_find(dis, name))
        assert rec["vgpr_count"] + rec.get("agpr_count", 0) <= 128, (name, rec["vgpr_count"])      # four workgroups of 8 waves per CU
        loads = [o for o in ops if o.startswith("global_load")]
        stores = [o for o in ops if o.startswith("global_store")]
        # the filtered and the plain path, widths 8, 4, 2 and 1 each: at least 8 + 4 + 2 + 1 quads in and as many out
        assert loads.count("global_load_dwordx4") >= 15 and stores.count("global_store_dwordx4") >= 15, (name, loads, stores)
        narrow = [o for o in loads + stores if re.search(r"byte|short|d16", o)]
        assert not narrow, (name, narrow)
        assert set(stores) == {"global_store_dwordx4"}, (name, sorted(set(stores)))
        assert set(loads) <= {"global_load_dwordx4", "global_load_dwordx2", "global_load_dword"}, (name, sorted(set(loads)))
        # two parities of 8 wave entries of 8 bytes: the predictors across wavefronts (split), the wave totals (merge)
        assert rec["group_segment_fixed_size"] == 128, (name, rec["group_segment_fixed_size"])


def test_barriers_of_the_full_group_kernels(code_object):
    """Per width one barrier on the plain path (planes_group's) and on the filtered path one for split (loads before stores; the
    predictors ride on it) and two for merge (loads before stores; the wave totals)."""
    _meta, dis = code_object
    assert mnemonics(_find(dis, FULL[0])).count("s_barrier") == 4 + 4
    assert mnemonics(_find(dis, FULL[1])).count("s_barrier") == 4 + 2 * 4


def test_the_tail_kernels_load_by_quads_through_lds(code_object, tail_records):
    meta, dis = code_object
    assert tail_records["split"]["group_segment_fixed_size"] == 8 * 8192                # the tail
    assert tail_records["merge"]["group_segment_fixed_size"] == 8 * 8192 + 64           # the tail and 8 wave totals
    for rec in tail_records.values():
        assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0
        assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == 512
    for name in TAILS:
        ops = mnemonics(_find(dis, name))
        assert "global_load_dwordx4" in ops and "s_barrier" in ops
        assert not [o for o in ops if re.match(r"global_load_(u|s)?(byte|short)", o)], "the tail reads by quads, never beyond the last one"
        assert {o for o in ops if o.startswith("global_store")} <= {"global_store_dword", "global_store_byte"}, name
