"""The XOR-base kernels in the shipped gfx950 code object (read on the CPU, as tests/test_codeobj_delta.py reads the delta
kernels): present, without scratch, spills, flat_, buffer_ or scratch_ accesses; the full-group kernels move their data -- buffer
and base -- by 16-byte global loads and stores alone and hand the base to its lanes through LDS by 16-byte accesses; the LDS bytes, barriers and vector registers of all four
kernels are the ones DESIGN.md 4.10 gives.  Metadata and mnemonics only."""
import re
import subprocess

import pytest

import test_codeobj_contract as CC
from test_codeobj_planes import code_object, mnemonics      # noqa: F401  (the fixture)

FULL = ("split_xor_kernel", "merge_xor_kernel")
TAILS = ("xor_tail_kernel",)           # both instantiations (split, merge) are listed under the one name
VGPRS = {"split_xor_kernel": 84, "merge_xor_kernel": 96, "split": 32, "merge": 35}      # DESIGN.md 4.10; the tails by instantiation
TAIL_SYMBOLS = {"split": "_ZN5gpuar15xor_tail_kernelILb0EEEvNS_7XorArgsE", "merge": "_ZN5gpuar15xor_tail_kernelILb1EEEvNS_7XorArgsE"}


@pytest.fixture(scope="module")
def tail_records(code_object, tmp_path_factory):
    """the metadata records of the two tail kernels, by their symbols"""
    d = tmp_path_factory.mktemp("codeobj_xor")
    fat, elf = str(d / "fat.bin"), str(d / "gfx950.elf")
    subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fat}", CC.LIB, str(d / "unused.so")])
    targets = subprocess.check_output([CC.TOOLS["clang-offload-bundler"], "--list", "--type=o", f"--input={fat}"], text=True).split()
    gfx = [t for t in targets if t.endswith("gfx950")]
    subprocess.check_call([CC.TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fat}", f"--targets={gfx[0]}", f"--output={elf}"])
    notes = subprocess.check_output([CC.TOOLS["llvm-readelf"], "--notes", elf], text=True)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(CC, "demangled", lambda sym: sym)
        meta = CC.parse_metadata(notes)
    assert all(sym in meta for sym in TAIL_SYMBOLS.values()), sorted(k for k in meta if "xor" in k)
    return {kind: meta[sym] for kind, sym in TAIL_SYMBOLS.items()}


def _find(table, name):
    assert name in table, (name, sorted(table))
    return table[name]


def test_the_xor_kernels_are_in_the_code_object(code_object):
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


def test_full_groups_move_by_16_byte_accesses_in_memory_and_in_lds(code_object):
    meta, dis = code_object
    for name in FULL:
        rec, ops = _find(meta, name), mnemonics(_find(dis, name))
        assert rec["vgpr_count"] == VGPRS[name] and rec.get("agpr_count", 0) == 0, (name, rec["vgpr_count"])
        assert rec["vgpr_count"] <= 128                        # two workgroups of 8 waves per CU by registers: 128 KiB of LDS fit too
        # one group of the base (w = 8: 64 KiB), written and read by quads alone: 2 + 4 + 8 of each (w = 1 goes without)
        assert rec["group_segment_fixed_size"] == 8 * 8192, (name, rec["group_segment_fixed_size"])
        lds = [o for o in ops if o.startswith("ds_")]
        assert sorted(lds) == ["ds_read_b128"] * 14 + ["ds_write_b128"] * 14, (name, lds)
        loads = [o for o in ops if o.startswith("global_load")]
        stores = [o for o in ops if o.startswith("global_store")]
        # widths 8, 4, 2 and 1: 15 quads of the buffer and 15 of the base on the XOR path, 15 on the plain path; 15 out on either
        # (the compiler may share a few between the paths)
        assert loads.count("global_load_dwordx4") >= 30 and stores.count("global_store_dwordx4") >= 15, (name, loads, stores)
        narrow = [o for o in loads + stores if re.search(r"byte|short|d16", o)]
        assert not narrow, (name, narrow)
        assert set(stores) == {"global_store_dwordx4"}, (name, sorted(set(stores)))
        assert set(loads) <= {"global_load_dwordx4", "global_load_dwordx2", "global_load_dword"}, (name, sorted(set(loads)))
        # the byte permutes of planes.h (8 for width 2, 32 for 4, 64 for 8), once on either path
        assert ops.count("v_perm_b32") == 2 * (8 + 32 + 64), (name, ops.count("v_perm_b32"))
        assert "v_readfirstlane_b32" in ops, name              # the width and the choice of path are uniform over the workgroup


def test_barriers_of_the_full_group_kernels(code_object):
    """Per width one barrier on the plain path (planes_group's) and one on the XOR path (loads before stores; the base's way through
    LDS rides on it), and for widths 2, 4 and 8 one behind the stores (the next group's base goes into the same LDS), split and
    merge alike."""
    _meta, dis = code_object
    for name in FULL:
        assert mnemonics(_find(dis, name)).count("s_barrier") == 4 + 4 + 3, name


def test_the_tail_kernels_go_through_lds(code_object, tail_records):
    meta, dis = code_object
    for kind, rec in tail_records.items():
        assert rec["group_segment_fixed_size"] == 8 * 8192                              # the tail, nothing else
        assert rec["vgpr_count"] == VGPRS[kind] and rec.get("agpr_count", 0) == 0, (kind, rec["vgpr_count"])
        assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0
        assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == 512
    for name in TAILS:
        ops = mnemonics(_find(dis, name))
        assert "global_load_dwordx4" in ops
        # per instantiation 4: single buffer (loads before stores), and in the batch loop planes_tail's, xor_tail's and the loop's own
        assert ops.count("s_barrier") == 2 * 4, (name, ops.count("s_barrier"))
        assert not [o for o in ops if re.match(r"global_load_(u|s)?short", o)], name
        assert {o for o in ops if o.startswith("global_store")} <= {"global_store_dword", "global_store_byte"}, name
