"""The mixed-filter kernels in the shipped gfx950 code object (read on the CPU, as tests/test_codeobj_xor.py reads the XOR
kernels): present, without scratch, spills, flat_, buffer_ or scratch_ accesses; the full-group kernels move their data -- buffer
and base -- by 16-byte global loads and stores alone (the one byte they load is the supergroup's mode); the LDS bytes and vector
registers of all five kernels are the ones DESIGN.md 4.16 gives.  Metadata and the mnemonics of memory accesses only."""
import re
import subprocess

import pytest

import test_codeobj_contract as CC
from test_codeobj_planes import code_object, mnemonics      # noqa: F401  (the fixture)

FULL = ("split_mixed_kernel", "merge_mixed_kernel")
TAILS = ("mixed_tail_kernel",)         # both instantiations (split, merge) are listed under the one name
CHOOSE = ("choose_modes_kernel",)
GROUP = 8 * 8192                       # one group of the base at width 8, or a whole tail
SLOTS = 2 * 8 * 8                      # the delta's predictor slots: two turns of eight 64-bit entries
# DESIGN.md 4.16; the tails by instantiation
VGPRS = {"split_mixed_kernel": 88, "merge_mixed_kernel": 97, "choose_modes_kernel": 40, "split": 76, "merge": 98}
LDS = {"split_mixed_kernel": GROUP + SLOTS, "merge_mixed_kernel": GROUP + SLOTS, "choose_modes_kernel": 0, "split": GROUP, "merge": GROUP + 8 * 8}
TAIL_SYMBOLS = {"split": "_ZN5gpuar17mixed_tail_kernelILb0EEEvNS_9MixedArgsE", "merge": "_ZN5gpuar17mixed_tail_kernelILb1EEEvNS_9MixedArgsE"}


@pytest.fixture(scope="module")
def tail_records(code_object, tmp_path_factory):
    """the metadata records of the two tail kernels, by their symbols"""
    d = tmp_path_factory.mktemp("codeobj_mixed")
    fat, elf = str(d / "fat.bin"), str(d / "gfx950.elf")
    subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fat}", CC.LIB, str(d / "unused.so")])
    targets = subprocess.check_output([CC.TOOLS["clang-offload-bundler"], "--list", "--type=o", f"--input={fat}"], text=True).split()
    gfx = [t for t in targets if t.endswith("gfx950")]
    subprocess.check_call([CC.TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fat}", f"--targets={gfx[0]}", f"--output={elf}"])
    notes = subprocess.check_output([CC.TOOLS["llvm-readelf"], "--notes", elf], text=True)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(CC, "demangled", lambda sym: sym)
        meta = CC.parse_metadata(notes)
    assert all(sym in meta for sym in TAIL_SYMBOLS.values()), sorted(k for k in meta if "mixed" in k)
    return {kind: meta[sym] for kind, sym in TAIL_SYMBOLS.items()}


def _find(table, name):
    assert name in table, (name, sorted(table))
    return table[name]


def test_the_three_kernel_families_are_in_the_code_object(code_object):
    meta, dis = code_object
    for name in FULL + TAILS + CHOOSE:
        assert len(_find(dis, name)) > 20 and _find(meta, name), name


def test_no_scratch_no_spills_no_flat_or_buffer_accesses(code_object):
    meta, dis = code_object
    for name in FULL + TAILS + CHOOSE:
        rec = _find(meta, name)
        assert rec["private_segment_fixed_size"] == 0, (name, rec["private_segment_fixed_size"])
        assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, name
        assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == (256 if name in CHOOSE else 512), name
        ops = mnemonics(_find(dis, name))
        bad = sorted({o for o in ops if o.startswith(("flat_", "buffer_", "scratch_"))})
        assert not bad, (name, bad)


def test_full_groups_move_by_16_byte_accesses_in_memory_and_in_lds(code_object):
    meta, dis = code_object
    for name in FULL:
        rec, ops = _find(meta, name), mnemonics(_find(dis, name))
        assert rec["vgpr_count"] == VGPRS[name] and rec.get("agpr_count", 0) == 0, (name, rec["vgpr_count"])
        assert rec["vgpr_count"] <= 128                        # two workgroups of 8 waves per CU by registers: their LDS fits too
        assert rec["group_segment_fixed_size"] == LDS[name] and 2 * LDS[name] <= CC.LDS_PER_CU, (name, rec["group_segment_fixed_size"])
        # the base's way through LDS is xor_group's: 2 + 4 + 8 quads written and read (w = 1 goes without); everything narrower is
        # the delta's predictors and wave totals
        lds = [o for o in ops if o.startswith("ds_") and not o.startswith("ds_bpermute")]
        assert lds.count("ds_write_b128") == 14 and lds.count("ds_read_b128") == 14, (name, sorted(lds))
        assert {o for o in lds if "b128" not in o} <= {"ds_write_b32", "ds_write_b64", "ds_read_b32", "ds_read_b64", "ds_read2_b32", "ds_read2_b64"}, (name, sorted(set(lds)))
        loads = [o for o in ops if o.startswith("global_load")]
        stores = [o for o in ops if o.startswith("global_store")]
        # widths 8, 4, 2 and 1 on three paths: 15 quads of the buffer on each and 15 of the base on the XOR path; 15 out on each
        # (the compiler may share a few between the paths)
        assert loads.count("global_load_dwordx4") >= 45 and stores.count("global_store_dwordx4") >= 30, (name, loads, stores)
        assert set(stores) == {"global_store_dwordx4"}, (name, sorted(set(stores)))
        assert set(loads) <= {"global_load_dwordx4", "global_load_dwordx2", "global_load_dword", "global_load_ubyte"}, (name, sorted(set(loads)))
        assert loads.count("global_load_ubyte") == 1, name     # the supergroup's mode: the only access below a dword
        narrow = [o for o in loads + stores if re.search(r"short|d16|sbyte", o)]
        assert not narrow, (name, narrow)
        assert "v_readfirstlane_b32" in ops, name              # the mode is uniform over the workgroup


def test_the_tail_and_the_choice(code_object, tail_records):
    meta, dis = code_object
    for kind, rec in tail_records.items():
        assert rec["group_segment_fixed_size"] == LDS[kind], (kind, rec["group_segment_fixed_size"])      # the tail; merge: and the delta's wave totals
        assert rec["vgpr_count"] == VGPRS[kind] and rec["vgpr_count"] <= 128 and rec.get("agpr_count", 0) == 0, (kind, rec["vgpr_count"])
        assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0
        assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == 512
    for name in TAILS:
        ops = mnemonics(_find(dis, name))
        assert "global_load_dwordx4" in ops
        assert not [o for o in ops if re.match(r"global_load_(u|s)?short", o)], name
        assert {o for o in ops if o.startswith("global_store")} <= {"global_store_dword", "global_store_byte"}, name
    for name in CHOOSE:
        rec, ops = _find(meta, name), mnemonics(_find(dis, name))
        assert rec["vgpr_count"] == VGPRS[name] and rec["group_segment_fixed_size"] == LDS[name], (name, rec["vgpr_count"])
        assert {o for o in ops if o.startswith("global_store")} == {"global_store_byte", "global_store_dword"}, name      # the mode and its total
        assert "s_barrier" not in ops and not [o for o in ops if o.startswith("ds_")], name
