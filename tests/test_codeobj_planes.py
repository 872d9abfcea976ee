"""The byte-plane kernels in the shipped gfx950 code object (read on the CPU, as tests/test_codeobj_contract.py reads the others):
present, without scratch, spills, flat_ or buffer_ accesses; the full-group kernels move their data by 16-byte global loads
and stores alone and regroup it in registers (v_perm_b32, no LDS); the tail kernel is the only one with narrow stores."""
import os
import re
import subprocess

import pytest

import test_codeobj_contract as CC

FULL = ("split_planes_kernel", "merge_planes_kernel")
TAIL = "planes_tail_kernel"


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    """(metadata by kernel, disassembly by kernel) of the library's gfx950 code object; the library is built when it is missing."""
    if not os.path.exists(CC.LIB):
        import __graft_entry__ as g
        g.build()
    missing = [p for p in CC.TOOLS.values() if not os.path.exists(p)]
    assert not missing, f"the ROCm LLVM tools that built the library are not where they were: {missing}"
    d = tmp_path_factory.mktemp("codeobj_planes")
    fat, elf = str(d / "fat.bin"), str(d / "gfx950.elf")
    subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fat}", CC.LIB, str(d / "unused.so")])
    targets = subprocess.check_output([CC.TOOLS["clang-offload-bundler"], "--list", "--type=o", f"--input={fat}"], text=True).split()
    gfx = [t for t in targets if t.endswith("gfx950")]
    assert len(gfx) == 1, targets
    subprocess.check_call([CC.TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fat}", f"--targets={gfx[0]}", f"--output={elf}"])
    notes = subprocess.check_output([CC.TOOLS["llvm-readelf"], "--notes", elf], text=True)
    dis = subprocess.check_output([CC.TOOLS["llvm-objdump"], "-d", "--no-show-raw-insn", elf], text=True)
    return CC.parse_metadata(notes), CC.parse_disassembly(dis)


def mnemonics(instructions):
    return [re.sub(r"^[0-9a-f]+:\s*", "", i).split()[0] for i in instructions if not i.endswith(":") and i != "..."]


def test_the_plane_kernels_are_in_the_code_object(code_object):
    meta, dis = code_object
    for name in FULL + (TAIL,):
        assert name in meta and name in dis and len(dis[name]) > 20, (name, sorted(meta))


def test_no_scratch_no_spills_no_flat_or_buffer_accesses(code_object):
    meta, dis = code_object
    for name in FULL + (TAIL,):
        rec = meta[name]
        assert rec["private_segment_fixed_size"] == 0, (name, rec["private_segment_fixed_size"])
        assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, name
        assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == 512, name
        ops = mnemonics(dis[name])
        bad = sorted({o for o in ops if o.startswith(("flat_", "buffer_", "scratch_"))})
        assert not bad, (name, bad)


def test_full_groups_move_by_16_byte_global_accesses_and_permute_in_registers(code_object):
    meta, dis = code_object
    for name in FULL:
        ops = mnemonics(dis[name])
        assert meta[name]["group_segment_fixed_size"] == 0 and not [o for o in ops if o.startswith("ds_")], f"{name} uses LDS"
        assert meta[name]["vgpr_count"] + meta[name].get("agpr_count", 0) <= 128, (name, meta[name]["vgpr_count"])      # four workgroups of 8 waves per CU
        loads = [o for o in ops if o.startswith("global_load")]
        stores = [o for o in ops if o.startswith("global_store")]
        # widths 8, 4, 2 and 1: 8 + 4 + 2 + 1 quads in, as many out (the compiler may share a few between the paths)
        assert loads.count("global_load_dwordx4") >= 8 and stores.count("global_store_dwordx4") >= 8, (name, loads, stores)
        # no byte or short access at all, and every STORE is a 16-byte one: what is left of the loads are the descriptors'
        narrow = [o for o in loads + stores if re.search(r"byte|short|d16", o)]
        assert not narrow, (name, narrow)
        assert set(stores) == {"global_store_dwordx4"}, (name, sorted(set(stores)))
        assert set(loads) <= {"global_load_dwordx4", "global_load_dwordx2", "global_load_dword"}, (name, sorted(set(loads)))
        # 8 permutes for width 2, 32 for 4, 64 for 8 (planes.h)
        assert ops.count("v_perm_b32") == 8 + 32 + 64, (name, ops.count("v_perm_b32"))
        assert ops.count("s_barrier") >= 1, name                # all loads before any store: what makes in place safe


def test_the_tail_kernel_loads_by_quads_through_lds(code_object):
    meta, dis = code_object
    ops = mnemonics(dis[TAIL])
    assert meta[TAIL]["group_segment_fixed_size"] == 8 * 8192
    assert "global_load_dwordx4" in ops and "s_barrier" in ops
    assert not [o for o in ops if re.match(r"global_load_(u|s)?(byte|short)", o)], "the tail reads by quads, never beyond the last one"
    assert {o for o in ops if o.startswith("global_store")} <= {"global_store_dword", "global_store_byte"}
