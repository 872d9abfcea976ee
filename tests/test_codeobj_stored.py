"""The estimate and packet-copy kernels in the shipped gfx950 code object (read on the CPU, as tests/test_codeobj_planes.py reads
the plane kernels): present, without scratch or spills, with the LDS their design says (estimate: 16 wavefronts x 8 copies x
256 u32 bins; the copy: none), wavefront size 64, and 16-byte global loads.  Metadata and mnemonic presence only."""
import os
import re
import subprocess

import pytest

import test_codeobj_contract as CC

ESTIMATE = "estimate_kernel"
MOVE = "move_packets_kernel"


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    """(metadata by kernel, disassembly by kernel) of the library's gfx950 code object; the library is built when it is missing."""
    if not os.path.exists(CC.LIB):
        import __graft_entry__ as g
        g.build()
    missing = [p for p in CC.TOOLS.values() if not os.path.exists(p)]
    assert not missing, f"the ROCm LLVM tools that built the library are not where they were: {missing}"
    d = tmp_path_factory.mktemp("codeobj_stored")
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


def test_both_kernels_are_in_the_code_object(code_object):
    meta, dis = code_object
    for name in (ESTIMATE, MOVE):
        assert name in meta and name in dis and len(dis[name]) > 20, (name, sorted(meta))


def test_no_scratch_no_spills_no_flat_or_buffer_accesses(code_object):
    meta, dis = code_object
    for name, threads in ((ESTIMATE, 1024), (MOVE, 512)):
        rec = meta[name]
        assert rec["private_segment_fixed_size"] == 0, (name, rec["private_segment_fixed_size"])
        assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, name
        assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == threads, name
        ops = mnemonics(dis[name])
        bad = sorted({o for o in ops if o.startswith(("flat_", "buffer_", "scratch_"))})
        assert not bad, (name, bad)
        assert "global_load_dwordx4" in ops, name


def test_the_estimate_kernel_keeps_one_histogram_per_wavefront_in_lds(code_object):
    meta, dis = code_object
    ops = mnemonics(dis[ESTIMATE])
    assert meta[ESTIMATE]["group_segment_fixed_size"] == 16 * 8 * 256 * 4          # nothing else: no array of the kernel was moved to LDS
    assert meta[ESTIMATE]["vgpr_count"] + meta[ESTIMATE].get("agpr_count", 0) <= 128, meta[ESTIMATE]["vgpr_count"]      # 16 wavefronts per CU
    assert "ds_add_u32" in ops and "ds_add_rtn_u32" not in ops
    assert "ds_read_b128" in ops and "ds_write_b128" in ops
    assert "s_barrier" not in ops, "a wavefront's histogram is its own"
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dword"}


def test_the_copy_kernel_uses_no_lds_and_stores_by_quads_dwords_and_bytes(code_object):
    meta, dis = code_object
    ops = mnemonics(dis[MOVE])
    assert meta[MOVE]["group_segment_fixed_size"] == 0 and not [o for o in ops if o.startswith("ds_")]
    assert not [o for o in ops if re.match(r"global_load_(u|s)?(byte|short)", o)], "a region is read by quads, never beyond the last one"
    stores = {o for o in ops if o.startswith("global_store")}
    assert {"global_store_dwordx4", "global_store_dword", "global_store_byte"} <= stores
    assert stores <= {"global_store_dwordx4", "global_store_dword", "global_store_byte", "global_store_byte_d16_hi"}, sorted(stores)
