"""The code-object facts DESIGN.md 4.14 quotes for move_bytes_kernel, read on the CPU from the metadata note of the gfx950 code
object inside the shipped library (skipped where the ROCm LLVM tools are missing): wavefront size 64, a workgroup of 256, no LDS, no
scratch, no spills, and the register counts the build gives as upper bounds; and, from the disassembly, that the bytes move the way
the design says -- 16-byte global loads and stores for the body, single bytes for the ragged ends, nothing flat."""
import collections

from test_codeobj_contract import code_object  # noqa: F401  (the module-scoped fixture: the shipped library's code object)

NAME = "move_bytes_kernel"
LDS, VGPRS, SGPRS, THREADS = 0, 20, 36, 256


def test_move_bytes_kernel_keeps_its_resources(code_object):  # noqa: F811
    meta, _disassembly = code_object
    assert NAME in meta, sorted(meta)
    rec = meta[NAME]
    assert rec["private_segment_fixed_size"] == 0, f"{rec['private_segment_fixed_size']} bytes of scratch per lane"
    assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, "spills"
    assert rec.get("uses_dynamic_stack") in ("false", False, 0)
    assert rec["group_segment_fixed_size"] == LDS, f"{rec['group_segment_fixed_size']} bytes of LDS per workgroup, not {LDS}"
    assert rec["max_flat_workgroup_size"] == THREADS and rec["wavefront_size"] == 64
    assert rec["vgpr_count"] + rec.get("agpr_count", 0) <= VGPRS, f"{rec['vgpr_count']} vector registers, more than {VGPRS}"
    assert rec["sgpr_count"] <= SGPRS, f"{rec['sgpr_count']} scalar registers, more than {SGPRS}"


def test_move_bytes_kernel_moves_quads_and_single_bytes_through_global_instructions(code_object):  # noqa: F811
    _meta, dis = code_object
    ops = collections.Counter(t.split()[0] for t in dis[NAME])
    assert not [op for op in ops if op.startswith(("flat_", "buffer_", "scratch_", "ds_"))], ops
    assert ops["global_load_dwordx4"] == 1 and ops["global_store_dwordx4"] == 1, ops          # the body: one loop
    assert ops["global_load_ubyte"] == 2 and ops["global_store_byte"] == 2, ops               # head and tail
    stores = [op for op in ops if op.startswith("global_store")]
    assert sorted(stores) == ["global_store_byte", "global_store_dwordx4"], stores            # nothing else is written (the status: an atomic)
