"""The code-object facts DESIGN.md 4.12 quotes for the three sparse kernels, read on the CPU from the metadata note of the gfx950
code object inside the shipped library (skipped where the ROCm LLVM tools are missing): no scratch, no spills, no LDS for the
scan and the pack, 8 KiB of LDS per wavefront of the workgroup for the unpack, and the measured register counts as upper bounds.
Metadata only: the disassembly is not read."""
import pytest

from test_codeobj_contract import code_object  # noqa: F401  (the module-scoped fixture: the shipped library's code object)

WAVES = 4                                    # kSparseWaves: wavefronts per workgroup of all three kernels
# kernel -> (LDS bytes per workgroup, vector registers measured, scalar registers measured)
FACTS = {
    "sparse_scan_kernel": (0, 95, 74),
    "sparse_pack_kernel": (0, 168, 72),
    "sparse_unpack_kernel": (WAVES * 8192, 52, 74),
}


@pytest.mark.parametrize("name", sorted(FACTS))
def test_the_sparse_kernels_keep_their_resources(code_object, name):  # noqa: F811
    meta, _disassembly = code_object
    assert name in meta, (name, sorted(meta))
    rec = meta[name]
    lds, vgprs, sgprs = FACTS[name]
    assert rec["private_segment_fixed_size"] == 0, f"{name}: {rec['private_segment_fixed_size']} bytes of scratch per lane"
    assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, f"{name}: spills"
    assert rec.get("uses_dynamic_stack") in ("false", False, 0)
    assert rec["group_segment_fixed_size"] == lds, f"{name}: {rec['group_segment_fixed_size']} bytes of LDS per workgroup, not {lds}"
    assert rec["max_flat_workgroup_size"] == WAVES * 64 and rec["wavefront_size"] == 64
    assert rec["vgpr_count"] + rec.get("agpr_count", 0) <= vgprs, f"{name}: {rec['vgpr_count']} vector registers, more than {vgprs}"
    assert rec["sgpr_count"] <= sgprs, f"{name}: {rec['sgpr_count']} scalar registers, more than {sgprs}"
