"""The XOR-base survey kernel in the shipped gfx950 code object (read on the CPU, as tests/test_codeobj_survey.py reads the plane
survey): present, a workgroup of 512 in wavefronts of 64, without scratch or spills, with the LDS DESIGN.md 4.15 states (the 64
residue histograms of 256 u32 bins, the 1 KiB exchange of the wave sums and the 512-byte exchange of the wave maxima), at most 128
vector registers (two workgroups per CU), 16-byte global loads, LDS adds without return, the byte rotation, single-dword stores,
and no flat, buffer or scratch access.  Metadata and mnemonic presence only."""
import test_codeobj_contract as CC                          # noqa: F401  (the parsers behind the fixture)
from test_codeobj_stored import code_object, mnemonics      # noqa: F401  (the fixture)

KERNEL = "survey_xor_kernel"


def test_the_kernel_is_in_the_code_object(code_object):
    meta, dis = code_object
    assert KERNEL in meta and KERNEL in dis and len(dis[KERNEL]) > 20, sorted(meta)


def test_no_scratch_no_spills_no_flat_buffer_or_scratch_accesses(code_object):
    meta, dis = code_object
    rec = meta[KERNEL]
    assert rec["private_segment_fixed_size"] == 0, rec["private_segment_fixed_size"]
    assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0
    assert rec["wavefront_size"] == 64 and rec["max_flat_workgroup_size"] == 512
    ops = mnemonics(dis[KERNEL])
    bad = sorted({o for o in ops if o.startswith(("flat_", "buffer_", "scratch_"))})
    assert not bad, bad


def test_the_lds_is_the_residue_histograms_and_the_two_exchanges(code_object):
    meta, _dis = code_object
    assert meta[KERNEL]["group_segment_fixed_size"] == 8 * 8 * 256 * 4 + 8 * 16 * 8 + 8 * 16 * 4      # 65.5 KiB: two workgroups per CU
    assert 2 * meta[KERNEL]["group_segment_fixed_size"] <= CC.LDS_PER_CU
    assert meta[KERNEL]["vgpr_count"] + meta[KERNEL].get("agpr_count", 0) <= 128                      # 16 wavefronts per CU


def test_it_loads_by_quads_counts_without_return_and_stores_single_words(code_object):
    _meta, dis = code_object
    ops = mnemonics(dis[KERNEL])
    assert "global_load_dwordx4" in ops
    assert "ds_add_u32" in ops and "ds_add_rtn_u32" not in ops
    assert "v_alignbyte_b32" in ops, "the lanes rotate their bytes so that a tensor equal to its base spreads over the residue histograms"
    assert "v_xor_b32_e32" in ops or "v_xor_b32_e64" in ops, "the buffer and its base meet in registers"
    assert "v_max_u32_e32" in ops or "v_max_u32_e64" in ops, "the scan words leave through a reduction by maximum"
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dword"}
