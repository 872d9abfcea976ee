"""Batch entry points on the CPU: the packet-count helper, every host-side argument check, batch.py's descriptors and
refusals, and the batch kernels' code-object contract (parsed with tests/test_codeobj_contract.py's own readers)."""
import ctypes as C
import os

import pytest

from test_codeobj_contract import PINNED, VEC, check_resources, code_object, step_regions  # noqa: F401  (code_object: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpuar_amd", "lib", "libgpuar_hip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("libgpuar_hip.so not built")
    from gpuar_amd import hip as H
    return H.load()


def counts(lib, sizes):
    n = len(sizes)
    arr = (C.c_uint64 * max(n, 1))(*sizes)
    fp = (C.c_uint64 * (n + 1))(*([0xDEAD] * (n + 1)))
    total = lib.gpuar_hip_batch_packet_count(arr, n, fp)
    return total, list(fp)


@pytest.mark.parametrize("sizes,want", [
    ([], [0]),
    ([0], [0, 0]),
    ([1], [0, 1]),
    ([8191], [0, 1]),
    ([8192], [0, 1]),
    ([8193], [0, 2]),
    ([0, 8193, 0, 1, 0], [0, 0, 2, 2, 3, 3]),
    ([8192 * 3, 0, 0, 16385], [0, 3, 3, 3, 6]),
])
def test_batch_packet_count_at_edge_sizes(lib, sizes, want):
    total, fp = counts(lib, sizes)
    assert total == want[-1] and fp == want


def test_batch_packet_count_without_output_and_without_sizes(lib):
    arr = (C.c_uint64 * 2)(8193, 1)
    assert lib.gpuar_hip_batch_packet_count(arr, 2, None) == 3
    assert lib.gpuar_hip_batch_packet_count(None, 0, None) == 0
    assert lib.gpuar_hip_batch_packet_count(None, 3, None) == 0


# fake device addresses: the host-side checks must answer before anything touches them
A16, A8, A4, ODD = 0x10000, 0x10008, 0x10004, 0x10001
OK, ALIGN, ARG = 0, -1, -2


def test_encode_batch_host_checks(lib):
    e = lib.gpuar_hip_encode_batch
    assert e(A16, A16, A16, 1, 1, A16, None, None, 7) == ARG                 # bad mode first
    assert e(None, None, None, 0, 0, None, None, None, 0) == OK              # no packets: nothing launched, nothing checked
    assert e(None, A16, A16, 1, 1, A16, None, None, 0) == ARG
    assert e(A16, None, A16, 1, 1, A16, None, None, 0) == ARG
    assert e(A16, A16, None, 1, 1, A16, None, None, 0) == ARG
    assert e(A16, A16, A16, 1, 1, None, None, None, 0) == ARG
    assert e(A16, A16, A16, 1, 1 << 32, A16, None, None, 0) == ARG
    assert e(A16, A16, A16, 1 << 32, 1, A16, None, None, 0) == ARG
    assert e(A16, A16, A16, 1, 1, A8, None, None, 0) == ALIGN               # slots: 16 bytes
    assert e(A16, A16, A16, 1, 1, A16, A16 + 2, None, 0) == ALIGN           # status: 4 bytes
    assert e(A4, A16, A16, 1, 1, A16, None, None, 0) == ALIGN               # descriptor arrays: 8 bytes
    assert e(A16, A4, A16, 1, 1, A16, None, None, 0) == ALIGN
    assert e(A16, A16, A4, 1, 1, A16, None, None, 0) == ALIGN


def test_decode_batch_host_checks(lib):
    d = lib.gpuar_hip_decode_batch
    assert d(None, None, 0, 0, None, None, None, None) == OK
    assert d(None, A16, 1, 1, A16, A16, None, None) == ARG
    assert d(A16, None, 1, 1, A16, A16, None, None) == ARG
    assert d(A16, A16, 1, 1, None, A16, None, None) == ARG
    assert d(A16, A16, 1, 1, A16, None, None, None) == ARG
    assert d(A16, A16, 1, 1 << 32, A16, A16, None, None) == ARG
    assert d(A8, A16, 1, 1, A16, A16, None, None) == ALIGN
    assert d(A16, A16, 1, 1, A16, A16, ODD, None) == ALIGN
    assert d(A16, A4, 1, 1, A16, A16, None, None) == ALIGN


def test_decode_stream_batch_host_checks(lib):
    d = lib.gpuar_hip_decode_stream_batch
    assert d(None, None, None, 0, 0, None, None, None, None) == OK
    assert d(None, A16, A16, 1, 1, A16, A16, None, None) == ARG
    assert d(A16, None, A16, 1, 1, A16, A16, None, None) == ARG
    assert d(A16, A16, None, 1, 1, A16, A16, None, None) == ARG
    assert d(A16, A16, A16, 1, 1, None, A16, None, None) == ARG
    assert d(A16, A16, A16, 1, 1, A16, None, None, None) == ARG
    assert d(A16, A16, A16, 1, 1 << 32, A16, A16, None, None) == ARG
    assert d(ODD, A16, A16, 1, 1, A16, A16, None, None) == ALIGN
    assert d(A16, A4, A16, 1, 1, A16, A16, None, None) == ALIGN
    assert d(A16, A16, A16, 1, 1, A16, A16, ODD, None) == ALIGN


def test_status_bit_is_distinct():
    from gpuar_amd import hip as H
    text = open(os.path.join(ROOT, "include", "gpuar_hip.h")).read()
    assert "#define GPUAR_STATUS_BAD_BATCH      0x4u" in text
    assert H.STATUS_BAD_BATCH == 4 and len({H.STATUS_SLOT_OVERFLOW, H.STATUS_BAD_PACKET, H.STATUS_BAD_BATCH}) == 3


# ---- batch.py's descriptors and refusals (CPU tensors and fake devices: nothing is launched) ----

class FakeTensor:
    """Just enough of a CUDA tensor for batch.describe."""
    def __init__(self, ptr, n, device="cuda:0", is_cuda=True, contiguous=True, itemsize=1):
        import torch
        self._ptr, self._n, self.device, self.is_cuda, self._c, self._isz = ptr, n, torch.device(device), is_cuda, contiguous, itemsize

    def numel(self):
        return self._n

    def element_size(self):
        return self._isz

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return self._ptr


@pytest.fixture
def batchmod(lib, monkeypatch):
    import torch
    from gpuar_amd import batch
    monkeypatch.setattr(torch, "Tensor", FakeTensor)         # describe() checks isinstance(t, torch.Tensor)
    return batch


def test_describe_builds_descriptors(batchmod):
    ts = [FakeTensor(0x1000, 0), FakeTensor(0x2000, 8193), FakeTensor(0x9000, 3, itemsize=4), FakeTensor(0, 0)]
    device, ptrs, sizes, fp, n = batchmod.describe(ts)
    assert str(device) == "cuda:0" and ptrs == [0, 0x2000, 0x9000, 0] and sizes == [0, 8193, 12, 0]
    assert fp == [0, 0, 2, 3, 3] and n == 3


@pytest.mark.parametrize("bad,msg", [
    (FakeTensor(0x2008, 16), "16-byte aligned"),
    (FakeTensor(0x2000, 16, is_cuda=False), "not a CUDA tensor"),
    (FakeTensor(0x2000, 16, contiguous=False), "not contiguous"),
    (FakeTensor(0x2000, 16, device="cuda:1"), "is on cuda:1"),
])
def test_describe_refuses_what_the_kernels_cannot_take(batchmod, bad, msg):
    from gpuar_amd.hip import GpuarError
    with pytest.raises(GpuarError, match=msg):
        batchmod.describe([FakeTensor(0x1000, 64), bad])


def test_describe_refuses_non_tensors(lib):
    from gpuar_amd import batch
    from gpuar_amd.hip import GpuarError
    with pytest.raises(GpuarError, match="not a tensor"):
        batch.describe([b"bytes"])


# ---- the batch kernels' code-object contract ----

SIBLING = {"encode_batch_kernel": "encode_kernel", "encode_small_batch_kernel": "encode_small_kernel",
           "decode_slots_batch_kernel": "decode_slots_kernel", "decode_stream_batch_kernel": "decode_stream_kernel"}


@pytest.mark.parametrize("kernel", sorted(SIBLING))
def test_batch_kernels_keep_their_siblings_budgets(code_object, kernel):
    meta, _ = code_object
    assert kernel in meta, sorted(meta)
    check_resources(SIBLING[kernel], meta[kernel])           # no scratch, no spills, the sibling's LDS and register budgets
    for field in ("group_segment_fixed_size", "max_flat_workgroup_size"):
        assert meta[kernel][field] == meta[SIBLING[kernel]][field], (kernel, field)


@pytest.mark.parametrize("kernel", ["decode_slots_batch_kernel", "decode_stream_batch_kernel"])
def test_batch_decoders_keep_the_hand_scheduled_step(code_object, kernel):
    """The same 83 / 79-instruction steps as decode_slots_kernel (tests/test_codeobj_contract.py), two loop bodies of 32."""
    import collections
    _, dis = code_object
    regions = step_regions(dis[kernel])
    assert len(regions) == 63, len(regions)
    shapes = collections.Counter()
    for r in regions:
        ops = [t.split()[0] for t in r]
        if any(o.startswith(("global_", "flat_", "s_cbranch", "s_branch")) for o in ops):
            continue
        shapes[(sum(1 for o in ops if VEC.match(o)), sum(1 for o in ops if o.startswith("ds_")))] += 1
        assert sorted(o for o in ops if o.startswith("s_")) == ["s_and_b64", "s_andn2_b64", "s_waitcnt", "s_waitcnt"], ops
    two = shapes.most_common(2)
    assert {k for k, _ in two} == {(79, 5), (83, 4)} and min(c for _, c in two) >= 20, shapes


@pytest.mark.parametrize("kernel", ["decode_slots_batch_kernel", "decode_stream_batch_kernel"])
def test_batch_decoders_leave_the_pinned_registers_alone(code_object, kernel):
    import re
    _, dis = code_object
    for t in dis[kernel]:
        if PINNED.search(t):
            op = t.split()[0]
            assert op in ("global_load_dwordx4", "ds_write2st64_b32", "v_mul_hi_u32"), t
            if op == "v_mul_hi_u32":
                assert re.match(r"v_mul_hi_u32 v\d+, v\d+, v2\d\d$", t), t


def _count(text, op):
    return sum(1 for t in text if t.split()[0] == op)


def test_batch_encoders_keep_whole_phase_bodies_past_the_wave_minimum(code_object):
    """The batch encoders' ragged schedule: a lane runs the unrolled whole-phase body for every whole phase
    it owns, not only up to the wavefront's shortest lane.  Without the masked loop the slots would be the same bytes, only
    slower, so no parity test sees it: it is pinned here by the bodies' signature instructions.
      throughput (encode_batch_kernel against encode_kernel, which holds each body once): the coder's body -- 16
      v_mul_hi_u32 and 16 global_store_dword for 8 symbols --, the low modeler's -- 8 v_bfe_i32 --, and the top modeler's
      masked phase next to the low modeler's second body -- 16 SDWA tag shifts -- are there once more;
      latency (encode_small_batch_kernel, whose roles have the masked loop and the deferred phase): the interval role's
      unrolled body (2 v_mul_hi_u32 per symbol) and the sink's (2 stores per symbol) are there as in encode_small_kernel."""
    _, dis = code_object
    one, batch = dis["encode_kernel"], dis["encode_batch_kernel"]
    assert _count(batch, "v_mul_hi_u32") - _count(one, "v_mul_hi_u32") >= 16
    assert _count(batch, "global_store_dword") - _count(one, "global_store_dword") >= 16
    assert _count(batch, "v_bfe_i32") - _count(one, "v_bfe_i32") >= 8
    assert _count(batch, "v_lshlrev_b32_sdwa") - _count(one, "v_lshlrev_b32_sdwa") >= 16
    small, small_batch = dis["encode_small_kernel"], dis["encode_small_batch_kernel"]
    assert _count(small_batch, "v_mul_hi_u32") >= _count(small, "v_mul_hi_u32") >= 32
    assert _count(small_batch, "global_store_dword") >= _count(small, "global_store_dword") >= 32
