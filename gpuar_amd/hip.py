"""ctypes bindings to libgpuar_hip.so (include/gpuar_hip.h).

There is no CPU fallback here: if the HIP library is missing or a call fails,
these functions raise.  Device buffers are torch uint8 CUDA tensors (torch is
used for allocation and stream handles only).
"""
from __future__ import annotations

import ctypes as C
import os

PACKET = 8192
SLOT = 8704
HEADER_LEN = 20
STATUS_SLOT_OVERFLOW = 0x1
STATUS_BAD_PACKET = 0x2
STATUS_BAD_BATCH = 0x4
STATUS_CHECKSUM = 0x8
KIND_ID = {"uniform": 0, "zipf": 1, "text": 2}

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgpuar_hip.so")

_int, _vp, _sz, _u32, _u64, _str = C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_char_p
_pu32, _pu64, _psz = C.POINTER(_u32), C.POINTER(_u64), C.POINTER(_sz)
_BATCH = [_vp, _vp, _vp, _sz, _sz]   # the descriptors of a batch: pointers, bytes, first_packet, n_buffers, n_packets


def _both(stem, restype, argtypes):
    """the split and the merge call of one filter: one prototype"""
    return {f"gpuar_hip_split_{stem}": (restype, argtypes), f"gpuar_hip_merge_{stem}": (restype, argtypes)}


# Every export of the library with its (restype, argtypes): the prototypes of include/gpuar_hip.h, each once.  d_status and stream
# are the two _vp at the end of the calls that take them.
SIGNATURES = {
    "initConstantRange": (None, []),
    "garCompressExecutor": (None, [_vp, _sz, _vp, _u32]),
    "garDecompressExecutor": (None, [_vp, _sz, _vp, _u32]),
    "gpuar_hip_packet_count": (_sz, [_sz]),
    "gpuar_hip_encode": (_int, [_vp, _sz, _vp, _vp, _vp]),
    "gpuar_hip_encode_mode": (_int, [_vp, _sz, _vp, _vp, _vp, _int]),
    "gpuar_hip_decode": (_int, [_vp, _sz, _vp, _vp, _vp]),
    "gpuar_hip_compact": (_int, [_vp, _sz, _vp, _vp, _vp]),
    "gpuar_hip_decode_stream": (_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "gpuar_hip_status": (_int, [_pu32]),
    "gpuar_hip_last_error": (_int, []),
    "gpuar_hip_error_string": (_str, [_int]),
    "gpuar_hip_version": (_str, []),
    "gpuar_hip_abi_version": (_int, []),
    "gpuar_hip_generate": (_int, [_int, _u64, _u64, _sz, _vp, _vp]),
    "gpuar_hip_copy": (_int, [_vp, _vp, _sz, _vp]),
    "gpuar_hip_clock_samples": (_int, [_int, _pu64, _int]),
    "gpuar_hip_batch_packet_count": (_sz, [_pu64, _sz, _pu64]),
    "gpuar_hip_encode_batch": (_int, [*_BATCH, _vp, _vp, _vp, _int]),
    "gpuar_hip_decode_batch": (_int, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "gpuar_hip_decode_stream_batch": (_int, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "gpuar_hip_crc32": (_int, [_vp, _sz, _vp, _vp]),
    "gpuar_hip_verify_crc32": (_int, [_vp, _sz, _vp, _vp, _vp, _vp]),
    "gpuar_hip_crc32_batch": (_int, [*_BATCH, _vp, _vp, _vp]),
    "gpuar_hip_verify_crc32_batch": (_int, [*_BATCH, _vp, _vp, _vp, _vp]),
    **_both("planes", _int, [_vp, _sz, _u32, _vp, _vp]),
    **_both("planes_batch", _int, [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    **_both("planes_host", _int, [_vp, _sz, _u32, _vp]),
    **_both("delta", _int, [_vp, _sz, _u32, _vp, _vp]),
    **_both("delta_batch", _int, [_vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    **_both("delta_host", _int, [_vp, _sz, _u32, _vp]),
    "gpuar_hip_delta_block_host": (_int, [_pu32, _u32, _int, _u64, _pu64]),
    **_both("xor", _int, [_vp, _vp, _sz, _u32, _vp, _vp]),
    **_both("xor_batch", _int, [_vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    **_both("xor_host", _int, [_vp, _vp, _sz, _u32, _vp]),
    "gpuar_hip_estimate": (_int, [_vp, _sz, _vp, _vp]),
    "gpuar_hip_estimate_batch": (_int, [*_BATCH, _vp, _vp, _vp]),
    "gpuar_hip_estimate_host": (_int, [_vp, _sz, _vp]),
    "gpuar_hip_move_packets": (_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "gpuar_hip_survey_planes": (_int, [_vp, _sz, _vp, _sz, _vp]),
    "gpuar_hip_survey_planes_batch": (_int, [*_BATCH, _vp, _sz, _vp, _vp]),
    "gpuar_hip_survey_planes_host": (_int, [_vp, _sz, _vp, _sz]),
    "gpuar_hip_choose_planes": (_u32, [_pu64, _u64]),
    "gpuar_hip_survey_delta": (_int, [_vp, _sz, _u32, _vp, _sz, _vp]),
    "gpuar_hip_survey_delta_batch": (_int, [*_BATCH, _u32, _vp, _sz, _vp, _vp]),
    "gpuar_hip_survey_delta_host": (_int, [_vp, _sz, _u32, _vp, _sz]),
    "gpuar_hip_choose_filter": (_int, [_pu64, _pu64, _u64, _pu32]),
    "gpuar_hip_sparse_len": (_u32, [_u32]),
    "gpuar_hip_sparse_rule": (_int, [_u32, _u32, _u32, _int]),
    "gpuar_hip_sparse_scan": (_int, [_vp, _sz, _vp, _vp]),
    "gpuar_hip_sparse_scan_batch": (_int, [*_BATCH, _vp, _vp, _vp]),
    "gpuar_hip_sparse_scan_host": (_int, [_vp, _sz, _vp]),
    "gpuar_hip_sparse_pack": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "gpuar_hip_sparse_unpack": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "gpuar_hip_sparse_pack_host": (_int, [_vp, _sz, _vp, _sz, _psz]),
    "gpuar_hip_sparse_unpack_host": (_int, [_vp, _sz, _vp, _sz]),
    "gpuar_hip_kinds_store": (_int, [_vp, _sz, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
    "gpuar_hip_kinds_expand": (_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "gpuar_hip_kinds_store_host": (_int, [_vp, _sz, _int, _int, _vp, _sz, _pu32, _psz]),
    "gpuar_hip_kinds_expand_host": (_int, [_vp, _sz, _u32, _vp, _sz]),
    "gpuar_hip_gip_read_host": (_int, [_vp, _sz, _pu64]),
    "gpuar_hip_gip_tables_host": (_int, [_vp, _sz, _vp, _vp, _vp, _sz]),
}
EXPORTS = list(SIGNATURES)
# The device calls declared in include/gpuar_hip_gip.h: a table of their own, because the tables that pin gpuar_hip.h are closed
# (INTEGRATION.md 3).  load() declares them beside SIGNATURES.
GIP_SIGNATURES = {
    "gpuar_hip_move_bytes": (_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
}
# The XOR-base survey, declared in include/gpuar_hip_xsurvey.h: a third table for the same reason (tests/test_capi_xsurvey_host.py).
XSURVEY_SIGNATURES = {
    "gpuar_hip_survey_xor": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "gpuar_hip_survey_xor_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp]),
    "gpuar_hip_survey_xor_host": (_int, [_vp, _vp, _sz, _vp, _vp, _sz]),
}
# The mixed filter, declared in include/gpuar_hip_mixed.h: a fourth table for the same reason (tests/test_mixed_host.py).
MIXED_SIGNATURES = {
    "gpuar_hip_mode_count": (_sz, [_sz]),
    "gpuar_hip_batch_mode_count": (_sz, [_pu64, _sz, _pu64]),
    "gpuar_hip_choose_mode": (_int, [_pu64, _pu64, _pu64, _u64, _pu64]),
    "gpuar_hip_choose_modes": (_int, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "gpuar_hip_choose_modes_batch": (_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp]),
    "gpuar_hip_choose_modes_host": (_int, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    **_both("mixed", _int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    **_both("mixed_batch", _int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    **_both("mixed_host", _int, [_vp, _vp, _sz, _vp, _vp]),
}
MIXED_MODES = 12                     # the valid modes of a supergroup are 0 .. 11: log2(width) | delta << 2 | base << 3
SUPERGROUP = 8 * PACKET              # the bytes one mode stands for
GIP_INFO_WORDS = 10                  # GPUAR_GIP_INFO_WORDS
SURVEY_WIDTHS = (1, 2, 4, 8)         # the rows of a survey
CLOCK_SLOTS = 256                    # GPUAR_CLOCK_SLOTS
ABI_VERSION = 2                      # GPUAR_HIP_ABI_VERSION of the header these bindings were written against
MODE_ID = {"auto": 0, "throughput": 1, "latency": 2, "table": 3}     # GPUAR_MODE_* ("table": encode() only, the batch encoders refuse it)

_lib = None


class GpuarError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Loads the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GpuarError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    # a library built from older sources lacks newer exports: say "rebuild" instead of dying with an AttributeError half-way
    # through the signatures
    missing = [name for name in (*EXPORTS, *GIP_SIGNATURES, *XSURVEY_SIGNATURES, *MIXED_SIGNATURES) if not hasattr(lib, name)]
    if missing:
        raise GpuarError(f"{LIB_PATH} lacks {missing}: it was built from older sources -- rebuild the library")
    for name, (restype, argtypes) in (*SIGNATURES.items(), *GIP_SIGNATURES.items(), *XSURVEY_SIGNATURES.items(), *MIXED_SIGNATURES.items()):
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    if lib.gpuar_hip_abi_version() != ABI_VERSION:
        raise GpuarError(f"{LIB_PATH} speaks ABI {lib.gpuar_hip_abi_version()}, these bindings {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def _mode_id(mode, env_var) -> int:
    """GPUAR_MODE_* for a call: the caller's `mode` ("auto" | "throughput" | "latency" | "table"), else the environment variable
    that tests and tools use to pin the encode kernel (GPUAR_ENCODE_MODE; there is no decode mode) -- read HERE, in the
    Python shim, never inside the library --, else auto."""
    name = mode if mode is not None else os.environ.get(env_var, "auto")
    if name not in MODE_ID:
        raise GpuarError(f"unknown kernel mode {name!r} (auto, throughput, latency, table)")
    return MODE_ID[name]


def _check(code: int, what: str) -> None:
    if code != 0:
        raise GpuarError(f"{what}: {load().gpuar_hip_error_string(code).decode()} (code {code})")


def _call(name: str, *args) -> None:
    """One call of an export that returns a code; anything but 0 raises with the export's name."""
    _check(getattr(load(), name)(*args), name)


def _stream_handle(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def packet_count(n_bytes: int) -> int:
    return (n_bytes + PACKET - 1) // PACKET


def _require_cuda_u8(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise GpuarError(f"{name} must be a contiguous uint8 CUDA tensor")


def _status_ptr(d_status):
    """Device address of a caller-owned status word (a 1-element int32/uint32 CUDA tensor), or None."""
    if d_status is None:
        return None
    import torch
    if not (isinstance(d_status, torch.Tensor) and d_status.is_cuda and d_status.element_size() == 4 and d_status.numel() >= 1):
        raise GpuarError("d_status must be a CUDA tensor of one 32-bit word")
    return d_status.data_ptr()


def _span(t, n_bytes, name="d_in"):
    """(n, its packet count): the bytes of the uint8 tensor `t` a call works on -- the first n_bytes, by default all."""
    n = t.numel() if n_bytes is None else n_bytes
    if n > t.numel():
        raise GpuarError(f"n_bytes is larger than {name}")
    return n, packet_count(n)


def encode(d_in, d_slots=None, stream=None, d_status=None, mode=None):
    """Encode the bytes of `d_in` into 8704-byte packet slots (garCompress layout).  `d_status`: this launch's
    own status word (a zeroed 1-element int32 CUDA tensor); None = the device's fallback word (status()).
    `mode`: "auto" | "throughput" | "latency" | "table" (gpuar_hip_encode_mode); None = $GPUAR_ENCODE_MODE, else auto."""
    import torch
    _require_cuda_u8(d_in, "d_in")
    n = d_in.numel()
    npk = packet_count(n)
    if d_slots is None:
        d_slots = torch.empty(max(npk, 1) * SLOT, dtype=torch.uint8, device=d_in.device)
    _require_cuda_u8(d_slots, "d_slots")
    if d_slots.numel() < npk * SLOT:
        raise GpuarError("d_slots too small")
    _call("gpuar_hip_encode_mode", d_in.data_ptr(), n, d_slots.data_ptr(), _status_ptr(d_status), _stream_handle(stream),
          _mode_id(mode, "GPUAR_ENCODE_MODE"))
    return d_slots


def decode(d_slots, n_packets: int, d_out=None, stream=None, d_status=None):
    """Decode `n_packets` slots into n_packets*8192 output bytes."""
    import torch
    _require_cuda_u8(d_slots, "d_slots")
    if d_slots.numel() < n_packets * SLOT:
        raise GpuarError("d_slots too small")
    if d_out is None:
        d_out = torch.empty(max(n_packets, 1) * PACKET, dtype=torch.uint8, device=d_slots.device)
    _require_cuda_u8(d_out, "d_out")
    if d_out.numel() < n_packets * PACKET:
        raise GpuarError("d_out too small")
    _call("gpuar_hip_decode", d_slots.data_ptr(), n_packets, d_out.data_ptr(), _status_ptr(d_status), _stream_handle(stream))
    return d_out


def compact(d_slots, n_packets: int, d_stream=None, d_offsets=None, stream=None):
    """Slots -> (back-to-back packet stream buffer, u64 offsets[n_packets+1]) on the device."""
    import torch
    _require_cuda_u8(d_slots, "d_slots")
    if d_stream is None:
        d_stream = torch.empty(max(n_packets, 1) * SLOT, dtype=torch.uint8, device=d_slots.device)
    if d_offsets is None:
        d_offsets = torch.empty(n_packets + 1, dtype=torch.int64, device=d_slots.device)
    _call("gpuar_hip_compact", d_slots.data_ptr(), n_packets, d_stream.data_ptr(), d_offsets.data_ptr(), _stream_handle(stream))
    return d_stream, d_offsets


def decode_stream(d_stream, d_offsets, n_packets: int, d_out=None, stream=None, d_status=None):
    import torch
    _require_cuda_u8(d_stream, "d_stream")
    if d_out is None:
        d_out = torch.empty(max(n_packets, 1) * PACKET, dtype=torch.uint8, device=d_stream.device)
    _call("gpuar_hip_decode_stream", d_stream.data_ptr(), d_offsets.data_ptr(), n_packets, d_out.data_ptr(), _status_ptr(d_status),
          _stream_handle(stream))
    return d_out


def batch_packet_count(sizes):
    """(first_packet as a list of n + 1 ints, packet count) for buffers of `sizes` bytes (gpuar_hip_batch_packet_count)."""
    n = len(sizes)
    arr = (C.c_uint64 * max(n, 1))(*sizes)
    fp = (C.c_uint64 * (n + 1))()
    total = load().gpuar_hip_batch_packet_count(arr, n, fp)
    return list(fp), int(total)


def _require_u64_desc(t, name, n):
    """A batch descriptor array: a contiguous 8-byte CUDA tensor (int64 / uint64) of at least n entries."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.element_size() == 8 and t.is_contiguous() and t.numel() >= n):
        raise GpuarError(f"{name} must be a contiguous 64-bit CUDA tensor of at least {n} entries")


def _require_batch(d_ptrs, d_bytes, d_first_packet, n_buffers, ptrs="d_ptrs", more=()):
    """The descriptors of a batch call: the pointers (named `ptrs`), d_bytes, d_first_packet, then `more`: (tensor, name) of n_buffers entries."""
    for t, name, n in ((d_ptrs, ptrs, n_buffers), (d_bytes, "d_bytes", n_buffers), (d_first_packet, "d_first_packet", n_buffers + 1),
                       *((t, name, n_buffers) for t, name in more)):
        _require_u64_desc(t, name, n)


def encode_batch(d_ptrs, d_bytes, d_first_packet, n_buffers: int, n_packets: int, d_slots=None, stream=None, d_status=None, mode=None,
                 device=None):
    """Encode a batch of buffers into n_packets slots (gpuar_hip_encode_batch).  d_ptrs / d_bytes / d_first_packet: device
    descriptor tensors (int64: buffer addresses, byte counts, n_buffers + 1 first packets).  `mode` as for encode()."""
    import torch
    _require_batch(d_ptrs, d_bytes, d_first_packet, n_buffers)
    if d_slots is None:
        d_slots = torch.empty(max(n_packets, 1) * SLOT, dtype=torch.uint8, device=device or d_ptrs.device)
    _require_cuda_u8(d_slots, "d_slots")
    if d_slots.numel() < n_packets * SLOT:
        raise GpuarError("d_slots too small")
    _call("gpuar_hip_encode_batch", d_ptrs.data_ptr(), d_bytes.data_ptr(), d_first_packet.data_ptr(), n_buffers, n_packets, d_slots.data_ptr(),
          _status_ptr(d_status), _stream_handle(stream), _mode_id(mode, "GPUAR_ENCODE_MODE"))
    return d_slots


def decode_batch(d_slots, d_first_packet, n_buffers: int, n_packets: int, d_out_ptrs, d_out_bytes, stream=None, d_status=None):
    """Decode n_packets slots of a batch into the buffers d_out_ptrs[b] (room d_out_bytes[b]) (gpuar_hip_decode_batch)."""
    _require_cuda_u8(d_slots, "d_slots")
    if d_slots.numel() < n_packets * SLOT:
        raise GpuarError("d_slots too small")
    for t, name, n in ((d_out_ptrs, "d_out_ptrs", n_buffers), (d_out_bytes, "d_out_bytes", n_buffers), (d_first_packet, "d_first_packet", n_buffers + 1)):
        _require_u64_desc(t, name, n)
    _call("gpuar_hip_decode_batch", d_slots.data_ptr(), d_first_packet.data_ptr(), n_buffers, n_packets, d_out_ptrs.data_ptr(),
          d_out_bytes.data_ptr(), _status_ptr(d_status), _stream_handle(stream))


def decode_stream_batch(d_stream, d_offsets, d_first_packet, n_buffers: int, n_packets: int, d_out_ptrs, d_out_bytes, stream=None,
                        d_status=None):
    """Decode a batch from its compacted stream (offsets in batch order, as compact() made them) (gpuar_hip_decode_stream_batch)."""
    _require_cuda_u8(d_stream, "d_stream")
    for t, name, n in ((d_offsets, "d_offsets", n_packets + 1), (d_out_ptrs, "d_out_ptrs", n_buffers), (d_out_bytes, "d_out_bytes", n_buffers),
                       (d_first_packet, "d_first_packet", n_buffers + 1)):
        _require_u64_desc(t, name, n)
    _call("gpuar_hip_decode_stream_batch", d_stream.data_ptr(), d_offsets.data_ptr(), d_first_packet.data_ptr(), n_buffers, n_packets,
          d_out_ptrs.data_ptr(), d_out_bytes.data_ptr(), _status_ptr(d_status), _stream_handle(stream))


def _require_crc(t, name, n):
    """A CRC array: a contiguous 4-byte CUDA tensor (int32 / uint32) of at least n entries."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.element_size() == 4 and t.is_contiguous() and t.numel() >= n):
        raise GpuarError(f"{name} must be a contiguous 32-bit CUDA tensor of at least {n} entries")


def _words(d_words, name, n, device, whole=False):
    """A call's result of n 32-bit words: the caller's tensor, or a new int32 one (`whole`: not cut to n where n is 0)."""
    import torch
    if d_words is None:
        d_words = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        d_words = d_words if whole else d_words[:n]
    _require_crc(d_words, name, n)
    return d_words


def _words_single(export, d_in, n_bytes, d_words, name, stream, whole=False):
    """The calls that give one 32-bit word per packet of one buffer (CRC, estimate, scan word): one prototype.  Returns d_words."""
    _require_cuda_u8(d_in, "d_in")
    n, npk = _span(d_in, n_bytes)
    d_words = _words(d_words, name, npk, d_in.device, whole)
    _call(export, d_in.data_ptr(), n, d_words.data_ptr(), _stream_handle(stream))
    return d_words


def _words_batch(export, d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_words, name, stream, d_status, device, whole=False):
    """The batch calls that give one 32-bit word per packet (CRC, estimate, scan word): one prototype.  Returns d_words."""
    _require_batch(d_ptrs, d_bytes, d_first_packet, n_buffers)
    d_words = _words(d_words, name, n_packets, device or d_ptrs.device, whole)
    _call(export, d_ptrs.data_ptr(), d_bytes.data_ptr(), d_first_packet.data_ptr(), n_buffers, n_packets, d_words.data_ptr(),
          _status_ptr(d_status), _stream_handle(stream))
    return d_words


def _words_host(name, data):
    """The host twins that give one 32-bit word per packet (estimate, scan word): a list of ints."""
    data = bytes(data)
    words = (C.c_uint32 * max(packet_count(len(data)), 1))()
    _call(name, data, len(data), words)
    return list(words)[:packet_count(len(data))]


def _first_bad_ptr(d_first_bad):
    if d_first_bad is None:
        return None
    import torch
    if not (isinstance(d_first_bad, torch.Tensor) and d_first_bad.is_cuda and d_first_bad.element_size() == 8 and d_first_bad.numel() >= 1):
        raise GpuarError("d_first_bad must be a CUDA tensor of one 64-bit word")
    return d_first_bad.data_ptr()


def crc32(d_in, n_bytes: int = None, d_crc=None, stream=None):
    """The CRC-32 (zlib.crc32) of every 8192-byte packet of the first `n_bytes` (default: all) bytes of `d_in`
    (gpuar_hip_crc32).  Returns d_crc: int32 CUDA tensor of packet_count(n_bytes) values (the uint32 bits; & 0xFFFFFFFF)."""
    return _words_single("gpuar_hip_crc32", d_in, n_bytes, d_crc, "d_crc", stream, whole=True)


def verify_crc32(d_out, d_crc, n_bytes: int = None, d_first_bad=None, d_status=None, stream=None):
    """Compare the packets of the first `n_bytes` (default: all) bytes of `d_out` with the CRCs `d_crc` (gpuar_hip_verify_crc32):
    a mismatch ORs STATUS_CHECKSUM into d_status (None: the fallback word) and takes the minimum of the packet index and
    d_first_bad (a 1-element int64 CUDA tensor the caller set to -1, i.e. UINT64_MAX), when given."""
    _require_cuda_u8(d_out, "d_out")
    n, npk = _span(d_out, n_bytes, "d_out")
    _require_crc(d_crc, "d_crc", npk)
    _call("gpuar_hip_verify_crc32", d_out.data_ptr(), n, d_crc.data_ptr(), _first_bad_ptr(d_first_bad), _status_ptr(d_status),
          _stream_handle(stream))


def crc32_batch(d_ptrs, d_bytes, d_first_packet, n_buffers: int, n_packets: int, d_crc=None, stream=None, d_status=None, device=None):
    """The CRC-32 of every packet of a batch (gpuar_hip_crc32_batch; descriptors as for encode_batch): d_crc[p] for batch packet p."""
    return _words_batch("gpuar_hip_crc32_batch", d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_crc, "d_crc", stream, d_status, device,
                        whole=True)


def verify_crc32_batch(d_ptrs, d_bytes, d_first_packet, n_buffers: int, n_packets: int, d_crc, d_first_bad=None, stream=None, d_status=None):
    """Verify a batch's decoded buffers against d_crc (gpuar_hip_verify_crc32_batch): d_bytes holds each buffer's ORIGINAL size;
    d_first_bad receives the lowest failing batch packet."""
    _require_batch(d_ptrs, d_bytes, d_first_packet, n_buffers)
    _require_crc(d_crc, "d_crc", n_packets)
    _call("gpuar_hip_verify_crc32_batch", d_ptrs.data_ptr(), d_bytes.data_ptr(), d_first_packet.data_ptr(), n_buffers, n_packets,
          d_crc.data_ptr(), _first_bad_ptr(d_first_bad), _status_ptr(d_status), _stream_handle(stream))


def _planes(name, d_in, elem_bytes, d_out, n_bytes, stream, *d_base):
    """One filter call on one buffer: planes and delta, and (with the one d_base) XOR.  Returns d_out."""
    import torch
    _require_cuda_u8(d_in, "d_in")
    for base in d_base:
        _require_cuda_u8(base, "d_base")
    n, _npk = _span(d_in, n_bytes)
    if any(n > base.numel() for base in d_base):
        raise GpuarError("d_base too small")
    if d_out is None:
        d_out = torch.empty(max(n, 1), dtype=torch.uint8, device=d_in.device)[:n]
    _require_cuda_u8(d_out, "d_out")
    if d_out.numel() < n:
        raise GpuarError("d_out too small")
    _call(name, d_in.data_ptr(), *(base.data_ptr() for base in d_base), n, elem_bytes, d_out.data_ptr(), _stream_handle(stream))
    return d_out


def split_planes(d_in, elem_bytes: int, d_out=None, n_bytes: int = None, stream=None):
    """Regroup the first `n_bytes` (default: all) bytes of `d_in`, taken as elements of `elem_bytes` bytes (1, 2, 4, 8), into byte
    planes (gpuar_hip_split_planes; the map is in include/gpuar_hip.h): packet k of every group of elem_bytes packets holds
    byte k of the group's 8192 elements.  `d_out` may be `d_in`.  Returns d_out."""
    return _planes("gpuar_hip_split_planes", d_in, elem_bytes, d_out, n_bytes, stream)


def merge_planes(d_in, elem_bytes: int, d_out=None, n_bytes: int = None, stream=None):
    """The inverse of split_planes (gpuar_hip_merge_planes); `d_out` may be `d_in`."""
    return _planes("gpuar_hip_merge_planes", d_in, elem_bytes, d_out, n_bytes, stream)


def _filter_batch(name, d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, stream, d_status, *extra):
    """One filter call on a batch; `extra`: the (tensor, name) that delta (d_filter) and XOR (d_base_ptrs) add behind d_elem_bytes."""
    _require_batch(d_in_ptrs, d_bytes, d_first_packet, n_buffers, "d_in_ptrs", ((d_elem_bytes, "d_elem_bytes"), *extra, (d_out_ptrs, "d_out_ptrs")))
    _call(name, d_in_ptrs.data_ptr(), d_bytes.data_ptr(), d_first_packet.data_ptr(), d_elem_bytes.data_ptr(), *(t.data_ptr() for t, _what in extra),
          n_buffers, n_packets, d_out_ptrs.data_ptr(), _status_ptr(d_status), _stream_handle(stream))


def split_planes_batch(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers: int, n_packets: int, d_out_ptrs, stream=None, d_status=None):
    """split_planes for every buffer of a batch in one call (gpuar_hip_split_planes_batch; descriptors as for encode_batch, plus
    one element width per buffer): buffer b goes from d_in_ptrs[b] to d_out_ptrs[b], which may be the same."""
    _filter_batch("gpuar_hip_split_planes_batch", d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, stream, d_status)


def merge_planes_batch(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers: int, n_packets: int, d_out_ptrs, stream=None, d_status=None):
    """The inverse of split_planes_batch (gpuar_hip_merge_planes_batch)."""
    _filter_batch("gpuar_hip_merge_planes_batch", d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, stream, d_status)


def _planes_host(name, data, elem_bytes):
    data = bytes(data)
    out = C.create_string_buffer(len(data))
    _call(name, data, len(data), elem_bytes, out)
    return out.raw


def split_planes_host(data, elem_bytes: int) -> bytes:
    """split_planes of a bytes-like object on the CPU (gpuar_hip_split_planes_host: no device is touched)."""
    return _planes_host("gpuar_hip_split_planes_host", data, elem_bytes)


def merge_planes_host(data, elem_bytes: int) -> bytes:
    """merge_planes of a bytes-like object on the CPU (gpuar_hip_merge_planes_host)."""
    return _planes_host("gpuar_hip_merge_planes_host", data, elem_bytes)


def split_delta(d_in, elem_bytes: int, d_out=None, n_bytes: int = None, stream=None):
    """split_planes of the element-wise differences (gpuar_hip_split_delta; include/gpuar_hip.h): inside every group of
    elem_bytes packets the elements, as little-endian unsigned integers of elem_bytes bytes (1, 2, 4, 8), are replaced by their
    difference to the element in front (mod 2^(8 elem_bytes); the first stays) and then regrouped into byte planes, in one pass.
    elem_bytes = 1 is a byte delta per packet.  `d_out` may be `d_in`.  Returns d_out."""
    return _planes("gpuar_hip_split_delta", d_in, elem_bytes, d_out, n_bytes, stream)


def merge_delta(d_in, elem_bytes: int, d_out=None, n_bytes: int = None, stream=None):
    """The inverse of split_delta (gpuar_hip_merge_delta): merge_planes, then the prefix sum inside every group; `d_out` may
    be `d_in`."""
    return _planes("gpuar_hip_merge_delta", d_in, elem_bytes, d_out, n_bytes, stream)


def split_delta_batch(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_filter, n_buffers: int, n_packets: int, d_out_ptrs, stream=None,
                      d_status=None):
    """split_planes_batch with a filter per buffer (gpuar_hip_split_delta_batch): d_filter[b] = 0 regroups buffer b as
    split_planes_batch does, 1 as split_delta; any other value is BAD_BATCH and the buffer is left alone."""
    _filter_batch("gpuar_hip_split_delta_batch", d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, stream, d_status,
                  (d_filter, "d_filter"))


def merge_delta_batch(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_filter, n_buffers: int, n_packets: int, d_out_ptrs, stream=None,
                      d_status=None):
    """The inverse of split_delta_batch (gpuar_hip_merge_delta_batch)."""
    _filter_batch("gpuar_hip_merge_delta_batch", d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, stream, d_status,
                  (d_filter, "d_filter"))


def split_delta_host(data, elem_bytes: int) -> bytes:
    """split_delta of a bytes-like object on the CPU (gpuar_hip_split_delta_host: no device is touched)."""
    return _planes_host("gpuar_hip_split_delta_host", data, elem_bytes)


def merge_delta_host(data, elem_bytes: int) -> bytes:
    """merge_delta of a bytes-like object on the CPU (gpuar_hip_merge_delta_host)."""
    return _planes_host("gpuar_hip_merge_delta_host", data, elem_bytes)


def delta_block_host(mixed, elem_bytes: int, undo: bool, carried: int):
    """One block of 16 elements (`mixed`: 4 * elem_bytes dwords) through the kernels' register transform, run on the CPU
    (gpuar_hip_delta_block_host): undo=False gives delta_block's differences with `carried` as the element in front; undo=True
    undelta_block's prefix sums plus `carried`.  Returns (dwords, the block's total -- 0 for undo=False)."""
    mixed = list(mixed)
    if len(mixed) != 4 * elem_bytes:
        raise GpuarError(f"delta_block_host: {len(mixed)} dwords for a width of {elem_bytes}")
    block = (C.c_uint32 * len(mixed))(*mixed)
    total = C.c_uint64(0)
    _call("gpuar_hip_delta_block_host", block, elem_bytes, 1 if undo else 0, carried & (2 ** 64 - 1), C.byref(total))
    return list(block), total.value


def split_xor(d_in, d_base, elem_bytes: int, d_out=None, n_bytes: int = None, stream=None):
    """split_planes of d_in ^ d_base (gpuar_hip_split_xor; include/gpuar_hip.h), in one pass: every byte of the first `n_bytes`
    is XORed with the same byte of the base, then the bytes are regrouped as elements of `elem_bytes` bytes (1, 2, 4, 8);
    elem_bytes = 1 is a plain XOR.  `d_out` may be `d_in`, never the base.  Returns d_out."""
    return _planes("gpuar_hip_split_xor", d_in, elem_bytes, d_out, n_bytes, stream, d_base)


def merge_xor(d_in, d_base, elem_bytes: int, d_out=None, n_bytes: int = None, stream=None):
    """The inverse of split_xor with the same base (gpuar_hip_merge_xor): merge_planes, then the XOR; `d_out` may be `d_in`."""
    return _planes("gpuar_hip_merge_xor", d_in, elem_bytes, d_out, n_bytes, stream, d_base)


def split_xor_batch(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_base_ptrs, n_buffers: int, n_packets: int, d_out_ptrs, stream=None,
                    d_status=None):
    """split_planes_batch with a base per buffer (gpuar_hip_split_xor_batch): d_base_ptrs[b] = 0 regroups buffer b as
    split_planes_batch does, a 16-byte aligned pointer as split_xor against the d_bytes[b] bytes there; a misaligned one is
    BAD_BATCH and the buffer is left alone."""
    _filter_batch("gpuar_hip_split_xor_batch", d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, stream, d_status,
                  (d_base_ptrs, "d_base_ptrs"))


def merge_xor_batch(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_base_ptrs, n_buffers: int, n_packets: int, d_out_ptrs, stream=None,
                    d_status=None):
    """The inverse of split_xor_batch (gpuar_hip_merge_xor_batch)."""
    _filter_batch("gpuar_hip_merge_xor_batch", d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, stream, d_status,
                  (d_base_ptrs, "d_base_ptrs"))


def _xor_host(name, data, base, elem_bytes):
    data, base = bytes(data), bytes(base)
    if len(base) != len(data):
        raise GpuarError(f"{name}: a base of {len(base)} bytes for {len(data)} bytes")
    out = C.create_string_buffer(len(data))
    _call(name, data, base, len(data), elem_bytes, out)
    return out.raw


def split_xor_host(data, base, elem_bytes: int) -> bytes:
    """split_xor of two bytes-like objects of one length on the CPU (gpuar_hip_split_xor_host: no device is touched)."""
    return _xor_host("gpuar_hip_split_xor_host", data, base, elem_bytes)


def merge_xor_host(data, base, elem_bytes: int) -> bytes:
    """merge_xor of two bytes-like objects of one length on the CPU (gpuar_hip_merge_xor_host)."""
    return _xor_host("gpuar_hip_merge_xor_host", data, base, elem_bytes)


def estimate(d_in, n_bytes: int = None, d_est=None, stream=None):
    """The predicted clen (header included) of every 8192-byte packet of the first `n_bytes` (default: all) bytes of `d_in`, from
    the packet's byte histogram alone (gpuar_hip_estimate; the definition is in include/gpuar_hip.h).  Returns d_est: int32 CUDA
    tensor of packet_count(n_bytes) values.  A packet is worth storing raw iff est[p] >= 4 + ulen[p] (stored_rule)."""
    return _words_single("gpuar_hip_estimate", d_in, n_bytes, d_est, "d_est", stream)


def estimate_batch(d_ptrs, d_bytes, d_first_packet, n_buffers: int, n_packets: int, d_est=None, stream=None, d_status=None, device=None):
    """The estimate of every packet of a batch (gpuar_hip_estimate_batch; descriptors as for encode_batch): d_est[p] for batch
    packet p."""
    return _words_batch("gpuar_hip_estimate_batch", d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_est, "d_est", stream, d_status, device)


def estimate_host(data) -> list:
    """estimate of a bytes-like object on the CPU (gpuar_hip_estimate_host: no device is touched): one int per packet."""
    return _words_host("gpuar_hip_estimate_host", data)


def _survey_rows(d_est, npk, device):
    """A survey's output of shape (4, stride), stride >= npk: the caller's contiguous 4-byte CUDA tensor, or a new int32 one of (4, npk)."""
    import torch
    if d_est is None:
        d_est = torch.empty((len(SURVEY_WIDTHS), npk), dtype=torch.int32, device=device)
    if not (isinstance(d_est, torch.Tensor) and d_est.is_cuda and d_est.element_size() == 4 and d_est.is_contiguous() and d_est.dim() == 2
            and d_est.shape[0] == len(SURVEY_WIDTHS) and d_est.shape[1] >= npk):
        raise GpuarError(f"d_est must be a contiguous 32-bit CUDA tensor of shape (4, at least {npk})")
    return d_est


def _survey(name, d_in, d_est, n_bytes, stream, *mask):
    """Either survey of one buffer; `mask`: the delta survey's widths_mask.  Returns d_est."""
    n, npk = _span(d_in, n_bytes)
    d_est = _survey_rows(d_est, npk, d_in.device)
    _call(name, d_in.data_ptr(), n, *mask, d_est.data_ptr(), d_est.shape[1], _stream_handle(stream))
    return d_est


def _survey_batch(name, d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_est, stream, d_status, device, *mask):
    """Either survey of a batch.  Returns d_est."""
    _require_batch(d_ptrs, d_bytes, d_first_packet, n_buffers)
    d_est = _survey_rows(d_est, n_packets, device or d_ptrs.device)
    _call(name, d_ptrs.data_ptr(), d_bytes.data_ptr(), d_first_packet.data_ptr(), n_buffers, n_packets, *mask, d_est.data_ptr(), d_est.shape[1],
          _status_ptr(d_status), _stream_handle(stream))
    return d_est


def _survey_host(name, data, *mask):
    """Either survey on the CPU: four lists, one per width of SURVEY_WIDTHS, of one int per packet."""
    data = bytes(data)
    npk = packet_count(len(data))
    est = (C.c_uint32 * max(len(SURVEY_WIDTHS) * npk, 1))()
    _call(name, data, len(data), *mask, est, npk)
    return [list(est[j * npk:(j + 1) * npk]) for j in range(len(SURVEY_WIDTHS))]


def survey_planes(d_in, d_est=None, n_bytes: int = None, stream=None):
    """The estimate of every packet of the first `n_bytes` (default: all) bytes of `d_in` split into byte planes of width 1, 2, 4
    and 8, from one read of the bytes and without splitting anything (gpuar_hip_survey_planes): row j of the result is what
    estimate(split_planes(d_in, SURVEY_WIDTHS[j])) gives.  Returns d_est: int32 CUDA tensor of shape (4, packet_count(n_bytes))
    (the caller's may be wider: its second dimension is the row stride)."""
    _require_cuda_u8(d_in, "d_in")
    return _survey("gpuar_hip_survey_planes", d_in, d_est, n_bytes, stream)


def survey_planes_batch(d_ptrs, d_bytes, d_first_packet, n_buffers: int, n_packets: int, d_est=None, stream=None, d_status=None, device=None):
    """The survey of every buffer of a batch in one launch (gpuar_hip_survey_planes_batch; descriptors as for encode_batch):
    d_est[j, p] for width SURVEY_WIDTHS[j] and batch packet p."""
    return _survey_batch("gpuar_hip_survey_planes_batch", d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_est, stream, d_status, device)


def survey_planes_host(data) -> list:
    """survey_planes of a bytes-like object on the CPU (gpuar_hip_survey_planes_host: no device is touched): four lists, one per
    width of SURVEY_WIDTHS, of one int per packet."""
    return _survey_host("gpuar_hip_survey_planes_host", data)


def choose_planes(totals, n_packets: int) -> int:
    """The width to split by, from the four predicted totals at widths 1, 2, 4, 8 (gpuar_hip_choose_planes): the smallest width
    whose total is at most the lowest total + n_packets."""
    totals = [int(t) for t in totals]
    if len(totals) != len(SURVEY_WIDTHS) or min(totals) < 0:
        raise GpuarError(f"choose_planes: four non-negative totals, not {totals}")
    return int(load().gpuar_hip_choose_planes((C.c_uint64 * 4)(*totals), n_packets))


def widths_mask(widths) -> int:
    """The widths_mask of the delta survey: bit j for width SURVEY_WIDTHS[j]; anything but a non-empty set of 1, 2, 4, 8 raises."""
    widths = list(widths)
    if not widths or any(w not in SURVEY_WIDTHS for w in widths):
        raise GpuarError(f"widths={widths}: a non-empty selection of {SURVEY_WIDTHS}")
    mask = 0
    for w in widths:
        mask |= 1 << SURVEY_WIDTHS.index(w)
    return mask


def survey_delta(d_in, d_est=None, n_bytes: int = None, stream=None, widths=SURVEY_WIDTHS):
    """The estimate of every packet of the first `n_bytes` (default: all) bytes of `d_in` filtered (delta) and split into byte
    planes of each width of `widths`, from one read of the bytes and without filtering or splitting anything into memory
    (gpuar_hip_survey_delta): row j of the result is what estimate(split_delta(d_in, SURVEY_WIDTHS[j])) gives.  Returns d_est:
    int32 CUDA tensor of shape (4, packet_count(n_bytes)) (the caller's may be wider: its second dimension is the row stride);
    the rows of widths that were not asked for are left as they were."""
    _require_cuda_u8(d_in, "d_in")
    return _survey("gpuar_hip_survey_delta", d_in, d_est, n_bytes, stream, widths_mask(widths))


def survey_delta_batch(d_ptrs, d_bytes, d_first_packet, n_buffers: int, n_packets: int, d_est=None, stream=None, d_status=None, device=None,
                       widths=SURVEY_WIDTHS):
    """The delta survey of every buffer of a batch in one launch (gpuar_hip_survey_delta_batch; descriptors as for encode_batch):
    d_est[j, p] for every width SURVEY_WIDTHS[j] of `widths` and batch packet p; the other rows are left as they were."""
    return _survey_batch("gpuar_hip_survey_delta_batch", d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_est, stream, d_status, device,
                         widths_mask(widths))


def survey_delta_host(data, widths=SURVEY_WIDTHS) -> list:
    """survey_delta of a bytes-like object on the CPU (gpuar_hip_survey_delta_host: no device is touched): four entries, one per
    width of SURVEY_WIDTHS -- a list of one int per packet, or None for a width that was not asked for."""
    data = bytes(data)
    mask = widths_mask(widths)
    rows = _survey_host("gpuar_hip_survey_delta_host", data, mask)
    return [row if mask >> j & 1 else None for j, row in enumerate(rows)]


def choose_filter(plain, filtered, n_packets: int) -> tuple:
    """(width, filter) from the four totals of the plane survey and the four of the delta survey (gpuar_hip_choose_filter): the
    filter at the width choose_planes picks from `filtered` iff that total + n_packets is at most the total of the width
    choose_planes picks from `plain`; else that width and no filter."""
    plain, filtered = [int(t) for t in plain], [int(t) for t in filtered]
    if len(plain) != len(SURVEY_WIDTHS) or len(filtered) != len(SURVEY_WIDTHS) or min(plain + filtered) < 0:
        raise GpuarError(f"choose_filter: two lists of four non-negative totals, not {plain} and {filtered}")
    width = C.c_uint32(0)
    on = load().gpuar_hip_choose_filter((C.c_uint64 * 4)(*plain), (C.c_uint64 * 4)(*filtered), n_packets, C.byref(width))
    return int(width.value), bool(on)


def _xsurvey_rows(d_est, d_scan, npk, device):
    """The two outputs of the XOR survey, each as _survey_rows takes it (None: a new tensor) or False for "not asked"; both of one
    row stride.  Returns the tensors (None for one not asked) and the stride."""
    if d_est is False and d_scan is False:
        raise GpuarError("survey_xor: d_est and d_scan cannot both be left out")
    d_est = None if d_est is False else _survey_rows(d_est, npk, device)
    d_scan = None if d_scan is False else _survey_rows(d_scan, npk, device)
    if d_est is not None and d_scan is not None and d_est.shape[1] != d_scan.shape[1]:
        raise GpuarError(f"d_est and d_scan must have one row stride, not {d_est.shape[1]} and {d_scan.shape[1]}")
    return d_est, d_scan, (d_est if d_est is not None else d_scan).shape[1]


def _ptr_or_null(t):
    return None if t is None else t.data_ptr()


def survey_xor(d_in, d_base, d_est=None, d_scan=None, n_bytes: int = None, stream=None):
    """The estimate and the sparse scan word of every packet of the first `n_bytes` (default: all) bytes of `d_in` XORed with
    `d_base` and split into byte planes of width 1, 2, 4 and 8, from one read of both and without XORing or splitting anything into
    memory (gpuar_hip_survey_xor): row j of d_est is what estimate(split_xor(d_in, d_base, SURVEY_WIDTHS[j])) gives, row j of d_scan
    what sparse_scan of it gives.  Returns (d_est, d_scan): int32 CUDA tensors of shape (4, packet_count(n_bytes)) (the caller's
    may be wider: their second dimension is the row stride, the same for both).  False for d_est or d_scan leaves that output out
    (None is returned in its place); not both."""
    _require_cuda_u8(d_in, "d_in")
    _require_cuda_u8(d_base, "d_base")
    n, npk = _span(d_in, n_bytes)
    if n > d_base.numel():
        raise GpuarError("n_bytes is larger than d_base")
    d_est, d_scan, stride = _xsurvey_rows(d_est, d_scan, npk, d_in.device)
    _call("gpuar_hip_survey_xor", d_in.data_ptr(), d_base.data_ptr(), n, _ptr_or_null(d_est), _ptr_or_null(d_scan), stride, _stream_handle(stream))
    return d_est, d_scan


def survey_xor_batch(d_ptrs, d_bytes, d_first_packet, d_base_ptrs, n_buffers: int, n_packets: int, d_est=None, d_scan=None, stream=None,
                     d_status=None, device=None):
    """The XOR survey of every buffer of a batch in one launch (gpuar_hip_survey_xor_batch; descriptors as for encode_batch, and
    d_base_ptrs: one base address per buffer, 0 for "no base" -- that buffer's rows are the plane survey's): d_est[j, p] and
    d_scan[j, p] for width SURVEY_WIDTHS[j] and batch packet p.  Outputs as for survey_xor."""
    _require_batch(d_ptrs, d_bytes, d_first_packet, n_buffers, more=((d_base_ptrs, "d_base_ptrs"),))
    d_est, d_scan, stride = _xsurvey_rows(d_est, d_scan, n_packets, device or d_ptrs.device)
    _call("gpuar_hip_survey_xor_batch", d_ptrs.data_ptr(), d_bytes.data_ptr(), d_first_packet.data_ptr(), d_base_ptrs.data_ptr(), n_buffers,
          n_packets, _ptr_or_null(d_est), _ptr_or_null(d_scan), stride, _status_ptr(d_status), _stream_handle(stream))
    return d_est, d_scan


def survey_xor_host(data, base, est: bool = True, scan: bool = True) -> tuple:
    """survey_xor of two bytes-like objects of one length on the CPU (gpuar_hip_survey_xor_host: no device is touched): (est, scan),
    each four lists, one per width of SURVEY_WIDTHS, of one int per packet -- or None where est / scan is False."""
    data, base = bytes(data), bytes(base)
    if len(data) != len(base):
        raise GpuarError(f"survey_xor_host: {len(data)} bytes against a base of {len(base)}")
    if not est and not scan:
        raise GpuarError("survey_xor_host: est and scan cannot both be left out")
    npk = packet_count(len(data))
    words = [(C.c_uint32 * max(len(SURVEY_WIDTHS) * npk, 1))() if on else None for on in (est, scan)]
    _call("gpuar_hip_survey_xor_host", data, base, len(data), words[0], words[1], npk)
    return tuple(None if w is None else [list(w[j * npk:(j + 1) * npk]) for j in range(len(SURVEY_WIDTHS))] for w in words)


def mode_count(n_bytes: int) -> int:
    """The modes of a buffer of n_bytes bytes: one per supergroup of 65536 bytes (gpuar_hip_mode_count)."""
    return (n_bytes + SUPERGROUP - 1) // SUPERGROUP


def batch_mode_count(sizes):
    """(first_mode as a list of n + 1 ints, mode count) for buffers of `sizes` bytes (gpuar_hip_batch_mode_count)."""
    n = len(sizes)
    arr = (C.c_uint64 * max(n, 1))(*sizes)
    fm = (C.c_uint64 * (n + 1))()
    total = load().gpuar_hip_batch_mode_count(arr, n, fm)
    return list(fm), int(total)


def mode_parts(mode: int) -> tuple:
    """(width, delta, base) of a mode byte; anything but 0 .. 11 raises."""
    if not 0 <= mode < MIXED_MODES:
        raise GpuarError(f"mode {mode}: the modes are 0 .. {MIXED_MODES - 1}")
    return 1 << (mode & 3), mode >> 2 == 1, mode >> 2 == 2


def choose_mode(plain, delta, xored, n_packets: int) -> tuple:
    """(mode, its predicted total) of one supergroup from its four totals at widths 1, 2, 4, 8 as planes alone, with the delta
    filter (None: not offered) and against the base (None: not offered) (gpuar_hip_choose_mode): choose_filter(plain, delta) --
    without delta, choose_planes(plain) --, then the base at choose_planes(xored) iff that total + n_packets is at most the total
    chosen so far."""
    rows = []
    for name, t in (("plain", plain), ("delta", delta), ("xored", xored)):
        if t is None and name != "plain":
            rows.append(None)
            continue
        t = [int(v) for v in t]
        if len(t) != len(SURVEY_WIDTHS) or min(t) < 0:
            raise GpuarError(f"choose_mode: {name} is four non-negative totals, not {t}")
        rows.append((C.c_uint64 * 4)(*t))
    total = C.c_uint64(0)
    mode = load().gpuar_hip_choose_mode(rows[0], rows[1], rows[2], n_packets, C.byref(total))
    if mode < 0:
        _check(mode, "gpuar_hip_choose_mode")
    return int(mode), int(total.value)


def _require_modes(d_modes, n):
    import torch
    if not (isinstance(d_modes, torch.Tensor) and d_modes.is_cuda and d_modes.dtype == torch.uint8 and d_modes.is_contiguous() and d_modes.numel() >= n):
        raise GpuarError(f"d_modes must be a contiguous uint8 CUDA tensor of at least {n} modes")


def _rows_ptr(d_rows, npk):
    """The address of a survey's rows for choose_modes (None: not offered) and their stride"""
    if d_rows is None:
        return None, None
    d_rows = _survey_rows(d_rows, npk, None)
    return d_rows.data_ptr(), d_rows.shape[1]


def _choose_rows(d_plain, d_delta, d_xored, npk):
    """The three row pointers of a choose_modes call and their one stride"""
    if d_plain is None:
        raise GpuarError("choose_modes needs the plane survey's rows")
    found = [_rows_ptr(t, npk) for t in (d_plain, d_delta, d_xored)]
    strides = {stride for _ptr, stride in found if stride is not None}
    if len(strides) != 1:
        raise GpuarError(f"the surveys' rows must have one row stride, not {sorted(strides)}")
    return [ptr for ptr, _stride in found], strides.pop()


def _choose_outputs(d_modes, d_totals, n_modes, device):
    import torch
    if d_modes is None:
        d_modes = torch.empty(max(n_modes, 1), dtype=torch.uint8, device=device)[:n_modes]
    _require_modes(d_modes, n_modes)
    return d_modes, _words(d_totals, "d_totals", n_modes, device)


def choose_modes(d_plain, d_delta, d_xored, n_bytes: int, d_modes=None, d_totals=None, stream=None, d_status=None):
    """The mode and the predicted total of every supergroup of one buffer of n_bytes bytes from the rows survey_planes, survey_delta
    (all four widths) and survey_xor (its d_est) gave for it (gpuar_hip_choose_modes; d_delta, d_xored: None where that filter is
    not offered; the rows have one stride).  Returns (d_modes: uint8 CUDA tensor of mode_count(n_bytes), d_totals: int32)."""
    ptrs, stride = _choose_rows(d_plain, d_delta, d_xored, packet_count(n_bytes))
    d_modes, d_totals = _choose_outputs(d_modes, d_totals, mode_count(n_bytes), d_plain.device)
    _call("gpuar_hip_choose_modes", *ptrs, stride, n_bytes, d_modes.data_ptr(), d_totals.data_ptr(), _status_ptr(d_status), _stream_handle(stream))
    return d_modes, d_totals


def choose_modes_batch(d_plain, d_delta, d_xored, d_bytes, d_first_packet, d_first_mode, n_buffers: int, n_packets: int, n_modes: int,
                       d_modes=None, d_totals=None, stream=None, d_status=None):
    """choose_modes for every buffer of a batch in one launch (gpuar_hip_choose_modes_batch): the rows are the batch surveys',
    d_first_mode (64-bit CUDA tensor) what batch_mode_count gives, supergroup s of buffer b gets entry d_first_mode[b] + s."""
    for t, name, n in ((d_bytes, "d_bytes", n_buffers), (d_first_packet, "d_first_packet", n_buffers + 1), (d_first_mode, "d_first_mode", n_buffers)):
        _require_u64_desc(t, name, n)
    ptrs, stride = _choose_rows(d_plain, d_delta, d_xored, n_packets)
    d_modes, d_totals = _choose_outputs(d_modes, d_totals, n_modes, d_plain.device)
    _call("gpuar_hip_choose_modes_batch", *ptrs, stride, d_bytes.data_ptr(), d_first_packet.data_ptr(), d_first_mode.data_ptr(), n_buffers, n_packets,
          n_modes, d_modes.data_ptr(), d_totals.data_ptr(), _status_ptr(d_status), _stream_handle(stream))
    return d_modes, d_totals


def choose_modes_host(plain, delta, xored, n_bytes: int) -> tuple:
    """choose_modes on the CPU (gpuar_hip_choose_modes_host: no device is touched) from what survey_planes_host, survey_delta_host
    and survey_xor_host's est gave (four lists of one int per packet each; delta, xored: None where not offered): (modes as bytes,
    the predicted totals as a list)."""
    npk, n_modes = packet_count(n_bytes), mode_count(n_bytes)
    rows = []
    for name, r in (("plain", plain), ("delta", delta), ("xored", xored)):
        if r is None and name != "plain":
            rows.append(None)
            continue
        if len(r) != len(SURVEY_WIDTHS) or any(row is None or len(row) != npk for row in r):
            raise GpuarError(f"choose_modes_host: {name} is four rows of {npk} estimates")
        rows.append((C.c_uint32 * max(len(SURVEY_WIDTHS) * npk, 1))(*(v for row in r for v in row)))
    modes, totals = (C.c_uint8 * max(n_modes, 1))(), (C.c_uint32 * max(n_modes, 1))()
    _call("gpuar_hip_choose_modes_host", rows[0], rows[1], rows[2], npk, n_bytes, modes, totals)
    return bytes(modes[:n_modes]), list(totals[:n_modes])


def _mixed(name, d_in, d_modes, d_base, d_out, n_bytes, stream, d_status):
    import torch
    _require_cuda_u8(d_in, "d_in")
    n, _npk = _span(d_in, n_bytes)
    if d_base is not None:
        _require_cuda_u8(d_base, "d_base")
        if n > d_base.numel():
            raise GpuarError("d_base too small")
    _require_modes(d_modes, mode_count(n))
    if d_out is None:
        d_out = torch.empty(max(n, 1), dtype=torch.uint8, device=d_in.device)[:n]
    _require_cuda_u8(d_out, "d_out")
    if d_out.numel() < n:
        raise GpuarError("d_out too small")
    _call(name, d_in.data_ptr(), _ptr_or_null(d_base), n, d_modes.data_ptr(), d_out.data_ptr(), _status_ptr(d_status), _stream_handle(stream))
    return d_out


def split_mixed(d_in, d_modes, d_base=None, d_out=None, n_bytes: int = None, stream=None, d_status=None):
    """Split the first `n_bytes` (default: all) bytes of `d_in` supergroup by supergroup (gpuar_hip_split_mixed; include/gpuar_hip_mixed.h):
    supergroup s -- 65536 bytes, the last one maybe fewer -- as split_planes, split_delta or split_xor (against the same bytes of
    `d_base`) would split it alone, at the width and with the filter d_modes[s] says (mode_parts).  `d_out` may be `d_in`, never
    the base.  A mode that is not valid, or asks for a base where there is none, is STATUS_BAD_BATCH and leaves its supergroup
    alone.  Returns d_out."""
    return _mixed("gpuar_hip_split_mixed", d_in, d_modes, d_base, d_out, n_bytes, stream, d_status)


def merge_mixed(d_in, d_modes, d_base=None, d_out=None, n_bytes: int = None, stream=None, d_status=None):
    """The inverse of split_mixed with the same modes and base (gpuar_hip_merge_mixed); `d_out` may be `d_in`."""
    return _mixed("gpuar_hip_merge_mixed", d_in, d_modes, d_base, d_out, n_bytes, stream, d_status)


def _mixed_batch(name, d_in_ptrs, d_bytes, d_first_packet, d_first_mode, d_modes, d_base_ptrs, n_buffers, n_packets, d_out_ptrs, stream, d_status):
    _require_batch(d_in_ptrs, d_bytes, d_first_packet, n_buffers, "d_in_ptrs",
                   ((d_first_mode, "d_first_mode"), (d_base_ptrs, "d_base_ptrs"), (d_out_ptrs, "d_out_ptrs")))
    _require_modes(d_modes, 0)
    _call(name, d_in_ptrs.data_ptr(), d_bytes.data_ptr(), d_first_packet.data_ptr(), d_first_mode.data_ptr(), d_modes.data_ptr(),
          d_base_ptrs.data_ptr(), n_buffers, n_packets, d_out_ptrs.data_ptr(), _status_ptr(d_status), _stream_handle(stream))


def split_mixed_batch(d_in_ptrs, d_bytes, d_first_packet, d_first_mode, d_modes, d_base_ptrs, n_buffers: int, n_packets: int, d_out_ptrs,
                      stream=None, d_status=None):
    """split_mixed for every buffer of a batch in one call (gpuar_hip_split_mixed_batch; descriptors as for split_xor_batch, with
    d_first_mode -- where buffer b's modes begin in d_modes, batch_mode_count -- in the widths' place; d_base_ptrs[b] = 0: no base)."""
    _mixed_batch("gpuar_hip_split_mixed_batch", d_in_ptrs, d_bytes, d_first_packet, d_first_mode, d_modes, d_base_ptrs, n_buffers, n_packets,
                 d_out_ptrs, stream, d_status)


def merge_mixed_batch(d_in_ptrs, d_bytes, d_first_packet, d_first_mode, d_modes, d_base_ptrs, n_buffers: int, n_packets: int, d_out_ptrs,
                      stream=None, d_status=None):
    """The inverse of split_mixed_batch (gpuar_hip_merge_mixed_batch)."""
    _mixed_batch("gpuar_hip_merge_mixed_batch", d_in_ptrs, d_bytes, d_first_packet, d_first_mode, d_modes, d_base_ptrs, n_buffers, n_packets,
                 d_out_ptrs, stream, d_status)


def _mixed_host(name, data, modes, base):
    data, modes = bytes(data), bytes(modes)
    if base is not None:
        base = bytes(base)
        if len(base) != len(data):
            raise GpuarError(f"{name}: a base of {len(base)} bytes for {len(data)} bytes")
    if len(modes) != mode_count(len(data)):
        raise GpuarError(f"{name}: {len(modes)} modes for {mode_count(len(data))} supergroups")
    out = C.create_string_buffer(len(data))
    _call(name, data, base, len(data), modes, out)
    return out.raw


def split_mixed_host(data, modes, base=None) -> bytes:
    """split_mixed of a bytes-like object on the CPU (gpuar_hip_split_mixed_host: no device is touched); `modes`: one byte per
    supergroup; a mode that is not valid, or a base mode without `base`, raises."""
    return _mixed_host("gpuar_hip_split_mixed_host", data, modes, base)


def merge_mixed_host(data, modes, base=None) -> bytes:
    """merge_mixed of a bytes-like object on the CPU (gpuar_hip_merge_mixed_host)."""
    return _mixed_host("gpuar_hip_merge_mixed_host", data, modes, base)


def stored_rule(est: int, ulen: int) -> bool:
    """Whether a packet of `ulen` bytes with estimate `est` is kept raw instead of coded (include/gpuar_hip.h)."""
    return est >= 4 + ulen


def move_packets(d_src_ptrs, d_dst_ptrs, d_bytes, n_regions: int, stream=None, d_status=None):
    """Copy n_regions regions of d_bytes[r] <= 8192 bytes from d_src_ptrs[r] to d_dst_ptrs[r], all 16-byte aligned
    (gpuar_hip_move_packets; the three descriptors are 64-bit CUDA tensors)."""
    for t, name in ((d_src_ptrs, "d_src_ptrs"), (d_dst_ptrs, "d_dst_ptrs"), (d_bytes, "d_bytes")):
        _require_u64_desc(t, name, n_regions)
    _call("gpuar_hip_move_packets", d_src_ptrs.data_ptr(), d_dst_ptrs.data_ptr(), d_bytes.data_ptr(), n_regions, _status_ptr(d_status),
          _stream_handle(stream))


def move_bytes(d_src_ptrs, d_dst_ptrs, d_bytes, n_regions: int, stream=None, d_status=None):
    """Copy n_regions regions of d_bytes[r] <= 8704 bytes from d_src_ptrs[r] to d_dst_ptrs[r], both at any byte alignment
    (gpuar_hip_move_bytes, include/gpuar_hip_gip.h; the three descriptors are 64-bit CUDA tensors).  Nothing outside a region is
    read or written: destinations may stand back to back.  A null pointer or a longer region is STATUS_BAD_BATCH."""
    for t, name in ((d_src_ptrs, "d_src_ptrs"), (d_dst_ptrs, "d_dst_ptrs"), (d_bytes, "d_bytes")):
        _require_u64_desc(t, name, n_regions)
    _call("gpuar_hip_move_bytes", d_src_ptrs.data_ptr(), d_dst_ptrs.data_ptr(), d_bytes.data_ptr(), n_regions, _status_ptr(d_status),
          _stream_handle(stream))


# what gpuar_hip_gip_read_host / gpuar_hip_gip_tables_host return for a file they refuse (GPUAR_GIP_*): the sentence, with
# {p} the packet and {at} the file offset the defect was found at, {v} the trailer version and {n} the file's bytes
GIP_DEFECTS = {
    1: "{n} bytes are fewer than the 20 of a .gip header",
    2: "bytes 0 .. 2 are not the version 0.1.0 of a .gip header",
    3: "the header's compressed size (bytes 12 .. 19) is below 20 or beyond the file's {n} bytes",
    4: "the trailer at offset {at} says version {v} but cannot be used: it is damaged, or carries a width, a flag or a packet kind "
       "(above 2) this reader does not know -- not a file to read without it",
    5: "{p} packets (counted up to offset {at}) are not what the header's uncompressed size needs",
    6: "the packet stream ends inside packet {p} at offset {at}",
    7: "packet {p} at offset {at}: a clen below 4 or above 8704",
    8: "packet {p} at offset {at}: the header's clen is not the trailer's",
    9: "packet {p} at offset {at}: ulen is not the bytes the packet has in the file",
    10: "packet {p} at offset {at}: a kind above 2",
    11: "packet {p} at offset {at}: a raw packet whose clen is not 4 + ulen",
    12: "packet {p} at offset {at}: a sparse packet whose record head is not valid for its clen and ulen",
    13: "the packets' lengths end at offset {at}, not where the stream ends",
}


def _host_bytes(blob):
    """A bytes-like object (or a numpy / CPU torch uint8 array) as a contiguous read-only numpy uint8 view, without a copy."""
    import numpy as np
    if hasattr(blob, "numpy") and not isinstance(blob, np.ndarray):      # a CPU torch tensor
        blob = blob.numpy()
    arr = blob if isinstance(blob, np.ndarray) else np.frombuffer(blob, dtype=np.uint8)
    if arr.dtype != np.uint8 or arr.ndim != 1 or not arr.flags.c_contiguous:
        raise GpuarError("a .gip file in memory is a contiguous one-dimensional array of uint8")
    return arr


def gip_read_host(blob, what="the file"):
    """(info, clens, crcs or None, kinds or None) of a whole .gip file in memory, from the CLI's own reader
    (gpuar_hip_gip_read_host, gpuar_hip_gip_tables_host: no device is touched): info as include/gpuar_hip.h lists it, the tables
    as numpy arrays (uint16, uint32, uint8); crcs where the trailer has them, kinds where it is version 6.  Raises GpuarError
    naming `what`, the defect and where it is."""
    import numpy as np
    arr = _host_bytes(blob)
    lib = load()
    info = (C.c_uint64 * GIP_INFO_WORDS)()
    nothing = C.create_string_buffer(1)                        # (an empty blob has no address: it is refused as too short, not as null)
    ptr = arr.ctypes.data if arr.size else C.addressof(nothing)

    def refuse(code):
        if code in GIP_DEFECTS:
            raise GpuarError(f"{what}: " + GIP_DEFECTS[code].format(p=info[8], at=info[9], v=info[3], n=arr.size))
        _check(code, f"{what}: gpuar_hip_gip_read_host")
    refuse(lib.gpuar_hip_gip_read_host(ptr, arr.size, info))
    n = int(info[4])
    clens = np.zeros(n, dtype=np.uint16)
    crcs = np.zeros(n, dtype=np.uint32) if info[6] & 1 else None
    kinds = np.zeros(n, dtype=np.uint8) if info[3] == 6 else None
    refuse(lib.gpuar_hip_gip_tables_host(ptr, arr.size, clens.ctypes.data, crcs.ctypes.data if crcs is not None else None,
                                         kinds.ctypes.data if kinds is not None else None, n))
    return [int(v) for v in info], clens, crcs, kinds


SPARSE_NONE = 0xFFFFFFFF             # GPUAR_SPARSE_NONE: a packet without a majority byte
KIND_CODED, KIND_RAW, KIND_SPARSE = 0, 1, 2      # what gpuar_hip_sparse_rule returns; the values of batch.Compressed.stored


def sparse_len(k: int) -> int:
    """The bytes of a sparse record with k exceptions (gpuar_hip_sparse_len): (4 + 3 k + 3) & ~3."""
    return int(load().gpuar_hip_sparse_len(k))


def sparse_rule(scan: int, est: int, ulen: int, stored_on: bool) -> int:
    """What a packet of `ulen` bytes with scan word `scan` and estimate `est` is kept as: KIND_CODED, KIND_RAW or KIND_SPARSE
    (gpuar_hip_sparse_rule; the definition is in include/gpuar_hip.h)."""
    return int(load().gpuar_hip_sparse_rule(scan & 0xFFFFFFFF, est, ulen, int(bool(stored_on))))


def sparse_scan(d_in, n_bytes: int = None, d_scan=None, stream=None):
    """The scan word of every 8192-byte packet of the first `n_bytes` (default: all) bytes of `d_in` (gpuar_hip_sparse_scan):
    (k << 8) | f for a packet whose majority byte f leaves k exceptions, SPARSE_NONE (-1 as int32) for one without.  Returns
    d_scan: int32 CUDA tensor of packet_count(n_bytes) values."""
    return _words_single("gpuar_hip_sparse_scan", d_in, n_bytes, d_scan, "d_scan", stream)


def sparse_scan_batch(d_ptrs, d_bytes, d_first_packet, n_buffers: int, n_packets: int, d_scan=None, stream=None, d_status=None, device=None):
    """The scan word of every packet of a batch (gpuar_hip_sparse_scan_batch; descriptors as for encode_batch)."""
    return _words_batch("gpuar_hip_sparse_scan_batch", d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_scan, "d_scan", stream, d_status,
                        device)


def sparse_scan_host(data) -> list:
    """sparse_scan of a bytes-like object on the CPU (gpuar_hip_sparse_scan_host: no device is touched): one int per packet."""
    return _words_host("gpuar_hip_sparse_scan_host", data)


def sparse_pack_host(data) -> bytes:
    """The sparse record of one packet (1 .. 8192 bytes) on the CPU (gpuar_hip_sparse_pack_host); raises for a packet without a
    majority byte."""
    data = bytes(data)
    rec = (C.c_uint8 * (4 + 3 * (PACKET // 2) + 4))()
    length = C.c_size_t(0)
    _call("gpuar_hip_sparse_pack_host", data, len(data), rec, len(rec), C.byref(length))
    return bytes(rec[:length.value])


def sparse_unpack_host(rec, n_bytes: int) -> bytes:
    """The packet of `n_bytes` from its sparse record on the CPU (gpuar_hip_sparse_unpack_host); raises for a record that is
    not valid."""
    rec = bytes(rec)
    out = (C.c_uint8 * max(n_bytes, 1))()
    _call("gpuar_hip_sparse_unpack_host", rec, len(rec), out, n_bytes)
    return bytes(out[:n_bytes])


def sparse_pack(d_src_ptrs, d_bytes, d_scan, d_dst_ptrs, n_regions: int, stream=None, d_status=None):
    """Write the sparse records of n_regions packets: d_bytes[r] <= 8192 bytes at d_src_ptrs[r] (16-byte aligned) with the scan
    word d_scan[r] (int32) into sparse_len(d_scan[r] >> 8) bytes at d_dst_ptrs[r] (4-byte aligned) (gpuar_hip_sparse_pack; the
    pointers and sizes are 64-bit CUDA tensors)."""
    for t, name in ((d_src_ptrs, "d_src_ptrs"), (d_bytes, "d_bytes"), (d_dst_ptrs, "d_dst_ptrs")):
        _require_u64_desc(t, name, n_regions)
    _require_crc(d_scan, "d_scan", n_regions)
    _call("gpuar_hip_sparse_pack", d_src_ptrs.data_ptr(), d_bytes.data_ptr(), d_scan.data_ptr(), d_dst_ptrs.data_ptr(), n_regions,
          _status_ptr(d_status), _stream_handle(stream))


def sparse_unpack(d_rec_ptrs, d_rec_bytes, d_dst_ptrs, d_bytes, n_regions: int, stream=None, d_status=None):
    """Rebuild n_regions packets of d_bytes[r] <= 8192 bytes at d_dst_ptrs[r] (16-byte aligned) from their records of d_rec_bytes[r]
    bytes at d_rec_ptrs[r] (4-byte aligned) (gpuar_hip_sparse_unpack; the four descriptors are 64-bit CUDA tensors).  A record that
    is not valid is STATUS_BAD_PACKET in the status word."""
    for t, name in ((d_rec_ptrs, "d_rec_ptrs"), (d_rec_bytes, "d_rec_bytes"), (d_dst_ptrs, "d_dst_ptrs"), (d_bytes, "d_bytes")):
        _require_u64_desc(t, name, n_regions)
    _call("gpuar_hip_sparse_unpack", d_rec_ptrs.data_ptr(), d_rec_bytes.data_ptr(), d_dst_ptrs.data_ptr(), d_bytes.data_ptr(), n_regions,
          _status_ptr(d_status), _stream_handle(stream))


def kinds_store_host(data, stored: bool, sparse: bool):
    """One packet (1 .. 8192 bytes) in its stream form on the CPU (gpuar_hip_kinds_store_host; gpuar_amd/csrc/kinds.h): (kind,
    packet) with the packet -- 4-byte header, then the bytes or the sparse record -- as bytes, or b"" for KIND_CODED (the
    encoder's packet stands)."""
    data = bytes(data)
    pkt = (C.c_uint8 * SLOT)()
    kind, clen = C.c_uint32(0), C.c_size_t(0)
    _call("gpuar_hip_kinds_store_host", data, len(data), int(bool(stored)), int(bool(sparse)), pkt, len(pkt), C.byref(kind), C.byref(clen))
    return int(kind.value), bytes(pkt[:clen.value])


def kinds_expand_host(pkt, kind: int, n_bytes: int) -> bytes:
    """The `n_bytes` of a raw (KIND_RAW) or sparse (KIND_SPARSE) packet in its stream form on the CPU
    (gpuar_hip_kinds_expand_host); raises for any other kind and for a packet that is not valid."""
    pkt = bytes(pkt)
    out = (C.c_uint8 * max(n_bytes, 1))()
    _call("gpuar_hip_kinds_expand_host", pkt, len(pkt), kind, out, n_bytes)
    return bytes(out[:n_bytes])


def kinds_store(d_in, d_est, d_scan, stored: bool, d_slots, n_bytes: int = None, d_kind=None, stream=None, d_status=None):
    """Behind encode() on the same stream: the kind of every packet of the first `n_bytes` (default: all) bytes of `d_in` from
    d_est (estimate) and d_scan (sparse_scan; None: sparse is off) into d_kind (uint8 CUDA tensor, one per packet; allocated when
    None), and the slots of the raw and sparse packets overwritten with their stream form (gpuar_hip_kinds_store).  A scan word
    that is not that of the packet's bytes is STATUS_BAD_BATCH: the slot stays the encoder's and the kind 0.  Returns d_kind."""
    import torch
    _require_cuda_u8(d_in, "d_in")
    _require_cuda_u8(d_slots, "d_slots")
    n = d_in.numel() if n_bytes is None else n_bytes
    n_packets = packet_count(n)
    if n > d_in.numel() or d_slots.numel() < n_packets * SLOT:
        raise GpuarError("d_in or d_slots is too small")
    _require_crc(d_est, "d_est", n_packets)
    if d_scan is not None:
        _require_crc(d_scan, "d_scan", n_packets)
    if d_kind is None:
        d_kind = torch.empty(n_packets, dtype=torch.uint8, device=d_in.device)
    _require_cuda_u8(d_kind, "d_kind")
    if d_kind.numel() < n_packets:
        raise GpuarError("d_kind is too small")
    _call("gpuar_hip_kinds_store", d_in.data_ptr(), n, d_est.data_ptr(), d_scan.data_ptr() if d_scan is not None else None, int(bool(stored)),
          d_slots.data_ptr(), d_kind.data_ptr(), _status_ptr(d_status), _stream_handle(stream))
    return d_kind


def kinds_expand(d_stream, d_offsets, d_kind, n_packets: int, d_out, n_bytes: int, stream=None, d_status=None):
    """Take the raw and sparse packets out of a compacted stream: packet p of kind d_kind[p] = 1 or 2 at d_stream + d_offsets[p]
    (any alignment) to d_out + 8192 p; coded packets (kind 0) are skipped (gpuar_hip_kinds_expand).  n_bytes: the bytes of the whole
    output, packet_count(n_bytes) == n_packets.  A packet that is not valid, or a kind above 2, is STATUS_BAD_PACKET."""
    _require_cuda_u8(d_stream, "d_stream")
    _require_cuda_u8(d_kind, "d_kind")
    _require_cuda_u8(d_out, "d_out")
    _require_u64_desc(d_offsets, "d_offsets", n_packets + 1)
    if d_kind.numel() < n_packets or d_out.numel() < n_bytes:
        raise GpuarError("d_kind or d_out is too small")
    _call("gpuar_hip_kinds_expand", d_stream.data_ptr(), d_offsets.data_ptr(), d_kind.data_ptr(), n_packets, d_out.data_ptr(), n_bytes,
          _status_ptr(d_status), _stream_handle(stream))
    return d_out


def status() -> int:
    """Reads and clears the device's FALLBACK status word -- what launches without a d_status of their own
    reported (synchronises the device).  The read and the clear are one atomic exchange on the device: every bit a
    launch ORs into the word is reported by exactly one status() call, even while other threads launch into it."""
    flags = C.c_uint32(0)
    _call("gpuar_hip_status", C.byref(flags))
    return int(flags.value)


def generate(kind: str, seed: int, n: int, offset: int = 0, device="cuda", out=None, stream=None):
    """Synthetic stream bytes [offset, offset+n) generated on the device (offset % 8 == 0)."""
    import torch
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=device)
    if kind == "zeros":
        out[:n].zero_()
        return out
    _call("gpuar_hip_generate", KIND_ID[kind], seed & 0xFFFFFFFFFFFFFFFF, offset, n, out.data_ptr(), _stream_handle(stream))
    return out


def device_copy(d_src, d_dst, n_bytes: int = None, stream=None):
    """Plain 16-byte-per-lane device copy (gpuar_hip_copy): the measured HBM roof of bench.py."""
    _require_cuda_u8(d_src, "d_src")
    _require_cuda_u8(d_dst, "d_dst")
    n = d_src.numel() if n_bytes is None else n_bytes
    if d_dst.numel() < n or d_src.numel() < n:
        raise GpuarError("copy: buffer too small")
    _call("gpuar_hip_copy", d_src.data_ptr(), d_dst.data_ptr(), n, _stream_handle(stream))
    return d_dst


def gip_header(n_uncompressed: int, n_stream: int) -> bytes:
    """20-byte container header (src/file_header.hpp:19-36,61-72): version 0.1.0,
    sizes little-endian in the 8-byte slots (low 4 bytes = what the reference
    writes; it leaves the other bytes uninitialised, we write the high half /
    zeros so files over 4 GiB stay representable)."""
    h = bytearray(HEADER_LEN)
    h[0:3] = bytes([0, 1, 0])
    h[4:12] = int(n_uncompressed).to_bytes(8, "little")
    h[12:20] = int(HEADER_LEN + n_stream).to_bytes(8, "little")
    return bytes(h)


def shader_clock_mhz(which: str, reset: bool = True):
    """The shader clock while the last launches of the throughput encode kernel (which = "encode") or of a decode kernel
    ("decode") ran, from the samples their workgroups left (gpuar_hip_clock_samples): (MHz, number of samples), or
    (None, 0) when no sampled workgroup has run to its end since the last reset.  Synchronises the device."""
    buf = (C.c_uint64 * (4 * CLOCK_SLOTS))()
    _call("gpuar_hip_clock_samples", {"encode": 0, "decode": 1}[which], buf, 1 if reset else 0)
    shader = real = n = 0
    for i in range(CLOCK_SLOTS):
        s0, r0, s1, r1 = buf[4 * i:4 * i + 4]
        if r0 and r1 > r0 and s1 > s0:              # a workgroup that started and ended since the reset
            shader, real, n = shader + (s1 - s0), real + (r1 - r0), n + 1
    return (shader / real * 100.0, n) if real else (None, 0)
