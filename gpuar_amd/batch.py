"""Many tensors compressed and decompressed in one launch (gpuar_hip_encode_batch / decode_batch / decode_stream_batch).

Each tensor is taken as its bytes and coded exactly as if it were encoded alone: buffer b's stream is the bytes
`gpuar c` writes for it behind the 20-byte header (Compressed.gip(b)).  The descriptors are built on the host and go to
the device in one copy; the status word is checked after every call and any bit raises.  There is no CPU fallback and
no silent copy: a tensor that is not 16-byte aligned is refused before anything is launched.

    c = batch.compress([w1, w2, w3])          # contiguous CUDA tensors on one device
    outs = batch.decompress(c)                # uint8 tensors, one per input

With checksum=True, compress also keeps the CRC-32 (zlib.crc32) of every packet's uncompressed bytes (Compressed.crc32);
decompress then checks what it decoded against them and raises GpuarError naming the buffer and packet that differ, and
Compressed.gip(b) carries them in the file's trailer (version 2), which `gpuar d` verifies.

With planes="auto" (or a width, or one width per tensor) every tensor's bytes are regrouped into byte planes before they are
coded (hip.split_planes: one launch for the batch, into a temporary buffer -- the inputs are never modified) and regrouped
back, in place in the output tensors, after they are decoded: typed data (bf16, fp32, int64 ...) compresses 7-26 % smaller
(DESIGN.md 4.6).  The CRCs are those of the ORIGINAL bytes.  Compressed.gip(b) then carries the width in a version-3 trailer
(`gpuar c --planes=W`), without which a reader would return the regrouped bytes.
"""
from __future__ import annotations

import bisect
import struct
from dataclasses import dataclass

from . import hip as H
from .hip import GpuarError


def _tensor_bytes(t, name):
    import torch
    if not isinstance(t, torch.Tensor):
        raise GpuarError(f"{name} is not a tensor")
    if not t.is_cuda:
        raise GpuarError(f"{name} is not a CUDA tensor")
    if not t.is_contiguous():
        raise GpuarError(f"{name} is not contiguous")
    return t.numel() * t.element_size()


def describe(tensors, what="tensors"):
    """Host-side descriptors of a list of tensors: (device, pointers, sizes, first_packet, packet count).  Raises GpuarError
    for anything the kernels could not take: a non-CUDA or non-contiguous tensor, tensors on different devices, or a
    non-empty tensor whose data is not 16-byte aligned."""
    tensors = list(tensors)
    ptrs, sizes, device = [], [], None
    for i, t in enumerate(tensors):
        n = _tensor_bytes(t, f"{what}[{i}]")
        if device is None:
            device = t.device
        elif t.device != device:
            raise GpuarError(f"{what}[{i}] is on {t.device}, the batch on {device}")
        if n and t.data_ptr() % 16:
            raise GpuarError(f"{what}[{i}] is not 16-byte aligned (data_ptr() % 16 = {t.data_ptr() % 16}); pass an aligned copy")
        ptrs.append(t.data_ptr() if n else 0)
        sizes.append(n)
    first_packet, n_packets = H.batch_packet_count(sizes)
    return device, ptrs, sizes, first_packet, n_packets


def _upload(device, *rows):
    """The descriptor rows (lists of ints) as ONE int64 device tensor (one copy), returned split back into rows."""
    import torch
    flat = [v if v < (1 << 63) else v - (1 << 64) for row in rows for v in row]
    host = torch.tensor(flat or [0], dtype=torch.int64).pin_memory() if torch.cuda.is_available() else torch.tensor(flat or [0], dtype=torch.int64)
    dev = host.to(device, non_blocking=True)
    out, at = [], 0
    for row in rows:
        out.append(dev[at:at + len(row)])
        at += len(row)
    return out, host


def _nothing():
    import contextlib
    return contextlib.nullcontext()


def _raise_on_status(d_status, what):
    flags = int(d_status.item())
    if flags:
        names = [n for bit, n in ((H.STATUS_SLOT_OVERFLOW, "SLOT_OVERFLOW"), (H.STATUS_BAD_PACKET, "BAD_PACKET"),
                                  (H.STATUS_BAD_BATCH, "BAD_BATCH"), (H.STATUS_CHECKSUM, "CHECKSUM")) if flags & bit]
        raise GpuarError(f"{what}: device status {flags:#x} ({', '.join(names) or 'unknown'})")


@dataclass
class Compressed:
    """A compressed batch: `stream` (uint8, device, exactly the compressed bytes) holds every buffer's packets back to back
    in batch order, `offsets`
    (int64, device, n_packets + 1) the packet offsets in it, `first_packet` (host list, n_buffers + 1) which packets
    belong to which buffer, `sizes` the buffers' byte counts, `crc32` (int32, device, n_packets; None unless compressed with
    checksum=True) the CRC-32 of every packet's uncompressed bytes, `planes` (host list, n_buffers; None unless compressed with
    planes=...) the element width each buffer's bytes were split into byte planes by (1: not split)."""
    stream: object
    offsets: object
    first_packet: list
    sizes: list
    crc32: object = None
    planes: list = None

    @property
    def n_buffers(self) -> int:
        return len(self.sizes)

    @property
    def n_packets(self) -> int:
        return self.first_packet[-1]

    def _offsets_host(self):
        if getattr(self, "_off", None) is None:
            self._off = self.offsets.cpu().tolist()
        return self._off

    def payload(self, b: int):
        """A view of buffer b's packet stream (the bytes behind the header of its .gip file)."""
        off = self._offsets_host()
        return self.stream[off[self.first_packet[b]]:off[self.first_packet[b + 1]]]

    def gip(self, b: int) -> bytes:
        """Buffer b as a whole .gip file: what `gpuar c` writes for it (with CRCs: what `gpuar c --checksum` writes; split into
        planes of width W > 1: what `gpuar c --planes=W` writes)."""
        p = self.payload(b)
        out = H.gip_header(self.sizes[b], p.numel()) + bytes(p.cpu().numpy().tobytes())
        w = self.planes[b] if self.planes is not None else 1
        if self.crc32 is not None or w > 1:
            off = self._offsets_host()
            lo, hi = self.first_packet[b], self.first_packet[b + 1]
            clens = [off[i + 1] - off[i] for i in range(lo, hi)]
            crcs = [v & 0xFFFFFFFF for v in self.crc32[lo:hi].cpu().tolist()] if self.crc32 is not None else None
            out += trailer_v3(clens, w, crcs) if w > 1 else trailer_v2(clens, crcs)
        return out


def trailer_v2(clens, crcs) -> bytes:
    """The .gip trailer version 2: "GIPX" u32 2 u64 n | u16 clen[n] | pad to 4 | u32 crc32[n] | pad to 8 |
    u64 trailer bytes "XPIG", little-endian."""
    n = len(clens)
    body = b"GIPX" + struct.pack("<IQ", 2, n) + struct.pack(f"<{n}H", *clens)
    body += bytes(-len(body) % 4) + struct.pack(f"<{n}I", *crcs)
    body += bytes(-len(body) % 8)
    return body + struct.pack("<Q", len(body) + 12) + b"XPIG"


def trailer_v3(clens, elem_bytes, crcs=None) -> bytes:
    """The .gip trailer version 3 of a file whose bytes were split into planes of `elem_bytes`: "GIPX" u32 3
    u64 n | u32 elem_bytes | u32 flags (bit 0: CRCs present) | u16 clen[n] | pad to 4 | u32 crc32[n] if flagged | pad to 8 |
    u64 trailer bytes "XPIG", little-endian, pads counted from "GIPX"."""
    n = len(clens)
    body = b"GIPX" + struct.pack("<IQII", 3, n, elem_bytes, 1 if crcs is not None else 0) + struct.pack(f"<{n}H", *clens)
    body += bytes(-len(body) % 4)
    if crcs is not None:
        body += struct.pack(f"<{n}I", *crcs)
    body += bytes(-len(body) % 8)
    return body + struct.pack("<Q", len(body) + 12) + b"XPIG"


def plane_widths(tensors, planes):
    """The element width per tensor that `planes` asks for: None -> None; "auto" -> each tensor's element_size() where that is
    2, 4 or 8 and the type is not complex, else 1 (not split); an int -> that width for every tensor; a list -> as given."""
    tensors = list(tensors)
    if planes is None:
        return None
    if isinstance(planes, str):
        if planes != "auto":
            raise GpuarError(f"planes={planes!r}: None, \"auto\", a width or a list of widths")
        return [t.element_size() if t.element_size() in (2, 4, 8) and not t.is_complex() else 1 for t in tensors]
    widths = [planes] * len(tensors) if isinstance(planes, int) else list(planes)
    if len(widths) != len(tensors) or not all(isinstance(w, int) and 0 < w < (1 << 63) for w in widths):
        raise GpuarError(f"planes: {len(widths)} widths for {len(tensors)} tensors, or a width that is not a positive int")
    return widths


def compress(tensors, mode=None, stream=None, checksum=False, planes=None) -> Compressed:
    """Encode every tensor of `tensors` (contiguous CUDA tensors on one device, each taken as its bytes) in one launch and
    compact the result.  `mode`: "auto" | "throughput" | "latency" (as hip.encode).  `checksum`: also compute the CRC-32 of
    every packet (Compressed.crc32; one more launch on the same stream).  `planes`: None | "auto" | a width | one width per
    tensor (plane_widths): split each tensor's bytes into byte planes of that element width before coding (one more launch,
    into a temporary buffer that is freed with the slots; widths of 1 are coded as they are).  The widths the kernels take
    are 1, 2, 4 and 8: any other raises from the device's status (BAD_BATCH)."""
    import torch
    tensors = list(tensors)
    device, ptrs, sizes, first_packet, n_packets = describe(tensors)
    widths = plane_widths(tensors, planes)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    n = len(sizes)
    with torch.cuda.stream(stream) if stream is not None else _nothing():
        d_status = torch.zeros(1, dtype=torch.int32, device=device)
        d_split = None
        if widths is not None and any(w != 1 for w in widths):
            # the split copies of the buffers that are split, back to back (each 16-byte aligned); the others are coded where they are
            at, split_ptrs = 0, []
            for p, size, w in zip(ptrs, sizes, widths):
                split_ptrs.append(at if w != 1 and size else None)
                at += (size + 15) // 16 * 16 if w != 1 else 0
            d_split = torch.empty(max(at, 16), dtype=torch.uint8, device=device)
            split_ptrs = [p if q is None else d_split.data_ptr() + q for p, q in zip(ptrs, split_ptrs)]
            (d_ptrs, d_bytes, d_fp, d_elem, d_coded), _keep = _upload(device, ptrs, sizes, first_packet, widths, split_ptrs)
            H.split_planes_batch(d_ptrs, d_bytes, d_fp, d_elem, n, n_packets, d_coded, stream=stream, d_status=d_status)
        else:
            (d_ptrs, d_bytes, d_fp), _keep = _upload(device, ptrs, sizes, first_packet)
            d_coded = d_ptrs
        d_slots = H.encode_batch(d_coded, d_bytes, d_fp, n, n_packets, stream=stream, d_status=d_status, mode=mode, device=device)
        d_stream, d_offsets = H.compact(d_slots, n_packets, stream=stream)
        d_crc = H.crc32_batch(d_ptrs, d_bytes, d_fp, n, n_packets, stream=stream, d_status=d_status, device=device) if checksum else None
        _raise_on_status(d_status, "encode_batch")
        # compact() wrote into a buffer of n_packets * 8704 bytes: keep only the compressed bytes (one copy), so that the
        # result takes what it compressed to, not ~1.06 x the input
        used = int(d_offsets[-1].item())
        d_stream = d_stream[:used].clone()
        del d_slots, d_split
    return Compressed(stream=d_stream, offsets=d_offsets, first_packet=first_packet, sizes=sizes,
                      crc32=d_crc[:n_packets] if d_crc is not None else None, planes=widths)


def decompress(c: Compressed, out=None, stream=None, verify=True):
    """Decode every buffer of `c` in one launch.  Returns a list of uint8 tensors, or fills the caller's tensors `out` (one per
    buffer, contiguous CUDA tensors of at least the buffer's bytes, 16-byte aligned) and returns them.  When `c` carries CRCs
    and `verify` is true, the decoded bytes are checked against them (one more launch): a mismatch raises GpuarError naming
    the first buffer and packet that differ.  Buffers that were split into byte planes are merged back in place in `out`
    after decoding and before verifying: the CRCs are those of the original bytes."""
    import torch
    device = c.stream.device
    if out is None:
        out = [torch.empty(n, dtype=torch.uint8, device=device) for n in c.sizes]
    elif len(out) != c.n_buffers:
        raise GpuarError(f"out has {len(out)} tensors, the batch {c.n_buffers} buffers")
    _dev, ptrs, room, _fp, _np = describe(out, "out")
    for b, (have, need) in enumerate(zip(room, c.sizes)):
        if have < need:
            raise GpuarError(f"out[{b}] holds {have} bytes, buffer {b} needs {need}")
    with torch.cuda.stream(stream) if stream is not None else _nothing():
        (d_ptrs, d_room, d_fp, d_sizes), _keep = _upload(device, ptrs, room, c.first_packet, c.sizes)
        d_status = torch.zeros(1, dtype=torch.int32, device=device)
        H.decode_stream_batch(c.stream, c.offsets, d_fp, c.n_buffers, c.n_packets, d_ptrs, d_room, stream=stream, d_status=d_status)
        _raise_on_status(d_status, "decode_stream_batch")      # (.item() waits for this stream)
        if c.planes is not None and any(w != 1 for w in c.planes) and c.n_packets:
            (d_elem,), _keep2 = _upload(device, c.planes)
            H.merge_planes_batch(d_ptrs, d_sizes, d_fp, d_elem, c.n_buffers, c.n_packets, d_ptrs, stream=stream, d_status=d_status)
            _raise_on_status(d_status, "merge_planes_batch")
        if c.crc32 is not None and verify and c.n_packets:
            d_first_bad = torch.full((1,), -1, dtype=torch.int64, device=device)
            H.verify_crc32_batch(d_ptrs, d_sizes, d_fp, c.n_buffers, c.n_packets, c.crc32, d_first_bad, stream=stream, d_status=d_status)
            flags = int(d_status.item())
            if flags & H.STATUS_CHECKSUM:
                p = int(d_first_bad.item())
                b = bisect.bisect_right(c.first_packet, p) - 1
                j = p - c.first_packet[b]
                raise GpuarError(f"checksum mismatch: buffer {b}, packet {j} (batch packet {p}), bytes {j * H.PACKET} .. "
                                 f"{min((j + 1) * H.PACKET, c.sizes[b])} of {c.sizes[b]} differ from what was compressed")
            _raise_on_status(d_status, "verify_crc32_batch")
    return out
