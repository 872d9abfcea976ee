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

With stored="auto" the packets that cannot shrink are not coded at all: one histogram pass (hip.estimate_batch) predicts every
packet's compressed size, the packets whose estimate is not smaller than their bytes are copied raw into Compressed.raw
(hip.move_packets) and only the others go through the encoder -- and, in decompress, the decoder.
estimate(tensors, ...) gives the predicted sizes without compressing anything.  In a .gip file a raw packet stands behind a 4-byte
header and a version-6 trailer says which packets are raw: Compressed.gip(b, kinds=True) writes that file for a
batch compressed with stored="auto"; without kinds=True a buffer that holds a raw packet raises, and so does a batch compressed
with a list of stored packets, which has no file form.

With planes="survey" the width of every tensor is chosen by measurement instead of by dtype: survey(tensors) predicts, in one
launch over the original bytes (hip.survey_planes_batch), what each tensor would compress to at widths 1, 2, 4 and 8, and
hip.choose_planes picks the smallest width within the estimate's resolution of the best.  That finds the
element width of typed data held as bytes -- a uint8 view of a checkpoint shard -- which planes="auto" cannot see.

With delta=True (or one bool per tensor) the elements of every group are replaced by their difference to the element in front
before they are split (hip.split_delta_batch: the same single launch), and summed up again, in place, after they are decoded
(hip.merge_delta_batch): ordered integers -- offsets, sorted indices, position ids, timestamps, samples -- compress 2-15 x
smaller, unordered data and floats grow.  The element width is that of `planes` (planes=None: bytes).
delta="auto" measures: it splits and estimates the batch both ways and filters the tensors for which that is predicted to pay.
Compressed.gip(b) then carries width and filter in a version-4 trailer (`gpuar c --delta --planes=W`).

delta="survey" makes the decision of delta="auto" without splitting anything: one hip.survey_delta_batch launch over the
original bytes predicts what every tensor compresses to WITH the filter at the widths in use, survey's launch what it does
without, and a tensor is filtered on the rule of "auto" (DESIGN.md 4.11).  Together with planes="survey" width and filter are
chosen together (hip.choose_filter): on position ids held as bytes the plane survey alone picks width 8, the pair (4, filter).

With base=[...] (one tensor of the same byte count, or None, per tensor) every tensor is XORed with its base before it is
split (hip.split_xor_batch: the same single launch, into the same temporary buffer) and XORed back, in place, after it is
decoded (hip.merge_xor_batch; decompress needs the same bases).  The next checkpoint of a model is almost the previous one:
against it a bf16 tensor compresses to 0.06-0.72 of what it does alone, against an unrelated base it grows.
base_auto=True measures and keeps the bases that are predicted to pay (Compressed.based); base_auto="survey" keeps the same ones
from two survey launches over the original bytes (hip.survey_xor_batch: the estimate and the scan word of every packet of the XORed,
split bytes at the four widths, without making them) and splits once, and with planes="survey" chooses width and base together;
survey_xor gives those totals to a caller of its own.  The CRCs are those of the original
bytes, so a wrong base in decompress is a checksum mismatch.  Compressed.gip(b) carries a version-5 trailer
(`gpuar c --base=FILE --planes=W`) and needs the CRCs.  A base together with `delta` is refused.

With sparse="auto" a packet that is one byte value almost everywhere is neither coded nor kept raw: one more pass
(hip.sparse_scan_batch) finds every packet's majority byte and counts its exceptions, and the packets whose record -- the byte, the
count, the exceptions' positions and values: 4 + 3 k bytes -- is smaller than their estimate go into Compressed.sparse
(hip.sparse_pack) and come back through hip.sparse_unpack.  That is what a base makes of everything that did not
change since it: compress(tensors, planes="auto", base=[...], sparse="auto") keeps an unchanged packet in 4 bytes where the
codec cannot go below 210.  Like a raw packet, a sparse one goes into a version-6 file: Compressed.gip(b, kinds=True).

With planes="mixed" width and filter are chosen per 64 KiB supergroup of every tensor instead of once per tensor: survey_mixed runs
the plane survey -- with delta="mixed" the delta survey, with base=[...] the XOR survey too --, one hip.choose_modes_batch launch
picks every supergroup's mode byte (width, delta or base; Compressed.modes), hip.split_mixed_batch splits the batch once and
hip.merge_mixed_batch merges it back in place.  That is for a blob of several tensors, a struct of arrays or a
checkpoint whose layers moved unequally; its predicted size is within two bytes per packet of the best single choice.  Such a batch
has no .gip form yet.

from_gip(files) is the way back: a list of .gip files -- what Compressed.gip or `gpuar c` wrote, any trailer version or none, as
bytes, arrays or paths -- becomes one Compressed, one buffer per file, and decompress decodes them all in one launch.  The files
are read and checked on the host by the CLI's own reader (read_gip: hip.gip_read_host, no GPU), their streams go to the device in
one copy, and where a file is version 6 one hip.move_bytes launch takes the interleaved coded, raw and sparse packets apart into
`stream`, `raw` and `sparse`.

    blobs = [c.gip(b) for b in range(c.n_buffers)]
    outs = batch.decompress(batch.from_gip(blobs))
"""
from __future__ import annotations

import bisect
import struct
from dataclasses import dataclass
from typing import NamedTuple

from . import hip as H
from .hip import GpuarError


def _is(value, word):
    """`value` is the string `word` (and no list, array or tensor that `==` would compare element by element)"""
    return isinstance(value, str) and value == word


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
    """The descriptor rows (lists of ints below 2^64 -- from 2^63 on they wrap, as pointers do -- or numpy integer arrays) as ONE int64
    device tensor (one pinned tensor, one copy), returned split back into rows, with the pinned tensor for the caller to hold."""
    import numpy as np
    import torch
    flat = np.concatenate([r.astype(np.int64, copy=False) if isinstance(r, np.ndarray) else np.array(r, dtype=np.uint64).view(np.int64) for r in rows]
                          + [np.zeros(1, dtype=np.int64)])
    host = torch.from_numpy(flat)
    if torch.cuda.is_available():
        host = host.pin_memory()
    dev = host.to(device, non_blocking=True)
    out, at = [], 0
    for row in rows:
        out.append(dev[at:at + len(row)])
        at += len(row)
    return out, host


def _offsets(lengths):
    """[0, lengths[0], lengths[0] + lengths[1], ...] (int64, on the lengths' device): where pieces of these lengths stand back to back."""
    import torch
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=lengths.device), torch.cumsum(lengths, 0)])


def _on(stream):
    """the context in which torch's own work goes to `stream` (None: to the current one)"""
    import contextlib
    import torch
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


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
    planes=...) the element width each buffer's bytes were split into byte planes by (1: not split), `delta` (host list of
    bools, n_buffers; None unless compressed with delta=...) which buffers went through the delta filter (their `planes`
    entry is the filter's element width), `based` (host list of bools, n_buffers; None unless compressed with base=...) which
    buffers were XORed with their base and need it again in decompress.

    Compressed with stored=...: `stored` (uint8, device, n_packets) is 1 for every batch packet that is kept raw, `raw` (uint8,
    device) holds those packets' bytes in batch order, each at a 16-byte-aligned offset, `raw_offsets` (int64, device,
    n_stored + 1) where; `stream` and `offsets` (n_coded + 1 entries) then cover the CODED packets only, in batch order.  All
    three are None otherwise.

    Compressed with sparse="auto": `stored` is the packet's kind -- 0 coded, 1 raw, 2 sparse, so that a stable sort by it gives the
    coded, the raw and the sparse packets, each in batch order --, `sparse` (uint8, device) holds the sparse packets' records
    (gpuar_amd/csrc/sparse.h) back to back in batch order, `sparse_offsets` (int64, device, n_sparse + 1) where; `raw` and
    `raw_offsets` are there too (empty without stored=...).  Both are None otherwise.

    Compressed with planes="mixed": `modes` (host list, n_buffers, of bytes: one mode per supergroup of 65536 bytes -- log2(width) |
    delta << 2 | base << 3, hip.mode_parts) says how every supergroup was split; `planes` and `delta` are then None, and `based[b]`
    says whether some supergroup of buffer b took the base.  None otherwise.

    `kinds_rule`: (stored == "auto", sparse == "auto") where the packets' kinds were chosen by hip.sparse_rule -- what
    gip(b, kinds=True) needs to know: such a buffer has a version-6 file, one with a list of stored packets has none."""
    stream: object
    offsets: object
    first_packet: list
    sizes: list
    crc32: object = None
    planes: list = None
    stored: object = None
    raw: object = None
    raw_offsets: object = None
    delta: list = None
    based: list = None
    sparse: object = None
    sparse_offsets: object = None
    kinds_rule: tuple = None
    modes: list = None

    @property
    def n_buffers(self) -> int:
        return len(self.sizes)

    @property
    def n_packets(self) -> int:
        return self.first_packet[-1]

    def _offsets_host(self):
        return self._host_copy("offsets")

    def _host_copy(self, name):
        """The host copy of the device field `name`, made on first use and kept (_offsets_host: that of the offsets): gip(b) for
        every buffer of the batch then costs one copy of the batch, not one per file.  `stream`, `raw`, `sparse`: bytes; the
        others: a list of ints; a field that is None: the empty one.  The fields are not written after compress."""
        kept = self.__dict__.setdefault("_host_copies", {})
        if name not in kept:
            t = getattr(self, name)
            if name in ("stream", "raw", "sparse"):
                kept[name] = t.cpu().numpy().tobytes() if t is not None else b""
            else:
                kept[name] = t.cpu().tolist() if t is not None else [0]
        return kept[name]

    @property
    def nbytes(self) -> int:
        """The compressed bytes: the coded packets' stream, the raw packets and the sparse packets' records."""
        return self.stream.numel() + (self.raw.numel() if self.raw is not None else 0) + (self.sparse.numel() if self.sparse is not None else 0)

    def _coded_range(self, b: int):
        """Buffer b's packets as a range of `offsets`: its batch packets, or -- with `stored` -- their ranks among the coded ones."""
        lo, hi = self.first_packet[b], self.first_packet[b + 1]
        if self.stored is None:
            return lo, hi
        rank = self._ranks()[H.KIND_CODED]
        if rank[hi] - rank[lo] != hi - lo:
            raise GpuarError(f"buffer {b} has {hi - lo - (rank[hi] - rank[lo])} stored (raw or sparse) packets: it has no packet stream of "
                             "coded packets alone; its .gip form is the version-6 file, gip(b, kinds=True), where the kinds came from the rule")
        return rank[lo], rank[hi]

    def _ranks(self):
        """Per kind k (0 coded, 1 raw, 2 sparse) a list of n_packets + 1 entries: how many packets of kind k stand in front of batch
        packet p -- packet p's place in `offsets`, `raw_offsets` or `sparse_offsets`.  Made on first use and kept."""
        if getattr(self, "_rank", None) is None:
            self._rank = [[0], [0], [0]]
            for kind in self._host_copy("stored"):
                for k, row in enumerate(self._rank):
                    row.append(row[-1] + (k == kind))
        return self._rank

    def payload(self, b: int):
        """A view of buffer b's packet stream (the bytes behind the header of its .gip file).  Raises GpuarError for a buffer that
        has a stored packet."""
        off = self._offsets_host()
        lo, hi = self._coded_range(b)
        return self.stream[off[lo]:off[hi]]

    def _kinds_packets(self, b: int):
        """(packet stream, clens, kinds) of buffer b with every packet in its stream form (gpuar_amd/csrc/kinds.h): the coded
        packets as they are, the raw and the sparse ones behind a 4-byte header put in front of them here, on the host."""
        lo, hi = self.first_packet[b], self.first_packet[b + 1]
        kinds = self._host_copy("stored")
        rank = [row[lo] for row in self._ranks()]          # how many packets of each kind stand in front of packet lo
        off = self._offsets_host()
        raw, raw_off = self._host_copy("raw"), self._host_copy("raw_offsets")
        rec, rec_off = self._host_copy("sparse"), self._host_copy("sparse_offsets")
        coded = self._host_copy("stream")
        packets = []
        for i, k in enumerate(kinds[lo:hi]):
            ulen, r = min(H.PACKET, self.sizes[b] - i * H.PACKET), rank[k]
            if k == H.KIND_CODED:
                packets.append(coded[off[r]:off[r + 1]])
            elif k == H.KIND_RAW:
                packets.append(struct.pack("<HH", 4 + ulen, ulen) + raw[raw_off[r]:raw_off[r] + ulen])
            else:
                packets.append(struct.pack("<HH", 4 + rec_off[r + 1] - rec_off[r], ulen) + rec[rec_off[r]:rec_off[r + 1]])
            rank[k] += 1
        return b"".join(packets), [len(p) for p in packets], kinds[lo:hi]

    def gip(self, b: int, kinds: bool = False) -> bytes:
        """Buffer b as a whole .gip file: what `gpuar c` writes for it (with CRCs: what `gpuar c --checksum` writes; split into
        planes of width W > 1: what `gpuar c --planes=W` writes; filtered: what `gpuar c --delta --planes=W` writes; XORed with
        a base: what `gpuar c --base=FILE --planes=W` writes, which needs the CRCs -- GpuarError without checksum=True).
        `kinds`: for a batch compressed with stored="auto" and / or sparse="auto", the file `gpuar c` writes with --stored=auto
        and / or --sparse=auto beside those flags -- every packet behind its 4-byte header, a version-6 trailer that says which is
        which; GpuarError for any other batch (a list of stored packets has no file form).  Without it a buffer that holds a
        raw or sparse packet raises, as ever."""
        if self.modes is not None:
            raise GpuarError(f"buffer {b} was compressed with planes=\"mixed\": its .gip form needs a trailer that carries a mode per "
                             "supergroup (version 7), which is not built yet")
        xored = bool(self.based[b]) if self.based is not None else False
        if xored and self.crc32 is None:
            raise GpuarError(f"buffer {b} was XORed with a base: its .gip form (trailer version 5) needs the CRCs that tell a reader "
                             "it was given the wrong base -- compress with checksum=True")
        if kinds:
            if self.kinds_rule is None or self.stored is None:
                raise GpuarError("gip(kinds=True) is the file of a batch compressed with stored=\"auto\" and / or sparse=\"auto\"")
            payload, clens, which = self._kinds_packets(b)
        else:
            off = self._offsets_host()
            lo, hi = self._coded_range(b)                  # (raises for a buffer that holds a stored packet, as payload(b) does)
            payload, clens, which = self._host_copy("stream")[off[lo]:off[hi]], [off[i + 1] - off[i] for i in range(lo, hi)], None
        out = H.gip_header(self.sizes[b], len(payload)) + payload
        w = self.planes[b] if self.planes is not None else 1
        filtered = bool(self.delta[b]) if self.delta is not None else False
        if which is not None or self.crc32 is not None or w > 1 or filtered or xored:
            lo, hi = self.first_packet[b], self.first_packet[b + 1]
            crcs = [v & 0xFFFFFFFF for v in self._host_copy("crc32")[lo:hi]] if self.crc32 is not None else None
            out += trailer(clens, w, crcs, delta=filtered, base=xored, kinds=which)
        return out


def trailer(clens, elem_bytes=1, crcs=None, delta=False, base=False, kinds=None) -> bytes:
    """The .gip trailer, little-endian, pads counted from "GIPX": version 5 for a file whose bytes were XORed with
    a base and split at a width of `elem_bytes` (1 too; flags bit 2 and bit 0 set: the CRCs are mandatory), else version 4 for a
    file whose bytes went through the delta filter at a width of `elem_bytes` (1 too), else version 3 for a file whose bytes were split into planes of
    `elem_bytes` > 1, else version 2 when `crcs` are given, else version 1.
    "GIPX" u32 version u64 n | versions 3, 4: u32 elem_bytes u32 flags (bit 0: CRCs present; version 4: bit 1, delta, set) |
    u16 clen[n] | with CRCs: pad to 4 u32 crc32[n] | pad to 8 | u64 trailer bytes "XPIG".
    `kinds` (one of 0 coded, 1 raw, 2 sparse per packet): version 6, which has version 3's fields whatever the rest says, bit 3
    of the flags set beside those above, and u8 kind[n] behind the CRCs (behind the pad to 4 where there are none)."""
    n = len(clens)
    if base and (delta or crcs is None):
        raise GpuarError("a version-5 trailer (base) carries CRCs and no delta flag")
    if kinds is not None and (len(kinds) != n or any(k not in (0, 1, 2) for k in kinds)):
        raise GpuarError("a version-6 trailer carries one kind (0, 1 or 2) per packet")
    body = b"GIPX" + struct.pack("<IQ", 6 if kinds is not None else 5 if base else 4 if delta else 3 if elem_bytes > 1 else 1 if crcs is None else 2, n)
    if elem_bytes > 1 or delta or base or kinds is not None:
        body += struct.pack("<II", elem_bytes, (0 if crcs is None else 1) | (2 if delta else 0) | (4 if base else 0) | (0 if kinds is None else 8))
    body += struct.pack(f"<{n}H", *clens)
    if crcs is not None:
        body += bytes(-len(body) % 4) + struct.pack(f"<{n}I", *crcs)
    if kinds is not None:
        body += bytes(-len(body) % 4) + bytes(kinds)
    body += bytes(-len(body) % 8)
    return body + struct.pack("<Q", len(body) + 12) + b"XPIG"


@dataclass
class GipFile:
    """A .gip file in memory as the CLI's reader sees it (read_gip): `uncompressed` bytes in `n_packets` packets, whose stream is
    bytes [stream_begin, stream_end) of the file (`stream`: a numpy view of them, no copy); the usable trailer's `version` (0: none),
    `elem_bytes` (1 where nothing says) and `flags` (bit 0 CRCs, bit 1 delta, bit 2 base, bit 3 kinds); per packet `clens`
    (uint16; from the trailer, else from walking the headers), `crcs` (uint32; None without them) and `kinds` (uint8; None unless
    version 6).  Every packet's header has been checked against these (include/gpuar_hip.h)."""
    uncompressed: int
    stream_begin: int
    stream_end: int
    version: int
    elem_bytes: int
    flags: int
    clens: object
    crcs: object
    kinds: object
    stream: object

    @property
    def n_packets(self) -> int:
        return len(self.clens)

    @property
    def delta(self) -> bool:
        return self.version in (4, 6) and bool(self.flags & 2)

    @property
    def based(self) -> bool:
        return self.version in (5, 6) and bool(self.flags & 4)


def read_gip(blob, what="the file") -> GipFile:
    """A whole .gip file -- bytes, bytearray, memoryview, a numpy or CPU torch uint8 array -- read on the host by the CLI's own
    reader (hip.gip_read_host: FileHeader::getInfo, Trailer::load and a check of every packet header; no GPU).  Any version
    `gpuar c` or Compressed.gip writes, and files without a trailer, reference-written ones included.  Raises GpuarError naming
    `what`, the defect and where it is: a short or foreign header, a compressed size beyond the file, a trailer of version 3 .. 6
    that cannot be used, a packet count, clen, ulen or kind that does not fit, a raw or sparse packet whose header does not fit
    its form.  The exceptions inside a sparse record and the bits of a coded packet are decompress's to judge."""
    arr = H._host_bytes(blob)
    info, clens, crcs, kinds = H.gip_read_host(arr, what)
    return GipFile(uncompressed=info[0], stream_begin=info[1], stream_end=info[2], version=info[3], elem_bytes=info[5], flags=info[6],
                   clens=clens, crcs=crcs, kinds=kinds, stream=arr[info[1]:info[2]])


def _gip_entry(entry, i):
    """files[i] of from_gip as (bytes-like or array, its name in messages); a path is read whole."""
    import os
    import numpy as np
    import torch
    if isinstance(entry, (str, os.PathLike)):
        try:
            return np.fromfile(entry, dtype=np.uint8), f"files[{i}] ({os.fspath(entry)})"
        except OSError as e:
            raise GpuarError(f"files[{i}] ({os.fspath(entry)}): {e}") from None
    if isinstance(entry, (bytes, bytearray, memoryview)) or (isinstance(entry, np.ndarray) and entry.dtype == np.uint8) or \
            (isinstance(entry, torch.Tensor) and not entry.is_cuda and entry.dtype == torch.uint8):
        return entry, f"files[{i}]"
    raise GpuarError(f"files[{i}] is a {type(entry).__name__}: a .gip file is bytes, a bytearray, a memoryview, a numpy or CPU torch uint8 "
                     "array, or a path")


def _gip_parse(files):
    """from_gip's host step: every file of the list read and checked (read_gip), and the list checked as a whole; no GPU."""
    if not isinstance(files, (list, tuple)):
        raise GpuarError("files: a list of .gip files (bytes-like objects, uint8 arrays or paths)")
    parsed = []
    for i, entry in enumerate(files):
        blob, what = _gip_entry(entry, i)
        parsed.append(read_gip(blob, what))
    with_crcs = [g.crcs is not None for g in parsed]
    if any(with_crcs):
        for i, g in enumerate(parsed):
            if g.crcs is None and g.n_packets:
                raise GpuarError(f"files[{i}] carries no CRCs, files[{with_crcs.index(True)}] does: a batch has them for every packet or "
                                 "for none (Compressed.crc32)")
    return parsed


def _gip_upload(parsed, total, device):
    """from_gip's upload: the files' packet streams (`total` bytes) back to back in one pinned tensor and on the device after one
    copy, on the current stream: (the device tensor, the pinned one for the caller to hold)."""
    import torch
    staging = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
    at, host = 0, staging.numpy()
    for g in parsed:
        host[at:at + g.stream.size] = g.stream
        at += g.stream.size
    return staging.to(device, non_blocking=True)[:total], staging


def from_gip(files, device=None, stream=None) -> Compressed:
    """The .gip files of `files` (a list; each bytes / bytearray / memoryview / a numpy or CPU torch uint8 array, or a path) as one
    Compressed, one buffer per file in list order: what Compressed.gip and `gpuar c` write, read back -- decompress(from_gip(...),
    base=[...]) then decodes a directory of files in one launch.  Every file is read and checked on the host first (read_gip);
    nothing is launched for a list with a bad file, for one where some files carry CRCs and others (with packets) do not
    (Compressed.crc32 is all or nothing), or for an entry of another type: GpuarError naming the file.

    The files' packet streams go back to back into one pinned buffer and to the device in one copy.  Where no file is version 6
    that copy IS `stream`.  Otherwise the packets -- coded, raw and sparse, interleaved at byte alignment -- are taken apart by
    ONE hip.move_bytes launch over region lists built on the device: a coded packet whole to its place in `stream`, a raw one's
    ulen bytes behind its header to its 16-byte-aligned slot of `raw`, a sparse one's record to its place in `sparse`; the status
    word is checked afterwards.

    The fields are those compress returns for the options the files record: `planes` is None where every file says width 1, no
    filter and no base (else a list), `delta` None where no file is filtered, `based` None where none has a base, `crc32` None
    where none has CRCs.  With a version-6 file in the list `stored`, `raw`, `raw_offsets`, `sparse` and `sparse_offsets` are all
    there (kind 0 for the packets of the other files; empty where no packet is of the kind) and `kinds_rule` is (a raw packet is
    there, a sparse one is) -- a file does not say which options wrote it; else they are None."""
    import torch
    parsed = _gip_parse(files)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with _on(stream):
        d_up, _staging = _gip_upload(parsed, sum(g.stream.size for g in parsed), device)
        return _gip_assemble(parsed, d_up, device, stream)


def _gip_assemble(parsed, d_up, device, stream):
    """from_gip's device step, on the current stream (`stream`, where one was given): the Compressed of the files `parsed` whose
    packet streams stand back to back in `d_up` -- the per-packet tables in one small copy, then the offsets; with a version-6 file
    the region lists and the one hip.move_bytes launch, and the status word checked."""
    import numpy as np
    import torch
    with_crcs = [g.crcs is not None for g in parsed]
    sizes = [g.uncompressed for g in parsed]
    first_packet, n_packets = H.batch_packet_count(sizes)
    mixed = any(g.version == 6 for g in parsed)
    u16, u8 = np.zeros(0, dtype=np.uint16), np.zeros(0, dtype=np.uint8)
    clens = np.concatenate([g.clens for g in parsed] + [u16]).astype(np.int64)
    widths = [g.elem_bytes for g in parsed]
    flags, bases = [g.delta for g in parsed], [g.based for g in parsed]
    d_stored = d_raw = d_raw_offsets = d_sparse = d_sparse_offsets = None
    rows = [clens]
    if any(with_crcs):
        rows.append(np.concatenate([g.crcs for g in parsed if g.crcs is not None]).view(np.int32))
    if mixed:
        kinds = np.concatenate([g.kinds if g.kinds is not None else np.zeros(g.n_packets, dtype=np.uint8) for g in parsed] + [u8]).astype(np.int64)
        ulens = np.concatenate([np.minimum(H.PACKET, size - H.PACKET * np.arange(g.n_packets, dtype=np.int64)) for g, size in zip(parsed, sizes)]
                               + [np.zeros(0, dtype=np.int64)])
        rows += [kinds, ulens]
    d_rows, _keep = _upload(device, *rows)
    d_clen = d_rows[0]
    d_crc = d_rows[1].to(torch.int32) if any(with_crcs) else None
    if not mixed:
        d_stream, d_offsets = d_up, _offsets(d_clen)
    else:
        d_kind, d_ulen = d_rows[-2], d_rows[-1]
        is_coded, is_raw = kinds == H.KIND_CODED, kinds == H.KIND_RAW
        n_coded, n_stored = int(is_coded.sum()), int(is_raw.sum())
        len16 = (ulens + 15) // 16 * 16
        d_stream = torch.empty(int(clens[is_coded].sum()), dtype=torch.uint8, device=device)
        d_raw = torch.zeros(int(len16[is_raw].sum()), dtype=torch.uint8, device=device)          # (zeros: the pads behind partial packets)
        d_sparse = torch.empty(int((clens - 4)[~is_coded & ~is_raw].sum()), dtype=torch.uint8, device=device)
        # the three region lists, on the device: per packet where it stands in the upload, what of it moves, and to where
        coded, raw = d_kind == H.KIND_CODED, d_kind == H.KIND_RAW
        d_len16, d_rec = (d_ulen + 15) // 16 * 16, d_clen - 4
        part = [torch.where(coded, d_clen, 0), torch.where(raw, d_len16, 0), torch.where(coded | raw, 0, d_rec)]
        place = [torch.cumsum(p, 0) - p for p in part]
        d_src = d_up.data_ptr() + (torch.cumsum(d_clen, 0) - d_clen) + torch.where(coded, 0, 4)
        d_dst = torch.where(coded, d_stream.data_ptr() + place[0], torch.where(raw, d_raw.data_ptr() + place[1], d_sparse.data_ptr() + place[2]))
        d_bytes = torch.where(coded, d_clen, torch.where(raw, d_ulen, d_rec))
        d_status = torch.zeros(1, dtype=torch.int32, device=device)
        if n_packets:
            H.move_bytes(d_src, d_dst, d_bytes, n_packets, stream=stream, d_status=d_status)
        in_stream, in_raw, in_sparse = _by_kind(d_kind, n_coded, n_stored)
        d_offsets, d_raw_offsets, d_sparse_offsets = _offsets(d_clen[in_stream]), _offsets(d_len16[in_raw]), _offsets(d_rec[in_sparse])
        d_stored = d_kind.to(torch.uint8)
        _raise_on_status(d_status, "move_bytes")           # (.item() waits for this stream: the upload is done with too)
    plain = all(w == 1 for w in widths) and not any(flags) and not any(bases)
    return Compressed(stream=d_stream, offsets=d_offsets, first_packet=first_packet, sizes=sizes, crc32=d_crc,
                      planes=None if plain else widths, stored=d_stored, raw=d_raw, raw_offsets=d_raw_offsets,
                      delta=flags if any(flags) else None, based=bases if any(bases) else None, sparse=d_sparse,
                      sparse_offsets=d_sparse_offsets,
                      kinds_rule=(bool(n_stored), bool(n_packets - n_coded - n_stored)) if mixed else None)


def plane_widths(tensors, planes):
    """The element width per tensor that `planes` asks for: None -> None; "auto" -> each tensor's element_size() where that is
    2, 4 or 8 and the type is not complex, else 1 (not split); an int -> that width for every tensor; a list -> as given.
    ("survey" is resolved by survey_widths, which launches; this function never does.)"""
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


def delta_flags(tensors, delta):
    """The filter per tensor that `delta` asks for: None -> None; a bool -> that for every tensor; a list -> as given, as bools.
    ("auto" and "survey" are resolved by compress and estimate, which launch; this function never does.)"""
    tensors = list(tensors)
    if delta is None:
        return None
    if isinstance(delta, str):
        raise GpuarError(f"delta={delta!r}: None, True, False, one bool per tensor, \"auto\" or \"survey\"")
    flags = [bool(delta)] * len(tensors) if isinstance(delta, (bool, int)) else [bool(f) for f in delta]
    if len(flags) != len(tensors):
        raise GpuarError(f"delta: {len(flags)} flags for {len(tensors)} tensors")
    return flags


def base_pointers(tensors, base, what="tensors"):
    """The base per tensor that `base` asks for, as device pointers (0: none): None -> None; a list with one entry per tensor,
    each None or a contiguous CUDA tensor of exactly the tensor's byte count, on the tensor's device and 16-byte aligned.
    Anything else raises GpuarError.  (A base of an empty tensor counts as none.)  This function never launches."""
    tensors = list(tensors)
    if base is None:
        return None
    if not isinstance(base, (list, tuple)):
        raise GpuarError("base: None or a list with a tensor or None per tensor")
    if len(base) != len(tensors):
        raise GpuarError(f"base: {len(base)} entries for {len(tensors)} {what}")
    return [0 if b is None else
            _base_pointer(b, i, getattr(t, "device", None), f"{what}[{i}]", lambda: _tensor_bytes(t, f"{what}[{i}]"), f"{what}[{i}]", "tensor")
            for i, (t, b) in enumerate(zip(tensors, base))]


def _base_pointer(t, i, device, where, need, whose, noun):
    """The device pointer of base[i] = `t` (0 where it has no bytes) after the checks every base gets, in compress and in decompress:
    on `device` (where that is known), a contiguous CUDA tensor of exactly need() bytes, 16-byte aligned.  `where`, `whose` and `noun`
    name what it belongs to in the messages."""
    if hasattr(t, "device") and device is not None and t.device != device:
        raise GpuarError(f"base[{i}] is on {t.device}, {where} on {device}")
    have, need = _tensor_bytes(t, f"base[{i}]"), need()
    if have != need:
        raise GpuarError(f"base[{i}] holds {have} bytes, {whose} {need}: a base has exactly its {noun}'s bytes")
    if need and t.data_ptr() % 16:
        raise GpuarError(f"base[{i}] is not 16-byte aligned (data_ptr() % 16 = {t.data_ptr() % 16}); pass an aligned copy")
    return t.data_ptr() if need else 0


class _Split(NamedTuple):
    """What _split returns: the descriptors on the device, d_coded the pointers of the bytes to code, and `hold`: whatever must stay alive
    while the launches run -- the temporary buffer the split copies stand in, the pinned host copy of the descriptors, the modes on the device."""
    d_ptrs: object
    d_bytes: object
    d_fp: object
    d_coded: object
    hold: object = None


class _Batch(NamedTuple):
    """A batch and its filter plan.  describe's five; what _arguments makes of the keywords -- the width per buffer (None: no planes, filter or
    base), the filter flag per buffer (None: no delta filter), the base pointer per buffer (0: none; None: no base), per buffer the modes of
    its supergroups as bytes (None: not mixed) --; what _prepare still has to choose by measurement: `delta_by` the flags (None, "auto" or
    "survey"), `base_by` which bases are kept (None, "auto" or "survey"), `mixed` the modes, with the delta filter offered if `mixed_delta`.
    Behind _prepare every `*_by` is None and the batch also has its _Split, the per-packet estimates of the bytes to code where _auto_base
    made them already (else None) and the status word of every launch so far."""
    device: object
    ptrs: list
    sizes: list
    first_packet: list
    n_packets: int
    widths: list = None
    flags: list = None
    bases: list = None
    modes: list = None
    delta_by: str = None
    base_by: str = None
    mixed: bool = False
    mixed_delta: bool = False
    split: _Split = None
    d_est: object = None
    d_status: object = None

    @property
    def n(self) -> int:
        return len(self.sizes)

    def packets(self, b: int) -> int:
        return self.first_packet[b + 1] - self.first_packet[b]


def _described(tensors, **plan) -> _Batch:
    """describe's five as a _Batch, with what the caller already has of its plan"""
    return _Batch(*describe(list(tensors)), **plan)


def _status_word(a: _Batch):
    """the batch's status word; a new one where nothing was launched for it yet"""
    import torch
    return a.d_status if a.d_status is not None else torch.zeros(1, dtype=torch.int32, device=a.device)


def _modes_tensor(a: _Batch):
    """The batch's modes (per buffer bytes) back to back as one uint8 device tensor (one entry at least)"""
    import torch
    flat = b"".join(a.modes)
    return torch.frombuffer(bytearray(flat or b"\0"), dtype=torch.uint8).to(a.device)


# The filters in front of the coder, in the order in which they win: (hip's split function, hip's merge function, the descriptor rows the
# two take in the widths' place and behind it -- None: the batch has nothing for this filter to do --, the device tensor they take behind
# the first of those rows, if any).  The mixed filter takes every buffer's first mode where the others take its width, and every buffer
# that has bytes; of the others, entry b of a row behind the widths is 0 iff buffer b is not filtered.
_FILTERS = (
    ("split_mixed_batch", "merge_mixed_batch", lambda a: [H.batch_mode_count(a.sizes)[0], a.bases or [0] * a.n] if a.modes is not None else None, _modes_tensor),
    ("split_xor_batch", "merge_xor_batch", lambda a: [a.widths, list(a.bases)] if a.bases is not None and any(a.bases) else None, None),
    ("split_delta_batch", "merge_delta_batch", lambda a: [a.widths, [int(f) for f in a.flags]] if a.flags is not None and any(a.flags) else None, None),
    ("split_planes_batch", "merge_planes_batch", lambda a: [a.widths] if a.widths is not None and any(w != 1 for w in a.widths) else None, None),
)


def _filter(a: _Batch):
    """(split function's name, merge function's name, descriptor rows, device tensor or None) of the filter this batch takes -- mixed, else
    a base over the delta filter over planes alone --; None where nothing is split."""
    for split, merge, rows, beside in _FILTERS:
        found = rows(a)
        if found is not None:
            return split, merge, found, beside(a) if beside is not None else None
    return None


def _filter_arguments(d_rows, d_beside):
    """what a split or merge function takes between the first packets and the counts: the rows on the device, `d_beside` behind the first"""
    return [*d_rows[:1], *([d_beside] if d_beside is not None else []), *d_rows[1:]]


def _split_layout(sizes, moved):
    """(bytes, per buffer its offset or None): the split copies of the buffers that are `moved` and have bytes, back to back (each 16-byte
    aligned); the others (None) are coded where they are."""
    at, places = 0, []
    for size, m in zip(sizes, moved):
        places.append(at if m and size else None)
        at += (size + 15) // 16 * 16 if m and size else 0
    return at, places


def _split(a: _Batch, stream) -> _Split:
    """The batch's descriptors on the device and -- where its plan asks for it -- its buffers split (one launch of the filter's split
    function, into a temporary buffer): into byte planes at `widths`; with `flags` (some of them true) the same launch also filters the
    flagged buffers (hip.split_delta_batch), with `bases` (some of them not 0) it XORs those buffers with their bases (hip.split_xor_batch):
    both get a split copy at any width; with `modes` it splits every supergroup by its mode, and every buffer that has bytes gets a copy."""
    import torch
    found = _filter(a)
    if found is None:
        (d_ptrs, d_bytes, d_fp), keep = _upload(a.device, a.ptrs, a.sizes, a.first_packet)
        return _Split(d_ptrs, d_bytes, d_fp, d_ptrs, keep)
    split, _merge, rows, d_beside = found
    total, places = _split_layout(a.sizes, [a.modes is not None or rows[0][b] != 1 or any(row[b] for row in rows[1:]) for b in range(a.n)])
    d_split = torch.empty(max(total, 16), dtype=torch.uint8, device=a.device)
    coded = [p if at is None else d_split.data_ptr() + at for p, at in zip(a.ptrs, places)]
    (d_ptrs, d_bytes, d_fp, *d_rows, d_coded), keep = _upload(a.device, a.ptrs, a.sizes, a.first_packet, *rows, coded)
    getattr(H, split)(d_ptrs, d_bytes, d_fp, *_filter_arguments(d_rows, d_beside), a.n, a.n_packets, d_coded, stream=stream, d_status=a.d_status)
    return _Split(d_ptrs, d_bytes, d_fp, d_coded, (d_split, d_beside, keep))


def _packets(d_ptrs, d_bytes, d_fp, n_buffers, n_packets):
    """Every batch packet as a buffer of its own, built on the device: (buffer index, pointer, bytes) per packet, int64 -- packet
    j of buffer b is min(8192, bytes[b] - j * 8192) bytes at ptrs[b] + j * 8192."""
    import torch
    device = d_ptrs.device
    counts = d_fp[1:n_buffers + 1] - d_fp[:n_buffers]
    buf = torch.repeat_interleave(torch.arange(n_buffers, dtype=torch.int64, device=device), counts, output_size=n_packets)
    at = (torch.arange(n_packets, dtype=torch.int64, device=device) - d_fp[buf]) * H.PACKET
    return buf, d_ptrs[buf] + at, torch.clamp(d_bytes[buf] - at, max=H.PACKET)


def _stored_auto(stored):
    """`stored` for the functions that take None or "auto" and no list of packets; anything else raises (before any launch)."""
    if stored is not None and stored != "auto":
        raise GpuarError(f"stored={stored!r}: None or \"auto\"")
    return stored


def _stored_argument(stored, n_packets):
    """`stored` as None, "auto" or a list of n_packets bools; anything else raises (before any launch)."""
    if stored is None or _is(stored, "auto"):
        return stored
    if isinstance(stored, str):
        raise GpuarError(f"stored={stored!r}: None, \"auto\" or one bool per packet")
    import torch
    flags = stored.tolist() if isinstance(stored, torch.Tensor) else list(stored)
    if len(flags) != n_packets:
        raise GpuarError(f"stored has {len(flags)} entries, the batch {n_packets} packets")
    return [bool(f) for f in flags]


def _by_kind(d_kind, n_coded, n_stored):
    """The batch packets that are coded, raw and sparse, each in batch order: a stable sort by the kind (0 coded, 1 raw, 2 sparse; any
    integer type) cut at the counts, which the caller has on the host.  No synchronisation."""
    import torch
    order = torch.argsort(d_kind, stable=True)
    return order[:n_coded], order[n_coded:n_coded + n_stored], order[n_coded + n_stored:]


def _partition(d_flags, d_len16, d_slen=None):
    """(n_stored, raw bytes, coded packets, stored packets, n_sparse, sparse bytes, sparse packets): the packets of every kind in
    batch order (_by_kind; one synchronisation for the counts).  d_slen: the bytes of
    every packet's sparse record; None where no packet is sparse (d_flags is then 0 or 1)."""
    import torch
    if d_slen is None:
        n_stored, raw_bytes = torch.stack([d_flags.sum(), (d_len16 * d_flags).sum()]).tolist()
        n_sparse = sparse_bytes = 0
    else:
        d_raw, d_sparse = (d_flags == H.KIND_RAW).to(torch.int64), (d_flags == H.KIND_SPARSE).to(torch.int64)
        n_stored, raw_bytes, n_sparse, sparse_bytes = torch.stack([d_raw.sum(), (d_len16 * d_raw).sum(), d_sparse.sum(), (d_slen * d_sparse).sum()]).tolist()
    coded, kept, packed = _by_kind(d_flags, d_flags.numel() - n_stored - n_sparse, n_stored)
    return n_stored, raw_bytes, coded, kept, n_sparse, sparse_bytes, packed


def _sparse_argument(sparse, stored):
    """`sparse` as None or "auto"; anything else raises (before any launch), and so does sparse="auto" beside a list of stored
    packets: the rule that chooses a packet's kind needs the estimate."""
    if sparse is None:
        return None
    if not _is(sparse, "auto"):
        raise GpuarError(f"sparse={sparse!r}: None or \"auto\"")
    if stored is not None and not _is(stored, "auto"):
        raise GpuarError("sparse=\"auto\" goes with stored=None or stored=\"auto\", not with a list of stored packets")
    return sparse


def _kinds(d_scan, d_est, d_len, stored_on):
    """hip.sparse_rule on the device: (kind, sparse record bytes) per packet, int64, from the scan words, the estimates and the
    packets' lengths.  d_scan None: no packet is sparse -- the rule of stored="auto" alone, (kind, None)."""
    import torch
    raw_ok = (d_est >= 4 + d_len) if stored_on else torch.zeros_like(d_len, dtype=torch.bool)
    if d_scan is None:
        return torch.where(raw_ok, H.KIND_RAW, H.KIND_CODED), None
    scan = d_scan.to(torch.int64) & 0xFFFFFFFF
    d_slen = (4 + 3 * (scan >> 8) + 3) & ~3
    is_sparse = (scan != H.SPARSE_NONE) & (d_slen + 1 < d_est) & (~raw_ok | (d_slen < d_len))
    return torch.where(is_sparse, H.KIND_SPARSE, torch.where(raw_ok, H.KIND_RAW, H.KIND_CODED)), d_slen


def _counts_as(d_est, d_len, stored_on, d_scan=None):
    """The counting rule: what every packet counts as in a predicted size, from the per-packet estimates (int64; one row, or the surveys'
    4 k rows), the packets' lengths and -- where sparse packets count -- the scan words (shaped as the estimates): as _kinds would keep
    it, a sparse packet as its record's bytes, a raw one as its own bytes, a coded one as its estimate."""
    import torch
    if d_scan is None and not stored_on:
        return d_est
    d_kind, d_slen = _kinds(d_scan, d_est, d_len, stored_on)
    counted = torch.where(d_kind == H.KIND_RAW, d_len.expand_as(d_est), d_est)
    return counted if d_slen is None else torch.where(d_kind == H.KIND_SPARSE, d_slen, counted)


def _per_buffer(d_est, buf, n):
    """d_est (one int64 per batch packet, or rows of them) summed over the packets of each of the n buffers (buf: every packet's buffer)"""
    import torch
    return torch.zeros(d_est.shape[:-1] + (n,), dtype=torch.int64, device=d_est.device).index_add_(d_est.dim() - 1, buf, d_est)


def _unit_first_packet(n, device):
    import torch
    return torch.arange(n + 1, dtype=torch.int64, device=device)


def _pays(a: _Batch, b, est_with, est_without):
    """The rule of delta="auto", delta="survey" and base_auto for buffer b: est_with + its packets <= est_without, and it has packets."""
    return a.packets(b) > 0 and est_with + a.packets(b) <= est_without


def _both_ways(a: _Batch, other: _Batch, stream, what, keep):
    """The batch split and estimated twice, without filter or base and as `other` -- the same batch with the flags or bases to try -- says:
    two split launches, two estimate_batch launches, one synchronisation; raises on any status bit, naming `what`.  Returns (the per-buffer
    totals without, those with, every packet's buffer, both _Splits, both per-packet estimates).  Without `keep` the last two are empty and
    the first split copy is freed in front of the second split; with it both copies stay (twice the temporary memory)."""
    import torch
    halves, estimates, totals = [], [], []
    for way in (a._replace(flags=None, bases=None), other):
        s = _split(way, stream)
        d_est = H.estimate_batch(s.d_coded, s.d_bytes, s.d_fp, a.n, a.n_packets, stream=stream, d_status=a.d_status, device=a.device)[:a.n_packets].to(torch.int64)
        buf, _ptr, _len = _packets(s.d_coded, s.d_bytes, s.d_fp, a.n, a.n_packets)
        totals.append(_per_buffer(d_est, buf, a.n))
        if keep:
            halves.append(s)
            estimates.append(d_est)
        del s                                              # (not kept: the split copy is freed in front of the next)
    without, with_ = torch.stack(totals).tolist()
    _raise_on_status(a.d_status, what)
    return without, with_, buf, halves, estimates


def _auto_delta(a: _Batch, stream):
    """delta="auto": per buffer, whether the filter is predicted to pay.  The batch is split and estimated twice, without and
    with the filter (_both_ways, neither copy kept), and a buffer takes the filter iff est_delta + its packets <= est_plain: one byte per
    packet is the estimate's resolution (as in choose_planes), and a tie goes to no filter."""
    if a.n_packets == 0:
        return [False] * a.n
    plain, filtered, *_rest = _both_ways(a, a._replace(flags=[True] * a.n), stream, "split_delta_batch", False)
    return [_pays(a, b, filtered[b], plain[b]) for b in range(a.n)]


def _auto_base(a: _Batch, stream):
    """base_auto=True: per buffer, whether its base is predicted to pay, and the batch split accordingly.  The batch is split and
    estimated twice, without and with the bases -- one split launch and one estimate launch more than the path with fixed bases and
    stored="auto" takes, and one synchronisation -- and a buffer keeps its base iff est_xor + its packets <= est_plain (the rule
    of _auto_delta; a tie goes to no base).  Nothing is split a third time: both split copies are kept (twice the temporary
    memory until the slots are freed) and every buffer is coded from the copy of its choice.  Returns (the choices, what _split
    returns with d_coded made of both copies and both held, the chosen copy's per-packet estimates); (all False, None, None)
    where there is nothing to choose."""
    import torch
    if a.n_packets == 0 or not any(a.bases):
        return [False] * a.n, None, None
    plain, xored, buf, (without, with_), estimates = _both_ways(a, a, stream, "split_xor_batch", True)
    keep = [bool(a.bases[b]) and _pays(a, b, xored[b], plain[b]) for b in range(a.n)]
    (d_keep,), pinned = _upload(a.device, [int(k) for k in keep])
    d_keep = d_keep != 0
    d_coded = torch.where(d_keep, with_.d_coded, without.d_coded)
    d_est = torch.where(d_keep[buf], estimates[1], estimates[0])
    return keep, _Split(with_.d_ptrs, with_.d_bytes, with_.d_fp, d_coded, (without.hold, with_.hold, pinned)), d_est


def _arguments(tensors, planes, stored, delta, base, base_auto, stream, sparse=None) -> _Batch:
    """The host step compress and estimate share: what both refuse of base, tensors, planes and delta, in this order and before any
    launch -- base_auto without a base, a base_auto that is a string other than "survey", a base beside `delta`, whatever base_pointers, describe, plane_widths and delta_flags refuse --,
    and planes="survey" resolved: the one step here that launches, on `stream`, with a `stored` that no caller takes refused in front
    of it.  A filter or a base without `planes` works on bytes (width 1).  With base_auto="survey" the same step chooses width and
    base together (survey_base_choice; `sparse` is what its totals count), and `base_by` has nothing left to choose."""
    import torch
    if base is None and base_auto:
        raise GpuarError("base_auto=True needs base=[...]")
    if isinstance(base_auto, str) and base_auto != "survey":
        raise GpuarError(f"base_auto={base_auto!r}: False, True or \"survey\"")
    mixed = _is(planes, "mixed")
    if _is(delta, "mixed") and not mixed:
        raise GpuarError("delta=\"mixed\" goes with planes=\"mixed\"")
    if mixed and delta is not None and not _is(delta, "mixed"):
        raise GpuarError(f"planes=\"mixed\" chooses the filter per supergroup: delta=None or \"mixed\", not {delta!r}")
    if mixed and base_auto:
        raise GpuarError("planes=\"mixed\" chooses the base per supergroup: base_auto has nothing left to choose")
    if base is not None and delta is not None and not mixed:
        raise GpuarError("base together with delta: that combination is not built (DESIGN.md 4.10)")
    a = _described(tensors, bases=base_pointers(tensors, base))
    if mixed:
        a = a._replace(mixed=True, mixed_delta=delta is not None)
    else:
        base_by = None if a.bases is None or not base_auto else "survey" if _is(base_auto, "survey") else "auto"
        if _is(planes, "survey"):
            stored = _stored_argument(stored, a.n_packets)
            with _on(stream):
                if _is(delta, "survey"):
                    planes, delta = _survey_choice(a, stored)
                elif base_by == "survey":
                    planes, kept = _survey_base_choice(a, stored if _is(stored, "auto") else None, sparse if _is(sparse, "auto") else None)
                    a, base_by = a._replace(bases=[q if keep else 0 for q, keep in zip(a.bases, kept)]), None
                else:
                    planes = _survey_widths(a, stored)
        widths = plane_widths(tensors, planes)
        if widths is None and (delta is not None or a.bases is not None):
            widths = [1] * a.n
        delta_by = delta if isinstance(delta, str) and delta in ("auto", "survey") else None
        a = a._replace(widths=widths, flags=None if delta_by else delta_flags(tensors, delta), delta_by=delta_by, base_by=base_by)
    if a.device is None:
        a = a._replace(device=torch.device("cuda", torch.cuda.current_device()))
    return a


def _prepare(a: _Batch, stream) -> _Batch:
    """The device step compress and estimate share, on the current stream (`stream`, where the caller is in its context): `a` with
    everything chosen that was left to measurement -- the modes of a mixed batch (_survey_mixed), the flags of delta="auto" / "survey", the
    bases base_auto keeps -- and with the batch split: by _auto_base where that has split it both ways, else by one _split."""
    import torch
    a = a._replace(d_status=torch.zeros(1, dtype=torch.int32, device=a.device))
    if a.mixed:
        a = a._replace(modes=[m for m, _total in _survey_mixed(a, a.mixed_delta)])
    if a.delta_by is not None:
        a = a._replace(flags=_auto_delta(a, stream) if a.delta_by == "auto" else _survey_delta_flags(a), delta_by=None)
    if a.base_by is not None:
        keep, split, d_est = _auto_base(a, stream) if a.base_by == "auto" else (_survey_base_keep(a), None, None)
        a = a._replace(bases=[q if k else 0 for q, k in zip(a.bases, keep)], base_by=None, split=split, d_est=d_est)
    return a if a.split is not None else a._replace(split=_split(a, stream))


def _survey_totals(a: _Batch, stored, plain, widths, what):
    """Per buffer the four totals of the plane survey (if `plain`) and of the delta survey at `widths` (if not None; a width
    that was not asked for: 0): one hip.survey_planes_batch launch, one hip.survey_delta_batch launch, one synchronisation, on the
    current stream.  stored="auto" (any other value: as None) counts a packet that would be kept raw as its own bytes.  Raises on any
    status bit, naming `what`."""
    import torch
    n, n_packets, device, d_status = a.n, a.n_packets, a.device, _status_word(a)
    (d_ptrs, d_bytes, d_fp), _keep = _upload(device, a.ptrs, a.sizes, a.first_packet)
    rows = []
    if plain:
        rows.append(H.survey_planes_batch(d_ptrs, d_bytes, d_fp, n, n_packets, d_status=d_status, device=device))
    if widths is not None:
        d_est = torch.zeros((len(H.SURVEY_WIDTHS), n_packets), dtype=torch.int32, device=device)
        rows.append(H.survey_delta_batch(d_ptrs, d_bytes, d_fp, n, n_packets, d_est=d_est, d_status=d_status, device=device, widths=widths))
    d_est = (rows[0] if len(rows) == 1 else torch.cat(rows)).to(torch.int64)
    buf, _ptr, d_len = _packets(d_ptrs, d_bytes, d_fp, n, n_packets)      # (a packet of a split layout has its original's length)
    both = _totals_per_buffer(_counts_as(d_est, d_len, _is(stored, "auto")), buf, n, d_status, what)
    return (both[0] if plain else None), (both[-1] if widths is not None else None)


def _totals_per_buffer(d_est, buf, n, d_status, what):
    """The surveys' one synchronisation: d_est (4 k rows of one int64 per batch packet, k surveys one under the other) summed over
    the packets of each of the n buffers (buf: every packet's buffer), as [survey][buffer][four totals]; raises on any status bit,
    naming `what`."""
    import torch
    *flat, flags = torch.cat([_per_buffer(d_est, buf, n).t().reshape(-1), d_status.to(torch.int64)]).tolist()      # the one synchronisation
    if flags:
        _raise_on_status(d_status, what)
    per = len(flat) // n
    return [[flat[per * b + 4 * k:per * b + 4 * k + 4] for b in range(n)] for k in range(per // 4)]


def _survey_xor_totals(a: _Batch, stored, sparse, plain, what):
    """Per buffer the four totals of the XOR survey against the batch's bases (one pointer per buffer, 0: none) and, if `plain`, the four
    of the bytes as they are: (plain or None, xored).  One hip.survey_xor_batch launch, for `plain` one launch more -- hip.survey_planes_batch,
    or, where sparse packets count, the XOR survey with base pointers of 0, which also gives scan words --, one synchronisation, on
    the current stream.  stored="auto" and sparse="auto" (any other value: as None) count every packet as _kinds' rule would keep
    it at that width: its record, its own bytes or its estimate (_counts_as).  Raises on any status bit, naming `what`."""
    import torch
    n, n_packets, device, d_status = a.n, a.n_packets, a.device, _status_word(a)
    count_sparse, stored_on = _is(sparse, "auto"), _is(stored, "auto")
    (d_ptrs, d_bytes, d_fp, d_bases, d_none), _keep = _upload(device, a.ptrs, a.sizes, a.first_packet, list(a.bases), [0] * n)
    want_scan = None if count_sparse else False
    sides = []
    if plain and count_sparse:
        sides.append(H.survey_xor_batch(d_ptrs, d_bytes, d_fp, d_none, n, n_packets, d_status=d_status, device=device))
    elif plain:
        sides.append((H.survey_planes_batch(d_ptrs, d_bytes, d_fp, n, n_packets, d_status=d_status, device=device), None))
    sides.append(H.survey_xor_batch(d_ptrs, d_bytes, d_fp, d_bases, n, n_packets, d_scan=want_scan, d_status=d_status, device=device))
    buf, _ptr, d_len = _packets(d_ptrs, d_bytes, d_fp, n, n_packets)      # (a packet of a split layout has its original's length)
    rows = [_counts_as(d_est[:, :n_packets].to(torch.int64), d_len, stored_on, d_scan[:, :n_packets] if count_sparse else None)
            for d_est, d_scan in sides]
    both = _totals_per_buffer(torch.cat(rows), buf, n, d_status, what)
    return (both[0] if plain else None), both[-1]


def _survey_pays(a: _Batch, keyword, offered, measure):
    """delta="survey" and base_auto="survey" with the widths fixed: per buffer, whether what is `offered` to it (the filter; its base) is
    predicted to pay at the buffer's width -- the decision of _auto_delta and _auto_base, est_with + its packets <= est_plain on coded
    estimates, from the (plain, with) totals of two surveys of the original bytes, which `measure` makes: two launches and one
    synchronisation, no split and no temporary.  A width the surveys do not have raises before any launch, naming `keyword`."""
    if a.n_packets == 0 or not any(offered):
        return [False] * a.n
    if any(w not in H.SURVEY_WIDTHS for w in a.widths):
        raise GpuarError(f"{keyword}=\"survey\": the widths are {H.SURVEY_WIDTHS}, not {sorted(set(a.widths) - set(H.SURVEY_WIDTHS))}")
    plain, tried = measure()
    rows = [H.SURVEY_WIDTHS.index(w) for w in a.widths]
    return [bool(offered[b]) and _pays(a, b, tried[b][j], plain[b][j]) for b, j in enumerate(rows)]


def _survey_delta_flags(a: _Batch):
    """delta="survey" with the widths fixed (_survey_pays): the plane survey and the delta survey masked to the widths in use"""
    used = sorted({w for w, size in zip(a.widths, a.sizes) if size})
    return _survey_pays(a, "delta", [True] * a.n, lambda: _survey_totals(a, None, True, used, "survey_delta_batch"))


def _survey_base_keep(a: _Batch):
    """base_auto="survey" with the widths fixed (_survey_pays): the plane survey and the XOR survey; a buffer without a base keeps none"""
    return _survey_pays(a, "base_auto", a.bases, lambda: _survey_xor_totals(a, None, None, True, "survey_xor_batch"))


def _chosen_together(a: _Batch, offered, measure):
    """Width and filter together: per buffer the (width, taken) hip.choose_filter picks from the (plain, with) totals `measure` makes --
    two survey launches and one synchronisation --, as (widths, taken); a buffer with nothing `offered` gets hip.choose_planes' width
    of its plain totals, and a batch without packets (1, False) throughout, without a launch."""
    if a.n_packets == 0:
        return [1] * a.n, [False] * a.n
    plain, tried = measure()
    choices = [H.choose_filter(plain[b], tried[b], a.packets(b)) if offered[b] else (H.choose_planes(plain[b], a.packets(b)), False)
               for b in range(a.n)]
    return [w for w, _t in choices], [t for _w, t in choices]


# survey, survey_widths, survey_choice and survey_base_choice on a batch that is described already: what _arguments calls too
def _survey_plain(a: _Batch, stored):
    if a.n_packets == 0:
        return [[0] * len(H.SURVEY_WIDTHS) for _ in a.sizes]
    return _survey_totals(a, stored, True, None, "survey_planes_batch")[0]


def _survey_widths(a: _Batch, stored):
    return [H.choose_planes(totals, a.packets(b)) for b, totals in enumerate(_survey_plain(a, "auto" if _is(stored, "auto") else None))]


def _survey_choice(a: _Batch, stored):
    return _chosen_together(a, [True] * a.n, lambda: _survey_totals(a, stored, True, H.SURVEY_WIDTHS, "survey_delta_batch"))


def _survey_base_choice(a: _Batch, stored, sparse):
    return _chosen_together(a, a.bases, lambda: _survey_xor_totals(a, stored, sparse, True, "survey_xor_batch"))


def survey(tensors, stored=None) -> list:
    """What every tensor would compress to at each byte-plane width, without splitting or encoding anything: per tensor the four
    predicted totals [T1, T2, T4, T8], T_w = estimate([t], planes=w, stored=stored)[0].  One hip.survey_planes_batch launch over
    the original bytes and one synchronisation.  stored="auto" counts a packet that would be kept raw as its own bytes."""
    stored = _stored_auto(stored)
    return _survey_plain(_described(tensors), stored)


def survey_widths(tensors, stored=None) -> list:
    """planes="survey": per tensor the width hip.choose_planes picks from survey(tensors, stored) (an empty tensor: 1)."""
    return _survey_widths(_described(tensors), stored)


def survey_delta(tensors, stored=None, widths=None) -> list:
    """What every tensor would compress to WITH the delta filter at each byte-plane width, without filtering, splitting or
    encoding anything: per tensor [D1, D2, D4, D8], D_w = estimate([t], planes=w, delta=True, stored=stored)[0], with None where
    `widths` (default: all four) does not ask for w.  One hip.survey_delta_batch launch over the original bytes and one
    synchronisation.  stored="auto" counts a packet that would be kept raw as its own bytes."""
    stored = _stored_auto(stored)
    widths = tuple(H.SURVEY_WIDTHS if widths is None else widths)
    H.widths_mask(widths)
    a = _described(tensors)
    if a.n_packets == 0:
        return [[0 if w in widths else None for w in H.SURVEY_WIDTHS] for _ in a.sizes]
    _plain, filtered = _survey_totals(a, stored, False, widths, "survey_delta_batch")
    return [[t if w in widths else None for w, t in zip(H.SURVEY_WIDTHS, row)] for row in filtered]


def survey_choice(tensors, stored=None):
    """planes="survey" with delta="survey": per tensor the (width, filter) hip.choose_filter picks from both surveys of its bytes
    (an empty tensor: (1, False)), as (widths, flags).  Two launches and one synchronisation."""
    return _survey_choice(_described(tensors), stored)


def _survey_xor_arguments(tensors, base, stored, sparse):
    """What survey_xor, survey_xor_widths and survey_base_choice refuse, before any launch, and the batch's description with its base pointers"""
    tensors = list(tensors)
    stored = _stored_auto(stored)
    sparse = _sparse_argument(sparse, stored)
    if base is None:
        raise GpuarError("survey_xor needs base=[...]")
    bases = base_pointers(tensors, base)
    return _described(tensors, bases=bases), stored, sparse


def _survey_xor(a: _Batch, stored, sparse):
    if a.n_packets == 0:
        return [[0] * len(H.SURVEY_WIDTHS) for _ in a.sizes]
    return _survey_xor_totals(a, stored, sparse, False, "survey_xor_batch")[1]


def survey_xor(tensors, base, stored=None, sparse=None) -> list:
    """What every tensor would compress to XORed against its base at each byte-plane width, without XORing, splitting or encoding
    anything: per tensor [X1, X2, X4, X8], X_w = estimate([t], planes=w, base=[b], stored=stored, sparse=sparse)[0]; a tensor whose
    base is None gets its plain totals.  One hip.survey_xor_batch launch over the original bytes and the bases, and one
    synchronisation; _kinds' rule is applied per width on the device, from the survey's est and scan rows."""
    return _survey_xor(*_survey_xor_arguments(tensors, base, stored, sparse))


def survey_xor_widths(tensors, base, stored=None, sparse=None) -> list:
    """For a caller who keeps the bases: per tensor the width hip.choose_planes picks from survey_xor's totals -- the width of the
    bytes that are coded, not of the original ones (an empty tensor: 1)."""
    a, stored, sparse = _survey_xor_arguments(tensors, base, stored, sparse)
    return [H.choose_planes(totals, a.packets(b)) for b, totals in enumerate(_survey_xor(a, stored, sparse))]


def survey_base_choice(tensors, base, stored=None, sparse=None):
    """planes="survey" with base_auto="survey": per tensor the (width, base kept) hip.choose_filter picks from the totals of its
    bytes as they are and XORed against its base (an empty tensor or one without a base: its plain width, no base), as (widths,
    kept).  Two launches and one synchronisation; with sparse="auto" both sides count sparse packets."""
    return _survey_base_choice(*_survey_xor_arguments(tensors, base, stored, sparse))


def _survey_mixed(a: _Batch, delta):
    """Per buffer (its modes as bytes, their predicted totals summed): the plane survey, the delta survey if `delta`, the XOR survey
    if some buffer has a base (the batch's bases: one pointer per buffer, 0: none; or None) -- a buffer without one gets its plane rows
    there, which never win --, then one hip.choose_modes_batch launch and one synchronisation, on the current stream."""
    import torch
    n, n_packets, device = a.n, a.n_packets, a.device
    first_mode, n_modes = H.batch_mode_count(a.sizes)
    if n_packets == 0:
        return [(b"", 0)] * n
    d_status = _status_word(a)
    (d_ptrs, d_bytes, d_fp, d_fm, d_bases), _keep = _upload(device, a.ptrs, a.sizes, a.first_packet, first_mode, a.bases or [0] * n)
    d_plain = H.survey_planes_batch(d_ptrs, d_bytes, d_fp, n, n_packets, d_status=d_status, device=device)
    d_delta = H.survey_delta_batch(d_ptrs, d_bytes, d_fp, n, n_packets, d_status=d_status, device=device) if delta else None
    d_xored = None
    if a.bases is not None and any(a.bases):
        d_xored, _scan = H.survey_xor_batch(d_ptrs, d_bytes, d_fp, d_bases, n, n_packets, d_scan=False, d_status=d_status, device=device)
    d_modes, d_totals = H.choose_modes_batch(d_plain, d_delta, d_xored, d_bytes, d_fp, d_fm, n, n_packets, n_modes, d_status=d_status)
    *flat, flags = torch.cat([d_modes.to(torch.int64), d_totals.to(torch.int64), d_status.to(torch.int64)]).tolist()      # the one synchronisation
    if flags:
        _raise_on_status(d_status, "choose_modes_batch")
    modes, totals = flat[:n_modes], flat[n_modes:]
    return [(bytes(modes[first_mode[b]:first_mode[b + 1]]), sum(totals[first_mode[b]:first_mode[b + 1]])) for b in range(n)]


def survey_mixed(tensors, delta=False, base=None) -> list:
    """What compress(tensors, planes="mixed", ...) would choose, without splitting or encoding anything: per tensor (modes, total) --
    the mode byte of every supergroup of 65536 bytes as bytes (hip.mode_parts) and the predicted compressed bytes under those
    modes.  `delta`: offer the delta filter (delta="mixed"); `base`: as compress, offer the base to the tensors that have one.  The
    surveys' launches over the original bytes, one hip.choose_modes_batch launch and one synchronisation.  The total is at most the
    lowest total any single (width, filter) offered gives the tensor, plus two bytes per packet (gpuar_amd/csrc/mixed.h)."""
    tensors = list(tensors)
    return _survey_mixed(_described(tensors, bases=base_pointers(tensors, base)), bool(delta))


def estimate(tensors, planes=None, stored=None, delta=None, base=None, base_auto=False, sparse=None) -> list:
    """The predicted compressed bytes of every tensor, without encoding anything: the sum of hip.estimate_batch's per-packet
    estimates (the packets' 4-byte headers included) over the tensor's packets -- of its bytes split into planes if `planes`
    asks for it (as compress), and with stored="auto" counting a packet that would be kept raw as its own bytes.  One
    split_planes_batch launch if asked for, one estimate_batch launch (planes="survey": survey's launch in front).  `delta`: as
    compress -- the estimate is that of the filtered, split bytes (delta="auto", "survey": of each tensor's better half).  `base`,
    `base_auto`: as compress -- the estimate is that of the XORed, split bytes (base_auto: of each tensor's better half, from
    _auto_base's two split and two estimate launches alone).  `sparse`: None | "auto": as compress -- one hip.sparse_scan_batch
    launch more, and a packet that would be kept sparse counts as its record's bytes."""
    import torch
    stored = _stored_auto(stored)                                # (no list of stored packets: compress alone takes one)
    sparse = _sparse_argument(sparse, stored)
    a = _arguments(list(tensors), planes, stored, delta, base, base_auto, None, sparse)
    if a.n_packets == 0:
        return [0] * a.n
    a = _prepare(a, None)
    d_coded, d_bytes, d_fp = a.split.d_coded, a.split.d_bytes, a.split.d_fp
    d_est = a.d_est
    if d_est is None:
        d_est = H.estimate_batch(d_coded, d_bytes, d_fp, a.n, a.n_packets, d_status=a.d_status, device=a.device).to(torch.int64)
    buf, _ptr, d_len = _packets(d_coded, d_bytes, d_fp, a.n, a.n_packets)
    d_scan = H.sparse_scan_batch(d_coded, d_bytes, d_fp, a.n, a.n_packets, d_status=a.d_status, device=a.device) if sparse == "auto" else None
    totals = _per_buffer(_counts_as(d_est[:a.n_packets], d_len, stored == "auto", d_scan), buf, a.n)
    _raise_on_status(a.d_status, "estimate_batch")
    return totals.tolist()


def _encode_kinds(a: _Batch, stored, sparse, mode, stream):
    """compress with `stored` or `sparse`: every packet a buffer of its own, and the packets go three ways, each in batch order -- the coded
    ones to the encoder, the raw ones to the copy (hip.move_packets), the sparse ones into records (hip.sparse_pack).  The kinds are
    _kinds' (from one estimate_batch launch -- _auto_base's, where that made one -- and, with sparse="auto", one hip.sparse_scan_batch
    launch on the bytes that would be coded) or the caller's list of stored packets; _partition makes the one synchronisation.  Returns
    Compressed's (stream, offsets, stored, raw, raw_offsets, sparse, sparse_offsets)."""
    import torch
    device, n, n_packets, d_status = a.device, a.n, a.n_packets, a.d_status
    d_coded, d_bytes, d_fp = a.split.d_coded, a.split.d_bytes, a.split.d_fp
    _buf, d_pkt_ptr, d_pkt_len = _packets(d_coded, d_bytes, d_fp, n, n_packets)
    d_scan = d_slen = d_sparse = d_sparse_offsets = None
    if stored == "auto" or sparse == "auto":
        d_est = a.d_est if a.d_est is not None else \
            H.estimate_batch(d_coded, d_bytes, d_fp, n, n_packets, stream=stream, d_status=d_status, device=device)
        if sparse == "auto":
            d_scan = H.sparse_scan_batch(d_coded, d_bytes, d_fp, n, n_packets, stream=stream, d_status=d_status, device=device)
        d_flags, d_slen = _kinds(d_scan, d_est[:n_packets], d_pkt_len, stored == "auto")
    else:
        d_flags = torch.tensor(stored, dtype=torch.int64).to(device)
    d_len16 = (d_pkt_len + 15) // 16 * 16
    n_stored, raw_bytes, coded, kept, n_sparse, sparse_bytes, packed = _partition(d_flags, d_len16, d_slen)
    n_coded = n_packets - n_stored - n_sparse
    d_stream, d_offsets = torch.empty(0, dtype=torch.uint8, device=device), torch.zeros(1, dtype=torch.int64, device=device)
    if n_coded:
        d_slots = H.encode_batch(d_pkt_ptr[coded], d_pkt_len[coded], _unit_first_packet(n_coded, device), n_coded, n_coded, stream=stream,
                                 d_status=d_status, mode=mode, device=device)
        d_stream, d_offsets = H.compact(d_slots, n_coded, stream=stream)
    d_raw = torch.zeros(raw_bytes, dtype=torch.uint8, device=device)           # (zeros: the pads behind partial packets)
    d_raw_offsets = _offsets(d_len16[kept])
    if n_stored:
        H.move_packets(d_pkt_ptr[kept], d_raw.data_ptr() + d_raw_offsets[:n_stored], d_pkt_len[kept], n_stored, stream=stream, d_status=d_status)
    if sparse == "auto":
        d_sparse = torch.empty(sparse_bytes, dtype=torch.uint8, device=device)         # (sparse_pack writes every byte, the pads too)
        d_sparse_offsets = _offsets(d_slen[packed])
        if n_sparse:
            H.sparse_pack(d_pkt_ptr[packed], d_pkt_len[packed], d_scan[:n_packets][packed], d_sparse.data_ptr() + d_sparse_offsets[:n_sparse],
                          n_sparse, stream=stream, d_status=d_status)
    return d_stream, d_offsets, d_flags.to(torch.uint8), d_raw, d_raw_offsets, d_sparse, d_sparse_offsets


def _decode_kinds(c: Compressed, d_ptrs, d_sizes, d_fp, stream, d_status):
    """_encode_kinds' mirror in decompress: every packet a buffer of its own towards the outputs (its room: the packet's own bytes) -- the
    coded ones are decoded, the raw ones copied, the sparse ones rebuilt from their records (hip.sparse_unpack)."""
    device = c.stream.device
    _buf, d_pkt_ptr, d_pkt_len = _packets(d_ptrs, d_sizes, d_fp, c.n_buffers, c.n_packets)
    n_coded = c.offsets.numel() - 1
    n_sparse = c.sparse_offsets.numel() - 1 if c.sparse_offsets is not None else 0
    n_stored = c.n_packets - n_coded - n_sparse
    coded, kept, packed = _by_kind(c.stored, n_coded, n_stored)
    if n_coded:
        H.decode_stream_batch(c.stream, c.offsets, _unit_first_packet(n_coded, device), n_coded, n_coded, d_pkt_ptr[coded], d_pkt_len[coded],
                              stream=stream, d_status=d_status)
    if n_stored:
        H.move_packets(c.raw.data_ptr() + c.raw_offsets[:n_stored], d_pkt_ptr[kept], d_pkt_len[kept], n_stored, stream=stream, d_status=d_status)
    if n_sparse:
        H.sparse_unpack(c.sparse.data_ptr() + c.sparse_offsets[:n_sparse], c.sparse_offsets[1:] - c.sparse_offsets[:n_sparse], d_pkt_ptr[packed],
                        d_pkt_len[packed], n_sparse, stream=stream, d_status=d_status)


def compress(tensors, mode=None, stream=None, checksum=False, planes=None, stored=None, delta=None, base=None, base_auto=False,
             sparse=None) -> Compressed:
    """Encode every tensor of `tensors` (contiguous CUDA tensors on one device, each taken as its bytes) in one launch and
    compact the result.  See Compressed.

    `mode`: "auto" | "throughput" | "latency" (as hip.encode).

    `checksum`: also compute the CRC-32 of every packet (Compressed.crc32; one more launch on the same stream).  The CRCs stay those of
    the original bytes whatever filter is in front.

    `planes`: None | "auto" | a width | one width per tensor (plane_widths) | "survey" | "mixed".  Split each tensor's bytes into byte
    planes of that element width before coding (one more launch, into a temporary buffer that is freed with the slots; widths of 1 are
    coded as they are).  The widths the kernels take are 1, 2, 4 and 8: any other raises from the device's status (BAD_BATCH).
    "survey" (survey_widths): the widths are chosen by a survey of the original bytes, one launch and one synchronisation in front, and
    recorded in Compressed.planes.
    "mixed": width and filter per supergroup of 65536 bytes (survey_mixed, then one hip.split_mixed_batch launch into the usual
    temporary; Compressed.modes): planes alone at the four widths, with delta="mixed" the delta filter too, with `base` the base too --
    here a base and the delta filter go together, a supergroup takes one of them or neither.  Beside it any other `delta` and `base_auto`
    raise before any launch, and so does delta="mixed" without it.

    `stored`: None | "auto" | one bool per batch packet.  Keep packets raw instead of coding them -- "auto": those whose estimate
    (hip.estimate_batch, on the filtered, split bytes) is not smaller than the packet; a sequence: those it names (a wrong length raises
    before any launch).

    `delta`: None | True | False | one bool per tensor | "auto" | "survey" (| "mixed", see `planes`).  Replace the elements of the flagged
    tensors, at the width `planes` gives (planes=None: 1), by their differences inside every group, in the launch that splits
    (hip.split_delta_batch).  "auto" flags the tensors for which two more split and two more estimate launches predict a gain
    (_auto_delta).  "survey" flags the same tensors from two survey launches over the original bytes and one synchronisation, without a
    split or a temporary (_survey_delta_flags), and with planes="survey" chooses width and filter together (survey_choice).  None takes
    exactly the path taken without the keyword.

    `base`: None | a list with, per tensor, None or a contiguous CUDA tensor of exactly the tensor's byte count on its device, 16-byte
    aligned (base_pointers; anything else raises before any launch, and so does a base together with `delta`).  XOR the tensor with it,
    at the width `planes` gives (planes=None: 1), in the launch that splits (hip.split_xor_batch, into the same temporary buffer: inputs
    and bases are never modified).  planes="survey" surveys the original bytes.  None takes exactly the path taken without the keyword.

    `base_auto`: False | True | "survey".  True keeps only the bases for which splitting and estimating the batch both ways predicts a
    gain (_auto_base: one split and one estimate launch more than fixed bases with stored="auto" take, one synchronisation, both split
    copies kept and none made a third time); Compressed.based says which.  "survey" keeps the same bases from one
    hip.survey_planes_batch and one hip.survey_xor_batch launch over the original bytes and one synchronisation, and then splits once: one
    temporary of the batch's size instead of two (_survey_base_keep; a width the surveys do not have, any but 1, 2, 4 and 8, raises before
    any launch, as with delta="survey", where base_auto=True gets BAD_BATCH from the split); with planes="survey" it chooses width and
    base together, on the bytes that would be coded (survey_base_choice), and records both in Compressed.planes and Compressed.based.

    `sparse`: None | "auto" (with stored None or "auto").  Keep the packets that are one byte value almost everywhere as that byte and a
    list of exceptions -- one estimate_batch launch (the one stored="auto" or base_auto made, where there is one) and one
    hip.sparse_scan_batch launch on the bytes that would be coded, hip.sparse_rule on the device, and the packets go three ways: coded,
    raw (hip.move_packets) and sparse (hip.sparse_pack, into Compressed.sparse).  None takes exactly the path taken without the keyword.

    `stored`, `sparse`, `checksum` and `mode` see the split bytes as ever, under planes="mixed" too."""
    a = _arguments(list(tensors), planes, stored, delta, base, base_auto, stream, sparse)
    stored = _stored_argument(stored, a.n_packets)               # (a list of stored packets too: estimate takes none)
    sparse = _sparse_argument(sparse, stored)
    d_stored = d_raw = d_raw_offsets = d_sparse = d_sparse_offsets = None
    with _on(stream):
        a = _prepare(a, stream)
        s, n, n_packets = a.split, a.n, a.n_packets
        if stored is None and sparse is None:
            d_slots = H.encode_batch(s.d_coded, s.d_bytes, s.d_fp, n, n_packets, stream=stream, d_status=a.d_status, mode=mode, device=a.device)
            d_stream, d_offsets = H.compact(d_slots, n_packets, stream=stream)
        else:
            d_stream, d_offsets, d_stored, d_raw, d_raw_offsets, d_sparse, d_sparse_offsets = _encode_kinds(a, stored, sparse, mode, stream)
        d_crc = H.crc32_batch(s.d_ptrs, s.d_bytes, s.d_fp, n, n_packets, stream=stream, d_status=a.d_status, device=a.device) if checksum else None
        _raise_on_status(a.d_status, "encode_batch")
        # compact() wrote into a buffer of n_packets * 8704 bytes: keep only the compressed bytes (one copy), so that the
        # result takes what it compressed to, not ~1.06 x the input
        used = int(d_offsets[-1].item())
        d_stream = d_stream[:used].clone()
    # (the slots and the split copies were held until here; they are freed on return)
    return Compressed(stream=d_stream, offsets=d_offsets, first_packet=a.first_packet, sizes=a.sizes,
                      crc32=d_crc[:n_packets] if d_crc is not None else None, planes=a.widths, stored=d_stored, raw=d_raw,
                      raw_offsets=d_raw_offsets, delta=a.flags, based=_based(a), sparse=d_sparse, sparse_offsets=d_sparse_offsets,
                      kinds_rule=(stored == "auto", sparse == "auto") if isinstance(stored, str) or sparse == "auto" else None, modes=a.modes)


def _based(a: _Batch):
    """Compressed.based of a prepared batch: which buffers were XORed with their base -- in a mixed batch, in some supergroup"""
    if a.bases is None:
        return None
    if a.modes is not None:
        return [any(H.mode_parts(m)[2] for m in modes) for modes in a.modes]
    return [bool(q) for q in a.bases]


def _decompress_bases(c: Compressed, ptrs, base, device):
    """decompress's base pointers (0 for a buffer that needs none), or None for a batch compressed without bases; what is missing, of
    another size, device or alignment, or overlaps a tensor of `out` (at `ptrs`) raises."""
    if c.based is None or not any(c.based):
        return None
    # the outputs as intervals by their start, with the furthest end so far: a base overlaps one iff that end lies behind its start
    spans = sorted((p, p + need, b) for b, (p, need) in enumerate(zip(ptrs, c.sizes)) if need)
    starts, reach = [s for s, _e, _b in spans], []
    for _s, e, b in spans:
        reach.append(max(reach[-1], (e, b)) if reach else (e, b))
    if not isinstance(base, (list, tuple)) or len(base) != c.n_buffers:
        raise GpuarError(f"this batch was compressed against bases: decompress needs base=[...] with {c.n_buffers} entries")
    bases = []
    for b, (t, need) in enumerate(zip(base, c.sizes)):
        if not c.based[b] or need == 0:
            bases.append(0)
            continue
        if t is None:
            raise GpuarError(f"buffer {b} was compressed against a base: base[{b}] is missing")
        at = _base_pointer(t, b, device, "the batch", lambda: need, f"buffer {b} has", "buffer")
        before = bisect.bisect_left(starts, at + need)                     # the outputs that start in front of the base's end
        if before and reach[before - 1][0] > at:
            raise GpuarError(f"base[{b}] overlaps out[{reach[before - 1][1]}]: the merge runs in place in `out` while the bases are read")
        bases.append(at)
    return bases


def decompress(c: Compressed, out=None, stream=None, verify=True, base=None):
    """Decode every buffer of `c` in one launch.  Returns a list of uint8 tensors, or fills the caller's tensors `out` (one per
    buffer, contiguous CUDA tensors of at least the buffer's bytes, 16-byte aligned) and returns them.  When `c` carries CRCs
    and `verify` is true, the decoded bytes are checked against them (one more launch): a mismatch raises GpuarError naming
    the first buffer and packet that differ.  Buffers that were split into byte planes are merged back in place in `out`
    after decoding and before verifying: the CRCs are those of the original bytes; where a buffer went through the delta filter,
    that launch is hip.merge_delta_batch, which also sums the differences up again; a batch compressed with planes="mixed" is merged by
    hip.merge_mixed_batch with its modes.  Packets that were stored raw are copied
    (one more launch), sparse packets rebuilt from their records (hip.sparse_unpack, one more launch; a record that is not valid
    raises: BAD_PACKET), the others decoded.  `base`: as in compress; every buffer with c.based[b] needs base[b], the tensor it
    was compressed against (a missing one, one of another size, device or alignment, or one that overlaps any tensor of `out`
    raises before any launch; entries of the other buffers are ignored); the merge is then hip.merge_xor_batch.  A base with other contents
    cannot be told from damage: with CRCs it is reported as the checksum mismatch, without them it goes unnoticed."""
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
    # the batch towards the outputs, with the plan it was compressed by
    a = _Batch(device, ptrs, c.sizes, c.first_packet, c.n_packets, c.planes, c.delta, _decompress_bases(c, ptrs, base, device), c.modes)
    with _on(stream):
        (d_ptrs, d_room, d_fp, d_sizes), _keep = _upload(device, ptrs, room, c.first_packet, c.sizes)
        d_status = torch.zeros(1, dtype=torch.int32, device=device)
        if c.stored is None:
            H.decode_stream_batch(c.stream, c.offsets, d_fp, c.n_buffers, c.n_packets, d_ptrs, d_room, stream=stream, d_status=d_status)
        elif c.n_packets:
            _decode_kinds(c, d_ptrs, d_sizes, d_fp, stream, d_status)
        _raise_on_status(d_status, "decode_stream_batch")      # (.item() waits for this stream)
        found = _filter(a) if c.n_packets else None
        if found is not None:
            _split_name, merge, rows, d_beside = found
            d_rows, _keep2 = _upload(device, *rows)
            getattr(H, merge)(d_ptrs, d_sizes, d_fp, *_filter_arguments(d_rows, d_beside), c.n_buffers, c.n_packets, d_ptrs, stream=stream, d_status=d_status)
            _raise_on_status(d_status, merge)
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
