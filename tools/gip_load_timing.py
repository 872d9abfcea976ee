"""gpuar_hip_move_bytes -- the kernel that takes the packets of a version-6 .gip stream apart -- against the copy
roof and against kinds_expand, which moves raw packets the same way (torch events, min of 7 launches), and batch.from_gip of one
large version-6 file, end to end.

    python tools/gip_load_timing.py [--gib G] [--file-gib F]

Prints, for G GiB (default 8) resident in HBM: the plain device copy (gpuar_hip_copy, the roof bench.py quotes); then move_bytes on
the three pure cases -- every packet raw (8192 bytes from 4 bytes behind each packet's place in a stream of 8196-byte packets, to
out + 8192 p), every packet coded (lengths 4 .. 8704, byte-aligned source and destination, both back to back), every packet sparse
(records of 4 .. 100 bytes from 4 bytes behind each packet's place, back to back) --, each checked against torch, and kinds_expand on
the all-raw stream.  Then, with --file-gib F > 0 (default 1), from_gip of the version-6 file of F GiB of bf16 weights compressed with
planes=2, stored="auto": the host parse (read_gip), the upload (pinned staging and one copy) and the device step (tables, region
lists, the move, the offsets), each waited for, in wall milliseconds -- a first run, which pins fresh host memory, and the better of
the two behind it -- and from_gip in one call.  No thresholds: the figures are for the reader.  The last line is the same as JSON.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gpuar_amd import batch  # noqa: E402
from gpuar_amd import hip as H  # noqa: E402

PACKET, SLOT = 8192, 8704


def best(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return min(s.elapsed_time(e) for s, e in ev)


def exclusive(lengths):
    return torch.cumsum(lengths, 0) - lengths


def kernels(gib, out):
    n = int(gib * (1 << 30)) // 65536 * 65536
    dev = torch.device("cuda:0")
    npk = n // PACKET
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d_in = H.generate("uniform", 42, n, device=dev)
    d_out = torch.empty(n, dtype=torch.uint8, device=dev)
    copy = best(lambda: H.device_copy(d_in, d_out, n))
    roof = 2 * n / 1e12 / (copy / 1e3)
    print(f"{gib:g} GiB, {npk} packets; copy {copy:.3f} ms = {roof:.2f} TB/s (read + write)")
    out.update(gib=gib, copy_ms=round(copy, 4), copy_roof_tbs=round(roof, 3))
    at = torch.arange(npk, dtype=torch.int64, device=dev)

    def report(case, ms, moved, extra=""):
        per_byte = (ms / moved) / (copy / n)
        print(f"  {case:34s} {ms:8.3f} ms   {2 * moved / 1e9 / ms:6.3f} TB/s in + out   {per_byte:5.2f} x the copy per byte{extra}")
        out.update({f"{case.split(':')[0].replace(' ', '_')}_ms": round(ms, 4), f"{case.split(':')[0].replace(' ', '_')}_bytes": moved})

    # every packet raw: the stream kinds_expand takes too
    d_stream = torch.empty(npk * (PACKET + 4), dtype=torch.uint8, device=dev)
    rows = d_stream.view(npk, PACKET + 4)
    rows[:, 4:] = d_in.view(npk, PACKET)
    rows[:, :4] = torch.tensor([(PACKET + 4) & 255, (PACKET + 4) >> 8, PACKET & 255, PACKET >> 8], dtype=torch.uint8, device=dev)
    src, dst = d_stream.data_ptr() + at * (PACKET + 4) + 4, d_out.data_ptr() + at * PACKET
    lengths = torch.full((npk,), PACKET, dtype=torch.int64, device=dev)
    d_out.fill_(0x5A)
    raw = best(lambda: H.move_bytes(src, dst, lengths, npk, d_status=status))
    assert torch.equal(d_out, d_in), "raw"
    report("move_bytes raw: +4 -> 16-aligned", raw, n)
    d_offsets = torch.arange(npk + 1, dtype=torch.int64, device=dev) * (PACKET + 4)
    d_kind = torch.ones(npk, dtype=torch.uint8, device=dev)
    d_out.fill_(0x5A)
    expand = best(lambda: H.kinds_expand(d_stream, d_offsets, d_kind, npk, d_out, n, d_status=status))
    assert torch.equal(d_out, d_in), "kinds_expand"
    report("kinds_expand raw: the same stream", expand, n, f"   (move_bytes: {raw / expand:4.2f} x kinds_expand)")
    del d_stream, rows, d_offsets, d_kind

    # every packet coded: lengths 4 .. 8704, byte -> byte, both sides back to back from an odd start
    g = torch.Generator(device=dev).manual_seed(7)
    lengths = torch.randint(4, SLOT + 1, (npk,), generator=g, device=dev, dtype=torch.int64)
    lengths = lengths[exclusive(lengths) + lengths + 3 <= n]                  # what fits the buffers
    regions, moved = lengths.numel(), int(lengths.sum().item())
    src, dst = d_in.data_ptr() + 1 + exclusive(lengths), d_out.data_ptr() + 3 + exclusive(lengths)
    d_out.fill_(0x5A)
    coded = best(lambda: H.move_bytes(src, dst, lengths, regions, d_status=status))
    assert torch.equal(d_out[3:3 + moved], d_in[1:1 + moved]) and int(d_out[2].item()) == 0x5A and int(d_out[3 + moved].item()) == 0x5A, "coded"
    report(f"move_bytes coded: byte -> byte, {regions} regions", coded, moved)

    # every packet sparse: records of 4 .. 100 bytes behind a 4-byte header, to back to back
    k = torch.randint(0, 33, (npk,), generator=g, device=dev, dtype=torch.int64)
    lengths = (4 + 3 * k + 3) & ~3
    moved = int(lengths.sum().item())
    src, dst = d_in.data_ptr() + exclusive(lengths + 4) + 4, d_out.data_ptr() + exclusive(lengths)
    sparse = best(lambda: H.move_bytes(src, dst, lengths, npk, d_status=status))
    keep = torch.ones(int((lengths + 4).sum().item()), dtype=torch.bool, device=dev)
    keep[(exclusive(lengths + 4)[:, None] + torch.arange(4, device=dev)[None, :]).reshape(-1)] = False
    assert torch.equal(d_out[:moved], d_in[:keep.numel()][keep]), "sparse"
    report(f"move_bytes sparse: {npk} records, {moved / npk:.1f} bytes each", sparse, moved, f"   ({sparse * 1e6 / npk:.2f} ns a region)")
    assert int(status.item()) == 0
    del d_in, d_out, keep
    torch.cuda.empty_cache()


def wall_ms(fn):
    """(the better of two runs in milliseconds, the last result)"""
    times = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times), result


def file_load(gib, out):
    dev = torch.device("cuda:0")
    elements = int(gib * (1 << 30)) // 65536 * 65536 // 2
    g = torch.Generator(device=dev).manual_seed(1)
    w = (torch.randn(elements, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    c = batch.compress([w], planes=2, stored="auto")
    blob = c.gip(0, kinds=True)
    kinds = torch.bincount(c.stored.to(torch.int64), minlength=3).tolist()
    del c
    def steps():
        """from_gip's three steps, each waited for: (parse, upload, device) in milliseconds, and the result"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parsed = batch._gip_parse([blob])
        t1 = time.perf_counter()
        d_up, _held = batch._gip_upload(parsed, sum(g.stream.size for g in parsed), dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        c2 = batch._gip_assemble(parsed, d_up, dev, None)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3))], c2

    runs = [steps() for _ in range(3)]               # the first run pins fresh host memory for the staging buffer; the others reuse it
    first = runs[0][0]
    (parse, upload, device), c2 = min(runs[1:], key=lambda r: sum(r[0]))
    whole, c3 = wall_ms(lambda: batch.from_gip([blob]))
    back = batch.decompress(c3)[0]
    assert torch.equal(back, w.view(torch.uint8)) and torch.equal(c2.stream, c3.stream) and torch.equal(c2.raw, c3.raw), "the round trip"
    print(f"from_gip of one version-6 file: {2 * elements} bytes of bf16, planes=2, stored=\"auto\" -> {len(blob)} bytes, "
          f"coded / raw / sparse {kinds[0]} / {kinds[1]} / {kinds[2]}\n"
          f"  first run:       host parse {first[0]:8.2f} ms   upload {first[1]:8.2f} ms   device {first[2]:8.2f} ms\n"
          f"  better of two:   host parse {parse:8.2f} ms   upload {upload:8.2f} ms   device {device:8.2f} ms   "
          f"(upload {len(blob) / 1e6 / upload:.1f} GB/s)   from_gip in one call {whole:8.2f} ms")
    out.update(file_gib=gib, file_bytes=len(blob), file_kinds=kinds, first_ms=[round(v, 3) for v in first], parse_ms=round(parse, 3),
               upload_ms=round(upload, 3), device_ms=round(device, 3), from_gip_ms=round(whole, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--file-gib", type=float, default=1.0)
    args = ap.parse_args()
    out = {}
    if args.gib > 0:
        kernels(args.gib, out)
    if args.file_gib > 0:
        file_load(args.file_gib, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
