"""The sparse-packet kernels against the copy roof and the estimate kernel, and what sparse packets do to batch.compress /
batch.decompress of a bf16 tensor against its base (torch events; the kernels: min of 7 launches, batch: min of 3).

    python tools/sparse_timing.py [--gib G] [--batch-gib B]

Prints, for G GiB (default 8) resident in HBM: the plain device copy (gpuar_hip_copy, the roof bench.py quotes); then on zeros, on
zeros with 0.1 % of the bytes changed and on uniform bytes gpuar_hip_estimate and gpuar_hip_sparse_scan on the same buffer, and -- on
the two buffers whose packets are sparse -- gpuar_hip_sparse_pack of all packets, gpuar_hip_sparse_unpack of all records (checked
against the buffer) and gpuar_hip_move_packets of as many packets as a yardstick.  Then, for B GiB (default 1) of bf16 weights
against a base with 0 %, 0.1 % and 1 % of the elements replaced: batch.compress / batch.decompress with planes=2, stored="auto",
with and without sparse="auto", end to end.  No thresholds: the figures are for the reader.  The last line is the same as JSON.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gpuar_amd import batch  # noqa: E402
from gpuar_amd import hip as H  # noqa: E402

PACKET = 8192


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


def sprinkle(d, share, seed):
    """changes about `share` of the bytes of d (uint8, device) to another value, in pieces"""
    g = torch.Generator(device=d.device).manual_seed(seed)
    piece = 1 << 28
    for at in range(0, d.numel(), piece):
        m = min(piece, d.numel() - at)
        where = torch.randint(0, m, (int(m * share),), generator=g, device=d.device)
        d[at:at + m][where] ^= torch.randint(1, 256, (where.numel(),), generator=g, device=d.device, dtype=torch.uint8)


def bf16_pair(n_bytes, share, dev):
    """(tensor, base): bf16 weights (normal x 0.02), the tensor being the base with `share` of its elements drawn afresh"""
    g = torch.Generator(device=dev).manual_seed(1)
    elements = n_bytes // 2
    base = torch.empty(elements, dtype=torch.bfloat16, device=dev)
    piece = 1 << 26
    for at in range(0, elements, piece):
        m = min(piece, elements - at)
        base[at:at + m] = (torch.randn(m, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    t = base.clone()
    if share:
        where = torch.randint(0, elements, (int(elements * share),), generator=g, device=dev)
        t[where] = (torch.randn(where.numel(), generator=g, device=dev) * 0.02).to(torch.bfloat16)
    return t, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--batch-gib", type=float, default=1.0)
    args = ap.parse_args()
    n = int(args.gib * (1 << 30)) // 65536 * 65536
    dev = torch.device("cuda:0")
    npk = H.packet_count(n)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d_in = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_dst = torch.empty(n, dtype=torch.uint8, device=dev)
    out = {"gib": args.gib, "batch_gib": args.batch_gib}

    copy = best(lambda: H.device_copy(d_in, d_dst, n))
    roof = 2 * n / 1e12 / (copy / 1e3)
    print(f"{args.gib:g} GiB, {npk} packets; copy {copy:.3f} ms = {roof:.2f} TB/s (read + write)")
    out.update(copy_ms=round(copy, 4), copy_roof_tbs=round(roof, 3))

    d_est = torch.empty(npk, dtype=torch.int32, device=dev)
    d_scan = torch.empty(npk, dtype=torch.int32, device=dev)
    index = torch.arange(npk, dtype=torch.int64, device=dev)
    src_p = d_in.data_ptr() + index * PACKET
    dst_p = d_dst.data_ptr() + index * PACKET
    sizes = torch.full((npk,), PACKET, dtype=torch.int64, device=dev)
    for kind in ("zeros", "sparse", "uniform"):
        if kind == "sparse":
            sprinkle(d_in, 0.001, 7)
        elif kind == "uniform":
            H.generate("uniform", 42, n, device=dev, out=d_in)
        est = best(lambda: H.estimate(d_in, d_est=d_est))
        scan = best(lambda: H.sparse_scan(d_in, d_scan=d_scan))
        head = d_in[:4 * PACKET].clone()
        assert [v & 0xFFFFFFFF for v in H.sparse_scan(head).cpu().tolist()] == H.sparse_scan_host(head.cpu().numpy().tobytes())
        print(f"  {kind:8s} estimate {est:7.3f} ms  {n / 1e6 / est:6.0f} GB/s;  sparse_scan {scan:7.3f} ms  {n / 1e6 / scan:6.0f} GB/s read  "
              f"{n / 1e12 / (scan / 1e3) / roof:5.1%} of the copy's rate, {scan / est:.2f} x estimate")
        out.update({f"{kind}_estimate_ms": round(est, 4), f"{kind}_scan_ms": round(scan, 4)})
        if kind == "uniform":
            assert int((d_scan != -1).sum().item()) == 0
            continue
        assert int((d_scan == -1).sum().item()) == 0
        lens = (4 + 3 * (d_scan.to(torch.int64) >> 8) + 3) & ~3
        offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        d_rec = torch.empty(int(offs[-1].item()), dtype=torch.uint8, device=dev)
        rec_p = d_rec.data_ptr() + offs[:npk]
        pack = best(lambda: H.sparse_pack(src_p, sizes, d_scan, rec_p, npk, d_status=status))
        d_dst.fill_(0x5A)
        unpack = best(lambda: H.sparse_unpack(rec_p, lens, dst_p, sizes, npk, d_status=status))
        assert torch.equal(d_dst, d_in)
        move = best(lambda: H.move_packets(src_p, dst_p, sizes, npk, d_status=status))
        print(f"           {d_rec.numel()} bytes of records ({d_rec.numel() / n:.5f} of the size);  sparse_pack {pack:7.3f} ms  {n / 1e6 / pack:6.0f} GB/s read;  "
              f"sparse_unpack {unpack:7.3f} ms  {n / 1e6 / unpack:6.0f} GB/s written;  move_packets {move:7.3f} ms  {n / 1e6 / move:6.0f} GB/s each way")
        out.update({f"{kind}_record_bytes": d_rec.numel(), f"{kind}_pack_ms": round(pack, 4), f"{kind}_unpack_ms": round(unpack, 4),
                    f"{kind}_move_packets_ms": round(move, 4)})
        del d_rec
    assert int(status.item()) == 0
    del d_in, d_dst, d_est, d_scan, src_p, dst_p, sizes, index

    m = int(args.batch_gib * (1 << 30)) // 65536 * 65536
    for share in (0.0, 0.001, 0.01):
        t, base = bf16_pair(m, share, dev)
        outs = [torch.empty(m, dtype=torch.uint8, device=dev)]
        for label, kw in (("stored", {}), ("stored + sparse", {"sparse": "auto"})):
            holder = {}

            def compress():
                holder["c"] = batch.compress([t], planes=2, base=[base], stored="auto", mode="throughput", **kw)
            comp = best(compress, reps=3)
            c = holder["c"]
            dec = best(lambda: batch.decompress(c, out=outs, base=[base]), reps=3)
            assert torch.equal(outs[0], t.view(torch.uint8))
            kinds = torch.bincount(c.stored.to(torch.int64), minlength=3).tolist()
            print(f"  {share:.1%} replaced, batch.compress({label}) {comp:8.3f} ms, decompress {dec:8.3f} ms, {c.nbytes / m:.5f} of the size "
                  f"(coded / raw / sparse packets: {kinds[0]} / {kinds[1]} / {kinds[2]})")
            key = f"replaced_{share:g}_{label.replace(' + ', '_')}"
            out.update({f"{key}_compress_ms": round(comp, 4), f"{key}_decompress_ms": round(dec, 4), f"{key}_ratio": round(c.nbytes / m, 6),
                        f"{key}_kinds": kinds})
            del c, holder
        del t, base, outs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
