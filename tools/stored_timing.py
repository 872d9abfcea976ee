"""The estimate and packet-copy kernels against the copy roof and the CRC kernel, and what storing incompressible packets does to
batch.compress / batch.decompress of typed tensors (torch events, min of 7).

    python tools/stored_timing.py [--gib G] [--baseline] [--root DIR]

Prints, for G GiB (default 8) resident in HBM: the plain device copy (gpuar_hip_copy, the roof bench.py quotes) and
crc32_kernel<false> on the same buffer as yardsticks; gpuar_hip_estimate on uniform(42), zeros and text (zeros is the LDS worst
case: its ratio to uniform is printed); gpuar_hip_move_packets on G / 2 GiB of whole packets; then, for bf16 and fp32 weights
(normal x 0.02) split into planes, the kernels alone -- encode of all packets against estimate + encode of the packets the rule
codes + the copy of those it stores, and the same for decode -- and batch.compress / batch.decompress with planes="auto", with
and without stored="auto", end to end.  With --baseline only what exists without the estimate is run (the copy, the CRC, encode
and decode of the split bytes, batch.compress / decompress with planes="auto"), so the same file times a checkout of the commit
in front of this feature: --root DIR imports gpuar_amd from that (built) checkout.  The last line is the same as JSON.
"""
import argparse
import json
import os
import sys

_root = argparse.ArgumentParser(add_help=False)
_root.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.abspath(_root.parse_known_args()[0].root))
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


def weights(dtype, n_bytes, dev):
    """normal x 0.02 of `dtype`, n_bytes of them, made on the device in pieces (a float32 temporary of the whole would be 2-4 x)."""
    out = torch.empty(n_bytes // dtype.itemsize, dtype=dtype, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    piece = 1 << 26
    for at in range(0, out.numel(), piece):
        m = min(piece, out.numel() - at)
        out[at:at + m] = (torch.randn(m, generator=g, device=dev) * 0.02).to(dtype)
    return out


def unit_descriptors(base_ptr, index, dev):
    """one-packet buffers for the whole packets `index` (int64 device tensor) of a buffer at base_ptr"""
    n = index.numel()
    return base_ptr + index * PACKET, torch.full((n,), PACKET, dtype=torch.int64, device=dev), torch.arange(n + 1, dtype=torch.int64, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--baseline", action="store_true", help="only what exists without the estimate (to time the commit in front of it)")
    ap.add_argument("--root", help="the checkout to import gpuar_amd from (default: this file's)")
    args = ap.parse_args()
    n = int(args.gib * (1 << 30)) // 65536 * 65536
    dev = torch.device("cuda:0")
    npk = H.packet_count(n)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d_in = H.generate("uniform", 42, n, device=dev)
    d_dst = torch.empty(n, dtype=torch.uint8, device=dev)
    out = {"gib": args.gib, "baseline": args.baseline}

    copy = best(lambda: H.device_copy(d_in, d_dst, n))
    roof = 2 * n / 1e12 / (copy / 1e3)
    d_crc = torch.empty(npk, dtype=torch.int32, device=dev)
    crc = best(lambda: H.crc32(d_in, d_crc=d_crc))
    print(f"{args.gib:g} GiB, {npk} packets; copy {copy:.3f} ms = {roof:.2f} TB/s (read + write); crc32 {crc:.3f} ms = {n / 1e6 / crc:.0f} GB/s read, "
          f"{n / 1e12 / (crc / 1e3) / roof:.1%} of the copy's rate")
    out.update(copy_ms=round(copy, 4), copy_roof_tbs=round(roof, 3), crc32_ms=round(crc, 4))

    if not args.baseline:
        d_est = torch.empty(npk, dtype=torch.int32, device=dev)
        for kind in ("uniform", "zeros", "text"):
            if kind != "uniform":
                H.generate(kind, 42, n, device=dev, out=d_dst)
            src = d_in if kind == "uniform" else d_dst
            ms = best(lambda: H.estimate(src, d_est=d_est))
            assert H.estimate(src[:4 * PACKET].clone()).cpu().tolist() == H.estimate_host(src[:4 * PACKET].cpu().numpy().tobytes())
            print(f"  estimate {kind:8s} {ms:7.3f} ms  {n / 1e6 / ms:6.0f} GB/s read  {n / 1e12 / (ms / 1e3) / roof:5.1%} of the copy's rate, {ms / crc:.2f} x crc32")
            out[f"estimate_{kind}_ms"] = round(ms, 4)
        print(f"  estimate zeros / uniform = {out['estimate_zeros_ms'] / out['estimate_uniform_ms']:.2f}")
        half = npk // 2
        index = torch.arange(half, dtype=torch.int64, device=dev)
        src_p, sizes, _fp = unit_descriptors(d_in.data_ptr(), index, dev)
        dst_p = d_dst.data_ptr() + index * PACKET
        ms = best(lambda: H.move_packets(src_p, dst_p, sizes, half, d_status=status))
        assert torch.equal(d_in[:half * PACKET], d_dst[:half * PACKET])
        print(f"  move_packets {half} packets ({half * PACKET / 2 ** 30:g} GiB) {ms:7.3f} ms  {2 * half * PACKET / 1e12 / (ms / 1e3):5.2f} TB/s (read + write)  "
              f"{2 * half * PACKET / 1e12 / (ms / 1e3) / roof:5.1%} of the copy")
        out["move_packets_ms"] = round(ms, 4)
    del d_in

    d_slots = torch.empty(npk * H.SLOT, dtype=torch.uint8, device=dev)
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        t = weights(dtype, n, dev)
        w = dtype.itemsize
        H.split_planes(t.view(torch.uint8), w, d_out=d_dst)
        # the kernels alone: everything coded ...
        enc_all = best(lambda: H.encode(d_dst, d_slots, d_status=status, mode="throughput"), reps=5)
        d_stream, d_off = H.compact(d_slots, npk)
        d_back = torch.empty(n, dtype=torch.uint8, device=dev)
        dec_all = best(lambda: H.decode_stream(d_stream, d_off, npk, d_back, d_status=status), reps=5)
        assert torch.equal(d_back, d_dst)
        all_bytes = int(d_off[-1].item())
        print(f"{name}: split into {w} planes; all {npk} packets coded: encode {enc_all:.3f} ms, decode {dec_all:.3f} ms, {all_bytes / n:.4f} of the size")
        out.update({f"{name}_encode_all_ms": round(enc_all, 4), f"{name}_decode_all_ms": round(dec_all, 4), f"{name}_ratio_all": round(all_bytes / n, 5)})
        del d_stream, d_off
        if not args.baseline:
            # ... against estimate + the coded packets through one-packet descriptors + the copy of the stored ones
            d_est = torch.empty(npk, dtype=torch.int32, device=dev)
            est = best(lambda: H.estimate(d_dst, d_est=d_est))
            flags = d_est >= 4 + PACKET
            coded, kept = torch.nonzero(~flags).reshape(-1), torch.nonzero(flags).reshape(-1)
            n_coded, n_kept = coded.numel(), kept.numel()
            c_ptr, c_len, c_fp = unit_descriptors(d_dst.data_ptr(), coded, dev)
            k_ptr, k_len, _ = unit_descriptors(d_dst.data_ptr(), kept, dev)
            d_raw = torch.empty(max(n_kept, 1) * PACKET, dtype=torch.uint8, device=dev)
            r_ptr = d_raw.data_ptr() + torch.arange(n_kept, dtype=torch.int64, device=dev) * PACKET
            enc = best(lambda: H.encode_batch(c_ptr, c_len, c_fp, n_coded, n_coded, d_slots=d_slots, d_status=status, mode="throughput"), reps=5)
            mov = best(lambda: H.move_packets(k_ptr, r_ptr, k_len, n_kept, d_status=status)) if n_kept else 0.0
            d_stream, d_off = H.compact(d_slots, n_coded)
            d_back.zero_()
            o_ptr = d_back.data_ptr() + coded * PACKET
            b_ptr = d_back.data_ptr() + kept * PACKET
            dec = best(lambda: H.decode_stream_batch(d_stream, d_off, c_fp, n_coded, n_coded, o_ptr, c_len, d_status=status), reps=5)
            back = best(lambda: H.move_packets(r_ptr, b_ptr, k_len, n_kept, d_status=status)) if n_kept else 0.0
            assert torch.equal(d_back, d_dst)
            some_bytes = int(d_off[-1].item()) + n_kept * PACKET
            print(f"  stored: {n_kept} of {npk} packets; estimate {est:.3f} + encode {enc:.3f} + move {mov:.3f} = {est + enc + mov:.3f} ms "
                  f"({(est + enc + mov) / enc_all:.1%} of coding all); decode {dec:.3f} + move {back:.3f} = {dec + back:.3f} ms ({(dec + back) / dec_all:.1%}); "
                  f"{some_bytes / n:.4f} of the size")
            out.update({f"{name}_stored_packets": n_kept, f"{name}_estimate_ms": round(est, 4), f"{name}_encode_coded_ms": round(enc, 4),
                        f"{name}_move_ms": round(mov, 4), f"{name}_decode_coded_ms": round(dec, 4), f"{name}_move_back_ms": round(back, 4),
                        f"{name}_ratio_stored": round(some_bytes / n, 5)})
            del d_stream, d_off, d_raw, d_est
        del d_back
        # end to end, as a caller sees it (descriptor work and the copies of the result included)
        for label, kw in (("planes", {}),) + ((("planes + stored", {"stored": "auto"}),) if not args.baseline else ()):
            holder = {}

            def compress():
                holder["c"] = batch.compress([t], planes="auto", mode="throughput", **kw)
            comp = best(compress, reps=3)
            c = holder["c"]
            outs = [torch.empty(n, dtype=torch.uint8, device=dev)]
            dec = best(lambda: batch.decompress(c, out=outs), reps=3)
            assert torch.equal(outs[0], t.view(torch.uint8))
            size = c.stream.numel() + (c.raw.numel() if getattr(c, "raw", None) is not None else 0)
            print(f"  batch.compress({label}) {comp:.3f} ms, decompress {dec:.3f} ms, {size / n:.4f} of the size")
            key = label.replace(" + ", "_")
            out.update({f"{name}_batch_{key}_compress_ms": round(comp, 4), f"{name}_batch_{key}_decompress_ms": round(dec, 4),
                        f"{name}_batch_{key}_ratio": round(size / n, 5)})
            del c, outs, holder
        del t
    assert int(status.item()) == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
