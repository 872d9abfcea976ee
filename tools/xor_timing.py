"""The fused XOR-base kernels against the plane kernels, the copy and a torch XOR pass, on the same buffers in the same run
(gpuar_hip_split_xor / merge_xor; torch events, min of 7).

    python tools/xor_timing.py [--gib G] [--codec-gib C]

Prints, for G GiB (default 8) of uniform(42) and a base of uniform(43) resident in HBM: the plain device copy of the same bytes
(gpuar_hip_copy) and a torch.bitwise_xor pass over them (buffer ^ base into a third buffer), then for element widths 1, 2, 4 and
8 split_xor and merge_xor out of place and in place beside split_planes and merge_planes (widths 2, 4, 8) as ms, and the claim
DESIGN.md 4.10 checks: the unfused design is an XOR pass of its own in front of (behind) the plane kernels, so fusing pays iff
    split_xor(w) < split_planes(w) + bitwise_xor    and    merge_xor(w) < merge_planes(w) + bitwise_xor
(w = 1, where planes is the identity: < bitwise_xor + copy out of place).  The yardsticks are the plane kernels and torch, never
the new kernels.  Then batch.compress(planes=2, base=...) and decompress against planes=2 alone on C GiB (default 1) of bf16
weights a normal step of 1e-4 from their base, with sizes.  The last line is the same as JSON.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gpuar_amd import batch  # noqa: E402
from gpuar_amd import hip as H  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--codec-gib", type=float, default=1.0)
    args = ap.parse_args()
    n = int(args.gib * (1 << 30)) // 65536 * 65536          # whole groups for every width: the full-group kernels are what is timed
    dev = torch.device("cuda:0")
    d_in = H.generate("uniform", 42, n, device=dev)
    d_base = H.generate("uniform", 43, n, device=dev)
    d_dst = torch.empty(n, dtype=torch.uint8, device=dev)
    moved = 2 * n / 1e12                                      # TB read + written without the base

    copy = best(lambda: H.device_copy(d_in, d_dst, n))
    xor = best(lambda: torch.bitwise_xor(d_in, d_base, out=d_dst))
    print(f"{args.gib:g} GiB uniform(42) and a base of uniform(43), {H.packet_count(n)} packets; copy {copy:.3f} ms = {moved / (copy / 1e3):.2f} TB/s "
          f"(read + write); torch.bitwise_xor {xor:.3f} ms = {1.5 * moved / (xor / 1e3):.2f} TB/s (two reads + write)")
    out = {"gib": args.gib, "copy_ms": round(copy, 4), "bitwise_xor_ms": round(xor, 4)}
    for w in (1, 2, 4, 8):
        for merge in (False, True):
            what = "merge" if merge else "split"
            fused = H.merge_xor if merge else H.split_xor
            planes = H.merge_planes if merge else H.split_planes
            t_xor = best(lambda: fused(d_in, d_base, w, d_out=d_dst))
            t_place = best(lambda: fused(d_dst, d_base, w, d_out=d_dst))
            t_planes = best(lambda: planes(d_in, w, d_out=d_dst)) if w > 1 else copy       # (planes at a width of 1 is the copy)
            t_planes_place = best(lambda: planes(d_dst, w, d_out=d_dst)) if w > 1 else 0.0
            bound = t_planes + xor
            print(f"  w = {w}  {what}_xor {t_xor:7.3f} ms ({1.5 * moved / (t_xor / 1e3):4.2f} TB/s), in place {t_place:7.3f} ms;  {what}_planes "
                  f"{t_planes:7.3f} ms, in place {t_planes_place:7.3f} ms;  unfused bound {bound:7.3f} ms: fused is {t_xor / bound:5.1%} of it "
                  f"-> {'holds' if t_xor < bound else 'MISSES'}")
            out.update({f"{what}_xor_w{w}_ms": round(t_xor, 4), f"{what}_xor_in_place_w{w}_ms": round(t_place, 4),
                        f"{what}_planes_w{w}_ms": round(t_planes, 4), f"{what}_planes_in_place_w{w}_ms": round(t_planes_place, 4),
                        f"{what}_claim_w{w}": bool(t_xor < bound)})
    # correctness of what was timed, on the device: split_xor is split_planes of the XOR, and merge_xor(split_xor(x)) == x
    for w in (1, 2, 4, 8):
        want = H.split_planes(torch.bitwise_xor(d_in, d_base), w)
        H.split_xor(d_in, d_base, w, d_out=d_dst)
        assert torch.equal(want, d_dst), f"split_xor(x, b) != split_planes(x ^ b) at width {w}"
        del want
        H.merge_xor(d_dst, d_base, w, d_out=d_dst)
        assert torch.equal(d_in, d_dst), f"merge_xor(split_xor(x)) != x at width {w}"
    del d_in, d_dst, d_base

    m = int(args.codec_gib * (1 << 30)) // 65536 * 65536 // 2
    g = torch.Generator(device=dev).manual_seed(1)
    weights = torch.randn(m, generator=g, device=dev) * 0.02
    base = weights.to(torch.bfloat16)
    t = (weights + torch.randn(m, generator=g, device=dev) * 1e-4).to(torch.bfloat16)
    del weights
    for name, kw, dkw in (("planes", {"planes": 2}, {}), ("base", {"planes": 2, "base": [base]}, {"base": [base]})):
        c = batch.compress([t], **kw)
        enc = best(lambda: batch.compress([t], **kw), reps=3)
        back = torch.empty_like(t)
        dec = best(lambda: batch.decompress(c, out=[back], **dkw), reps=3)
        assert torch.equal(back.view(torch.int16), t.view(torch.int16))
        print(f"  bf16 weights a 1e-4 step from the base, {args.codec_gib:g} GiB, {name:6s}: {c.nbytes} bytes = {c.nbytes / (2 * m):.4f} of the input; "
              f"compress {enc:.2f} ms, decompress {dec:.2f} ms")
        out.update({f"codec_{name}_bytes": c.nbytes, f"codec_{name}_fraction": round(c.nbytes / (2 * m), 5),
                    f"codec_{name}_compress_ms": round(enc, 3), f"codec_{name}_decompress_ms": round(dec, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
