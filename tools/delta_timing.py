"""The fused delta kernels against the plane kernels and the copy, on the same buffers in the same run (gpuar_hip_split_delta /
merge_delta; torch events, min of 7).

    python tools/delta_timing.py [--gib G] [--codec-gib C]

Prints, for G GiB (default 8) of uniform(42) resident in HBM: the plain device copy of the same bytes (gpuar_hip_copy), then for
element widths 1, 2, 4 and 8 split_delta and merge_delta out of place and in place beside split_planes and merge_planes (widths
2, 4, 8) as ms, and the claim DESIGN.md 4.9 checks: the cheapest unfused design is a filter pass of its own, and no pass is
faster than the copy, so fusing pays iff
    split_delta(w) < split_planes(w) + copy    and    merge_delta(w) < merge_planes(w) + copy        (w = 1: < 2 x copy).
Then batch.compress(planes=8, delta=True) and decompress against planes=8 alone on C GiB (default 1) of sorted int64, with
sizes.  The last line is the same as JSON.
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
    d_dst = torch.empty(n, dtype=torch.uint8, device=dev)
    moved = 2 * n / 1e12                                      # TB read + written

    copy = best(lambda: H.device_copy(d_in, d_dst, n))
    print(f"{args.gib:g} GiB uniform(42), {H.packet_count(n)} packets; copy {copy:.3f} ms = {moved / (copy / 1e3):.2f} TB/s (read + write)")
    out = {"gib": args.gib, "copy_ms": round(copy, 4)}
    for w in (1, 2, 4, 8):
        for merge in (False, True):
            what = "merge" if merge else "split"
            delta = H.merge_delta if merge else H.split_delta
            planes = H.merge_planes if merge else H.split_planes
            t_delta = best(lambda: delta(d_in, w, d_out=d_dst))
            t_place = best(lambda: delta(d_dst, w, d_out=d_dst))
            t_planes = best(lambda: planes(d_in, w, d_out=d_dst)) if w > 1 else copy       # (planes at a width of 1 is the copy)
            t_planes_place = best(lambda: planes(d_dst, w, d_out=d_dst)) if w > 1 else 0.0
            bound = t_planes + copy
            print(f"  w = {w}  {what}_delta {t_delta:7.3f} ms ({moved / (t_delta / 1e3):4.2f} TB/s), in place {t_place:7.3f} ms;  {what}_planes "
                  f"{t_planes:7.3f} ms, in place {t_planes_place:7.3f} ms;  unfused bound {bound:7.3f} ms: fused is {t_delta / bound:5.1%} of it "
                  f"-> {'holds' if t_delta < bound else 'MISSES'}")
            out.update({f"{what}_delta_w{w}_ms": round(t_delta, 4), f"{what}_delta_in_place_w{w}_ms": round(t_place, 4),
                        f"{what}_planes_w{w}_ms": round(t_planes, 4), f"{what}_planes_in_place_w{w}_ms": round(t_planes_place, 4),
                        f"{what}_claim_w{w}": bool(t_delta < bound)})
    # correctness of what was timed, on the device: merge(split(x)) == x at every width
    for w in (1, 2, 4, 8):
        H.split_delta(d_in, w, d_out=d_dst)
        H.merge_delta(d_dst, w, d_out=d_dst)
        assert torch.equal(d_in, d_dst), f"merge_delta(split_delta(x)) != x at width {w}"
    del d_in, d_dst

    m = int(args.codec_gib * (1 << 30)) // 65536 * 65536 // 8
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.cumsum(torch.randint(0, 64, (m,), generator=g, device=dev, dtype=torch.int64), 0)      # sorted int64: CSR offsets
    for name, kw in (("planes", {"planes": 8}), ("delta", {"planes": 8, "delta": True})):
        c = batch.compress([t], **kw)
        enc = best(lambda: batch.compress([t], **kw), reps=3)
        back = torch.empty_like(t)
        dec = best(lambda: batch.decompress(c, out=[back]), reps=3)
        assert torch.equal(back, t)
        print(f"  sorted int64, {args.codec_gib:g} GiB, {name:6s}: {c.nbytes} bytes = {c.nbytes / (8 * m):.4f} of the input; compress {enc:.2f} ms, "
              f"decompress {dec:.2f} ms")
        out.update({f"codec_{name}_bytes": c.nbytes, f"codec_{name}_fraction": round(c.nbytes / (8 * m), 5),
                    f"codec_{name}_compress_ms": round(enc, 3), f"codec_{name}_decompress_ms": round(dec, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
