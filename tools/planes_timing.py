"""Byte-plane split / merge kernels against the copy roof and the codec (gpuar_hip_split_planes / merge_planes; torch events, min of 7).

    python tools/planes_timing.py [--gib G]

Prints, for G GiB (default 8) of uniform(42) resident in HBM: the plain device copy of the same bytes (gpuar_hip_copy, the roof
bench.py quotes; a split or merge moves the same 2 n bytes), then for element widths 2, 4 and 8 split and merge out of place and
in place as ms, TB/s (read + write) and fraction of that roof, and the throughput encoder alone against split + encode and the
decoder alone against decode + merge in place (what `gpuar c --planes` / `gpuar d` run per chunk).  The last line is the same
as JSON.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

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
    args = ap.parse_args()
    n = int(args.gib * (1 << 30)) // 65536 * 65536          # whole groups for every width: the full-group kernels are what is timed
    dev = torch.device("cuda:0")
    d_in = H.generate("uniform", 42, n, device=dev)
    d_dst = torch.empty(n, dtype=torch.uint8, device=dev)
    npk = H.packet_count(n)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    moved = 2 * n / 1e12                                      # TB read + written

    copy = best(lambda: H.device_copy(d_in, d_dst, n))
    roof = moved / (copy / 1e3)
    print(f"{args.gib:g} GiB uniform(42), {npk} packets; copy roof {copy:.3f} ms = {roof:.2f} TB/s (read + write)")
    out = {"gib": args.gib, "copy_ms": round(copy, 4), "copy_roof_tbs": round(roof, 3)}
    for w in (2, 4, 8):
        rows = (("split", lambda: H.split_planes(d_in, w, d_out=d_dst)), ("merge", lambda: H.merge_planes(d_in, w, d_out=d_dst)),
                ("split in place", lambda: H.split_planes(d_dst, w, d_out=d_dst)), ("merge in place", lambda: H.merge_planes(d_dst, w, d_out=d_dst)))
        for name, fn in rows:
            ms = best(fn)
            rate = moved / (ms / 1e3)
            print(f"  w = {w}  {name:15s} {ms:7.3f} ms  {rate:5.2f} TB/s  {rate / roof:5.1%} of the copy in this run")
            out[f"{name.replace(' ', '_')}_w{w}_ms"] = round(ms, 4)
    # correctness of what was timed, on the device: merge(split(x)) == x
    H.split_planes(d_in, 8, d_out=d_dst)
    H.merge_planes(d_dst, 8, d_out=d_dst)
    assert torch.equal(d_in, d_dst), "merge(split(x)) != x"

    d_slots = torch.empty(npk * H.SLOT, dtype=torch.uint8, device=dev)
    for w in (2, 8):
        enc = best(lambda: H.encode(d_in, d_slots, d_status=status, mode="throughput"), reps=5)
        both = best(lambda: (H.split_planes(d_in, w, d_out=d_dst), H.encode(d_dst, d_slots, d_status=status, mode="throughput")), reps=5)
        dec = best(lambda: H.decode(d_slots, npk, d_dst, d_status=status), reps=5)
        back = best(lambda: (H.decode(d_slots, npk, d_dst, d_status=status), H.merge_planes(d_dst, w, d_out=d_dst)), reps=5)
        print(f"  w = {w}  encode {enc:.3f} ms, split + encode {both:.3f} ms (+{both / enc - 1:.1%}); decode {dec:.3f} ms, "
              f"decode + merge in place {back:.3f} ms (+{back / dec - 1:.1%})")
        out.update({f"encode_w{w}_ms": round(enc, 4), f"split_encode_w{w}_ms": round(both, 4), f"decode_w{w}_ms": round(dec, 4),
                    f"decode_merge_w{w}_ms": round(back, 4)})
    assert int(status.item()) == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
