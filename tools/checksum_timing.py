"""Per-packet CRC-32 kernels against the copy roof and the encoder (gpuar_hip_crc32 / verify_crc32; torch events, min of 7).

    python tools/checksum_timing.py [--gib G]

Prints, for G GiB (default 8) of uniform(42) resident in HBM: the plain device copy of the same bytes (gpuar_hip_copy, the
roof bench.py quotes), compute and verify as ms, GB/s and fraction of that roof, and the throughput encoder alone against
encode followed by the CRC launch (what `gpuar c --checksum` runs per chunk).  The last line is the same as JSON.
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
    n = int(args.gib * (1 << 30)) // 16 * 16
    dev = torch.device("cuda:0")
    d_in = H.generate("uniform", 42, n, device=dev)
    npk = H.packet_count(n)
    d_crc = torch.empty(npk, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    first_bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
    gb = n / 1e9

    d_dst = torch.empty(n, dtype=torch.uint8, device=dev)
    copy = best(lambda: H.device_copy(d_in, d_dst, n))
    del d_dst
    roof = 2 * gb / (copy / 1e3)                     # read + write bytes per second
    crc = best(lambda: H.crc32(d_in, d_crc=d_crc))
    verify = best(lambda: H.verify_crc32(d_in, d_crc, d_first_bad=first_bad, d_status=status))
    assert int(status.item()) == 0 and int(first_bad.item()) == -1, "verify of the CRCs just computed failed"
    print(f"{args.gib:g} GiB uniform(42), {npk} packets; copy roof {copy:.3f} ms = {roof / 1e3:.2f} TB/s (read + write)")
    for name, ms in (("compute", crc), ("verify", verify)):
        rate = gb / (ms / 1e3)
        print(f"  {name:8s} {ms:7.3f} ms  {rate:7.1f} GB/s  {rate / roof:5.1%} of the copy roof  (a read-only pass at the roof: "
              f"{gb / roof * 1e3:.3f} ms)")

    d_slots = torch.empty(npk * H.SLOT, dtype=torch.uint8, device=dev)
    enc = best(lambda: H.encode(d_in, d_slots, d_status=status, mode="throughput"), reps=5)
    both = best(lambda: (H.encode(d_in, d_slots, d_status=status, mode="throughput"), H.crc32(d_in, d_crc=d_crc)), reps=5)
    print(f"  encode {enc:.3f} ms, encode + CRC {both:.3f} ms (+{both / enc - 1:.1%})")
    print(json.dumps({"gib": args.gib, "copy_ms": round(copy, 4), "copy_roof_tbs": round(roof / 1e3, 3), "crc_ms": round(crc, 4),
                      "verify_ms": round(verify, 4), "crc_gbs": round(gb / (crc / 1e3), 1), "verify_gbs": round(gb / (verify / 1e3), 1),
                      "encode_ms": round(enc, 4), "encode_crc_ms": round(both, 4)}))


if __name__ == "__main__":
    main()
