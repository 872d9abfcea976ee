"""The two kernels that put raw and sparse packets into a packet stream and take them out, against the copy roof and the passes
they run beside (torch events, min of 7 launches), and what `--stored=auto --sparse=auto` do to the CLI's wall time and file size
(the better of two runs).

    python tools/kinds_timing.py [--gib G] [--cli-gib C] [--dir D] [--baseline-bin PATH]

Prints, for G GiB (default 8) resident in HBM: the plain device copy (gpuar_hip_copy, the roof bench.py quotes); then on zeros (every
packet sparse), on uniform bytes with stored on (every packet raw) and on text (every packet coded: the pass reads est and scan and
returns) gpuar_hip_encode alone, gpuar_hip_estimate, gpuar_hip_sparse_scan, gpuar_hip_kinds_store behind them, gpuar_hip_compact,
and gpuar_hip_kinds_expand out of the compacted stream (checked against the buffer).  Then, with --cli-gib C > 0 (default 0: no CLI
part), for C GiB of bf16 weights in directory D: `gpuar c --planes=2` and `gpuar c --base=B --planes=2` (the file a 1e-4 step from
its base), each without and with the two flags, and `gpuar d` of each file -- wall seconds and file sizes; with --baseline-bin, the
same without the flags through that gpuar (the parent commit's build), in the same run.  No thresholds: the figures are for the
reader.  The last line is the same as JSON.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

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


def kernels(gib, out):
    n = int(gib * (1 << 30)) // 65536 * 65536
    dev = torch.device("cuda:0")
    npk = H.packet_count(n)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d_in = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_out = torch.empty(n, dtype=torch.uint8, device=dev)
    d_slots = torch.empty(npk * SLOT, dtype=torch.uint8, device=dev)
    d_stream = torch.empty(npk * SLOT, dtype=torch.uint8, device=dev)
    d_offsets = torch.empty(npk + 1, dtype=torch.int64, device=dev)
    d_est = torch.empty(npk, dtype=torch.int32, device=dev)
    d_scan = torch.empty(npk, dtype=torch.int32, device=dev)
    d_kind = torch.empty(npk, dtype=torch.uint8, device=dev)
    copy = best(lambda: H.device_copy(d_in, d_out, n))
    roof = 2 * n / 1e12 / (copy / 1e3)
    print(f"{gib:g} GiB, {npk} packets; copy {copy:.3f} ms = {roof:.2f} TB/s (read + write)")
    out.update(gib=gib, copy_ms=round(copy, 4), copy_roof_tbs=round(roof, 3))
    for kind, stored, sparse, want in (("zeros", True, True, 2), ("uniform", True, True, 1), ("text", True, True, 0)):
        if kind != "zeros":
            H.generate(kind, 42, n, device=dev, out=d_in)
        enc = best(lambda: H.encode(d_in, d_slots, d_status=status, mode="throughput"), reps=3)
        est = best(lambda: H.estimate(d_in, d_est=d_est))
        scan = best(lambda: H.sparse_scan(d_in, d_scan=d_scan))
        store = best(lambda: H.kinds_store(d_in, d_est, d_scan if sparse else None, stored, d_slots, d_kind=d_kind, d_status=status))
        counts = torch.bincount(d_kind.to(torch.int64), minlength=3).tolist()
        assert counts[want] == npk, (kind, counts)
        compact = best(lambda: H.compact(d_slots, npk, d_stream, d_offsets))
        stream_bytes = int(d_offsets[-1].item())
        d_out.fill_(0x5A)
        expand = best(lambda: H.kinds_expand(d_stream, d_offsets, d_kind, npk, d_out, n, d_status=status))
        if want:
            assert torch.equal(d_out, d_in), kind
        moved = n + stream_bytes                            # what the pass reads and writes, where it moves anything
        print(f"  {kind:8s} (coded / raw / sparse {counts[0]} / {counts[1]} / {counts[2]}; stream {stream_bytes / n:.5f} of the size)\n"
              f"           encode {enc:8.3f} ms   estimate {est:7.3f} ms   sparse_scan {scan:7.3f} ms   compact {compact:7.3f} ms\n"
              f"           kinds_store {store:7.3f} ms ({store / copy:5.2f} x the copy, {moved / 1e9 / store:6.3f} TB/s in + out)   "
              f"kinds_expand {expand:7.3f} ms ({expand / copy:5.2f} x the copy, {moved / 1e9 / expand:6.3f} TB/s in + out)")
        out.update({f"{kind}_encode_ms": round(enc, 4), f"{kind}_estimate_ms": round(est, 4), f"{kind}_scan_ms": round(scan, 4),
                    f"{kind}_store_ms": round(store, 4), f"{kind}_compact_ms": round(compact, 4), f"{kind}_expand_ms": round(expand, 4),
                    f"{kind}_stream_bytes": stream_bytes})
    assert int(status.item()) == 0
    del d_in, d_out, d_slots, d_stream, d_offsets, d_est, d_scan, d_kind
    torch.cuda.empty_cache()


def wall(cmd):
    """the better of two runs, in seconds"""
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        times.append(time.perf_counter() - t0)
    return min(times), max(times)


def cli(gib, where, baseline, out):
    dev = torch.device("cuda:0")
    elements = int(gib * (1 << 30)) // 65536 * 65536 // 2
    g = torch.Generator(device=dev).manual_seed(1)
    paths = {k: os.path.join(where, f"kinds_timing_{k}") for k in ("base", "in", "gip", "back")}
    piece = 1 << 26
    with open(paths["base"], "wb") as fb, open(paths["in"], "wb") as fi:
        for at in range(0, elements, piece):
            m = min(piece, elements - at)
            w = torch.randn(m, generator=g, device=dev) * 0.02
            fb.write(w.to(torch.bfloat16).view(torch.uint8).cpu().numpy().tobytes())
            fi.write((w + torch.randn(m, generator=g, device=dev) * 1e-4).to(torch.bfloat16).view(torch.uint8).cpu().numpy().tobytes())
    torch.cuda.synchronize()
    gpuar = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")
    both = ["--stored=auto", "--sparse=auto"]
    for case, flags, based in (("planes", ["--planes=2"], []), ("base", ["--planes=2"], [f"--base={paths['base']}"])):
        rows = [("no flags", gpuar, []), ("--stored=auto --sparse=auto", gpuar, both)] + ([("parent commit", baseline, [])] if baseline else [])
        for label, exe, extra in rows:
            lo, hi = wall([exe, "c", *flags, *based, *extra, f"--in={paths['in']}", f"--out={paths['gip']}"])
            size = os.path.getsize(paths["gip"])
            dlo, dhi = wall([exe, "d", *based, f"--in={paths['gip']}", f"--out={paths['back']}"])
            assert subprocess.run(["cmp", "-s", paths["in"], paths["back"]]).returncode == 0, (case, label, "the round trip")
            print(f"  {case:6s} {label:28s} compress {lo:6.3f} s (other run {hi:6.3f})   decompress {dlo:6.3f} s (other run {dhi:6.3f})   "
                  f"{size} bytes = {size / (2 * elements):.5f} of the size")
            key = f"cli_{case}_{label.split()[0].strip('-').replace('=auto', '')}"
            out.update({f"{key}_compress_s": round(lo, 4), f"{key}_compress_other_s": round(hi, 4), f"{key}_decompress_s": round(dlo, 4),
                        f"{key}_decompress_other_s": round(dhi, 4), f"{key}_bytes": size})
    out["cli_gib"] = gib
    for p in paths.values():
        os.remove(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--cli-gib", type=float, default=0.0)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--baseline-bin", default=None)
    args = ap.parse_args()
    out = {}
    if args.gib > 0:
        kernels(args.gib, out)
    if args.cli_gib > 0:
        cli(args.cli_gib, args.dir, args.baseline_bin, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
