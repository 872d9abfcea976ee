"""The XOR-base survey kernel against the launches it replaces, against the plane survey and against the copy roof (torch events,
min of 7), on the same resident buffers in the same run.

    python tools/xor_survey_timing.py [--gib G] [--kinds uniform,bf16_step,equal,compress] [--timeout S]
                                         [--lib PATH]

--lib PATH times another build of libgpuar_hip.so (tools/exp_build.sh) instead of the product one, in every child.

For every kind of input a child process of its own (this file with --kind, under a time limit of its own; the first child that
fails ends the run) makes a buffer and its base of G GiB each (default 8) resident in HBM and times:
    copy          gpuar_hip_copy of the buffer (the roof bench.py quotes)
    planes        gpuar_hip_survey_planes of the buffer: the plane survey, one launch, one read
    planes_xored  the same of buffer ^ base made beforehand: the bytes the XOR survey counts, without the second read
    one[w]        what one width of the survey replaces: split_xor(w) into a temporary + estimate of it
    xor           gpuar_hip_survey_xor, both outputs: one launch, two reads               (a) xor / one[w], (b) xor / planes
    xor_est       the same with the est rows alone
and checks the survey's rows against estimate(split_xor) and sparse_scan(split_xor) on the whole buffer.  Inputs: uniform against
uniform, bf16 weights (normal x 0.02) a normal step of 1e-4 from their base, and a tensor equal to its base (all zeros behind the
XOR: every lane on one bin, the LDS worst case).  The kind `compress` times batch.compress(base_auto="survey") against
base_auto=True on 1 GiB of the bf16 pair at w = 2, 4 and 8 and checks that both keep the base and write the same stream.  The last
line of every child, and of the run, is JSON.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ["uniform", "bf16_step", "equal", "compress"]
WIDTHS = (1, 2, 4, 8)


def best(fn, reps=7):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return min(s.elapsed_time(e) for s, e in ev)


def make_pair(kind, n, dev):
    """(buffer, base) of n bytes each of `kind` on the device, made in pieces (no temporary of the whole size)."""
    import torch
    from gpuar_amd import hip as H
    if kind == "uniform":
        return H.generate("uniform", 42, n, device=dev), H.generate("uniform", 43, n, device=dev)
    if kind == "equal":
        x = H.generate("uniform", 42, n, device=dev)
        return x, x.clone()
    x = torch.empty(n // 2, dtype=torch.bfloat16, device=dev)
    b = torch.empty(n // 2, dtype=torch.bfloat16, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    piece = 1 << 26
    for at in range(0, x.numel(), piece):
        m = min(piece, x.numel() - at)
        w = torch.randn(m, generator=g, device=dev) * 0.02
        b[at:at + m] = w.to(torch.bfloat16)
        x[at:at + m] = (w + torch.randn(m, generator=g, device=dev) * 1e-4).to(torch.bfloat16)
    return x.view(torch.uint8), b.view(torch.uint8)


def child(kind, gib):
    import torch
    from gpuar_amd import hip as H
    n = int(gib * (1 << 30)) // 65536 * 65536
    dev = torch.device("cuda:0")
    npk = H.packet_count(n)
    d_in, d_base = make_pair(kind, n, dev)
    d_tmp = torch.empty(n, dtype=torch.uint8, device=dev)
    d_est = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_scan = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_planes = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_one = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_word = torch.empty(npk, dtype=torch.int32, device=dev)

    def one(j):
        H.split_xor(d_in, d_base, WIDTHS[j], d_out=d_tmp)
        H.estimate(d_tmp, d_est=d_one[j])

    copy = best(lambda: H.device_copy(d_in, d_tmp, n))
    planes = best(lambda: H.survey_planes(d_in, d_est=d_planes))
    torch.bitwise_xor(d_in, d_base, out=d_tmp)
    planes_y = best(lambda: H.survey_planes(d_tmp, d_est=d_one))                 # the bytes the XOR survey counts, from one read
    xor = best(lambda: H.survey_xor(d_in, d_base, d_est=d_est, d_scan=d_scan))
    assert torch.equal(d_one, d_est), "the est rows differ from the plane survey of the XORed bytes"
    xor_est = best(lambda: H.survey_xor(d_in, d_base, d_est=d_planes, d_scan=False))
    assert torch.equal(d_planes, d_est), "the est rows differ when the scan rows are left out"
    one_ms = []
    for j in range(4):
        one_ms.append(best(lambda: one(j)))
        assert torch.equal(d_one[j], d_est[j]), f"row {j} of the XOR survey differs from estimate(split_xor(...))"
        H.sparse_scan(d_tmp, d_scan=d_word)
        assert torch.equal(d_word, d_scan[j]), f"scan row {j} of the XOR survey differs from sparse_scan(split_xor(...))"
    assert H.status() == 0
    totals = d_est.to(torch.int64).sum(dim=1).tolist()
    out = {"kind": kind, "gib": gib, "packets": npk, "copy_ms": round(copy, 4), "planes_ms": round(planes, 4), "planes_xored_ms": round(planes_y, 4),
           "xor_ms": round(xor, 4), "xor_est_ms": round(xor_est, 4), "one_ms": [round(v, 4) for v in one_ms], "xored": totals}
    print(f"{kind:10s} copy {copy:7.3f} ms  planes {planes:7.3f} ms  planes of the XORed bytes {planes_y:7.3f} ms  xor survey {xor:7.3f} ms = "
          f"{2 * n / 1e6 / xor:5.0f} GB/s read (est rows alone {xor_est:7.3f} ms), (b) {xor / planes:.3f} of the plane survey of the buffer, "
          f"{xor / planes_y:.3f} of that of the XORed bytes")
    for j, w in enumerate(WIDTHS):
        print(f"{'':10s} w = {w}: split_xor + estimate {one_ms[j]:7.3f} ms  (a) {xor / one_ms[j]:.3f}")
    print(json.dumps(out))


def child_compress(gib):
    import time
    import torch
    from gpuar_amd import batch
    dev = torch.device("cuda:0")
    x, b = make_pair("bf16_step", int(gib * (1 << 30)) // 65536 * 65536, dev)
    out = {"kind": "compress", "gib": gib, "true_ms": [], "survey_ms": [], "fixed_ms": []}

    def wall(w, reps=3, **kwargs):
        times = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = batch.compress([x], planes=w, base=[b], **kwargs)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return min(times[1:]), c

    for w in (2, 4, 8):
        true_ms, t = wall(w, base_auto=True)
        survey_ms, s = wall(w, base_auto="survey")
        fixed_ms, f = wall(w)
        assert t.based == s.based == [True] and torch.equal(t.stream, s.stream) and torch.equal(t.offsets, s.offsets)
        del t, s, f
        out["true_ms"].append(round(true_ms, 3))
        out["survey_ms"].append(round(survey_ms, 3))
        out["fixed_ms"].append(round(fixed_ms, 3))
        print(f"compress   {gib:g} GiB of bf16 against its base, planes={w}: fixed base {fixed_ms:8.2f} ms  base_auto=True {true_ms:8.2f} ms  "
              f"base_auto=\"survey\" {survey_ms:8.2f} ms = {survey_ms / true_ms:.3f} of True (wall clock, min of 3)")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--compress-gib", type=float, default=1.0)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--kind", help="(the child) measure this kind in this process")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds every child may take")
    ap.add_argument("--lib", default=None, help="an experiment build of libgpuar_hip.so to time instead of the product one")
    args = ap.parse_args()
    lib = ["--lib", os.path.abspath(args.lib)] if args.lib else []
    if args.kind:
        if lib:
            from gpuar_amd import hip as H
            H.LIB_PATH = lib[1]
        if args.kind == "compress":
            child_compress(args.compress_gib)
        else:
            child(args.kind, args.gib)
        return 0
    results = []
    for kind in args.kinds.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kind", kind, "--gib", str(args.gib), "--compress-gib",
                                str(args.compress_gib)] + lib, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{kind}: no result within {args.timeout:g} s; nothing more is started", flush=True)
            return 1
        if r.returncode != 0:
            print(f"{kind}: exit status {r.returncode}; nothing more is started\n{r.stdout}{r.stderr}", flush=True)
            return 1
        lines = r.stdout.strip().splitlines()
        print("\n".join(lines[:-1]), flush=True)
        results.append(json.loads(lines[-1]))
    timed = [r for r in results if r["kind"] != "compress"]
    if timed:
        worst = max(r["xor_ms"] / v for r in timed for v in r["one_ms"])
        print(f"(a) xor survey / split_xor + estimate of one width: worst {worst:.3f}")
        for r in timed:
            kind, ratio, ratio_y = r["kind"], r["xor_ms"] / r["planes_ms"], r["xor_ms"] / r["planes_xored_ms"]
            print(f"(b) xor survey / plane survey on {kind}: {ratio:.3f} of the buffer's, {ratio_y:.3f} of the XORed bytes'")
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
