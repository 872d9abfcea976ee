"""The plane-width survey kernel against the seven launches it replaces, against estimate_kernel alone and against the copy roof
(torch events, min of 7), on the same resident buffers in the same run.

    python tools/survey_timing.py [--gib G] [--kinds uniform,zeros,text,bf16,fp32,int64] [--timeout S] [--lib PATH]

--lib PATH times another build of libgpuar_hip.so (tools/exp_build.sh) instead of the product one, in every child.

For every kind of input a child process of its own (this file with --kind, under a time limit of its own; the first child that
fails ends the run) makes G GiB (default 8) resident in HBM and times:
    copy      gpuar_hip_copy of the buffer (the roof bench.py quotes)
    estimate  gpuar_hip_estimate of the buffer: estimate_kernel alone, the w = 1 row
    seven     what the survey replaces: estimate of the buffer, then split_planes into a temporary and estimate of it for
              w = 2, 4 and 8 -- 3 split + 4 estimate launches
    survey    gpuar_hip_survey_planes: one launch, all four rows
and checks the survey's rows against the seven-launch path's on the whole buffer.  Inputs: uniform(42), zeros, text(42), bf16 and
fp32 weights (normal x 0.02) and int64 indices below 50000.  The last line of every child, and of the run, is JSON.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ["uniform", "zeros", "text", "bf16", "fp32", "int64"]
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


def make_input(kind, n, dev):
    """n bytes of `kind` on the device, made in pieces (no temporary of the whole size)."""
    import torch
    from gpuar_amd import hip as H
    if kind in ("uniform", "zeros", "text"):
        return H.generate(kind, 42, n, device=dev)
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32, "int64": torch.int64}[kind]
    out = torch.empty(n // dtype.itemsize, dtype=dtype, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    piece = 1 << 26
    for at in range(0, out.numel(), piece):
        m = min(piece, out.numel() - at)
        if kind == "int64":
            out[at:at + m] = torch.randint(0, 50000, (m,), generator=g, device=dev, dtype=torch.int64)
        else:
            out[at:at + m] = (torch.randn(m, generator=g, device=dev) * 0.02).to(dtype)
    return out.view(torch.uint8)


def child(kind, gib):
    import torch
    from gpuar_amd import hip as H
    n = int(gib * (1 << 30)) // 65536 * 65536
    dev = torch.device("cuda:0")
    npk = H.packet_count(n)
    d_in = make_input(kind, n, dev)
    d_tmp = torch.empty(n, dtype=torch.uint8, device=dev)
    d_seven = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_survey = torch.empty((4, npk), dtype=torch.int32, device=dev)

    def seven():
        H.estimate(d_in, d_est=d_seven[0])
        for j in (1, 2, 3):
            H.split_planes(d_in, WIDTHS[j], d_out=d_tmp)
            H.estimate(d_tmp, d_est=d_seven[j])

    copy = best(lambda: H.device_copy(d_in, d_tmp, n))
    est = best(lambda: H.estimate(d_in, d_est=d_seven[0]))
    old = best(seven)
    new = best(lambda: H.survey_planes(d_in, d_est=d_survey))
    assert torch.equal(d_seven, d_survey), "the survey's rows differ from estimate(split_planes(...))"
    assert H.status() == 0
    totals = d_survey.to(torch.int64).sum(dim=1).tolist()
    out = {"kind": kind, "gib": gib, "packets": npk, "copy_ms": round(copy, 4), "estimate_ms": round(est, 4), "seven_ms": round(old, 4),
           "survey_ms": round(new, 4), "totals": totals, "chosen": H.choose_planes(totals, npk)}
    print(f"{kind:8s} copy {copy:7.3f} ms  estimate {est:7.3f} ms  seven launches {old:7.3f} ms  survey {new:7.3f} ms = "
          f"{n / 1e6 / new:5.0f} GB/s read, {new / old:5.1%} of the seven, {new / est:.2f} x estimate; chosen width {out['chosen']}")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
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
        child(args.kind, args.gib)
        return 0
    results = []
    for kind in args.kinds.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kind", kind, "--gib", str(args.gib)] + lib, capture_output=True,
                               text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{kind}: no result within {args.timeout:g} s; nothing more is started", flush=True)
            return 1
        if r.returncode != 0:
            print(f"{kind}: exit status {r.returncode}; nothing more is started\n{r.stdout}{r.stderr}", flush=True)
            return 1
        lines = r.stdout.strip().splitlines()
        print("\n".join(lines[:-1]), flush=True)
        results.append(json.loads(lines[-1]))
    if "uniform" in args.kinds and "zeros" in args.kinds:
        by = {r["kind"]: r for r in results}
        print(f"survey zeros / uniform = {by['zeros']['survey_ms'] / by['uniform']['survey_ms']:.2f}")
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
