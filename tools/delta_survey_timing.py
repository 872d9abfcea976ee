"""The delta survey kernel against the launches it replaces, against the plane survey and against the copy roof (torch events, min
of 7), on the same resident buffers in the same run.

    python tools/delta_survey_timing.py [--gib G] [--kinds uniform,zeros,sorted_int64,position_ids,bf16,compress] [--timeout S]
                                         [--lib PATH]

--lib PATH times another build of libgpuar_hip.so (tools/exp_build.sh) instead of the product one, in every child.

For every kind of input a child process of its own (this file with --kind, under a time limit of its own; the first child that
fails ends the run) makes G GiB (default 8) resident in HBM and times:
    copy          gpuar_hip_copy of the buffer (the roof bench.py quotes)
    planes        gpuar_hip_survey_planes: the plane survey, one launch
    eight         what one delta survey replaces: split_delta into a temporary and estimate of it for w = 1, 2, 4 and 8
    delta         gpuar_hip_survey_delta with all four widths: one launch                              (a) delta / eight
    auto[w]       what batch.compress(delta="auto") runs at width w: split_planes(w) + estimate, split_delta(w) + estimate
                  (w = 1: no split_planes launch, the bytes are estimated where they are)
    survey[w]     what delta="survey" runs instead: survey_planes + survey_delta masked to w            (b) survey[w] / auto[w]
and checks the survey's rows against the eight-launch path's on the whole buffer.  Inputs: uniform(42), zeros, int64
cumsum(integers(0, 64)), int32 arange % 4096 and bf16 weights (normal x 0.02).  The kind `compress` times
batch.compress(planes=8, delta="survey") against delta="auto" on 1 GiB of sorted int64 and checks that both flag the tensor
and write the same stream.  The last line of every child, and of the run, is JSON.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/delta_survey_timing.py --kind position_ids --gib 2 --profile
runs the launches of (b) at w = 1 and the four-width delta survey three times each, untimed, in this process.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ["uniform", "zeros", "sorted_int64", "position_ids", "bf16", "compress"]
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
    if kind in ("uniform", "zeros"):
        return H.generate(kind, 42, n, device=dev)
    dtype = {"bf16": torch.bfloat16, "position_ids": torch.int32, "sorted_int64": torch.int64}[kind]
    out = torch.empty(n // dtype.itemsize, dtype=dtype, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    piece, carried = 1 << 26, 0
    for at in range(0, out.numel(), piece):
        m = min(piece, out.numel() - at)
        if kind == "sorted_int64":
            out[at:at + m] = torch.cumsum(torch.randint(0, 64, (m,), generator=g, device=dev, dtype=torch.int64), 0) + carried
            carried = int(out[at + m - 1].item())
        elif kind == "position_ids":
            out[at:at + m] = (torch.arange(at, at + m, device=dev, dtype=torch.int64) % 4096).to(torch.int32)
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
    d_eight = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_delta = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_planes = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_one = torch.empty((4, npk), dtype=torch.int32, device=dev)
    d_plain = torch.empty(npk, dtype=torch.int32, device=dev)

    def eight():
        for j, w in enumerate(WIDTHS):
            H.split_delta(d_in, w, d_out=d_tmp)
            H.estimate(d_tmp, d_est=d_eight[j])

    def auto(j):
        w = WIDTHS[j]
        if w == 1:
            H.estimate(d_in, d_est=d_plain)
        else:
            H.split_planes(d_in, w, d_out=d_tmp)
            H.estimate(d_tmp, d_est=d_plain)
        H.split_delta(d_in, w, d_out=d_tmp)
        H.estimate(d_tmp, d_est=d_eight[j])

    def survey(j):
        H.survey_planes(d_in, d_est=d_planes)
        H.survey_delta(d_in, d_est=d_one, widths=(WIDTHS[j],))

    copy = best(lambda: H.device_copy(d_in, d_tmp, n))
    planes = best(lambda: H.survey_planes(d_in, d_est=d_planes))
    old = best(eight)
    new = best(lambda: H.survey_delta(d_in, d_est=d_delta))
    assert torch.equal(d_eight, d_delta), "the delta survey's rows differ from estimate(split_delta(...))"
    auto_ms, survey_ms, one_ms = [], [], []
    for j in range(4):
        auto_ms.append(best(lambda: auto(j)))
        survey_ms.append(best(lambda: survey(j)))
        one_ms.append(best(lambda: H.survey_delta(d_in, d_est=d_one, widths=(WIDTHS[j],))))
        assert torch.equal(d_one[j], d_delta[j]), f"the masked delta survey's row {j} differs"
    assert H.status() == 0
    plain = d_planes.to(torch.int64).sum(dim=1).tolist()
    filtered = d_delta.to(torch.int64).sum(dim=1).tolist()
    out = {"kind": kind, "gib": gib, "packets": npk, "copy_ms": round(copy, 4), "planes_ms": round(planes, 4), "eight_ms": round(old, 4),
           "delta_ms": round(new, 4), "delta_one_ms": [round(v, 4) for v in one_ms], "auto_ms": [round(v, 4) for v in auto_ms],
           "survey_ms": [round(v, 4) for v in survey_ms], "plain": plain, "filtered": filtered, "chosen": list(H.choose_filter(plain, filtered, npk))}
    print(f"{kind:13s} copy {copy:7.3f} ms  planes {planes:7.3f} ms  eight launches {old:7.3f} ms  delta survey {new:7.3f} ms = "
          f"{n / 1e6 / new:5.0f} GB/s read, (a) {new / old:.3f} of the eight; chosen {out['chosen']}")
    for j, w in enumerate(WIDTHS):
        print(f"{'':13s} w = {w}: delta survey alone {one_ms[j]:7.3f} ms  auto {auto_ms[j]:7.3f} ms  survey {survey_ms[j]:7.3f} ms  "
              f"(b) {survey_ms[j] / auto_ms[j]:.3f}")
    print(json.dumps(out))


def child_profile(kind, gib, reps=3):
    """The launches of comparison (b) at w = 1, and the delta survey with all widths, `reps` times each and untimed: the workload
    for rocprofv3 --kernel-trace --stats, and for a counter pass of its own."""
    import torch
    from gpuar_amd import hip as H
    n = int(gib * (1 << 30)) // 65536 * 65536
    dev = torch.device("cuda:0")
    npk = H.packet_count(n)
    d_in = make_input(kind, n, dev)
    d_tmp = torch.empty(n, dtype=torch.uint8, device=dev)
    d_rows = torch.empty((4, npk), dtype=torch.int32, device=dev)
    for _ in range(reps):
        H.estimate(d_in, d_est=d_rows[0])
        H.split_delta(d_in, 1, d_out=d_tmp)
        H.estimate(d_tmp, d_est=d_rows[0])
        H.survey_planes(d_in, d_est=d_rows)
        H.survey_delta(d_in, d_est=d_rows, widths=(1,))
        H.survey_delta(d_in, d_est=d_rows)
    torch.cuda.synchronize()
    assert H.status() == 0
    print(json.dumps({"kind": kind, "gib": gib, "profiled": reps}))


def child_compress(gib):
    import time
    import torch
    from gpuar_amd import batch
    dev = torch.device("cuda:0")
    t = make_input("sorted_int64", int(gib * (1 << 30)) // 65536 * 65536, dev).view(torch.int64)

    def wall(delta, reps=3):
        times = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = batch.compress([t], planes=8, delta=delta)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return min(times[1:]), c

    auto_ms, a = wall("auto")
    survey_ms, s = wall("survey")
    fixed_ms, _f = wall(True)
    assert a.delta == s.delta == [True] and torch.equal(a.stream, s.stream) and torch.equal(a.offsets, s.offsets)
    out = {"kind": "compress", "gib": gib, "auto_ms": round(auto_ms, 3), "survey_ms": round(survey_ms, 3), "fixed_ms": round(fixed_ms, 3),
           "nbytes": s.nbytes}
    print(f"compress      {gib:g} GiB of sorted int64, planes=8: delta=True {fixed_ms:8.2f} ms  delta=\"auto\" {auto_ms:8.2f} ms  "
          f"delta=\"survey\" {survey_ms:8.2f} ms = {survey_ms / auto_ms:.3f} of auto (wall clock, min of 3)")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--compress-gib", type=float, default=1.0)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--kind", help="(the child) measure this kind in this process")
    ap.add_argument("--profile", action="store_true", help="with --kind: run the launches untimed, for a profiler (see child_profile)")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds every child may take")
    ap.add_argument("--lib", default=None, help="an experiment build of libgpuar_hip.so to time instead of the product one")
    args = ap.parse_args()
    lib = ["--lib", os.path.abspath(args.lib)] if args.lib else []
    if args.kind:
        if lib:
            from gpuar_amd import hip as H
            H.LIB_PATH = lib[1]
        if args.profile:
            child_profile(args.kind, args.gib)
        elif args.kind == "compress":
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
        print(f"(a) delta survey / eight launches: worst {max(r['delta_ms'] / r['eight_ms'] for r in timed):.3f}")
        print(f"(b) two surveys / what delta=\"auto\" runs: worst {max(s / a for r in timed for s, a in zip(r['survey_ms'], r['auto_ms'])):.3f}")
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
