"""The mixed-filter kernels against the dedicated kernel of each mode, the copy and one survey launch, on the same buffers in the
same run (gpuar_hip_split_mixed / merge_mixed, gpuar_hip_choose_modes; torch events).

    python tools/mixed_timing.py [--gib G] [--codec-gib C] [--reps R]

1. For G GiB (default 4) of uniform(42) and a base of uniform(43) resident in HBM: the plain device copy of the same bytes
   (gpuar_hip_copy), then for each of the 12 modes split_mixed and merge_mixed with that mode in every supergroup beside the
   dedicated kernel of that mode (split_planes / split_delta / split_xor at its width; planes at a width of 1 is the copy), and
   both with the cyclic mix 0, 1, ..., 11.  Each pair is timed alternately, new / dedicated / new / dedicated ..., R times each
   (default 7), and reported as the minimum and the median with the ratio of the medians: what the 64 KiB of LDS that the XOR
   path needs costs the modes that do not use it shows here.  The yardsticks are the dedicated kernels and the copy, never the
   new kernels.
2. choose_modes on the survey rows of the same buffer beside one survey_planes launch over it.
3. batch.compress(planes="mixed", delta="mixed") beside batch.compress(planes="survey", delta="survey") and decompress of both on
   C GiB (default 1) of the constructed mix (bf16 weights, sorted int64 offsets, fp32, uniform bytes in the proportions 8 : 4 : 3 : 1)
   and on C GiB of homogeneous bf16 weights, where the finer choice gains nothing, with sizes.
What was timed is checked on the device: merge_mixed(split_mixed(x)) == x and split_mixed with one mode everywhere == the
dedicated kernel.  The last line is the same as JSON.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gpuar_amd import batch  # noqa: E402
from gpuar_amd import hip as H  # noqa: E402


def alternate(fns, reps):
    """[(min ms, median ms) per function]: the functions warmed up once each, then timed in turn, `reps` rounds"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    events = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            events[i].append((s, e))
    torch.cuda.synchronize()
    times = [[s.elapsed_time(e) for s, e in row] for row in events]
    return [(min(t), statistics.median(t)) for t in times]


def dedicated(mode, merge):
    w, delta, base = H.mode_parts(mode)
    if base:
        fn = H.merge_xor if merge else H.split_xor
        return lambda d_in, d_base, d_out: fn(d_in, d_base, w, d_out=d_out)
    fn = (H.merge_delta if merge else H.split_delta) if delta else (H.merge_planes if merge else H.split_planes)
    if w == 1 and not delta:
        return lambda d_in, d_base, d_out: H.device_copy(d_in, d_out)
    return lambda d_in, d_base, d_out: fn(d_in, w, d_out=d_out)


def constructed(n_bytes, dev, seed=1):
    """(tensor, base) of about n_bytes: bf16 weights a base apart in one element of a thousand, sorted int64 offsets, fp32, uniform
    bytes, 8 : 4 : 3 : 1, each part a whole number of supergroups; the base is unrelated outside the bf16 part"""
    g = torch.Generator(device=dev).manual_seed(seed)
    unit = n_bytes // 16 // H.SUPERGROUP * H.SUPERGROUP
    weights = (torch.randn(8 * unit // 2, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    moved = torch.rand(weights.numel(), generator=g, device=dev) < 1e-3
    base = torch.where(moved, (torch.randn(weights.numel(), generator=g, device=dev) * 0.02).to(torch.bfloat16), weights)
    offsets = torch.cumsum(torch.randint(1, 1000, (4 * unit // 8,), generator=g, device=dev), 0)
    floats = torch.randn(3 * unit // 4, generator=g, device=dev)
    noise = torch.randint(0, 256, (unit,), generator=g, device=dev, dtype=torch.uint8)
    x = torch.cat([weights.view(torch.uint8), offsets.view(torch.uint8), floats.view(torch.uint8), noise])
    rest = torch.randint(0, 256, (x.numel() - base.numel() * 2,), generator=g, device=dev, dtype=torch.uint8)
    return x, torch.cat([base.view(torch.uint8), rest])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--codec-gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"gib": args.gib, "codec_gib": args.codec_gib, "reps": args.reps}

    # 1. the kernels
    n = int(args.gib * (1 << 30)) // (12 * H.SUPERGROUP) * (12 * H.SUPERGROUP)      # whole supergroups, the cyclic mix a whole number of times
    n_modes = H.mode_count(n)
    d_in = H.generate("uniform", 42, n, device=dev)
    d_base = H.generate("uniform", 43, n, device=dev)
    d_dst = torch.empty(n, dtype=torch.uint8, device=dev)
    d_back = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    moved = 2 * n / 1e12
    (copy_min, copy_med), = alternate([lambda: H.device_copy(d_in, d_dst, n)], args.reps)
    print(f"{n / (1 << 30):.3f} GiB uniform(42) and a base of uniform(43), {n_modes} supergroups; copy {copy_min:.3f} ms min, {copy_med:.3f} ms median = "
          f"{moved / (copy_med / 1e3):.2f} TB/s (read + write)")
    out.update({"bytes": n, "copy_min_ms": round(copy_min, 4), "copy_median_ms": round(copy_med, 4)})
    for mode in range(H.MIXED_MODES):
        d_modes = torch.full((n_modes,), mode, dtype=torch.uint8, device=dev)
        for merge in (False, True):
            what = "merge" if merge else "split"
            new = H.merge_mixed if merge else H.split_mixed
            old = dedicated(mode, merge)
            (new_min, new_med), (old_min, old_med) = alternate(
                [lambda: new(d_in, d_modes, d_base, d_out=d_dst, d_status=status), lambda: old(d_in, d_base, d_dst)], args.reps)
            w, delta, base = H.mode_parts(mode)
            print(f"  mode {mode:2d} ({'base ' if base else 'delta' if delta else 'plane'} w = {w})  {what}_mixed {new_min:7.3f} min {new_med:7.3f} median;  "
                  f"dedicated {old_min:7.3f} min {old_med:7.3f} median;  mixed / dedicated {new_med / old_med:6.3f}")
            out.update({f"{what}_mixed_m{mode}_ms": [round(new_min, 4), round(new_med, 4)], f"{what}_dedicated_m{mode}_ms": [round(old_min, 4), round(old_med, 4)]})
        # what was timed is what the dedicated kernel gives, and it comes back
        H.split_mixed(d_in, d_modes, d_base, d_out=d_dst, d_status=status)
        dedicated(mode, False)(d_in, d_base, d_back)
        assert torch.equal(d_dst, d_back), f"split_mixed with mode {mode} everywhere differs from the dedicated kernel"
        H.merge_mixed(d_dst, d_modes, d_base, d_out=d_dst, d_status=status)
        assert torch.equal(d_dst, d_in), f"merge_mixed(split_mixed(x)) != x at mode {mode}"
    d_modes = (torch.arange(n_modes, device=dev) % H.MIXED_MODES).to(torch.uint8)
    (s_min, s_med), (m_min, m_med), (c_min, c_med) = alternate(
        [lambda: H.split_mixed(d_in, d_modes, d_base, d_out=d_dst, d_status=status), lambda: H.merge_mixed(d_in, d_modes, d_base, d_out=d_back, d_status=status),
         lambda: H.device_copy(d_in, d_back, n)], args.reps)
    print(f"  the cyclic mix 0 .. 11: split_mixed {s_min:7.3f} min {s_med:7.3f} median, merge_mixed {m_min:7.3f} min {m_med:7.3f} median; copy {c_med:7.3f} median")
    out.update({"split_mixed_cyclic_ms": [round(s_min, 4), round(s_med, 4)], "merge_mixed_cyclic_ms": [round(m_min, 4), round(m_med, 4)]})
    H.split_mixed(d_in, d_modes, d_base, d_out=d_dst, d_status=status)
    H.merge_mixed(d_dst, d_modes, d_base, d_out=d_dst, d_status=status)
    assert torch.equal(d_dst, d_in) and int(status.item()) == 0
    del d_dst, d_back

    # 2. the choice beside one survey launch
    d_plain = H.survey_planes(d_in)
    d_delta = H.survey_delta(d_in)
    d_xored, _scan = H.survey_xor(d_in, d_base, d_scan=False)
    d_m, d_t = H.choose_modes(d_plain, d_delta, d_xored, n, d_status=status)
    (ch_min, ch_med), (sv_min, sv_med) = alternate(
        [lambda: H.choose_modes(d_plain, d_delta, d_xored, n, d_modes=d_m, d_totals=d_t, d_status=status), lambda: H.survey_planes(d_in, d_est=d_plain)], args.reps)
    print(f"  choose_modes over {n_modes} supergroups (three surveys' rows) {ch_min:.3f} ms min {ch_med:.3f} median; one survey_planes launch "
          f"{sv_min:.3f} min {sv_med:.3f} median")
    out.update({"choose_modes_ms": [round(ch_min, 4), round(ch_med, 4)], "survey_planes_ms": [round(sv_min, 4), round(sv_med, 4)]})
    del d_in, d_base, d_plain, d_delta, d_xored

    # 3. the batch API
    m = int(args.codec_gib * (1 << 30))
    mix, _mix_base = constructed(m, dev)
    del _mix_base
    g = torch.Generator(device=dev).manual_seed(2)
    bf16 = (torch.randn(m // 2, generator=g, device=dev) * 0.02).to(torch.bfloat16).view(torch.uint8)
    for name, t in (("mix", mix), ("bf16", bf16)):
        results = {}
        for label, kw in (("mixed", {"planes": "mixed", "delta": "mixed"}), ("survey", {"planes": "survey", "delta": "survey"})):
            results[label] = batch.compress([t], **kw)
        enc = alternate([lambda: batch.compress([t], planes="mixed", delta="mixed"), lambda: batch.compress([t], planes="survey", delta="survey")], 3)
        back = torch.empty_like(t)
        dec = alternate([lambda: batch.decompress(results["mixed"], out=[back]), lambda: batch.decompress(results["survey"], out=[back])], 3)
        batch.decompress(results["mixed"], out=[back])
        assert torch.equal(back, t)
        for i, label in enumerate(("mixed", "survey")):
            c = results[label]
            print(f"  {name:4s} {t.numel() / (1 << 30):.3f} GiB, {label:6s}: {c.nbytes} bytes = {c.nbytes / t.numel():.4f} of the input; compress "
                  f"{enc[i][0]:.2f} ms min {enc[i][1]:.2f} median, decompress {dec[i][0]:.2f} ms min {dec[i][1]:.2f} median")
            out.update({f"codec_{name}_{label}_bytes": c.nbytes, f"codec_{name}_{label}_compress_ms": [round(v, 3) for v in enc[i]],
                        f"codec_{name}_{label}_decompress_ms": [round(v, 3) for v in dec[i]]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
