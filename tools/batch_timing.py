"""Batch encode / decode against single-buffer calls (gpuar_hip_encode_batch, decode_batch; torch events, min of 7).

    python tools/batch_timing.py [--quick]

Lines: K = 1 over 8 GiB uniform(42) against hip.encode / hip.decode; 1024 x (1 MiB + 4097 B) (throughput kernel) and
128 x (1 MiB + 4097 B) (latency kernel) against single-buffer calls on the same total bytes and against K separate
calls; 16384 x 3000 B (every packet short).  --quick: the 8 GiB line on 1 GiB.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

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


def batch_case(sizes, mode, separate=True):
    """(batch enc, batch dec, single enc, single dec, separate enc, separate dec) in ms, and whether everything round-trips"""
    gap = [(n + 15) // 16 * 16 for n in sizes]
    arena = torch.empty(sum(gap) + 16, dtype=torch.uint8, device="cuda")
    starts, at = [], 0
    for g in gap:
        starts.append(at)
        at += g
    total = sum(sizes)
    H.generate("uniform", 42, arena.numel(), out=arena)
    views = [arena[s:s + n] for s, n in zip(starts, sizes)]
    fp, npk = H.batch_packet_count(sizes)
    d = torch.tensor([v.data_ptr() for v in views] + sizes + fp, dtype=torch.int64).cuda()
    k = len(sizes)
    d_ptrs, d_bytes, d_fp = d[:k], d[k:2 * k], d[2 * k:]
    slots = torch.empty(npk * H.SLOT, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(arena)
    outs = torch.tensor([out.data_ptr() + s for s in starts], dtype=torch.int64).cuda()
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    enc = best(lambda: H.encode_batch(d_ptrs, d_bytes, d_fp, k, npk, d_slots=slots, d_status=st, mode=mode))
    dec = best(lambda: H.decode_batch(slots, d_fp, k, npk, outs, d_bytes, d_status=st))
    ok = int(st.item()) == 0 and all(torch.equal(out[s:s + n], v) for s, n, v in zip(starts, sizes, views))
    flat = arena[:total]
    single_pk = H.packet_count(total)
    s_slots = torch.empty(single_pk * H.SLOT, dtype=torch.uint8, device="cuda")
    s_out = torch.empty(single_pk * PACKET, dtype=torch.uint8, device="cuda")
    s_enc = best(lambda: H.encode(flat, s_slots, mode=mode))
    s_dec = best(lambda: H.decode(s_slots, single_pk, s_out))
    sep_enc = sep_dec = float("nan")
    if separate:
        per = [torch.empty(max(H.packet_count(n), 1) * H.SLOT, dtype=torch.uint8, device="cuda") for n in sizes]
        per_out = [torch.empty(max(H.packet_count(n), 1) * PACKET, dtype=torch.uint8, device="cuda") for n in sizes]
        sep_enc = best(lambda: [H.encode(v, p, mode=mode) for v, p in zip(views, per)], reps=3)
        sep_dec = best(lambda: [H.decode(p, H.packet_count(v.numel()), o) for v, p, o in zip(views, per, per_out)], reps=3)
    return enc, dec, s_enc, s_dec, sep_enc, sep_dec, ok, total


def line(name, r):
    enc, dec, s_enc, s_dec, sep_enc, sep_dec, ok, total = r
    print(f"{name:34s} {total / 2**20:9.1f} MiB  batch enc {enc:8.3f} ms dec {dec:8.3f} ms | one buffer enc {s_enc:8.3f} dec {s_dec:8.3f} "
          f"(x{enc / s_enc:5.3f} / x{dec / s_dec:5.3f}) | separate calls enc {sep_enc:9.3f} dec {sep_dec:9.3f} "
          f"(x{sep_enc / enc:6.1f} / x{sep_dec / dec:6.1f}) | round trip {ok}", flush=True)


def main():
    quick = "--quick" in sys.argv
    H.load()
    big = (1 if quick else 8) * 2**30
    line("K=1 uniform(42)", batch_case([big], "auto", separate=False))
    mib = 2**20 + 4097
    line("1024 x (1 MiB + 4097 B) throughput", batch_case([mib] * 1024, "throughput"))
    line("128 x (1 MiB + 4097 B) latency", batch_case([mib] * 128, "latency"))
    line("16384 x 3000 B auto", batch_case([3000] * 16384, "auto", separate=False))


if __name__ == "__main__":
    main()
