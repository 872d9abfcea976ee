"""The packet-form kernels under concurrent streams and host threads: the contract that tests/test_gpu_concurrency.py pins for the
coders and tests/test_gpu_filter_concurrency.py for the filters, here for sparse_scan, sparse_scan_batch, sparse_pack,
sparse_unpack, kinds_store, kinds_expand (4.13), move_bytes (4.14) and for what gpuar_amd/batch.py composes from
them: compress(..., sparse="auto"), Compressed.gip(b, kinds=True) and from_gip.  The rules are those of the filter module: every
call takes an explicit stream; a launch ORs its flags into its own status word and into no other; a launch without a word uses
the fallback word, which status() reports once; and a run whose producer was too short FAILS, it does not pass.

Every test works the same way: a serial pass (one launch at a time, synchronised) is pinned against existing host code --
hip.sparse_scan_host, sparse_pack_host, sparse_unpack_host, kinds_store_host, kinds_expand_host, estimate_host, sparse_rule,
numpy slicing for move_bytes --; then the same work runs concurrently and must give the same bytes, with every status word
exactly what its own launch should report.  Everything is integer-exact.  Comparisons run on the device; one copy of the verdicts
per test.

Stream / thread i runs WORKLOADS[i]: a packet count, the bytes of the short last packet and a mix of packet kinds (fills with 0,
2, 64 and 100 exceptions, uniform bytes that are kept raw, text that is coded), drawn from nine template packets whose scan word,
estimate, kind, record and stream form come from the host functions.  Workloads 6 and 7 have 8197 and 24 581 packets: sparse_scan,
kinds_store and kinds_expand launch at most 8192 wavefronts, so theirs go round the chip and loop while seven other streams
contend for it.  The slots kinds_store works on hold a made-up header (clen 4 + p % 251) in front of canaries, as in
tests/test_gpu_address_edges.py: a coded packet's slot must come back untouched.

1. Stream order.  On a non-blocking stream s that is not the current stream the producer of the filter module runs (a chain of
   device_copy calls over 256 MiB, sized at run time by that module's rule), its last links deliver the real input where the
   canary was, the call under test is enqueued behind it with stream=s, and a copy of its output behind that.  An event behind
   the producer must still be pending after the last enqueue, or the test fails as "producer too short".  A launch that went to
   any other stream reads the canary, or is overwritten by the feed, and differs.  All seven kernels, workloads 2 and 6.  A
   control sends sparse_scan to another stream on purpose and must differ.  batch.compress(sparse="auto") and batch.from_gip
   wait for their stream themselves, so for them the producer must be pending when the call begins; compress has a control
   of its own (test_stream_order_of_the_batch_calls, which says what it can and cannot show for from_gip).
2. Fan-out with status isolation, one family at a time, eight streams.  Stream 1 carries the defect and only its words may
   have the flag: a misaligned buffer in sparse_scan_batch (BAD_BATCH, its scan words keep the canary); an exception count that is
   one too many in the scan word sparse_pack and kinds_store are given (BAD_BATCH: no record written; kind 0, the slot
   untouched); a record whose second position repeats the first in sparse_unpack and kinds_expand (BAD_PACKET: the packet's own
   bytes are unspecified and left out of the comparison, every other byte is compared); a region of 8705 bytes in move_bytes
   (BAD_BATCH, its destination keeps the canary).
3. The fallback word: each entry point that takes d_status=None with that one defect; status() reports it once and is then 0.
4. Mixed co-residency: a 256 MiB throughput encode next to sparse_unpack and kinds_expand (32 KiB of LDS per workgroup),
   kinds_store (248 vector registers), sparse_scan and move_bytes, the encoder enqueued first or last.
5. Six host threads, each with its own stream: batch.compress(..., sparse="auto") with stored None and "auto", planes=2, base=
   with a tensor equal to its base, checksum=True, then decompress, Compressed.gip(b, kinds=True) -> from_gip -> decompress.  The
   serial pass is pinned (kinds against hip.sparse_rule on the host scan words and estimates of the bytes that are coded, records
   against sparse_pack_host, round trips exact); the threads must reproduce every field of Compressed.

Would catch: a launch on the NULL or the current stream (1), a status word shared between launches or a flag ORed into the
fallback word beside the launch's own (2, 3), LDS or register state that survives a wavefront's trip when the chip is shared (2,
4), torch temporaries of _partition or of from_gip's region lists made on one stream and used on another (5).

Not covered here: the region kernels (sparse_pack, sparse_unpack, move_bytes) take a region per wavefront or workgroup and their
grid-stride loops start at 2^22 workgroups; tests/test_gpu_grid_cap.py runs their later passes on a build whose cap is 3, as it
does for move_packets and the filters.  Tensors on a device
that is not the current one; from_gip from paths (the files are bytes in memory here).  Fixed seeds throughout.

Time, pytest --durations=0 on an MI355X, the module alone: 11 passed in 3.2 s.  One producer link (a 256 MiB device_copy) ran
87.0 us on the GPU and took 5.0 us of host time to enqueue; the slowest call's feeds, launch and copies took 115 us to enqueue.
    0.35 s  setup of test_stream_order[2] (the eight workloads and their references, the producer's two 256 MiB buffers)
    0.29 s  test_mixed_co_residency[encoder_first] (the first encode of the process)
    0.28 s  test_stream_order_of_the_batch_calls (three chains of 64 links, each waited for)
    0.25 s  test_thread_batch_sparse_auto_and_from_gip (the serial pass with its host references, then the six threads)
    0.10 s  test_stream_order[2] (seven kernels, each serial and behind a chain of at least 64 links, and the control)
    0.05 s  test_stream_order[6]
    0.01 s  test_mixed_co_residency[encoder_last], test_fan_out[kinds], test_fan_out[scan]; the rest is under 0.005 s.
Launches under test: 15 in each test_stream_order (seven kernels serial and ordered, and the control), up to 32 in each of the
fan-outs of two entry points and 16 in move_bytes' (eight streams, serial and concurrent), 6 in test_fallback_word, 12 in each
co-residency variant beside the two encodes.  Memory: about 3 GiB for the workloads and their references (workload 7 alone
has 201 MB of packets and 214 MB of slots, each as input, buffer and reference), 0.5 GiB for the producer, 0.6 GiB for the
encode with its slots.
"""
import struct
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import kinds_ref as K
from sparse_ref import _packet as _filled
from concurrency_checks import _fail_on, _same, _status, _streams, _words
from test_gpu_filter_concurrency import Case, _blank, _dev, _enqueue_behind_producer, _links, _r16, producer  # noqa: F401 (producer: a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
MiB = 1 << 20
CANARY = 0xA5
CANARY32 = 0xA5A5A5A5 - (1 << 32)
GUARD = 256
SEED = 20261020
MOVES = 4096                         # move_bytes takes the first MOVES packets of a workload's stream apart
BAD_BUFFER, BAD_REGION = 2, 5        # stream 1's defects: the batch buffer with the misaligned pointer, the region of 8705 bytes

# (packets, bytes of the last one, the share of sparse / raw / coded templates): stream / thread i runs workload i
WORKLOADS = [
    (1, 1, (1, 0, 0)),
    (65, 77, (2, 1, 1)),
    (301, 4097, (1, 1, 1)),
    (5, PACKET, (1, 1, 0)),
    (1001, 8191, (3, 1, 1)),
    (2050, 1, (1, 3, 1)),
    (8192 + 5, 100, (1, 1, 3)),
    (3 * 8192 + 5, 77, (2, 1, 1)),
]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()          # raises if the HIP library is missing: no fallback
    return hip


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# templates, workloads and their references
# ---------------------------------------------------------------------------------------------------------------------
def _form(H, x):
    """(scan word, estimate, kind, the packet in its stream form or b"", its record or b"") of one packet, from the host functions."""
    raw = x.tobytes()
    scan, est = H.sparse_scan_host(raw)[0], H.estimate_host(raw)[0]
    kind, pkt = H.kinds_store_host(raw, True, True)
    assert kind == H.sparse_rule(scan, est, x.size, True) == K.kind_of(x, True, True)
    rec = pkt[4:] if kind == K.SPARSE else b""
    if kind == K.SPARSE:
        assert rec == H.sparse_pack_host(raw) and H.sparse_unpack_host(rec, x.size) == raw and H.kinds_expand_host(pkt, kind, x.size) == raw
    elif kind == K.RAW:
        assert pkt == struct.pack("<HH", 4 + x.size, x.size) + raw and H.kinds_expand_host(pkt, kind, x.size) == raw
    return scan, est, kind, pkt, rec


@pytest.fixture(scope="module")
def T(H):
    """The nine template packets, by kind: five sparse, two raw, two coded."""
    rng = np.random.default_rng([SEED, 0])
    lanes = np.arange(64)
    text = np.frombuffer(K.TEXT[:PACKET], dtype=np.uint8).copy()
    xs = [np.zeros(PACKET, dtype=np.uint8), np.full(PACKET, 0xFF, dtype=np.uint8), _filled(PACKET, 0x00, np.arange(100) * 81 + 7),
          _filled(PACKET, 0x55, [9, 4000]), _filled(PACKET, 0x80, lanes * 128 + (lanes * 37) % 128),
          rng.integers(0, 256, PACKET, dtype=np.uint8), rng.integers(0, 256, PACKET, dtype=np.uint8), text, np.roll(text, 41)]
    forms = [_form(H, x) for x in xs]
    assert [f[2] for f in forms] == [K.SPARSE] * 5 + [K.RAW] * 2 + [K.CODED] * 2
    return xs, forms


class Load:
    """Workload i: its bytes, the references of the seven kernels as images on the device (canaries behind them), the buffers
    they work on and one `Op` per kernel.  bad: the defects of the module docstring's part 2, and the references changed to what
    the contract says of them."""

    def __init__(self, H, T, i, bad=False):
        npk, last, shares = WORKLOADS[i]
        rng = np.random.default_rng([SEED, 1, i])
        weights = np.repeat(np.array(shares, dtype=np.float64) / np.array([5, 2, 2]), [5, 2, 2])
        idx = rng.choice(9, npk, p=weights / weights.sum())
        if bad:
            idx[3] = 2                                       # (the packet that carries the defect: 100 exceptions)
        xs, forms = list(T[0]), list(T[1])
        tail = xs[idx[-1]][:last].copy()                     # the short last packet: a template cut, a form of its own
        xs.append(tail)
        forms.append(_form(H, tail))
        idx[-1] = 9
        self.i, self.npk, self.n, self.bad = i, npk, (npk - 1) * PACKET + last, bad
        n, S = self.n, _r16(self.n) + GUARD
        size = np.full(npk, PACKET, dtype=np.int64)
        size[-1] = last
        scan = np.array([f[0] for f in forms], dtype=np.uint32)[idx]
        est = np.array([f[1] for f in forms], dtype=np.uint32)[idx]
        kind = np.array([f[2] for f in forms], dtype=np.uint8)[idx]
        made_up = 4 + np.arange(npk) % 251
        clen = np.where(kind == K.CODED, made_up, np.array([len(f[3]) for f in forms])[idx]).astype(np.int64)
        images = np.full((10, PACKET), CANARY, dtype=np.uint8)
        slot_t = np.full((10, SLOT), CANARY, dtype=np.uint8)
        for t, (x, f) in enumerate(zip(xs, forms)):
            images[t, :x.size] = x
            slot_t[t, :len(f[3])] = np.frombuffer(f[3], dtype=np.uint8)
        d_idx = _dev(idx)
        rows = _dev(images)[d_idx]                           # packet p in row p, canaries behind the short last one
        pad = _blank(GUARD + 16)
        self.x_img = torch.cat([rows.view(-1), pad])[:S].clone()
        before = _blank(npk * SLOT + GUARD)
        b = before[:npk * SLOT].view(npk, SLOT)
        b[:, 0] = _dev(made_up.astype(np.uint8))
        b[:, 1] = 0
        b[:, 2] = _dev((size & 255).astype(np.uint8))
        b[:, 3] = _dev((size >> 8).astype(np.uint8))
        good_after = before.clone()
        good_after[:npk * SLOT].view(npk, SLOT).copy_(torch.where(_dev(kind == K.CODED)[:, None], b, _dev(slot_t)[d_idx]))
        # the stream: compact (tested elsewhere) of the reference slots, its offsets pinned against the clens
        d_stream, d_offsets = H.compact(good_after[:npk * SLOT], npk)
        offs = np.concatenate([[0], np.cumsum(clen)])
        assert d_offsets.cpu().numpy().tolist() == offs.tolist(), f"workload {i}: compact's offsets are not the sums of the clens"
        total = int(offs[-1])
        stream = torch.cat([d_stream[:total], _blank(_r16(total) - total + GUARD)])
        del d_stream
        sp = np.flatnonzero(kind == K.SPARSE)
        assert sp.size or i == 3 or npk == 1
        rec_len = clen[sp] - 4
        rec_off = np.concatenate([[0], np.cumsum(rec_len)]).astype(np.int64)
        recs = np.full(_r16(int(rec_off[-1])) + GUARD, CANARY, dtype=np.uint8)
        recs[:rec_off[-1]] = np.frombuffer(b"".join(forms[idx[p]][4] for p in sp), dtype=np.uint8)
        scan_in, kind_want, after, keep_out, keep_upk = scan.copy(), kind.copy(), good_after, None, None
        stream_in, recs_in, recs_want = stream, recs.copy(), recs.copy()
        if bad:
            p_bad, j_bad = 3, int(np.flatnonzero(sp == 3)[0])
            assert kind[p_bad] == K.SPARSE and scan[p_bad] >> 8 == 100
            scan_in[p_bad] += 1 << 8                         # one exception too many: BAD_BATCH
            kind_want[p_bad] = K.CODED
            after = good_after.clone()
            after[p_bad * SLOT:(p_bad + 1) * SLOT] = before[p_bad * SLOT:(p_bad + 1) * SLOT]
            recs_want[rec_off[j_bad]:rec_off[j_bad + 1]] = CANARY
            recs_in[rec_off[j_bad] + 6:rec_off[j_bad] + 8] = recs_in[rec_off[j_bad] + 4:rec_off[j_bad] + 6]      # pos[1] = pos[0]: BAD_PACKET
            stream_in = stream.clone()
            at = int(offs[p_bad]) + 8
            stream_in[at + 2:at + 4] = stream_in[at:at + 2]
            keep_out = torch.ones(S, dtype=torch.bool, device="cuda")
            keep_out[p_bad * PACKET:(p_bad + 1) * PACKET] = False
            keep_upk = torch.ones(_r16(sp.size * PACKET) + GUARD, dtype=torch.bool, device="cuda")
            keep_upk[j_bad * PACKET:(j_bad + 1) * PACKET] = False
        out_rows = torch.where(_dev(kind != K.CODED)[:, None], rows, torch.full_like(rows, CANARY))
        out_img = torch.cat([out_rows.view(-1), pad])[:S].clone()
        upk_img = torch.cat([rows[_dev(sp)].view(-1), _blank(_r16(sp.size * PACKET) - sp.size * PACKET + GUARD)])
        # the batch of sparse_scan_batch: the workload cut at packet boundaries into up to seven buffers, in a shuffled order
        cuts = sorted({0, npk} | {int(c) for c in rng.integers(1, max(npk, 2), 6) if c < npk})
        chunks = [(a, b_) for a, b_ in zip(cuts[:-1], cuts[1:])]
        chunks = [chunks[j] for j in rng.permutation(len(chunks))]
        sizes = [int(size[a:b_].sum()) for a, b_ in chunks]
        fp, total_pk = H.batch_packet_count(sizes)
        assert total_pk == npk
        scan_b = np.concatenate([scan[a:b_] for a, b_ in chunks])
        bad_buffer = bad and len(chunks) > BAD_BUFFER
        assert bad_buffer == bad
        if bad:
            scan_b[fp[BAD_BUFFER]:fp[BAD_BUFFER + 1]] = CANARY32 & 0xFFFFFFFF
        # move_bytes: the first packets of the stream to one block, back to back in reversed order
        m = min(npk, MOVES)
        mv_len = clen[:m].copy()
        mv_dst = (int(mv_len.sum()) - np.cumsum(mv_len)).astype(np.int64)
        host_stream = stream[:int(offs[m])].cpu().numpy()
        mv = np.full(_r16(int(mv_len.sum())) + GUARD, CANARY, dtype=np.uint8)
        for r in range(m):
            if not (bad and r == BAD_REGION):
                mv[mv_dst[r]:mv_dst[r] + mv_len[r]] = host_stream[offs[r]:offs[r + 1]]
        mv_bytes = mv_len.copy()
        if bad:
            assert m > BAD_REGION
            mv_bytes[BAD_REGION] = SLOT + 1

        def words(a):
            """32-bit words and canaries behind them, as bytes on the device."""
            img = np.full((a.size + 2 + 3) // 4 * 4, CANARY32 & 0xFFFFFFFF, dtype=np.uint32)
            img[:a.size] = a
            return _dev(img.view(np.uint8))

        kind_img = np.full(_r16(npk) + GUARD, CANARY, dtype=np.uint8)
        kind_img[:npk] = kind_want
        # the buffers the calls work on
        a, st, rin = _blank(S), _blank(stream.numel()), _blank(recs.size)
        e, eb = _blank(words(scan).numel()), _blank(words(scan_b).numel())
        rout, upk, slots, kd, out, mvd = _blank(recs.size), _blank(upk_img.numel()), _blank(before.numel()), _blank(kind_img.size), _blank(S), _blank(mv.size)
        d_est, d_scan_in, d_scan_sp = _dev(est.view(np.int32)), _dev(scan_in.view(np.int32)), _dev(scan_in[sp].view(np.int32))
        d_kind_in, d_offs = _dev(kind), _dev(offs.astype(np.int64))
        ptrs = np.array([a.data_ptr() + c[0] * PACKET for c in chunks], dtype=np.int64)
        if bad:
            ptrs[BAD_BUFFER] += 8
        desc = _dev(np.concatenate([ptrs, sizes, fp]).astype(np.int64))
        nb = len(chunks)
        d_ptrs, d_bytes, d_fp = desc[:nb], desc[nb:2 * nb], desc[2 * nb:]
        k = sp.size
        pack = _dev(np.concatenate([a.data_ptr() + sp * PACKET, size[sp], rout.data_ptr() + rec_off[:-1]]).astype(np.int64))
        unpack = _dev(np.concatenate([rin.data_ptr() + rec_off[:-1], rec_len, upk.data_ptr() + np.arange(k) * PACKET, size[sp]]).astype(np.int64))
        moves = _dev(np.concatenate([st.data_ptr() + offs[:m], mvd.data_ptr() + mv_dst, mv_bytes]).astype(np.int64))
        tag = f"workload {i} ({npk} packets, {n} bytes, {k} sparse)"
        flag = lambda f: f if bad else 0
        self.tag = tag
        self.ops = [
            Op("sparse_scan", "scan", f"sparse_scan, {tag}", [(self.x_img, a)],
               lambda s, _w: H.sparse_scan(a, n_bytes=n, d_scan=e.view(torch.int32), stream=s), [(e, words(scan), None)], None),
            Op("sparse_scan_batch", "scan", f"sparse_scan_batch over {nb} buffers, {tag}", [(self.x_img, a)],
               lambda s, w: H.sparse_scan_batch(d_ptrs, d_bytes, d_fp, nb, npk, d_scan=eb.view(torch.int32), stream=s, d_status=w),
               [(eb, words(scan_b), None)], flag(H.STATUS_BAD_BATCH)),
            Op("sparse_pack", "records", f"sparse_pack of {k} packets, {tag}", [(self.x_img, a)],
               lambda s, w: k and H.sparse_pack(pack[:k], pack[k:2 * k], d_scan_sp, pack[2 * k:], k, stream=s, d_status=w),
               [(rout, _dev(recs_want), None)], flag(H.STATUS_BAD_BATCH)),
            Op("sparse_unpack", "records", f"sparse_unpack of {k} records, {tag}", [(_dev(recs_in), rin)],
               lambda s, w: k and H.sparse_unpack(unpack[:k], unpack[k:2 * k], unpack[2 * k:3 * k], unpack[3 * k:], k, stream=s, d_status=w),
               [(upk, upk_img, keep_upk)], flag(H.STATUS_BAD_PACKET)),
            Op("kinds_store", "kinds", f"kinds_store, {tag}", [(self.x_img, a), (before, slots)],
               lambda s, w: H.kinds_store(a, d_est, d_scan_in, True, slots[:npk * SLOT], n_bytes=n, d_kind=kd[:npk], stream=s, d_status=w),
               [(slots, after, None), (kd, _dev(kind_img), None)], flag(H.STATUS_BAD_BATCH)),
            Op("kinds_expand", "kinds", f"kinds_expand, {tag}", [(stream_in, st)],
               lambda s, w: H.kinds_expand(st, d_offs, d_kind_in, npk, out, n, stream=s, d_status=w), [(out, out_img, keep_out)], flag(H.STATUS_BAD_PACKET)),
            Op("move_bytes", "move_bytes", f"move_bytes of {m} regions, {tag}", [(stream, st)],
               lambda s, w: H.move_bytes(moves[:m], moves[m:2 * m], moves[2 * m:], m, stream=s, d_status=w), [(mvd, _dev(mv), None)], flag(H.STATUS_BAD_BATCH)),
        ]
        self.by_name = {op.entry: op for op in self.ops}


class Op:
    """One call of a workload: `feeds` [(image, buffer)] put its inputs in place, run(stream, word) enqueues it, `outs` [(buffer,
    the image it must equal afterwards, the bytes that are compared or None for all)], `flag`: what its status word must hold
    afterwards (None: the call takes no word)."""

    def __init__(self, entry, family, name, feeds, run, outs, flag):
        self.entry, self.family, self.name, self.feeds, self.run, self.outs, self.flag = entry, family, name, feeds, run, outs, flag

    def fill(self):
        for image, buf in self.feeds:
            buf.copy_(image)
        for buf, _want, _keep in self.outs:
            if all(buf is not fed for _image, fed in self.feeds):
                buf.fill_(CANARY)

    def verdicts(self, tag, against):
        return [(f"{self.name}{tag}: output {j} differs from {against}, or canaries behind it or in what the call must leave alone are gone",
                 _same(buf, want) if keep is None else (buf.eq(want) | ~keep).all()) for j, (buf, want, keep) in enumerate(self.outs)]

    def case(self):
        return Case(self.name, self.feeds, self.run, [(buf, want) for buf, want, _keep in self.outs])


@pytest.fixture(scope="module")
def W(H, T):
    ws = [Load(H, T, i) for i in range(len(WORKLOADS))]
    torch.cuda.synchronize()
    return ws


def _serial(ops, words, tag=" (serial)"):
    """Each op alone on the current stream, synchronised: its verdicts against the references."""
    v = []
    for j, op in enumerate(ops):
        op.fill()
        op.run(None, words[j:j + 1])
        torch.cuda.synchronize()
        v += op.verdicts(tag, "the reference")
    return v


# ---------------------------------------------------------------------------------------------------------------------
# 1. stream order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 6])
def test_stream_order(H, W, producer, i):
    """Each of the seven kernels reads what the work in front of it on ITS stream wrote and is read by what comes behind it
    there.  Serial pass: feeds, call, synchronise, against the references; its enqueue is timed.  Ordered pass: see the module
    docstring.  A call that is not on `stream=` fails its own check here; a producer that is over before the last enqueue
    fails the test as inconclusive."""
    ops = W[i].ops
    cases = [op.case() for op in ops]
    words = _status(2 * len(cases))
    s, other = _streams(2)
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    H.device_copy(producer[0][:4096], producer[1][:4096], stream=s)          # (the streams' first launches are not timed)
    H.device_copy(producer[0][:4096], producer[1][:4096], stream=other)
    torch.cuda.synchronize()
    verdicts, short, slowest = [], [], 0.0
    for c, case in enumerate(cases):
        results, _pending, call_host = _enqueue_behind_producer(H, producer, None, case, words[2 * c:2 * c + 1], None, 0)
        torch.cuda.synchronize()
        slowest = max(slowest, call_host)
        for j, ((buf, want), r) in enumerate(zip(case.outs, results)):
            verdicts.append((f"{case.name} (serial): output {j} differs from the reference or its canaries are gone", _same(buf, want) & _same(r, want)))
        links = _links(producer, call_host)
        results, pending, _host = _enqueue_behind_producer(H, producer, s, case, words[2 * c + 1:2 * c + 2], s, links)
        s.synchronize()
        if not pending:
            short.append(f"{case.name} ({links} links for an enqueue of {call_host * 1e6:.0f} us)")
        for j, ((_buf, want), r) in enumerate(zip(case.outs, results)):
            verdicts.append((f"{case.name}: behind a producer on its stream, output {j} differs from the serial result "
                             "(the call did not run on stream=, or wrote behind its output)", _same(r, want)))
    control = cases[0]
    results, pending, _host = _enqueue_behind_producer(H, producer, s, control, None, other, _links(producer, slowest))
    torch.cuda.synchronize()
    control_differs = bool((~_same(results[0], control.outs[0][1])).item())
    print(f"slowest enqueue of a call with its feeds and copies: {slowest * 1e6:.0f} us")
    if not pending:
        short.append(f"the control ({control.name} on another stream)")
    assert not short, f"producer too short: it was over before the last enqueue of {len(short)} calls, which proves nothing: " + "; ".join(short[:8])
    assert control_differs, f"producer too short: the control ({control.name} enqueued on ANOTHER stream) gave the serial result"
    _words(verdicts, words, [0] * (2 * len(cases)), [f"{case.name}{tag}" for case in cases for tag in (" (serial)", "")])
    _fail_on(verdicts)
    assert H.status() == 0, "a launch reported into the fallback word"


def test_stream_order_of_the_batch_calls(H, W, producer):
    """batch.compress(..., sparse="auto") and batch.from_gip behind the producer.  Both read counts on the host and so wait for
    their stream themselves: the producer cannot be pending after them and must be pending when they BEGIN (checked right before
    the call, else "producer too short").  compress reads a buffer that holds canaries until the last link delivers workload 2:
    a launch of its pipeline (estimate_batch, sparse_scan_batch, the encoder, move_packets, sparse_pack) on another stream sees
    the canaries, and every field must equal the serial pass; a control with stream= another stream must differ.  from_gip's
    input is host memory, uploaded by the call itself on its stream: its move_bytes launch on another stream would read the
    upload's memory before the upload.  That memory is whatever the allocator hands out, so the cache is emptied and a block of
    canaries freed in front of the call; this is the best that can be done from outside and is weaker than the other checks."""
    from gpuar_amd import batch
    k = W[2]
    n = k.n
    a = _blank(k.x_img.numel())
    kw = dict(sparse="auto", stored="auto", checksum=True)
    a.copy_(k.x_img)
    want = batch.compress([a[:n]], **kw)
    files = [want.gip(0, kinds=True)]
    want_back = batch.from_gip(files)
    torch.cuda.synchronize()
    assert set(want.stored.cpu().tolist()) == {K.CODED, K.RAW, K.SPARSE} and torch.equal(batch.decompress(want_back)[0], a[:n])
    s, other = _streams(2)
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    p, q = producer[:2]
    links = _links(producer, 0.0)

    def behind_producer(call, feed):
        torch.cuda.synchronize()
        for _ in range(links):
            H.device_copy(p, q, stream=s)
        if feed:
            H.device_copy(k.x_img, a, stream=s)
        behind = torch.cuda.Event()
        behind.record(s)
        pending = not behind.query()
        got = call()
        torch.cuda.synchronize()
        return got, pending

    a.fill_(CANARY)
    got, pending_c = behind_producer(lambda: batch.compress([a[:n]], stream=s, **kw), True)
    a.fill_(CANARY)
    control, pending_x = behind_producer(lambda: batch.compress([a[:n]], stream=other, **kw), True)
    torch.cuda.empty_cache()
    junk = _blank(64 * MiB)
    del junk
    back, pending_g = behind_producer(lambda: batch.from_gip(files, stream=s), False)
    assert pending_c and pending_x and pending_g, f"producer too short: {links} links were over before compress, the control or from_gip began: " \
                                                  f"{(pending_c, pending_x, pending_g)}"
    assert not torch.equal(control.stored, want.stored), "producer too short: compress on ANOTHER stream gave the serial kinds"
    verdicts = []
    for which, c, ref in (("compress", got, want), ("from_gip", back, want_back)):
        assert (c.planes, c.delta, c.based, c.first_packet, c.sizes, c.kinds_rule) == (ref.planes, ref.delta, ref.based, ref.first_packet, ref.sizes, ref.kinds_rule)
        for field in FIELDS:
            verdicts.append((f"{which} behind a producer on its stream: {field} differs from the serial pass", _same_or_none(getattr(c, field), getattr(ref, field))))
    _fail_on(verdicts)
    assert H.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. fan-out with status isolation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def defective(H, T):
    """Workload 1 with one defect per entry point."""
    load = Load(H, T, 1, bad=True)
    torch.cuda.synchronize()
    return load


@pytest.mark.parametrize("family", ["scan", "records", "kinds", "move_bytes"])
def test_fan_out(H, W, defective, family):
    """The calls of one family on each of eight streams at once, every launch with its own status word.  Stream 1 runs the
    defective workload: the flag of its defect in its own words and in no other, what the contract says is left alone keeps its
    canary, and every other byte of every stream equals the serial result."""
    loads = [defective if i == 1 else w for i, w in enumerate(W)]
    ops = [[op for op in load.ops if op.family == family] for load in loads]
    per = len(ops[0])
    k8 = len(loads)
    words = _status(2 * per * k8)
    verdicts = []
    for i in range(k8):
        verdicts += _serial(ops[i], words[per * i:per * (i + 1)], f" (stream {i}, serial)")
    for mine in ops:
        for op in mine:
            op.fill()
    streams = _streams(k8)
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        for j, op in enumerate(ops[i]):
            op.run(s, words[per * (k8 + i) + j:per * (k8 + i) + j + 1])
    torch.cuda.synchronize()
    for i in range(k8):
        for op in ops[i]:
            verdicts += op.verdicts(f" (stream {i})", "the serial result")
    expected = [op.flag or 0 for mine in ops for op in mine] * 2
    assert sum(1 for f in expected if f) == 2 * sum(1 for op in ops[1] if op.flag)
    _words(verdicts, words, expected, [f"{op.name}{tag}" for tag in (" (serial)", "") for mine in ops for op in mine])
    _fail_on(verdicts)
    assert H.status() == 0, f"{family}: a launch reported into the fallback word"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the fallback word
# ---------------------------------------------------------------------------------------------------------------------
def test_fallback_word(H, defective):
    """d_status=None: the launch reports into the fallback word; status() returns the flag once and clears it."""
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert H.status() == 0
    seen = []
    for op in defective.ops:
        if op.flag is None:
            continue
        op.fill()
        torch.cuda.synchronize()
        op.run(s, None)
        seen.append((op.entry, op.flag, H.status(), H.status()))
    assert len(seen) == 6
    wrong = [f"{name}: status() gave {first:#x}, then {second:#x} (want {flag:#x}, then 0)" for name, flag, first, second in seen if (first, second) != (flag, 0)]
    assert not wrong, "the fallback word after a launch without a word of its own: " + "; ".join(wrong)
    assert H.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. mixed co-residency
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["encoder_first", "encoder_last"])
def test_mixed_co_residency(H, W, order):
    """A throughput encode of 256 MiB on stream A next to kinds_expand of workload 7 on B and sparse_unpack of workload 7 on C
    (32 KiB of LDS per workgroup each), kinds_store of workload 6 on D (248 vector registers), sparse_scan of workload 7 on E
    and move_bytes of workload 4 on F; the encoder enqueued first or last.  Every output equals its serial result (the encoder's
    slots: the serial launch's, which tests/test_gpu_concurrency.py pins against the reference encoder) and every status word is 0."""
    from test_gpu_concurrency import _slots_equal
    n = 256 * MiB + 5 * PACKET + 13
    npk = H.packet_count(n)
    d_in = H.generate("text", 640, n)
    word = _status(1)
    want_slots = H.encode(d_in, d_status=word, mode="throughput")
    ops = [W[7].by_name["kinds_expand"], W[7].by_name["sparse_unpack"], W[6].by_name["kinds_store"], W[7].by_name["sparse_scan"], W[4].by_name["move_bytes"]]
    serial_words = _status(len(ops))
    verdicts = _serial(ops, serial_words)
    _words(verdicts, torch.cat([word, serial_words]), [0] * (1 + len(ops)), ["encode (serial)"] + [f"{op.name} (serial)" for op in ops])
    for op in ops:
        op.fill()
    slots = torch.full((npk * SLOT,), 0xEE, dtype=torch.uint8, device="cuda")
    words = _status(1 + len(ops))
    streams = _streams(1 + len(ops))
    launches = [lambda op=op, s=s, j=j: op.run(s, words[j + 1:j + 2]) for j, (op, s) in enumerate(zip(ops, streams[1:]))]
    encoder = lambda: H.encode(d_in, slots, stream=streams[0], d_status=words[0:1], mode="throughput")
    launches = [encoder] + launches if order == "encoder_first" else launches + [encoder]
    torch.cuda.synchronize()
    for launch in launches:
        launch()
    torch.cuda.synchronize()
    verdicts.append((f"{order}: stream A: encode throughput, text {n} bytes ({npk} packets): slots differ from the serial slots", _slots_equal(slots, want_slots, npk)))
    for op in ops:
        verdicts += op.verdicts(f" ({order}, beside the encoder)", "the serial result")
    _words(verdicts, words, [0] * (1 + len(ops)), [f"{order}: encode"] + [f"{order}: {op.name}" for op in ops])
    _fail_on(verdicts)
    assert H.status() == 0, "sparse_scan reports into the fallback word and had nothing to report"


# ---------------------------------------------------------------------------------------------------------------------
# 5. the batch API from threads
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ("stream", "offsets", "crc32", "stored", "raw", "raw_offsets", "sparse", "sparse_offsets")


def _same_or_none(a, b):
    if a is None or b is None:
        return torch.tensor(a is None and b is None, device="cuda")
    return _same(a, b)


def _thread_runs(W):
    """Six batches: [(name, tensors (uint8 on the device), bases or None, keywords of compress, whether the files go through
    from_gip)].  Every batch has an empty tensor, a one-byte one, the bytes of two or three workloads and, in the based ones, a
    tensor that equals its base."""
    data = lambda i: W[i].x_img[:W[i].n].clone()
    small = [torch.empty(0, dtype=torch.uint8, device="cuda"), data(0)]
    same = data(2)
    return [
        ("sparse=auto", small + [data(1), data(4)], None, dict(sparse="auto"), False),
        ("sparse=auto, stored=auto", small + [data(2), data(5)], None, dict(sparse="auto", stored="auto"), True),
        ("sparse=auto, stored=auto, planes=2", small + [data(3), data(4), data(6)[:40 * PACKET + 6].clone()], None, dict(sparse="auto", stored="auto", planes=2), True),
        ("sparse=auto, base=[...] with a tensor equal to its base, checksum", small + [same, data(1)], [None, None, same.clone(), data(1).flip(0).contiguous()],
         dict(sparse="auto", checksum=True), True),
        ("sparse=auto, stored=auto, checksum", small + [data(5), data(1)], None, dict(sparse="auto", stored="auto", checksum=True), True),
        ("sparse=auto, stored=auto, planes=2, base=[...], checksum", small + [same.clone(), data(4)], [None, None, same.clone(), None],
         dict(sparse="auto", stored="auto", planes=2, checksum=True), True),
    ]


def _pin(H, c, name, tensors, bases, kw):
    """The serial Compressed against the host: each packet's kind is hip.sparse_rule of the host scan word and estimate of the
    bytes that are coded (the tensor XORed with its base, split into planes), and the sparse records are sparse_pack_host's."""
    import planes_ref as P
    import xor_ref as X
    w = kw.get("planes", 1)
    kinds, recs = [], []
    for b, t in enumerate(tensors):
        x = t.cpu().numpy()
        if bases is not None and bases[b] is not None:
            coded = X.numpy_split_xor(x, bases[b].cpu().numpy(), w)
        else:
            coded = P.numpy_split(x, w) if w > 1 else x
        raw = coded.tobytes()
        if not raw:
            continue
        for p, (scan, est) in enumerate(zip(H.sparse_scan_host(raw), H.estimate_host(raw))):
            part = raw[p * PACKET:(p + 1) * PACKET]
            kind = H.sparse_rule(scan, est, len(part), kw.get("stored") == "auto")
            kinds.append(kind)
            if kind == K.SPARSE:
                recs.append(H.sparse_pack_host(part))
    assert c.stored.cpu().tolist() == kinds, f"{name} (serial): the kinds differ from hip.sparse_rule on the host scan words and estimates"
    assert K.SPARSE in kinds, f"{name}: kinds {sorted(set(kinds))} only"
    assert c.sparse.cpu().numpy().tobytes() == b"".join(recs), f"{name} (serial): the records differ from sparse_pack_host's"
    assert c.sparse_offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64).tolist()


def test_thread_batch_sparse_auto_and_from_gip(H, W):
    """batch.compress(..., sparse="auto", stream=s), decompress, and -- where every buffer has a version-6 file -- Compressed.gip(b,
    kinds=True), from_gip and decompress again, from six threads at once, each with its own stream and keyword family: the
    three-way _partition and from_gip's region lists are torch operations between launches on a side stream, with temporaries
    made and freed while other threads do the same.  The serial pass is pinned by _pin and by exact round trips; the threads
    must reproduce every field of both Compressed objects."""
    from gpuar_amd import batch
    runs = [dict(name=name, tensors=tensors, bases=bases, kw=kw, gip=gip) for name, tensors, bases, kw, gip in _thread_runs(W)]
    torch.cuda.synchronize()

    def work(r, stream):
        kw = dict(r["kw"], base=r["bases"]) if r["bases"] is not None else r["kw"]
        c = batch.compress(r["tensors"], stream=stream, **kw)
        outs = batch.decompress(c, stream=stream, base=r["bases"])
        back = outs2 = None
        if r["gip"]:
            if stream is not None:
                stream.synchronize()                         # (gip reads the fields on the host)
            files = [c.gip(b, kinds=True) for b in range(c.n_buffers)]
            back = batch.from_gip(files, stream=stream)
            outs2 = batch.decompress(back, stream=stream, base=r["bases"])
        return c, outs, back, outs2

    for t, r in enumerate(runs):
        r["serial"] = work(r, None)
        torch.cuda.synchronize()
        c, outs, back, outs2 = r["serial"]
        tag = f"thread {t} (serial): {r['name']}"
        _pin(H, c, tag, r["tensors"], r["bases"], r["kw"])
        if r["bases"] is not None:
            assert c.based[2] and set(c.stored[c.first_packet[2]:c.first_packet[3]].cpu().tolist()) == {K.SPARSE}, f"{tag}: a tensor equal to its base is not all sparse"
        for b, v in enumerate(r["tensors"]):
            assert torch.equal(outs[b], v), f"{tag}: buffer {b} does not round-trip"
            assert outs2 is None or torch.equal(outs2[b], v), f"{tag}: buffer {b} does not round-trip through gip and from_gip"
        if back is not None:
            for field in ("stream", "offsets", "stored", "raw", "raw_offsets", "sparse", "sparse_offsets"):
                assert torch.equal(getattr(back, field), getattr(c, field)), f"{tag}: from_gip's {field} is not compress's"
    assert H.status() == 0

    k = len(runs)
    streams = _streams(k)
    start = threading.Barrier(k)
    torch.cuda.synchronize()

    def run(t):
        start.wait()
        return work(runs[t], streams[t])

    with ThreadPoolExecutor(k) as pool:
        results = [f.result() for f in [pool.submit(run, t) for t in range(k)]]
    torch.cuda.synchronize()
    verdicts = []
    for t, (got, r) in enumerate(zip(results, runs)):
        tag = f"thread {t}: {r['name']}"
        for which, c, want in (("compress", got[0], r["serial"][0]), ("from_gip", got[2], r["serial"][2])):
            if want is None:
                assert c is None
                continue
            assert (c.planes, c.delta, c.based, c.first_packet, c.sizes, c.kinds_rule) == \
                (want.planes, want.delta, want.based, want.first_packet, want.sizes, want.kinds_rule), f"{tag}: {which}'s host fields differ from the serial run's"
            for field in FIELDS:
                verdicts.append((f"{tag}: {which}'s {field} differs from the serial run's", _same_or_none(getattr(c, field), getattr(want, field))))
        for which, outs in (("decompress", got[1]), ("decompress of from_gip", got[3])):
            for b, v in enumerate(r["tensors"] if outs is not None else []):
                verdicts.append((f"{tag}: {which}: buffer {b} ({v.numel()} bytes) does not round-trip", _same(outs[b], v)))
    _fail_on(verdicts)
    assert H.status() == 0, "a launch of the module reported into the fallback word"
