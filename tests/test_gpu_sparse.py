"""Sparse packets on the MI355X: sparse_scan (one buffer and a batch), sparse_pack and sparse_unpack against the host definitions
on the packets of tests/sparse_ref.py, with canaries behind every record and every destination; inconsistent scan words and damaged
records; and batch.compress(sparse="auto") / decompress / estimate: the round trip, the kinds against the host rule applied to the
host-side split / XORed bytes, the coded packets against the same call without `sparse`, and the sizes the feature is built for."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import planes_ref as R
import sparse_ref as S
import xor_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
GUARD = 64


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def cases():
    return S.cases()


@pytest.fixture(scope="module")
def device_cases(H, cases):
    """every packet in an allocation of its own that ends with the 16-byte piece that holds its last byte (never modified)"""
    bufs = []
    for _name, x in cases:
        t = torch.full(((x.size + 15) // 16 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        t[:x.size] = torch.from_numpy(x).cuda()
        bufs.append(t)
    return bufs


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _i64(values):
    return torch.tensor([v if v < (1 << 63) else v - (1 << 64) for v in values], dtype=torch.int64, device="cuda")


def _i32(values):
    return torch.tensor([v if v < (1 << 31) else v - (1 << 32) for v in values], dtype=torch.int32, device="cuda")


def _u32(t):
    return [v & 0xFFFFFFFF for v in t.cpu().tolist()]


# ---- sparse_scan ------------------------------------------------------------------------------------------------------

def test_scan_of_single_buffers_equals_the_host_scan(H, cases, device_cases):
    for (name, x), t in zip(cases, device_cases):
        assert _u32(H.sparse_scan(t, n_bytes=x.size)) == [S.scan(x)] == H.sparse_scan_host(x.tobytes()), name
    parts = [x for _name, x in cases if x.size == PACKET][:6] + [cases[10][1]]      # several packets and a short last one
    data = np.concatenate(parts)
    t = torch.zeros((data.size + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    t[:data.size] = torch.from_numpy(data).cuda()
    assert _u32(H.sparse_scan(t, n_bytes=data.size)) == [S.scan(x) for x in parts]
    assert H.status() == 0


def test_scan_of_a_batch_equals_the_host_scan_and_skips_an_unusable_descriptor(H, cases, device_cases):
    n = len(cases)
    sizes = [x.size for _name, x in cases]
    first_packet, n_packets = H.batch_packet_count(sizes)
    assert n_packets == n
    ptrs = [t.data_ptr() for t in device_cases]
    status = _status()
    got = H.sparse_scan_batch(_i64(ptrs), _i64(sizes), _i64(first_packet), n, n_packets, d_status=status)
    assert int(status.item()) == 0
    want = [S.scan(x) for _name, x in cases]
    assert _u32(got) == want
    bad = len(cases) - 1                                       # a misaligned buffer: BAD_BATCH, its word is left alone
    ptrs[bad] += 8
    d_scan = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    H.sparse_scan_batch(_i64(ptrs), _i64(sizes), _i64(first_packet), n, n_packets, d_scan=d_scan, d_status=status)
    assert int(status.item()) == H.STATUS_BAD_BATCH
    got = _u32(d_scan)
    assert got[:bad] == want[:bad] and got[bad] == 0x5A5A5A5A


# ---- sparse_pack ------------------------------------------------------------------------------------------------------

def _pack(H, srcs, sizes, scans, rooms, src_shift=None, dst_shift=None):
    """one sparse_pack launch: region r gets rooms[r] bytes plus a guard in a buffer of 0x5A, at an offset that is 4 mod 16 (the
    weakest alignment a record may have); returns (status, the buffer on the host, the offsets)"""
    offs, at = [], 4
    for room in rooms:
        offs.append(at)
        at += (room + GUARD + 15) // 16 * 16
    dst = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    n = len(sizes)
    src_ptrs = [t.data_ptr() + (src_shift or {}).get(r, 0) for r, t in enumerate(srcs)]
    dst_ptrs = [dst.data_ptr() + o + (dst_shift or {}).get(r, 0) for r, o in enumerate(offs)]
    status = _status()
    H.sparse_pack(_i64(src_ptrs), _i64(sizes), _i32(scans), _i64(dst_ptrs), n, d_status=status)
    return int(status.item()), dst.cpu().numpy(), offs + [at]


def test_pack_writes_the_hosts_records_and_nothing_behind_them(H, cases, device_cases):
    keep = [i for i, (_name, x) in enumerate(cases) if S.scan(x) != S.NONE]
    recs = [S.pack(cases[i][1]) for i in keep]
    flags, got, offs = _pack(H, [device_cases[i] for i in keep], [cases[i][1].size for i in keep], [S.scan(cases[i][1]) for i in keep],
                             [len(r) for r in recs])
    assert flags == 0
    assert (got[:4] == 0x5A).all()
    for r, (i, rec) in enumerate(zip(keep, recs)):
        assert rec == H.sparse_pack_host(cases[i][1].tobytes())
        assert got[offs[r]:offs[r] + len(rec)].tobytes() == rec, cases[i][0]
        assert (got[offs[r] + len(rec):offs[r + 1]] == 0x5A).all(), (cases[i][0], "wrote behind the record")
    for i in keep:
        x = cases[i][1]
        assert (device_cases[i].cpu().numpy()[:x.size] == x).all()


def test_an_inconsistent_scan_is_bad_batch_and_writes_nothing(H):
    x = S.GOOD                                                 # 300 bytes of 7 with 4 exceptions
    t = torch.zeros(304, dtype=torch.uint8, device="cuda")
    t[:300] = torch.from_numpy(x).cuda()
    long = torch.full((2 * PACKET,), 7, dtype=torch.uint8, device="cuda")
    good, rec = S.scan(x), S.pack(x)
    assert good == (4 << 8) | 7
    other = int(x[5])                                          # a byte value that occurs once: 299 exceptions, no majority
    regions = [                                                # (source, bytes, scan, shifts): every one but the first and the last is refused
        (t, 300, good, 0, 0),
        (t, 300, (5 << 8) | 7, 0, 0),                          # one exception too many
        (t, 300, (3 << 8) | 7, 0, 0),                          # one too few
        (t, 300, (0 << 8) | 7, 0, 0),
        (t, 300, S.NONE, 0, 0),
        (t, 300, (4 << 8) | 8, 0, 0),                          # another fill: 300 exceptions
        (t, 300, (299 << 8) | other, 0, 0),                    # the count is right, the fill is no majority
        (t, 300, good, 8, 0),                                  # a misaligned source
        (t, 300, good, 0, 2),                                  # a misaligned record
        (long, PACKET + 1, 7, 0, 0),                           # more than a packet
        (t, 0, 7, 0, 0),                                       # no bytes
        (t, 300, good, 0, 0),
    ]
    n = len(regions)
    flags, got, offs = _pack(H, [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], [1024] * n,
                             src_shift={r: v[3] for r, v in enumerate(regions)}, dst_shift={r: v[4] for r, v in enumerate(regions)})
    assert flags == H.STATUS_BAD_BATCH
    for r in range(n):
        mine = got[offs[r]:offs[r + 1]]
        if r in (0, n - 1):
            assert mine[:len(rec)].tobytes() == rec and (mine[len(rec):] == 0x5A).all(), r
        else:
            assert (mine == 0x5A).all(), (r, "a refused region was written")


# ---- sparse_unpack ----------------------------------------------------------------------------------------------------

def _unpack(H, recs, rec_bytes, sizes, rec_shift=None, dst_shift=None):
    """one sparse_unpack launch: the records back to back in one buffer, each at an offset that is 4 mod 16, the destinations in a
    buffer of 0x5A with a guard behind each; returns (status, the destinations on the host, their offsets)"""
    rec_offs, at = [], 4
    for rec in recs:
        rec_offs.append(at)
        at += (len(rec) + 15) // 16 * 16
    held = np.full(at + 16, 0xC3, dtype=np.uint8)
    for o, rec in zip(rec_offs, recs):
        held[o:o + len(rec)] = np.frombuffer(rec, dtype=np.uint8)
    d_rec = torch.from_numpy(held).cuda()
    offs, at = [], 0
    for n in sizes:
        offs.append(at)
        at += (n + GUARD + 15) // 16 * 16
    dst = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    rec_ptrs = [d_rec.data_ptr() + o + (rec_shift or {}).get(r, 0) for r, o in enumerate(rec_offs)]
    dst_ptrs = [dst.data_ptr() + o + (dst_shift or {}).get(r, 0) for r, o in enumerate(offs)]
    status = _status()
    H.sparse_unpack(_i64(rec_ptrs), _i64(rec_bytes), _i64(dst_ptrs), _i64(sizes), len(sizes), d_status=status)
    return int(status.item()), dst.cpu().numpy(), offs + [at]


def test_unpack_is_byte_exact_and_nothing_behind_a_packet_is_written(H, cases):
    keep = [(name, x) for name, x in cases if S.scan(x) != S.NONE]
    recs = [S.pack(x) for _name, x in keep]
    flags, got, offs = _unpack(H, recs, [len(r) for r in recs], [x.size for _name, x in keep])
    assert flags == 0
    for r, (name, x) in enumerate(keep):
        assert (got[offs[r]:offs[r] + x.size] == x).all(), name
        assert (got[offs[r] + x.size:offs[r + 1]] == 0x5A).all(), (name, "wrote behind the packet")
    # a record with room behind it (rec_bytes larger than the record) is the same record
    flags, again, _offs = _unpack(H, recs[:8], [len(r) + 12 for r in recs[:8]], [x.size for _name, x in keep[:8]])
    assert flags == 0 and (again == got[:again.size]).all()


@pytest.mark.parametrize("name,rec,rec_bytes,n", S.damaged(), ids=[d[0] for d in S.damaged()])
def test_a_damaged_record_is_bad_packet_and_its_neighbours_are_untouched(H, name, rec, rec_bytes, n):
    held = np.frombuffer(rec, dtype=np.uint8).copy()           # first: the host definition refuses it
    out = np.zeros(n, dtype=np.uint8)
    assert H.load().gpuar_hip_sparse_unpack_host(C.c_void_p(held.ctypes.data), rec_bytes, C.c_void_p(out.ctypes.data), n) == -2
    good = S.pack(S.GOOD)
    flags, got, offs = _unpack(H, [good, rec, good], [len(good), rec_bytes, len(good)], [S.GOOD_N, n, S.GOOD_N])
    assert flags == H.STATUS_BAD_PACKET                        # and no other bit
    for r in (0, 2):
        assert (got[offs[r]:offs[r] + S.GOOD_N] == S.GOOD).all(), r
        assert (got[offs[r] + S.GOOD_N:offs[r + 1]] == 0x5A).all(), r
    assert (got[offs[1] + n:offs[2]] == 0x5A).all(), "wrote outside the damaged record's packet"


def test_unusable_unpack_regions_are_bad_batch_and_are_skipped(H):
    good = S.pack(S.GOOD)
    long = S.pack(np.zeros(PACKET, dtype=np.uint8))
    flags, got, offs = _unpack(H, [good, good, good, long, good, good], [16, 16, 16, 4, 16, 16], [S.GOOD_N, S.GOOD_N, S.GOOD_N, PACKET + 1, 0, S.GOOD_N],
                               rec_shift={1: 2}, dst_shift={2: 8})
    assert flags == H.STATUS_BAD_BATCH
    for r in (0, 5):
        assert (got[offs[r]:offs[r] + S.GOOD_N] == S.GOOD).all() and (got[offs[r] + S.GOOD_N:offs[r + 1]] == 0x5A).all(), r
    assert (got[offs[1]:offs[5]] == 0x5A).all(), "a refused region was written"


def test_host_side_checks(H):
    lib = H.load()
    desc = torch.zeros(8, dtype=torch.int64, device="cuda")
    q = desc.data_ptr()
    for fn in (lib.gpuar_hip_sparse_pack, lib.gpuar_hip_sparse_unpack):
        assert fn(None, None, None, None, 0, None, None) == 0
        for missing in range(4):
            args = [q, q, q, q]
            args[missing] = None
            assert fn(*args, 1, None, None) == -2, missing
        for off in range(4):
            args = [q, q, q, q]
            args[off] = q + (2 if fn is lib.gpuar_hip_sparse_pack and off == 2 else 4)
            assert fn(*args, 1, None, None) == -1, off
        assert fn(q, q, q, q, 1, q + 2, None) == -1
    assert lib.gpuar_hip_sparse_scan(None, 0, None, None) == 0 and lib.gpuar_hip_sparse_scan(None, 100, q, None) == -2
    assert lib.gpuar_hip_sparse_scan(q, 100, None, None) == -2 and lib.gpuar_hip_sparse_scan(q + 8, 100, q, None) == -1
    assert lib.gpuar_hip_sparse_scan_batch(q, q, q, 1, 0, q, None, None) == 0 and lib.gpuar_hip_sparse_scan_batch(q, q, q, 1, 1, None, None, None) == -2
    assert lib.gpuar_hip_sparse_scan_batch(q, q, q, 1, 1, q + 2, None, None) == -1


# ---- batch.compress(sparse="auto") ------------------------------------------------------------------------------------

def raw(t):
    """the tensor's bytes on the host"""
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1) if t.numel() else np.empty(0, dtype=np.uint8)


def _bf16_pair(elements, replaced, seed):
    """(tensor, base): bf16 weights, the tensor being the base with `replaced` of its elements drawn afresh"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(elements, generator=g) * 0.02).to(torch.bfloat16)
    t = base.clone()
    if replaced:
        where = torch.randperm(elements, generator=g)[:replaced]
        t[where] = (torch.randn(replaced, generator=g) * 0.02).to(torch.bfloat16)
    return t.cuda(), base.cuda()


COMBOS = [(stored, side) for stored in (None, "auto") for side in (False, True)]


@pytest.fixture(scope="module")
def mixed(H):
    """zeros, a bf16 tensor equal to its base, one with 0.1 % of its elements replaced, uniform bytes, text, an empty tensor and
    tensors of 1, 2 and 3 bytes -- with what batch.compress makes of them with and without sparse="auto", for stored None and
    "auto", on the default and on a side stream (shared by the tests below, never modified)."""
    from gpuar_amd import batch, synth
    g = torch.Generator().manual_seed(3)
    same, same_base = _bf16_pair((2 * PACKET + 100) // 2, 0, 5)
    near, near_base = _bf16_pair(16 * PACKET, 16 * PACKET // 1000, 6)          # 32 packets
    ts = [
        torch.zeros(2 * PACKET + 100, dtype=torch.uint8, device="cuda"),
        same,
        near,
        torch.randint(0, 256, (3 * PACKET,), generator=g, dtype=torch.uint8).cuda(),
        torch.from_numpy(synth.text(4, 20000)).cuda(),
        torch.empty(0, dtype=torch.float32, device="cuda"),
        torch.full((1,), 9, dtype=torch.uint8, device="cuda"),
        torch.full((2,), 9, dtype=torch.uint8, device="cuda"),
        torch.full((3,), 9, dtype=torch.uint8, device="cuda"),
    ]
    bases = [None, same_base, near_base] + [None] * 6
    torch.cuda.synchronize()
    made = {}
    for stored, side in COMBOS:
        stream = torch.cuda.Stream() if side else None
        plain = batch.compress(ts, planes="auto", base=bases, checksum=True, stored=stored, stream=stream)
        sparse = batch.compress(ts, planes="auto", base=bases, checksum=True, stored=stored, stream=stream, sparse="auto")
        back = batch.decompress(sparse, base=bases, stream=stream)
        if stream is not None:
            stream.synchronize()
        made[stored, side] = (plain, sparse, back)
    return ts, bases, made


def host_kinds(H, ts, bases, widths, stored_on):
    """per batch packet (kind, size): the host rule on the host-side split / XORed bytes; the size of a coded packet is its estimate"""
    out = []
    for t, b, w in zip(ts, bases, widths):
        split = X.numpy_split_xor(raw(t), raw(b), w) if b is not None else R.numpy_split(raw(t), w)
        est, scan = H.estimate_host(split.tobytes()), H.sparse_scan_host(split.tobytes())
        for p, (e, s) in enumerate(zip(est, scan)):
            ulen = min(PACKET, split.size - p * PACKET)
            assert s == S.scan(split[p * PACKET:p * PACKET + ulen])
            kind = H.sparse_rule(s, e, ulen, stored_on)
            assert kind == S.rule(s, e, ulen, stored_on)
            out.append((kind, S.sparse_len(s >> 8) if kind == S.SPARSE else ulen if kind == S.RAW else e))
    return out


@pytest.mark.parametrize("stored,side", COMBOS)
def test_round_trip_and_kinds_are_the_host_rules(H, mixed, stored, side):
    ts, bases, made = mixed
    plain, c, back = made[stored, side]
    assert c.planes == [1, 2, 2, 1, 1, 4, 1, 1, 1] and c.sizes == plain.sizes and c.first_packet == plain.first_packet
    for b, (o, t) in enumerate(zip(back, ts)):
        assert o.dtype == torch.uint8 and (o.cpu().numpy() == raw(t)).all(), b
    want = host_kinds(H, ts, bases, c.planes, stored == "auto")
    kinds = c.stored.cpu().tolist()
    assert c.stored.dtype == torch.uint8 and kinds == [k for k, _size in want]
    assert kinds.count(S.SPARSE) > 0 and kinds.count(S.CODED) > 0 and (kinds.count(S.RAW) > 0) == (stored == "auto")
    n_coded, n_raw, n_sparse = (kinds.count(k) for k in (S.CODED, S.RAW, S.SPARSE))
    assert c.offsets.numel() == n_coded + 1 and c.raw_offsets.numel() == n_raw + 1 and c.sparse_offsets.numel() == n_sparse + 1
    assert int(c.sparse_offsets[-1].item()) == c.sparse.numel() == sum(size for k, size in want if k == S.SPARSE)
    assert c.nbytes == c.stream.numel() + c.raw.numel() + c.sparse.numel() < plain.nbytes
    assert torch.equal(c.crc32, plain.crc32)                                   # the CRCs of the original bytes, all packets
    # the records are the host's, in batch order
    recs, offs = c.sparse.cpu().numpy(), c.sparse_offsets.cpu().tolist()
    rank, p = 0, 0
    for t, b, w in zip(ts, bases, c.planes):
        split = X.numpy_split_xor(raw(t), raw(b), w) if b is not None else R.numpy_split(raw(t), w)
        for j in range((split.size + PACKET - 1) // PACKET):
            if kinds[p] == S.SPARSE:
                assert recs[offs[rank]:offs[rank + 1]].tobytes() == S.pack(split[j * PACKET:(j + 1) * PACKET]), p
                rank += 1
            p += 1
    assert rank == n_sparse


@pytest.mark.parametrize("stored,side", COMBOS)
def test_the_coded_packets_are_the_packets_of_the_call_without_sparse(H, mixed, stored, side):
    _ts, _bases, made = mixed
    plain, c, _back = made[stored, side]
    kinds = c.stored.cpu().tolist()
    plain_kinds = plain.stored.cpu().tolist() if plain.stored is not None else [0] * len(kinds)
    off_c, off_p = c.offsets.cpu().tolist(), plain.offsets.cpu().tolist()
    stream_c, stream_p = c.stream.cpu().numpy(), plain.stream.cpu().numpy()
    rank_c = rank_p = 0
    for p, (kind, plain_kind) in enumerate(zip(kinds, plain_kinds)):
        if kind == S.CODED:
            assert plain_kind == 0, p
            assert stream_c[off_c[rank_c]:off_c[rank_c + 1]].tobytes() == stream_p[off_p[rank_p]:off_p[rank_p + 1]].tobytes(), p
            rank_c += 1
        if kind == S.RAW:
            assert plain_kind == 1, p                                          # what was raw without `sparse` is raw or sparse with it
        rank_p += plain_kind == 0
    assert rank_c == len(off_c) - 1 and rank_p == len(off_p) - 1


def test_sparse_none_is_the_call_without_the_keyword(H, mixed):
    from gpuar_amd import batch
    ts, bases, made = mixed
    for stored in (None, "auto"):
        plain = made[stored, False][0]
        assert plain.sparse is None and plain.sparse_offsets is None
        c = batch.compress(ts, planes="auto", base=bases, checksum=True, stored=stored, sparse=None)
        assert torch.equal(c.stream, plain.stream) and torch.equal(c.offsets, plain.offsets)
        assert c.sparse is None and c.sparse_offsets is None
        assert (c.stored is None) == (stored is None) and (stored is None or (torch.equal(c.stored, plain.stored) and torch.equal(c.raw, plain.raw)))
    with pytest.raises(H.GpuarError, match="sparse"):
        batch.compress(ts, sparse="always")
    with pytest.raises(H.GpuarError, match="sparse"):
        batch.compress(ts[:1], sparse="auto", stored=[True] * 3)


@pytest.mark.parametrize("stored", [None, "auto"])
def test_the_sizes_the_feature_is_built_for(H, mixed, stored):
    from gpuar_amd import batch
    ts, bases, _made = mixed
    same = batch.compress([ts[1]], planes="auto", base=[bases[1]], checksum=True, stored=stored, sparse="auto")
    assert same.n_packets == 3 and same.nbytes == 4 * same.n_packets and same.stream.numel() == 0
    assert same.stored.cpu().tolist() == [S.SPARSE] * 3
    assert (batch.decompress(same, base=[bases[1]])[0].cpu().numpy() == raw(ts[1])).all()
    near = batch.compress([ts[2]], planes=2, base=[bases[2]], checksum=True, stored=stored, sparse="auto")
    plain = batch.compress([ts[2]], planes=2, base=[bases[2]], checksum=True, stored=stored)
    want = host_kinds(H, [ts[2]], [bases[2]], [2], stored == "auto")
    assert [k for k, _size in want] == [S.SPARSE] * 32 == near.stored.cpu().tolist()
    total = sum(size for _k, size in want)
    print(f"0.1 % replaced, stored={stored}: {near.nbytes} bytes sparse, {plain.nbytes} without")
    assert near.nbytes == total < plain.nbytes
    assert batch.estimate([ts[2]], planes=2, base=[bases[2]], stored=stored, sparse="auto") == [total]
    assert (batch.decompress(near, base=[bases[2]])[0].cpu().numpy() == raw(ts[2])).all()


@pytest.mark.parametrize("stored", [None, "auto"])
def test_estimate_counts_a_sparse_packet_as_its_record(H, mixed, stored):
    from gpuar_amd import batch
    ts, bases, made = mixed
    c = made[stored, False][1]
    want = host_kinds(H, ts, bases, c.planes, stored == "auto")
    per_tensor = [sum(size for _k, size in want[c.first_packet[b]:c.first_packet[b + 1]]) for b in range(len(ts))]
    assert batch.estimate(ts, planes="auto", base=bases, stored=stored, sparse="auto") == per_tensor
    assert batch.estimate(ts, planes="auto", base=bases, stored=stored, sparse=None) == batch.estimate(ts, planes="auto", base=bases, stored=stored)


def test_gip_and_payload_refuse_a_buffer_with_a_sparse_packet(H, mixed):
    _ts, _bases, made = mixed
    plain, c, _back = made[None, False]
    kinds = c.stored.cpu().tolist()
    seen = set()
    for b in range(c.n_buffers):
        mine = kinds[c.first_packet[b]:c.first_packet[b + 1]]
        if any(mine):
            assert S.SPARSE in mine
            with pytest.raises(H.GpuarError, match="sparse"):
                c.gip(b)
            with pytest.raises(H.GpuarError, match="sparse"):
                c.payload(b)
        elif not plain.based[b]:
            assert c.gip(b) == plain.gip(b), b
        seen.add(any(mine))
    assert seen == {True, False}


def test_a_corrupted_record_raises_from_decompress(H, mixed):
    from gpuar_amd import batch
    _ts, bases, made = mixed
    c = made["auto", False][1]
    offs = c.sparse_offsets.cpu().tolist()
    longest = max(range(len(offs) - 1), key=lambda r: offs[r + 1] - offs[r])
    assert offs[longest + 1] - offs[longest] >= 8                               # a record with an exception
    for at, flip in ((offs[longest], 0x01),                                     # the fill: the packet comes back wrong (CHECKSUM)
                     (offs[longest] + 1, 0x01),                                 # the reserved byte: BAD_PACKET
                     (offs[longest] + 4, 0x40)):                                # a position
        damaged = c.sparse.clone()
        damaged[at] ^= flip
        with pytest.raises(H.GpuarError):
            batch.decompress(dataclasses.replace(c, sparse=damaged), base=bases)
    assert len(batch.decompress(c, base=bases)) == c.n_buffers                  # the undamaged batch still decodes
