"""The second and later passes of the grid-stride loops, on the MI355X: the sixteen kernels whose grid is capped by kPlaneGridCap
(the full-group and tail kernels of the three filters, move_packets, move_bytes, sparse_pack, sparse_unpack) run here through
tests/_build/libgpuar_hip_gridcap3.so, the shipped kernels -- test_grid_cap_host.py holds the two code objects equal byte for
byte -- behind launch code that gives them 3 workgroups at most (tests/grid_cap_build.py).  So every workgroup strides on, dozens
of times, over inputs of kilobytes: LDS is reused from group to group and from buffer to buffer, the delta's `turn` alternates,
the `continue`s of unusable descriptors are taken between passes that do work, and wavefronts of one workgroup leave their loop
on different passes.  With the shipped cap of 2^22 none of that happens below 32 GiB.

Every case is compared with the project's numpy / host reference AND with the shipped library's output for the same call (the
bytes must not depend on the grid); the batch, move and sparse launches run twice on the same inputs.  Inputs are seeded uniform
bytes, different in every group and base, so that a stale LDS slot gives wrong bytes.  Behind every output stand guard bytes,
and every status word is read.  The shapes are those of grid_cap_build.py; test_grid_cap_host.py asserts, from the pass arithmetic
alone, where their passes, ragged ends and defective items fall.  Each test keeps under 64 MiB of device memory."""
import dataclasses

import numpy as np
import pytest

import delta_ref as D
import grid_cap_build as G
import planes_ref as R
import sparse_ref as S
import xor_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT, GUARD = G.PACKET, G.SLOT, G.GUARD
IN_FILL, OUT_FILL = 0xA5, 0x5A
BAD_BATCH, BAD_PACKET = 0x4, 0x2


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    G.load()
    assert hip.STATUS_BAD_BATCH == BAD_BATCH and hip.STATUS_BAD_PACKET == BAD_PACKET
    return hip


@pytest.fixture(autouse=True)
def under_64_mib(H):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    yield
    assert torch.cuda.max_memory_allocated() - before < 64 << 20


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _i64(values):
    return torch.tensor(np.asarray(values, dtype=np.int64), dtype=torch.int64, device="cuda")


def _i32(values):
    return torch.tensor([v if v < (1 << 31) else v - (1 << 32) for v in values], dtype=torch.int32, device="cuda")


def shipped_and_capped(H, run):
    """[run() through the shipped library, through the capped one, through the capped one again]"""
    out = [run()]
    for _again in range(2):
        with G.capped() as capped:
            assert capped is H and H.load() is G.load()
            out.append(run())
    assert H.load() is not G.load()
    return out


def test_the_swap_puts_the_shipped_library_back_when_the_body_raises(H):
    shipped = H.load()
    with pytest.raises(ZeroDivisionError):
        with G.capped():
            assert H.load() is G.load() is not shipped
            1 / 0
    assert H.load() is shipped
    assert G.load().gpuar_hip_version() == shipped.gpuar_hip_version()


# ---- (a) one buffer, each filter ----------------------------------------------------------------------------------------

def _reference(name, x, w, base=None, filtered=True):
    if not filtered or name == "planes":
        return R.numpy_split(x, w)
    return D.numpy_split_delta(x, w) if name == "delta" else X.numpy_split_xor(x, base, w)


def _guarded(host, fill):
    t = torch.full((host.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    t[:host.size] = torch.from_numpy(host).cuda()
    return t


@pytest.mark.parametrize("w", G.WIDTHS)
@pytest.mark.parametrize("name", G.FILTERS)
def test_single_buffer_split_and_merge_over_many_passes(H, name, w):
    """n = k w 8192 + r, k = 2, 3, 4, 7, 11 groups over 3 workgroups: split and merge, out of place and in place, against numpy
    and against the shipped library; merge(split(x)) = x; the guards stay; the status word stays 0"""
    for i, n in enumerate(G.single_sizes(w)):
        x, base = G.seeded(n, 1000 * w + i), G.seeded(n, 5000 * w + i)
        want = _reference(name, x, w, base)
        assert np.array_equal(R.numpy_merge(want, w) if name == "planes" else D.numpy_merge_delta(want, w) if name == "delta"
                              else X.numpy_merge_xor(want, base, w), x)
        d_in, d_base = _guarded(x, IN_FILL), _guarded(base, IN_FILL)
        extra = (d_base,) if name == "xor" else ()
        split, merge = getattr(H, f"split_{name}"), getattr(H, f"merge_{name}")

        def run():
            d_out = torch.full((n + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
            split(d_in, *extra, w, d_out=d_out, n_bytes=n)
            d_back = torch.full((n + GUARD,), 0x3C, dtype=torch.uint8, device="cuda")
            merge(d_out, *extra, w, d_out=d_back, n_bytes=n)
            d_place = d_out.clone()
            merge(d_place, *extra, w, d_out=d_place, n_bytes=n)                # in place
            d_again = d_place.clone()
            split(d_again, *extra, w, d_out=d_again, n_bytes=n)
            return H.status(), d_out.cpu().numpy(), d_back.cpu().numpy(), d_place.cpu().numpy(), d_again.cpu().numpy()

        ran = shipped_and_capped(H, run)
        for which, (flags, out, back, place, again) in enumerate(ran):
            where = (name, w, n, ("shipped", "capped", "capped again")[which])
            assert flags == 0, where
            assert np.array_equal(out[:n], want), (*where, int(np.flatnonzero(out[:n] != want)[0]))
            assert np.array_equal(back[:n], x), (*where, "merge", int(np.flatnonzero(back[:n] != x)[0]))
            assert np.array_equal(place[:n], x), (*where, "merge in place")
            assert np.array_equal(again[:n], want), (*where, "split in place")
            assert (out[n:] == OUT_FILL).all() and (back[n:] == 0x3C).all() and (place[n:] == OUT_FILL).all() and (again[n:] == OUT_FILL).all(), where
        assert np.array_equal(d_in.cpu().numpy()[:n], x) and (d_in[n:] == IN_FILL).all() and np.array_equal(d_base.cpu().numpy()[:n], base)


# ---- (b), (c) batches, each filter ----------------------------------------------------------------------------------------

class Batch:
    """The batch of grid_cap_build.py on the device: hosts and bases of seeded bytes in arenas with guards between the buffers,
    and one descriptor tensor; `n`: how many of the 48 buffers, `defect`: what is wrong with buffer BAD_BUFFER"""

    def __init__(self, H, name, n=G.N_BUFFERS, defect=None):
        self.name, self.n, self.defect = name, n, defect
        self.sizes, self.widths = G.BATCH_SIZES[:n], list(G.BATCH_WIDTHS[:n])
        self.filtered = [bool(f) for f in (G.BATCH_DELTA if name == "delta" else G.BATCH_BASED if name == "xor" else [0] * n)[:n]]
        self.hosts = [G.seeded(size, 3 * b + 1) for b, size in enumerate(self.sizes)]
        self.bases = [G.seeded(size, 3 * b + 2) for b, size in enumerate(self.sizes)]
        self.want = [_reference(name, h, w, q, f) for h, w, q, f in zip(self.hosts, self.widths, self.bases, self.filtered)]
        self.offs, self.total = G.layout(self.sizes)
        self.src, self.base, self.split = self.arena(self.hosts, IN_FILL), self.arena(self.bases, IN_FILL), self.arena(self.want, IN_FILL)
        self.fp, self.npk = H.batch_packet_count(self.sizes)
        assert self.fp == G.first_packets(self.sizes)
        extra = [int(f) for f in self.filtered] if name == "delta" else [self.base.data_ptr() + o if f else 0 for o, f in zip(self.offs, self.filtered)]
        self.out_shift = [0] * n
        if defect == "width_3":
            self.widths[G.BAD_BUFFER] = 3
        elif defect == "misaligned_output":
            self.out_shift[G.BAD_BUFFER] = 8
        elif defect == "filter_2":
            extra[G.BAD_BUFFER] = 2
        elif defect == "misaligned_base":
            extra[G.BAD_BUFFER] += 8
        else:
            assert defect is None
        self.d_bytes, self.d_fp, self.d_w, self.d_extra, self.d_zero = _i64(self.sizes), _i64(self.fp), _i64(self.widths), _i64(extra), _i64([0] * n)

    def arena(self, parts, fill):
        host = np.full(self.total, fill, dtype=np.uint8)
        for o, p in zip(self.offs, parts):
            host[o:o + p.size] = p
        return torch.from_numpy(host).cuda()

    def ptrs(self, arena, shifted=False):
        return _i64([arena.data_ptr() + o + (s if shifted else 0) for o, s in zip(self.offs, self.out_shift)])

    def call(self, H, merge, d_in, d_out, extra=None, name=None):
        """one launch pair (full groups, tails) with a status word of its own; returns the word"""
        name = name or self.name
        fn = getattr(H, f"{'merge' if merge else 'split'}_{name}_batch")
        more = () if name == "planes" else (self.d_extra if extra is None else extra,)
        status = _status()
        fn(d_in, self.d_bytes, self.d_fp, self.d_w, *more, self.n, self.npk, d_out, d_status=status)
        return int(status.item())

    def check(self, got, want, where, skip=()):
        """`got` (an arena on the host) holds want[b] at every buffer not in `skip`, and the fill everywhere else"""
        for b, (o, p) in enumerate(zip(self.offs, want)):
            end = self.offs[b + 1] if b + 1 < self.n else self.total
            if b in skip:
                assert (got[o:end] == OUT_FILL).all(), (*where, b, "the refused buffer was written")
                continue
            assert np.array_equal(got[o:o + p.size], p), (*where, b, p.size, self.widths[b], self.filtered[b], int(np.flatnonzero(got[o:o + p.size] != p)[0]))
            assert (got[o + p.size:end] == OUT_FILL).all(), (*where, b, "wrote behind the buffer")


@pytest.mark.parametrize("name", G.FILTERS)
def test_batch_split_and_merge_over_many_passes(H, name):
    """48 buffers, 544 packets, 3 workgroups: each makes 181 passes or more, does 45 groups or more and 16 tails, through the same LDS; filtered and planes-alone
    buffers mixed.  Against numpy per buffer, against the shipped library, twice; merge in place restores the input; with the
    optional part off everywhere the output is split_planes_batch's."""
    t = Batch(H, name)
    d_src = t.ptrs(t.src)

    def run():
        dst = torch.full((t.total,), OUT_FILL, dtype=torch.uint8, device="cuda")
        d_dst = t.ptrs(dst)
        flags = [t.call(H, False, d_src, d_dst)]
        split = dst.cpu().numpy()
        flags.append(t.call(H, True, d_dst, d_dst))                            # merge in place
        return flags, split, dst.cpu().numpy()

    for which, (flags, split, merged) in enumerate(shipped_and_capped(H, run)):
        where = (name, ("shipped", "capped", "capped again")[which])
        assert flags == [0, 0], where
        t.check(split, t.want, (*where, "split"))
        t.check(merged, t.hosts, (*where, "merge in place"))
    assert np.array_equal(t.src.cpu().numpy(), t.arena(t.hosts, IN_FILL).cpu().numpy()), "the split changed its input"
    if name != "planes":                                                       # no filter / no base anywhere: the planes call's output
        with G.capped():
            off, plain = (torch.full((t.total,), OUT_FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
            assert t.call(H, False, d_src, t.ptrs(off), extra=t.d_zero) == 0
            assert t.call(H, False, d_src, t.ptrs(plain), name="planes") == 0
            assert torch.equal(off, plain)
            t.check(off.cpu().numpy(), [R.numpy_split(h, w) for h, w in zip(t.hosts, t.widths)], (name, "optional part off"))


@pytest.mark.parametrize("name,defect", [(name, defect) for name in G.FILTERS for defect in G.DEFECTS[name]])
def test_an_unusable_descriptor_on_a_later_pass_is_flagged_and_skipped(H, name, defect):
    """47 buffers (the tail kernels' last pass is ragged), buffer 25 unusable: every workgroup meets its packets after passes that
    did work and does work after them; BAD_BATCH in the launch's own word, the buffer's output still all guard bytes, every other
    buffer right -- split and merge."""
    t = Batch(H, name, n=G.N_BUFFERS - 1, defect=defect)

    def run():
        out = []
        for merge, src in ((False, t.src), (True, t.split)):
            dst = torch.full((t.total,), OUT_FILL, dtype=torch.uint8, device="cuda")
            flags = t.call(H, merge, t.ptrs(src), t.ptrs(dst, shifted=True))
            out.append((flags, dst.cpu().numpy()))
        return out

    for which, ran in enumerate(shipped_and_capped(H, run)):
        for (flags, got), want, way in zip(ran, (t.want, t.hosts), ("split", "merge")):
            where = (name, defect, way, ("shipped", "capped", "capped again")[which])
            assert flags == BAD_BATCH, where
            t.check(got, want, where, skip=(G.BAD_BUFFER,))


# ---- (d) move_packets and move_bytes --------------------------------------------------------------------------------------

def _move_packets(H, parts, lengths, src_rooms):
    """one move_packets launch: region r is lengths[r] bytes of parts[r]; the destinations stand back to back at the 16-byte grain
    the kernel asks for, so the gap behind a region is the 0 .. 15 guard bytes up to the next"""
    src_offs, total = G.layout(src_rooms, guard=0)
    src = np.full(total + 16, IN_FILL, dtype=np.uint8)
    for o, p in zip(src_offs, parts):
        src[o:o + p.size] = p
    d_src = torch.from_numpy(src).cuda()
    dst_offs, room = G.layout(lengths, guard=0)
    dst = torch.full((64 + room + 64,), OUT_FILL, dtype=torch.uint8, device="cuda")
    status = _status()
    H.move_packets(_i64([d_src.data_ptr() + o for o in src_offs]), _i64([dst.data_ptr() + 64 + o for o in dst_offs]), _i64(lengths), len(lengths),
                   d_status=status)
    return int(status.item()), dst.cpu().numpy(), [64 + o for o in dst_offs]


@pytest.mark.parametrize("n_regions", G.MOVE_REGIONS)
def test_move_packets_over_many_passes(H, n_regions):
    from test_gpu_ragged_quads import LENGTHS
    assert G.RAGGED_LENGTHS == LENGTHS
    lengths = G.MOVE_PACKETS_LENGTHS[:n_regions]
    parts = [G.seeded(n, 70 + r) for r, n in enumerate(lengths)]
    want = np.full(64 + G.layout(lengths, guard=0)[1] + 64, OUT_FILL, dtype=np.uint8)
    ran = shipped_and_capped(H, lambda: _move_packets(H, parts, lengths, lengths))
    for r, (o, p) in enumerate(zip(ran[0][2], parts)):
        want[o:o + p.size] = p
    for flags, got, _offs in ran:
        assert flags == 0
        assert np.array_equal(got, want), (n_regions, int(np.flatnonzero(got != want)[0]))


def test_move_packets_skips_a_region_of_8193_bytes_on_a_later_pass(H):
    lengths = list(G.MOVE_PACKETS_LENGTHS)
    bad = G.MOVE_BAD_REGION
    lengths[bad] = PACKET + 1
    parts = [G.seeded(n, 170 + r) for r, n in enumerate(lengths)]
    ran = shipped_and_capped(H, lambda: _move_packets(H, parts, lengths, lengths))
    want = np.full(ran[0][1].size, OUT_FILL, dtype=np.uint8)
    for r, (o, p) in enumerate(zip(ran[0][2], parts)):
        if r != bad:
            want[o:o + p.size] = p
    for flags, got, _offs in ran:
        assert flags == BAD_BATCH
        assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])


@pytest.fixture(scope="module")
def pool(H):
    """the pool of tests/test_gpu_gip_read.py: 64 KiB + a slot of seeded bytes that every source region is taken from"""
    data = np.random.default_rng(14).integers(0, 256, 65536 + SLOT + 16, dtype=np.uint8)
    d = torch.from_numpy(data).cuda()
    assert d.data_ptr() % 16 == 0
    return data, d


def _move_bytes_round(H, pool, first, n_regions, defect=None):
    """regions first .. first + n_regions of move_bytes_regions(), back to back; returns (status, got, want)"""
    from test_gpu_gip_read import _expected, _move
    src, dst, lengths = (v[first:first + n_regions] for v in G.move_bytes_regions())
    shift = dst[0] - (dst[0] % 16) - 64                     # the first destination keeps its residue, 64 .. 79 guard bytes in front
    dst = [d - shift for d in dst]
    nulls, skip = (), ()
    if defect is not None:
        r, what = defect
        skip = (r,)
        if what == "long":
            lengths = list(lengths)
            lengths[r] = SLOT + 1                           # (its neighbours stay where they are: the region is skipped as a whole)
        else:
            nulls = ((r, what),)
    out_bytes = dst[-1] + lengths[-1] + 64 + SLOT
    got, status = _move(H, pool, src, dst, lengths, out_bytes, nulls=nulls)
    return status, got, _expected(pool, src, dst, lengths, out_bytes, skip=skip)


@pytest.mark.parametrize("n_regions", G.MOVE_REGIONS)
def test_move_bytes_over_many_passes(H, pool, n_regions):
    """destinations back to back at byte grain; the three launches of 100 regions hold every (src & 15, dst & 15) pair"""
    for first in range(0, 100 * G.MOVE_BYTES_ROUNDS if n_regions == 100 else 1, 100):
        for status, got, want in shipped_and_capped(H, lambda: _move_bytes_round(H, pool, first, n_regions)):
            assert status == 0
            assert np.array_equal(got, want), (n_regions, first, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("what", ["src", "dst", "long"])
def test_move_bytes_skips_a_defective_region_on_a_later_pass(H, pool, what):
    """a null source, a null destination, 8705 bytes: flagged, skipped, the neighbours -- which touch it -- exact"""
    for status, got, want in shipped_and_capped(H, lambda: _move_bytes_round(H, pool, 100, 100, defect=(G.MOVE_BAD_REGION, what))):
        assert status == BAD_BATCH
        assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]))


# ---- (e) sparse_pack and sparse_unpack ------------------------------------------------------------------------------------

def _device_packets(packets):
    from test_gpu_ragged_quads import _device
    return [_device(x) for _name, x in packets]


@pytest.mark.parametrize("n_regions", G.SPARSE_REGIONS)
def test_sparse_pack_and_unpack_over_many_passes(H, n_regions):
    """12 wavefronts over 11 .. 113 regions: the host's records and nothing behind them, the packets byte-exact"""
    from test_gpu_sparse import _pack, _unpack
    packets = G.sparse_packets(n_regions)
    recs = [H.sparse_pack_host(x.tobytes()) for _name, x in packets]
    assert all(rec == S.pack(x) for rec, (_name, x) in zip(recs, packets))
    srcs, sizes = _device_packets(packets), [x.size for _name, x in packets]
    scans = [S.scan(x) for _name, x in packets]
    for flags, got, offs in shipped_and_capped(H, lambda: _pack(H, srcs, sizes, scans, [len(r) for r in recs])):
        assert flags == 0
        assert (got[:4] == OUT_FILL).all()
        for r, ((name, _x), rec) in enumerate(zip(packets, recs)):
            assert got[offs[r]:offs[r] + len(rec)].tobytes() == rec, (n_regions, r, name)
            assert (got[offs[r] + len(rec):offs[r + 1]] == OUT_FILL).all(), (n_regions, r, name, "wrote behind the record")
    for flags, got, offs in shipped_and_capped(H, lambda: _unpack(H, recs, [len(r) for r in recs], sizes)):
        assert flags == 0
        for r, (name, x) in enumerate(packets):
            assert got[offs[r]:offs[r] + x.size].tobytes() == x.tobytes() == H.sparse_unpack_host(recs[r], x.size), (n_regions, r, name)
            assert (got[offs[r] + x.size:offs[r + 1]] == OUT_FILL).all(), (n_regions, r, name, "wrote behind the packet")


def test_sparse_pack_refuses_an_inconsistent_scan_word_on_a_later_pass(H):
    from test_gpu_sparse import _pack
    packets = G.sparse_packets(113)
    bad = G.SPARSE_BAD_REGION
    recs = [S.pack(x) for _name, x in packets]
    scans = [S.scan(x) for _name, x in packets]
    scans[bad] += 1 << 8                                      # one exception too many
    srcs, sizes = _device_packets(packets), [x.size for _name, x in packets]
    for flags, got, offs in shipped_and_capped(H, lambda: _pack(H, srcs, sizes, scans, [len(r) for r in recs])):
        assert flags == BAD_BATCH
        for r, rec in enumerate(recs):
            keep = 0 if r == bad else len(rec)
            assert got[offs[r]:offs[r] + keep].tobytes() == rec[:keep], r
            assert (got[offs[r] + keep:offs[r + 1]] == OUT_FILL).all(), (r, "wrote behind the record, or into the refused region")


@pytest.mark.parametrize("name,rec,rec_bytes,n", S.damaged(), ids=[d[0] for d in S.damaged()])
def test_sparse_unpack_refuses_a_damaged_record_on_a_later_pass(H, name, rec, rec_bytes, n):
    """region 37 of 113 (wavefront 1, its fourth pass): BAD_PACKET, its destination untouched, and region 49 -- the same
    wavefront's next, built in the LDS the damaged record was scattered into -- exact, like every other"""
    from test_gpu_sparse import _unpack
    packets = G.sparse_packets(113)
    bad = G.SPARSE_BAD_REGION
    recs = [S.pack(x) for _name, x in packets]
    lens, sizes = [len(r) for r in recs], [x.size for _name, x in packets]
    recs[bad], lens[bad], sizes[bad] = rec, rec_bytes, n
    for flags, got, offs in shipped_and_capped(H, lambda: _unpack(H, recs, lens, sizes)):
        assert flags == BAD_PACKET
        for r, (_name, x) in enumerate(packets):
            keep = 0 if r == bad else x.size
            assert got[offs[r]:offs[r] + keep].tobytes() == x.tobytes()[:keep], (name, r)
            assert (got[offs[r] + keep:offs[r + 1]] == OUT_FILL).all(), (name, r, "wrote behind the packet, or into the refused region")


# ---- (f) batch.py through the capped library ------------------------------------------------------------------------------

def _same_fields(a, b, where):
    for f in dataclasses.fields(a):
        u, v = getattr(a, f.name), getattr(b, f.name)
        if isinstance(u, torch.Tensor):
            assert isinstance(v, torch.Tensor) and u.dtype == v.dtype and torch.equal(u, v), (*where, f.name)
        else:
            assert u == v, (*where, f.name)


def test_batch_compress_decompress_and_gip_do_not_depend_on_the_grid(H):
    """batch.compress / decompress / Compressed.gip / from_gip on the typed tensors of test_gpu_delta.py: every field of the
    result through the capped library equals the shipped library's, and every round trip is exact"""
    from gpuar_amd import batch
    from test_gpu_delta import raw, typed_tensors
    ts, flags = typed_tensors()
    hosts = [raw(t).copy() for t in ts]
    bases = []
    for b, h in enumerate(hosts):                              # the tensor with one byte in 200 changed: XORed, sparse packets; none for the uniform bytes: raw
        q = h.copy()
        q[::200] ^= 0x41
        bases.append(torch.from_numpy(q).cuda() if h.size and b % 4 != 3 and b != 6 else None)
    kinds = dict(planes="auto", base=bases, stored="auto", sparse="auto")
    options = {"delta": dict(planes="auto", delta=flags), "delta_crc": dict(planes="auto", delta=flags, checksum=True, stored="auto"),
               "kinds": kinds, "kinds_crc": dict(kinds, checksum=True)}

    def run():
        out = {}
        for key, kw in options.items():
            c = batch.compress(ts, **kw)
            back = [o.cpu().numpy() for o in batch.decompress(c, base=kw.get("base"))]
            files = [c.gip(b, kinds=True) for b in range(len(ts))] if key == "kinds_crc" else [c.gip(b) for b in range(len(ts))] if key == "delta" else None
            again = batch.from_gip(files) if files else None
            back_again = [o.cpu().numpy() for o in batch.decompress(again, base=kw.get("base"))] if files else None
            out[key] = (c, back, files, again, back_again)
        return out

    shipped, capped, capped_again = shipped_and_capped(H, run)
    for key in options:
        for other, which in ((capped, "capped"), (capped_again, "capped again")):
            (c0, back0, files0, again0, _b0), (c1, back1, files1, again1, back_again1) = shipped[key], other[key]
            _same_fields(c0, c1, (key, which))
            assert files0 == files1, (key, which)
            for b, (o, h) in enumerate(zip(back1, hosts)):
                assert np.array_equal(o, h), (key, which, b)
            if files1:
                _same_fields(again0, again1, (key, which, "from_gip"))
                for b, (o, h) in enumerate(zip(back_again1, hosts)):
                    assert np.array_equal(o, h), (key, which, "from_gip", b)
    c = capped["kinds_crc"][0]
    kinds_used = set(c.stored.cpu().tolist())
    assert kinds_used == {0, 1, 2}, kinds_used                # coded, raw (move_packets) and sparse (sparse_pack / unpack) packets
    assert capped["delta"][0].delta == flags and capped["kinds"][0].based == [q is not None for q in bases]
