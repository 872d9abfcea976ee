"""Reading .gip files back into a batch on the MI355X: hip.move_bytes against numpy at every pair of source and
destination residues mod 16 and with destinations back to back at byte grain, canaries around every destination; its bad regions
and edge cases; batch.from_gip against batch.compress field for field over the option sets that leave a trace in a file; files
written by `gpuar-host c`; mixed lists; and the damage that only the device sees.  No test reads outside its own buffers: the
kernel's reads are bounded by argument (every load lies in [src, src + bytes)), its writes are shown by the canaries."""
import dataclasses
import os
import struct

import numpy as np
import pytest

import gip_files as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
GUARD, CANARY = 64, 0x5A
LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, 4100, 8195, 8196, 8703, 8704)
BAD_BATCH = 0x4


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def batch(H):
    from gpuar_amd import batch
    return batch


@pytest.fixture(scope="module")
def pool():
    """(host bytes, device tensor): 64 KiB + a slot of random bytes every source region is taken from; 16-byte aligned"""
    data = np.random.default_rng(14).integers(0, 256, 65536 + SLOT + 16, dtype=np.uint8)
    d = torch.from_numpy(data).cuda()
    assert d.data_ptr() % 16 == 0
    return data, d


def _i64(values, device="cuda"):
    return torch.tensor(np.asarray(values, dtype=np.int64), dtype=torch.int64, device=device)


def _move(H, pool, src_off, dst_off, lengths, out_bytes, stream=None, nulls=()):
    """One move_bytes launch: region r is lengths[r] bytes from pool + src_off[r] to out + dst_off[r], out being out_bytes of canary.
    `nulls`: (r, "src" | "dst") pointers passed as null.  Returns (out as numpy, the status word)."""
    data, d_pool = pool
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 16 == 0
        src = d_pool.data_ptr() + np.asarray(src_off, dtype=np.int64)
        dst = out.data_ptr() + np.asarray(dst_off, dtype=np.int64)
        for r, side in nulls:
            (src if side == "src" else dst)[r] = 0
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        H.move_bytes(_i64(src), _i64(dst), _i64(lengths), len(lengths), stream=stream, d_status=status)
        if stream is not None:
            stream.synchronize()
        return out.cpu().numpy(), int(status.item())


def _expected(pool, src_off, dst_off, lengths, out_bytes, skip=()):
    want = np.full(out_bytes, CANARY, dtype=np.uint8)
    for r, (s, d, n) in enumerate(zip(src_off, dst_off, lengths)):
        if r not in skip:
            want[d:d + n] = pool[0][s:s + n]
    return want


def test_move_bytes_at_every_pair_of_residues_and_every_length_in_one_launch(H, pool):
    window = GUARD + 16 + SLOT + GUARD                        # 8848 = 553 * 16: every window starts 16-byte aligned
    assert window % 16 == 0
    src_off, dst_off, lengths = [], [], []
    for s in range(16):
        for d in range(16):
            for n in LENGTHS:
                r = len(lengths)
                src_off.append((r * 37 % 4096) * 16 + s)
                dst_off.append(r * window + GUARD + d)
                lengths.append(n)
    assert len(lengths) == 16 * 16 * len(LENGTHS) and max(o + n for o, n in zip(src_off, lengths)) <= pool[0].size
    got, status = _move(H, pool, src_off, dst_off, lengths, len(lengths) * window)
    assert status == 0
    want = _expected(pool, src_off, dst_off, lengths, got.size)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        r = bad // window
        pytest.fail(f"byte {bad - dst_off[r]} of region {r}: src % 16 = {src_off[r] % 16}, dst % 16 = {dst_off[r] % 16}, {lengths[r]} bytes")


@pytest.mark.parametrize("start", range(16))
def test_move_bytes_destinations_back_to_back(H, pool, start):
    """About 1000 regions whose destinations stand back to back from a start of residue `start`: half of the lengths are 1 .. 8704,
    half 1 .. 48, so that several regions share one 16-byte piece.  An aligned store that reached beyond its region would land in a
    neighbour (or in the canaries around the whole)."""
    rng = np.random.default_rng(100 + start)
    lengths = np.where(rng.integers(0, 2, 1000) == 1, rng.integers(1, SLOT + 1, 1000), rng.integers(1, 49, 1000))
    lengths[:3] = (SLOT, 1, SLOT)
    src_off = rng.integers(0, 65536, lengths.size)
    dst_off = GUARD + start + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    total = int(lengths.sum())
    # the regions go to the kernel in a shuffled order: which workgroup moves which is no property of the layout
    order = rng.permutation(lengths.size)
    got, status = _move(H, pool, src_off[order], dst_off[order], lengths[order], GUARD + start + total + GUARD + 16)
    assert status == 0
    want = np.concatenate([pool[0][s:s + n] for s, n in zip(src_off, lengths)])
    assert np.array_equal(got[GUARD + start:GUARD + start + total], want)
    assert (got[:GUARD + start] == CANARY).all() and (got[GUARD + start + total:] == CANARY).all()


def test_move_bytes_bad_regions_and_edge_cases(H, pool):
    window = GUARD + SLOT + 16 + GUARD
    lengths = [100, SLOT + 1, 77, 4100, 0, 33, SLOT]
    src_off = [3, 5, 7, 11, 13, 17, 19]
    dst_off = [r * window + GUARD + 1 + r for r in range(len(lengths))]
    got, status = _move(H, pool, src_off, dst_off, lengths, len(lengths) * window, nulls=((2, "src"), (3, "dst")))
    assert status == BAD_BATCH
    assert np.array_equal(got, _expected(pool, src_off, dst_off, lengths, got.size, skip=(1, 2, 3)))     # the bad regions untouched, their neighbours right
    # a region of 0 bytes writes nothing and is no bad region
    got, status = _move(H, pool, [1, 2], [GUARD, GUARD + 40], [0, 9], 256)
    assert status == 0 and np.array_equal(got, _expected(pool, [1, 2], [GUARD, GUARD + 40], [0, 9], 256))
    # n_regions == 0: nothing is launched, nothing is looked at
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    none = torch.zeros(1, dtype=torch.int64, device="cuda")
    H.move_bytes(none, none, none, 0, d_status=word)
    assert H.load().gpuar_hip_move_bytes(None, None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert int(word.item()) == 0
    # the bindings refuse descriptors that are not 64-bit device tensors
    with pytest.raises(H.GpuarError, match="d_bytes must be a contiguous 64-bit CUDA tensor"):
        H.move_bytes(none, none, none.to(torch.int32), 1)


def test_move_bytes_on_a_side_stream(H, pool):
    rng = np.random.default_rng(5)
    lengths = rng.integers(1, SLOT + 1, 200)
    src_off = rng.integers(0, 65536, lengths.size)
    dst_off = GUARD + 5 + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    size = GUARD + 5 + int(lengths.sum()) + GUARD
    here, status_here = _move(H, pool, src_off, dst_off, lengths, size)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    there, status_there = _move(H, pool, src_off, dst_off, lengths, size, stream=side)
    assert status_here == status_there == 0 and np.array_equal(here, there)
    assert np.array_equal(here, _expected(pool, src_off, dst_off, lengths, size))


# ---- from_gip against compress ---------------------------------------------------------------------------------------------

SIZES = (0, 1, PACKET, PACKET + 1, 5 * PACKET + 4097)


def _bf16(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n // 2 + 1, generator=g) * 0.02).to(torch.bfloat16).view(torch.uint8)[:n].numpy().copy()


@pytest.fixture(scope="module")
def tensors():
    """(inputs as numpy, the same on the device, bases on the device: each tensor with one byte in 977 changed -- and one base equal
    to its tensor)"""
    host = [G.family(fam, n, seed=3) for n in SIZES for fam in G.FAMILIES] + [_bf16(n, 40 + i) for i, n in enumerate(SIZES)]
    dev = [torch.from_numpy(x).cuda() for x in host]
    bases = [torch.from_numpy(G.base_of(x)).cuda() for x in host]
    bases[-1] = dev[-1].clone()
    return host, dev, bases


OPTION_SETS = [
    ("none", {}),
    ("checksum", dict(checksum=True)),
    ("planes2", dict(planes=2)),
    ("planes8_delta", dict(planes=8, delta=True)),
    ("base_checksum_planes2", dict(base=True, checksum=True, planes=2)),
    ("stored", dict(stored="auto")),
    ("sparse", dict(sparse="auto")),
    ("stored_sparse_checksum_planes2_base", dict(stored="auto", sparse="auto", checksum=True, planes=2, base=True)),
]
TENSOR_FIELDS = ("stream", "offsets", "crc32", "stored", "raw", "raw_offsets", "sparse", "sparse_offsets")
LIST_FIELDS = ("first_packet", "sizes", "planes", "delta", "based", "kinds_rule")


def _same_fields(c, c2, what):
    """c2 = from_gip of c's files holds what c holds.  One field has two spellings of "none" in compress itself: without
    sparse="auto" a batch has sparse = sparse_offsets = None, with it and no sparse packet an empty tensor and [0]; a version-6 file
    does not say which, and from_gip gives the second."""
    for name in TENSOR_FIELDS:
        a, b = getattr(c, name), getattr(c2, name)
        if a is None and name in ("sparse", "sparse_offsets") and c.stored is not None:
            a = torch.zeros(1 if name == "sparse_offsets" else 0, dtype=b.dtype, device=b.device)
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, name)
    for name in LIST_FIELDS:
        assert getattr(c, name) == getattr(c2, name), (what, name, getattr(c, name), getattr(c2, name))


@pytest.mark.parametrize("name,options", OPTION_SETS, ids=[s[0] for s in OPTION_SETS])
def test_from_gip_gives_back_what_compress_returned(batch, tensors, name, options):
    host, dev, bases = tensors
    options = dict(options)
    base = bases if options.pop("base", False) else None
    kinds = "stored" in options or "sparse" in options
    c = batch.compress(dev, base=base, **options)
    blobs = [c.gip(b, kinds=kinds) for b in range(c.n_buffers)]
    c2 = batch.from_gip(blobs)
    _same_fields(c, c2, name)
    assert [c2.gip(b, kinds=kinds) for b in range(c2.n_buffers)] == blobs
    for b, (out, x) in enumerate(zip(batch.decompress(c2, base=base), host)):
        assert np.array_equal(out.cpu().numpy(), x), (name, b)
    if kinds:
        kinds_host = c.stored.cpu().numpy()
        assert (kinds_host != 0).any() and len(set(kinds_host.tolist())) >= 2       # the set does exercise the move


def test_from_gip_on_a_side_stream_and_from_every_container(batch, tensors, tmp_path):
    host, dev, _bases = tensors
    c = batch.compress(dev, stored="auto", sparse="auto", checksum=True)
    blobs = [c.gip(b, kinds=True) for b in range(c.n_buffers)]
    held = []
    for b, blob in enumerate(blobs):
        if b % 5 == 4:
            path = tmp_path / f"buffer{b}.gip"
            path.write_bytes(blob)
            held.append(str(path) if b % 2 else path)
        else:
            held.append((blob, bytearray(blob), memoryview(blob), np.frombuffer(blob, dtype=np.uint8))[b % 5])
    held[0] = torch.frombuffer(bytearray(blobs[0]), dtype=torch.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    c2 = batch.from_gip(held, device="cuda", stream=side)
    side.synchronize()
    _same_fields(c, c2, "side stream")
    for out, x in zip(batch.decompress(c2), host):
        assert np.array_equal(out.cpu().numpy(), x)


# ---- files the CLI wrote ---------------------------------------------------------------------------------------------------

def _cli_inputs():
    big = 3 * PACKET + 4097
    return [G.family(fam, big) for fam in G.FAMILIES] + [G.family("text", n) for n in (0, 1, PACKET, PACKET + 1)]


@pytest.mark.parametrize("name,flags,says", G.FLAG_SETS, ids=[s[0] for s in G.FLAG_SETS])
def test_files_of_the_cli_decode_through_from_gip(batch, tmp_path, name, flags, says):
    inputs = _cli_inputs()
    based = bool(says.get("base"))
    blobs = [G.write(tmp_path, x, flags, G.base_of(x) if based else None) for x in inputs]
    c = batch.from_gip(blobs)
    assert c.sizes == [x.size for x in inputs] and (c.crc32 is not None) == bool(says.get("crcs")) and (c.stored is not None) == (says["version"] == 6)
    assert (c.planes or [1] * len(inputs)) == [says.get("elem", 1)] * len(inputs)
    assert c.delta == ([True] * len(inputs) if says.get("delta") else None) and c.based == ([True] * len(inputs) if based else None)
    base = [torch.from_numpy(G.base_of(x)).cuda() for x in inputs] if based else None
    for b, (out, x) in enumerate(zip(batch.decompress(c, base=base), inputs)):
        assert np.array_equal(out.cpu().numpy(), x), (name, b)
    if says["version"] == 6:
        want = [k for blob, x in zip(blobs, inputs) for k in G.expected(blob, x, says)["kinds"]]
        assert c.stored.cpu().tolist() == want


def test_a_mixed_list_of_files(batch, tmp_path):
    from gpuar_amd.hip import GpuarError
    x = [G.family("sparse", 3 * PACKET + 4097), G.family("text", 2 * PACKET + 5), G.family("uniform", PACKET + 1)]
    mixed = G.write(tmp_path, x[0], ["--stored=auto", "--sparse=auto"])
    plain = G.write(tmp_path, x[1], [])
    planes = G.write(tmp_path, x[2], ["--planes=4", "--checksum"])
    with pytest.raises(GpuarError, match=r"files\[0\] carries no CRCs, files\[2\] does"):
        batch.from_gip([mixed, plain, planes])
    c = batch.from_gip([G.write(tmp_path, x[0], ["--stored=auto", "--sparse=auto", "--checksum"]), G.write(tmp_path, x[1], ["--checksum"]), planes])
    assert c.planes == [1, 1, 4] and c.delta is None and c.based is None and c.kinds_rule is not None
    kinds = c.stored.cpu().tolist()
    assert len(kinds) == 4 + 3 + 2 and kinds[4:] == [0] * 5 and 2 in kinds[:4]       # kind 0 for the packets of the other files
    for out, want in zip(batch.decompress(c), x):
        assert np.array_equal(out.cpu().numpy(), want)
    # without a version-6 file the upload is the stream
    split = G.write(tmp_path, x[2], ["--planes=4"])
    c = batch.from_gip([plain, split])
    assert c.stored is None and c.raw is None and c.sparse is None and c.kinds_rule is None and c.crc32 is None and c.planes == [1, 4]
    assert c.stream.cpu().numpy().tobytes() == plain[20:] + split[20:G.walk(split)[2]]
    assert c.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(G.walk(plain)[0] + G.walk(split)[0])]).tolist()
    for out, want in zip(batch.decompress(c), x[1:]):
        assert np.array_equal(out.cpu().numpy(), want)
    assert batch.from_gip([]).n_buffers == 0


def test_from_gip_refuses_a_bad_list_before_any_launch(batch, tmp_path):
    from gpuar_amd.hip import GpuarError
    good = G.write(tmp_path, G.family("text", PACKET + 1), [])
    with pytest.raises(GpuarError, match=r"files\[1\] is a int"):
        batch.from_gip([good, 123])
    with pytest.raises(GpuarError, match=r"files\[0\] is a Tensor"):
        batch.from_gip([torch.zeros(64, dtype=torch.uint8, device="cuda")])
    with pytest.raises(GpuarError, match=r"files\[1\]: packet 0 at offset 20: ulen is not"):
        batch.from_gip([good, G.patched(good, 22, struct.pack("<H", 8191))])
    with pytest.raises(GpuarError, match=r"files\[0\] \(.*missing\.gip\)"):
        batch.from_gip([str(tmp_path / "missing.gip")])
    with pytest.raises(GpuarError, match="a list of .gip files"):
        batch.from_gip(good)


# ---- damage that only the device sees ----------------------------------------------------------------------------------------

def test_damage_inside_a_packet_is_reported_by_decompress(batch, tmp_path):
    from gpuar_amd.hip import GpuarError
    x = G.family("sparse", 2 * PACKET)
    good = G.write(tmp_path, x, ["--sparse=auto"])
    g = batch.read_gip(good)
    assert g.kinds.tolist() == [2, 2]
    rec = 20 + 4                                               # packet 0's record: head, then the exceptions' positions
    k = struct.unpack("<H", good[rec + 2:rec + 4])[0]
    assert k >= 2
    bad = G.patched(good, rec + 4 + 2, good[rec + 4:rec + 4 + 2])                # position 1 = position 0: not ascending
    c = batch.from_gip([bad])                                  # the head is whole: the reader has nothing to refuse
    with pytest.raises(GpuarError, match="BAD_PACKET"):
        batch.decompress(c)
    assert np.array_equal(batch.decompress(batch.from_gip([good]))[0].cpu().numpy(), x)
    # a flipped byte in a coded packet of a file with CRCs: the checksum error names buffer and packet
    y = G.family("text", 2 * PACKET + 77)
    coded = G.write(tmp_path, y, ["--checksum"])
    clens = G.walk(coded)[0]
    at = 20 + clens[0] + 12
    flipped = G.patched(coded, at, bytes([coded[at] ^ 0xFF]))
    with pytest.raises(GpuarError, match=r"checksum mismatch: buffer 1, packet 1 "):
        batch.decompress(batch.from_gip([coded, flipped]))
