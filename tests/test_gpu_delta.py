"""The delta filter on the MI355X: gpuar_hip_split_delta / merge_delta and their batch forms against the numpy restatement of the
definition (delta_ref.py), batch.compress(delta=...) / decompress against the reference oracle's stream of the filtered, split
bytes, and `gpuar c --delta` on the GPU against gpuar-host.  Every device buffer has guard bytes behind what a call may write,
and every status word is read."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import delta_ref as D
import planes_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")
HOST_CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")
GUARD = 256


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    codec = O.require_best()
    assert codec.kind == O.expected_kind()
    return codec


def guarded(host: np.ndarray, fill):
    t = torch.full((host.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    t[:host.size] = torch.from_numpy(host).cuda()
    return t, host.size


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


# ---- one buffer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", D.WIDTHS)
def test_single_buffer_split_and_merge_against_numpy(H, w):
    """Every length that crosses a block, a wavefront (1024 elements), a group and the tail, on three kinds of bytes."""
    for kind in D.KINDS:
        for n in D.lengths_for(w):
            x = D.bytes_of(kind, n, w, seed=1000 * w + n % 997)
            want = D.numpy_split_delta(x, w)
            d_in, _ = guarded(x, 0xA5)
            d_out = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
            H.split_delta(d_in, w, d_out=d_out, n_bytes=n)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[:n] == want).all(), (kind, w, n, int(np.flatnonzero(got[:n] != want)[0]))
            assert (got[n:] == 0x5A).all(), (kind, w, n, "split wrote behind n")
            assert (d_in.cpu().numpy()[:n] == x).all() and (d_in[n:] == 0xA5).all(), (kind, w, n, "split changed its input")
            # merge, out of place
            d_back = torch.full((n + GUARD,), 0x3C, dtype=torch.uint8, device="cuda")
            H.merge_delta(d_out, w, d_out=d_back, n_bytes=n)
            torch.cuda.synchronize()
            back = d_back.cpu().numpy()
            assert (back[:n] == x).all(), (kind, w, n, int(np.flatnonzero(back[:n] != x)[0]))
            assert (back[n:] == 0x3C).all(), (kind, w, n, "merge wrote behind n")
            # merge and split, in place
            H.merge_delta(d_out, w, d_out=d_out, n_bytes=n)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[:n] == x).all(), (kind, w, n, "merge in place")
            assert (got[n:] == 0x5A).all(), (kind, w, n, "merge in place wrote behind n")
            H.split_delta(d_out, w, d_out=d_out, n_bytes=n)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[:n] == want).all() and (got[n:] == 0x5A).all(), (kind, w, n, "split in place")


def test_single_buffer_error_codes(H):
    lib = H.load()
    d = torch.zeros(4 * PACKET + 64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    for fn in (lib.gpuar_hip_split_delta, lib.gpuar_hip_merge_delta):
        assert fn(p + 4, PACKET, 2, p + 2 * PACKET, None) == -1                # GPUAR_ERR_ALIGNMENT
        assert fn(p, PACKET, 2, p + 2 * PACKET + 8, None) == -1
        assert fn(p, PACKET, 3, p + 2 * PACKET, None) == -2                    # GPUAR_ERR_ARGUMENT: the width
        assert fn(p, 2 * PACKET, 2, p + PACKET, None) == -2                    # partial overlap
        assert fn(p + PACKET, 2 * PACKET, 2, p, None) == -2
        assert fn(p, 0, 2, p, None) == 0
    torch.cuda.synchronize()
    assert int(d.count_nonzero().item()) == 0
    with pytest.raises(H.GpuarError):
        H.split_delta(d, 3)


# ---- batches ----------------------------------------------------------------------------------------------------------

def _layout(sizes):
    at, offs = 0, []
    for n in sizes:
        offs.append(at)
        at += (n + GUARD + 15) // 16 * 16
    return offs, at


def test_batch_call_on_many_buffers_of_every_width_and_filter(H):
    """300 buffers of seeded sizes, widths 1, 2, 4, 8 and filter flags 0 / 1 in one call, against numpy; guard bytes behind
    every output; merge in place restores; with the filter all 0 the output is split_planes_batch's."""
    rng = np.random.default_rng(78)
    sizes = [0, 1, 15, 16, 17, 8191, 8192, 8193, 65535, 65536, 65537, 3 * 65536 + 4097] + [int(v) for v in rng.integers(0, 200000, 288)]
    widths = [int(v) for v in rng.choice([1, 2, 4, 8], len(sizes))]
    widths[:12] = [8, 2, 8, 2, 4, 4, 1, 2, 8, 1, 8, 8]
    filt = [int(v) for v in rng.integers(0, 2, len(sizes))]
    filt[:12] = [1] * 12
    hosts = [D.bytes_of("uniform", n, 1, seed=3 * i + 1) for i, n in enumerate(sizes)]
    offs, at = _layout(sizes)
    src = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    for o, h in zip(offs, hosts):
        src[o:o + h.size] = torch.from_numpy(h).cuda()
    dst = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    fp, npk = H.batch_packet_count(sizes)
    n = len(sizes)
    desc = torch.tensor([src.data_ptr() + o for o in offs] + [dst.data_ptr() + o for o in offs] + sizes + fp + widths + filt + [0] * n,
                        dtype=torch.int64, device="cuda")
    d_in, d_out, d_bytes, d_fp = desc[:n], desc[n:2 * n], desc[2 * n:3 * n], desc[3 * n:4 * n + 1]
    d_w, d_f, d_zero = desc[4 * n + 1:5 * n + 1], desc[5 * n + 1:6 * n + 1], desc[6 * n + 1:]
    status = _status()
    H.split_delta_batch(d_in, d_bytes, d_fp, d_w, d_f, n, npk, d_out, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    for b, (o, h, w, f) in enumerate(zip(offs, hosts, widths, filt)):
        want = D.numpy_split_delta(h, w) if f else R.numpy_split(h, w)
        assert (got[o:o + h.size] == want).all(), (b, h.size, w, f)
        end = offs[b + 1] if b + 1 < n else at
        assert (got[o + h.size:end] == 0x5A).all(), (b, h.size, w, f, "wrote behind the buffer")
    # merge in place restores the inputs
    H.merge_delta_batch(d_out, d_bytes, d_fp, d_w, d_f, n, npk, d_out, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    want = src.cpu().numpy()
    for b, (o, h) in enumerate(zip(offs, hosts)):
        assert (want[o:o + h.size] == h).all(), (b, "the split changed its input")
        assert (got[o:o + h.size] == h).all(), (b, h.size, widths[b], filt[b])
        end = offs[b + 1] if b + 1 < n else at
        assert (got[o + h.size:end] == 0x5A).all(), (b, "merge wrote behind the buffer")
    # no filter anywhere: the planes call's output
    dst.fill_(0x5A)
    H.split_delta_batch(d_in, d_bytes, d_fp, d_w, d_zero, n, npk, d_out, d_status=status)
    plain = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    d_plain = d_out - dst.data_ptr() + plain.data_ptr()
    H.split_planes_batch(d_in, d_bytes, d_fp, d_w, n, npk, d_plain, d_status=status)
    assert int(status.item()) == 0
    assert torch.equal(dst, plain)


def test_batch_call_flags_unusable_descriptors_and_leaves_them_alone(H):
    sizes = [3 * PACKET, 2 * PACKET + 5, 4 * PACKET]
    src = torch.arange(16 * PACKET, device="cuda").to(torch.uint8)
    dst = torch.full((16 * PACKET,), 0x5A, dtype=torch.uint8, device="cuda")
    offs = [0, 4 * PACKET, 8 * PACKET]
    fp, npk = H.batch_packet_count(sizes)
    host = src.cpu().numpy()

    def call(widths, filt, out_offs):
        dst.fill_(0x5A)
        desc = torch.tensor([src.data_ptr() + o for o in offs] + [dst.data_ptr() + o for o in out_offs] + sizes + fp + widths + filt,
                            dtype=torch.int64, device="cuda")
        status = _status()
        H.split_delta_batch(desc[0:3], desc[6:9], desc[9:13], desc[13:16], desc[16:19], 3, npk, desc[3:6], d_status=status)
        return int(status.item()), dst.cpu().numpy()

    def others_done(got):
        assert (got[:sizes[0]] == D.numpy_split_delta(host[:sizes[0]], 2)).all()
        assert (got[offs[2]:offs[2] + sizes[2]] == D.numpy_split_delta(host[offs[2]:offs[2] + sizes[2]], 4)).all()

    flags, got = call([2, 2, 4], [1, 2, 1], offs)                             # a filter of 2
    assert flags == H.STATUS_BAD_BATCH
    assert (got[offs[1]:offs[2]] == 0x5A).all(), "the buffer with the unusable filter was written"
    others_done(got)
    flags, got = call([2, 3, 4], [1, 1, 1], offs)                             # a width of 3
    assert flags == H.STATUS_BAD_BATCH and (got[offs[1]:offs[2]] == 0x5A).all()
    others_done(got)
    flags, got = call([2, 2, 4], [1, 1, 1], [offs[0], offs[1] + 8, offs[2]])  # a misaligned output pointer
    assert flags == H.STATUS_BAD_BATCH and (got[offs[1]:offs[2]] == 0x5A).all()
    others_done(got)
    flags, got = call([2, 2, 4], [1, 1, 1], offs)
    assert flags == 0 and (got[offs[1]:offs[1] + sizes[1]] == D.numpy_split_delta(host[offs[1]:offs[1] + sizes[1]], 2)).all()


# ---- batch.compress ---------------------------------------------------------------------------------------------------

def raw(t):
    """the tensor's bytes on the host"""
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1) if t.numel() else np.empty(0, dtype=np.uint8)


def typed_tensors():
    """(tensors, filter per tensor): ordered integers of every width with groups and tails, and data the filter is not for"""
    g = torch.Generator().manual_seed(2)
    steps = lambda n, hi: torch.cumsum(torch.randint(0, hi, (n,), generator=g, dtype=torch.int64), 0)
    ts = [
        steps(2 * PACKET + 9, 64).cuda(),                                     # int64: 2 groups and a tail
        steps(5 * PACKET + 333, 1000).to(torch.int32).cuda(),
        steps(3 * PACKET + 1, 40).to(torch.int16).cuda(),
        (steps(3 * PACKET + 77, 5) % 256).to(torch.uint8).cuda(),             # a byte delta per packet
        (torch.randn(4 * PACKET + 77, generator=g) * 0.02).cuda(),            # fp32: planes alone
        torch.empty(0, dtype=torch.int32, device="cuda"),
        torch.randint(0, 256, (8191,), generator=g, dtype=torch.uint8).cuda(),
        steps(100, 3).to(torch.int16).cuda(),                                 # less than a packet
        steps(PACKET, 7).to(torch.int32).cuda(),                              # one group exactly
    ]
    return ts, [True, True, True, True, False, True, False, True, True]


def test_compress_codes_the_filtered_split_bytes_and_decompress_returns_the_bits(H, oracle):
    from gpuar_amd import batch
    ts, flags = typed_tensors()
    before = [raw(t).copy() for t in ts]
    c = batch.compress(ts, planes="auto", delta=flags)
    assert c.planes == [8, 4, 2, 1, 4, 4, 1, 2, 4] and c.delta == flags
    assert c.sizes == [b.size for b in before] and c.crc32 is None
    for t, b in zip(ts, before):
        assert (raw(t) == b).all(), "compress modified its input"
    for b, (host, w, f) in enumerate(zip(before, c.planes, flags)):
        coded = D.numpy_split_delta(host, w) if f else R.numpy_split(host, w)
        want = oracle.encode_stream(coded).tobytes() if host.size else b""
        assert c.payload(b).cpu().numpy().tobytes() == want, (b, w, f)
    outs = batch.decompress(c)
    for b, (o, host) in enumerate(zip(outs, before)):
        assert o.dtype == torch.uint8 and (o.cpu().numpy() == host).all(), b
    mine = [torch.empty_like(t) for t in ts]                                  # into the caller's tensors, of the inputs' own types
    assert batch.decompress(c, out=mine) is mine
    for b, (o, t) in enumerate(zip(mine, ts)):
        assert torch.equal(o, t), b
    # the filter pays on this batch
    plain = batch.compress(ts, planes="auto")
    assert plain.delta is None and c.stream.numel() < 0.7 * plain.stream.numel()
    assert batch.estimate(ts, planes="auto", delta=flags) == [sum(H.estimate_host(
        (D.numpy_split_delta(h, w) if f else R.numpy_split(h, w)).tobytes())) for h, w, f in zip(before, c.planes, flags)]
    # delta without planes: bytes; True: every tensor
    c1 = batch.compress(ts[3:4], delta=True)
    assert c1.planes == [1] and c1.delta == [True]
    assert c1.payload(0).cpu().numpy().tobytes() == oracle.encode_stream(D.numpy_split_delta(before[3], 1)).tobytes()
    assert torch.equal(batch.decompress(c1)[0], ts[3])
    with pytest.raises(H.GpuarError):
        batch.compress(ts, delta=[True])
    with pytest.raises(H.GpuarError):
        batch.compress(ts, delta="always")


def test_checksums_stay_those_of_the_original_bytes_and_stored_composes(H):
    from gpuar_amd import batch
    ts, flags = typed_tensors()
    c = batch.compress(ts, planes="auto", delta=flags, checksum=True)
    want = [zlib.crc32(raw(t)[p * PACKET:(p + 1) * PACKET].tobytes()) for t in ts for p in range((raw(t).size + PACKET - 1) // PACKET)]
    assert [v & 0xFFFFFFFF for v in c.crc32.cpu().tolist()] == want
    for o, t in zip(batch.decompress(c), ts):
        assert (o.cpu().numpy() == raw(t)).all()
    s = batch.compress(ts, planes="auto", delta=flags, checksum=True, stored="auto")
    assert s.delta == flags and int(s.stored.sum().item()) >= 1               # (the uniform bytes of tensor 6 cannot shrink)
    for o, t in zip(batch.decompress(s), ts):
        assert (o.cpu().numpy() == raw(t)).all()


def test_delta_none_and_false_take_the_path_of_the_call_without_the_keyword(H):
    from gpuar_amd import batch
    ts, _flags = typed_tensors()
    for planes in (None, "auto"):
        a, b = batch.compress(ts, planes=planes), batch.compress(ts, planes=planes, delta=None)
        assert torch.equal(a.stream, b.stream) and torch.equal(a.offsets, b.offsets) and a.delta is None and b.delta is None
        assert a.planes == b.planes
        off = batch.compress(ts, planes=planes, delta=False)
        assert torch.equal(a.stream, off.stream) and off.delta == [False] * len(ts)
        assert off.gip(1) == a.gip(1)


def test_delta_auto_makes_the_choices_of_the_host_rule(H):
    from gpuar_amd import batch
    table = D.table_inputs()
    ts = [torch.from_numpy(D.raw_bytes(a).copy()).cuda() for a, _w in table.values()]
    widths = [w for _a, w in table.values()]
    c = batch.compress(ts, planes=widths, delta="auto")
    assert c.delta == [name in D.TABLE_DELTA_WINS for name in table], dict(zip(table, c.delta))
    for o, t in zip(batch.decompress(c), ts):
        assert torch.equal(o, t)
    fixed = batch.estimate(ts, planes=widths, delta=c.delta)
    assert batch.estimate(ts, planes=widths, delta="auto") == fixed
    assert all(a <= b for a, b in zip(fixed, batch.estimate(ts, planes=widths)))


# ---- the command line on the GPU --------------------------------------------------------------------------------------

def _run(cli, *args):
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1")
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (args, r.stdout, r.stderr)


def cli_input(n, w):
    rng = np.random.default_rng(n + w)
    v = np.cumsum(rng.integers(0, 50, n // w + 1)).astype(np.uint64).astype(D.UINT[w])
    return v.astype("<u%d" % w).view(np.uint8)[:n].copy()


def delta_args(w):
    return ["--delta"] + ([f"--planes={w}"] if w > 1 else [])


@pytest.mark.parametrize("w", D.WIDTHS)
def test_cli_delta_on_the_gpu_writes_the_file_gpuar_host_writes(H, tmp_path, w):
    from gpuar_amd import batch
    for n in (0, 1, w - 1, 8191, w * PACKET, w * PACKET + 1, 70 * PACKET + 13, 1000 * PACKET + 4099):
        big = n > 100 * PACKET
        data = cli_input(n, w)
        src = tmp_path / "in.dat"
        data.tofile(src)
        _run(HOST_CLI, "c", "--host", "--checksum", *delta_args(w), "--threads", "16", f"--in={src}", f"--out={tmp_path / 'h.gip'}")
        want = (tmp_path / "h.gip").read_bytes()
        end = struct.unpack_from("<Q", want, 12)[0]
        assert struct.unpack_from("<4sIQII", want, end) == (b"GIPX", 4, (n + PACKET - 1) // PACKET, w, 3)
        for extra in ((), ("--batch=100",)) if big else ((),):
            _run(CLI, "c", "--checksum", *delta_args(w), *extra, f"--in={src}", f"--out={tmp_path / 'g.gip'}")
            assert (tmp_path / "g.gip").read_bytes() == want, (w, n, extra)
        for d_extra in ((), ("--batch=100",), ("--host",)) if big else ((), ("--host",)):
            _run(CLI, "d", *d_extra, f"--in={tmp_path / 'g.gip'}", f"--out={tmp_path / 'back.dat'}")
            assert (tmp_path / "back.dat").read_bytes() == data.tobytes(), (w, n, d_extra)
        if big or n == w * PACKET + 1:
            # without CRCs: the same packets, a trailer without the CRC array; Compressed.gip(b) is either file
            _run(CLI, "c", *delta_args(w), f"--in={src}", f"--out={tmp_path / 'n.gip'}")
            plain = (tmp_path / "n.gip").read_bytes()
            assert plain[:end] == want[:end] and struct.unpack_from("<4sIQII", plain, end) == (b"GIPX", 4, (n + PACKET - 1) // PACKET, w, 2)
            _run(CLI, "d", f"--in={tmp_path / 'n.gip'}", f"--out={tmp_path / 'back.dat'}")
            assert (tmp_path / "back.dat").read_bytes() == data.tobytes()
            t = torch.from_numpy(data).cuda()
            assert batch.compress([t], planes=w, delta=True, checksum=True).gip(0) == want
            assert batch.compress([t], planes=w, delta=True).gip(0) == plain


def test_gpu_decode_refuses_unusable_delta_trailers_and_catches_damage(H, tmp_path):
    n, w = 200 * PACKET + 100, 4
    data = cli_input(n, w)
    src, gip = tmp_path / "in.dat", tmp_path / "g.gip"
    data.tofile(src)
    _run(CLI, "c", "--checksum", "--delta", f"--planes={w}", "--batch=64", f"--in={src}", f"--out={gip}")
    good = gip.read_bytes()
    end = struct.unpack_from("<Q", good, 12)[0]
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1")

    def decode(blob):
        (tmp_path / "bad.gip").write_bytes(bytes(blob))
        return subprocess.run([CLI, "d", "--batch=64", f"--in={tmp_path / 'bad.gip'}", f"--out={tmp_path / 'bad.out'}"], capture_output=True, text=True,
                              timeout=300, env=env)
    clen0 = struct.unpack_from("<H", good, end + 24)[0]
    for at, fmt, value in ((end + 16, "<I", 3), (end + 20, "<I", 7), (end + 20, "<I", 1), (end + 24, "<H", clen0 + 1)):
        bad = bytearray(good)
        struct.pack_into(fmt, bad, at, value)
        r = decode(bad)
        assert r.returncode == 1 and "version 4" in r.stderr and "version 3" not in r.stderr, (at, r.returncode, r.stderr)
        assert (tmp_path / "bad.out").read_bytes() == b""
    # a flipped bit deep in the stream: caught by the CRCs of the merged bytes, named within the damaged packet's group
    clens = struct.unpack_from("<200H", good, end + 24)
    p = 133
    for shift in range(0, 400, 7):
        bad = bytearray(good)
        bad[20 + sum(clens[:p]) + clens[p] // 2 + shift] ^= 0x04
        r = decode(bad)
        if r.returncode == 1 and "Checksum mismatch" in r.stderr:
            named = int(r.stderr.split("Checksum mismatch: packet ")[1].split(" ")[0])
            assert p // w * w <= named < p // w * w + w, r.stderr
            break
        assert r.returncode == 0 and (tmp_path / "bad.out").read_bytes() == data.tobytes(), r.stderr      # (a flip in bits nobody decodes)
    else:
        pytest.fail("no flip was caught")
