"""Byte-plane splitting on the MI355X: gpuar_hip_split_planes / merge_planes and their batch forms against the numpy restatement
of the definition (planes_ref.py), batch.compress(planes=...) / decompress against the reference oracle's stream of the split
bytes, the CRCs of a split batch, and `gpuar c --planes` on the GPU against gpuar-host.  Every device buffer has guard bytes
behind what a call may write, and every status word is read."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

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
    """host's bytes on the device with GUARD bytes of `fill` behind them: (whole tensor, n)."""
    t = torch.full((host.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    t[:host.size] = torch.from_numpy(host).cuda()
    return t, host.size


def data_for(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def lengths_for(w):
    G = w * PACKET
    return [0, 1, w - 1, 8191, 8192, G - 1, G, G + 1, 3 * G + 4097, (64 << 20) + 5]


# ---- one buffer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [2, 4, 8])
def test_single_buffer_split_and_merge_against_numpy(H, w):
    for n in lengths_for(w):
        x = data_for(n, 1000 * w + n % 997)
        want = R.numpy_split(x, w)
        d_in, _ = guarded(x, 0xA5)
        d_out = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        H.split_planes(d_in, w, d_out=d_out, n_bytes=n)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:n] == want).all(), (w, n, int(np.flatnonzero(got[:n] != want)[0]))
        assert (got[n:] == 0x5A).all(), (w, n, "split wrote behind n")
        assert (d_in.cpu().numpy()[:n] == x).all() and (d_in[n:] == 0xA5).all(), (w, n, "split changed its input")
        # merge, out of place
        d_back = torch.full((n + GUARD,), 0x3C, dtype=torch.uint8, device="cuda")
        H.merge_planes(d_out, w, d_out=d_back, n_bytes=n)
        torch.cuda.synchronize()
        back = d_back.cpu().numpy()
        assert (back[:n] == x).all() and (back[n:] == 0x3C).all(), (w, n)
        # merge and split, in place
        H.merge_planes(d_out, w, d_out=d_out, n_bytes=n)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:n] == x).all(), (w, n, "merge in place")
        assert (got[n:] == 0x5A).all(), (w, n, "merge in place wrote behind n")
        H.split_planes(d_out, w, d_out=d_out, n_bytes=n)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:n] == want).all() and (got[n:] == 0x5A).all(), (w, n, "split in place")


def test_single_buffer_width_one_copies(H):
    x = data_for(3 * PACKET + 77, 5)
    d_in, n = guarded(x, 0xA5)
    d_out = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    H.split_planes(d_in, 1, d_out=d_out, n_bytes=n)
    H.merge_planes(d_in, 1, d_out=d_in, n_bytes=n)                  # in place: no launch
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[:n] == x).all() and (got[n:] == 0x5A).all()
    assert (d_in.cpu().numpy()[:n] == x).all()


def test_single_buffer_error_codes(H):
    lib = H.load()
    d = torch.zeros(4 * PACKET + 64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    for fn in (lib.gpuar_hip_split_planes, lib.gpuar_hip_merge_planes):
        assert fn(p + 4, PACKET, 2, p + 2 * PACKET, None) == -1                # GPUAR_ERR_ALIGNMENT
        assert fn(p, PACKET, 2, p + 2 * PACKET + 8, None) == -1
        assert fn(p, PACKET, 3, p + 2 * PACKET, None) == -2                    # GPUAR_ERR_ARGUMENT: the width
        assert fn(p, 2 * PACKET, 2, p + PACKET, None) == -2                    # partial overlap
        assert fn(p + PACKET, 2 * PACKET, 2, p, None) == -2
        assert fn(p, 0, 2, p, None) == 0 and fn(p, PACKET, 1, p, None) == 0
    torch.cuda.synchronize()
    assert int(d.count_nonzero().item()) == 0
    with pytest.raises(H.GpuarError):
        H.split_planes(d, 3)


# ---- batches ----------------------------------------------------------------------------------------------------------

def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def test_batch_call_on_many_buffers_of_every_width(H):
    """300 buffers of seeded sizes (empty ones, sub-group ones, several groups with a tail) and widths 1, 2, 4, 8 in one call,
    out of place and in place, against numpy; guard bytes behind every output."""
    rng = np.random.default_rng(77)
    sizes = [0, 1, 15, 16, 17, 8191, 8192, 8193, 65535, 65536, 65537, 3 * 65536 + 4097] + [int(v) for v in rng.integers(0, 200000, 288)]
    widths = [int(v) for v in rng.choice([1, 2, 4, 8], len(sizes))]
    widths[:12] = [8, 2, 8, 2, 4, 4, 2, 2, 8, 8, 8, 8]
    hosts = [data_for(n, 3 * i + 1) for i, n in enumerate(sizes)]
    at, offs = 0, []
    for n in sizes:
        offs.append(at)
        at += (n + GUARD + 15) // 16 * 16
    src = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    for o, h in zip(offs, hosts):
        src[o:o + h.size] = torch.from_numpy(h).cuda()
    dst = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    fp, npk = H.batch_packet_count(sizes)
    n = len(sizes)
    desc = torch.tensor([src.data_ptr() + o for o in offs] + [dst.data_ptr() + o for o in offs] + sizes + fp + widths, dtype=torch.int64, device="cuda")
    d_in, d_out, d_bytes, d_fp, d_w = desc[:n], desc[n:2 * n], desc[2 * n:3 * n], desc[3 * n:4 * n + 1], desc[4 * n + 1:]
    status = _status()
    H.split_planes_batch(d_in, d_bytes, d_fp, d_w, n, npk, d_out, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    for b, (o, h, w) in enumerate(zip(offs, hosts, widths)):
        assert (got[o:o + h.size] == R.numpy_split(h, w)).all(), (b, h.size, w)
        end = offs[b + 1] if b + 1 < n else at
        assert (got[o + h.size:end] == 0x5A).all(), (b, h.size, w, "wrote behind the buffer")
    # merge in place restores the inputs
    H.merge_planes_batch(d_out, d_bytes, d_fp, d_w, n, npk, d_out, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    want = src.cpu().numpy()
    for b, (o, h) in enumerate(zip(offs, hosts)):
        assert (want[o:o + h.size] == h).all(), (b, "the split changed its input")
        assert (got[o:o + h.size] == h).all(), (b, h.size, widths[b])
        end = offs[b + 1] if b + 1 < n else at
        assert (got[o + h.size:end] == 0x5A).all(), (b, "merge wrote behind the buffer")


def test_batch_call_flags_unusable_descriptors_and_leaves_them_alone(H):
    sizes = [3 * PACKET, 2 * PACKET + 5, 4 * PACKET]
    widths = [2, 3, 4]
    src = torch.arange(16 * PACKET, device="cuda").to(torch.uint8)
    dst = torch.full((16 * PACKET,), 0x5A, dtype=torch.uint8, device="cuda")
    offs = [0, 4 * PACKET, 8 * PACKET]
    fp, npk = H.batch_packet_count(sizes)
    host = src.cpu().numpy()

    def call(widths, out_offs, fp=fp):
        dst.fill_(0x5A)
        desc = torch.tensor([src.data_ptr() + o for o in offs] + [dst.data_ptr() + o for o in out_offs] + sizes + fp + widths, dtype=torch.int64, device="cuda")
        status = _status()
        H.split_planes_batch(desc[0:3], desc[6:9], desc[9:13], desc[13:16], 3, npk, desc[3:6], d_status=status)
        return int(status.item()), dst.cpu().numpy()

    flags, got = call(widths, offs)                                           # a width of 3
    assert flags == H.STATUS_BAD_BATCH
    assert (got[offs[1]:offs[2]] == 0x5A).all(), "the buffer with the unusable width was written"
    assert (got[:sizes[0]] == R.numpy_split(host[:sizes[0]], 2)).all()
    assert (got[offs[2]:offs[2] + sizes[2]] == R.numpy_split(host[offs[2]:offs[2] + sizes[2]], 4)).all()
    flags, got = call([2, 2, 4], [offs[0], offs[1] + 8, offs[2]])             # a misaligned output pointer
    assert flags == H.STATUS_BAD_BATCH and (got[offs[1]:offs[2]] == 0x5A).all()
    flags, got = call([2, 2, 4], offs, [0, 3, 5, 10])                         # a buffer that owns fewer packets than its bytes make
    assert flags == H.STATUS_BAD_BATCH and (got[offs[1]:offs[2]] == 0x5A).all()
    flags, got = call([2, 2, 4], offs)
    assert flags == 0 and (got[offs[1]:offs[1] + sizes[1]] == R.numpy_split(host[offs[1]:offs[1] + sizes[1]], 2)).all()


def typed_tensors():
    g = torch.Generator().manual_seed(1)
    normal = lambda n: torch.randn(n, generator=g) * 0.02
    return [
        normal(5 * PACKET + 333).to(torch.bfloat16).cuda(),                   # 2 bytes: 5 groups and a tail
        normal(3 * PACKET + 1).to(torch.float16).cuda(),
        normal(4 * PACKET + 77).cuda(),                                       # fp32
        torch.randint(0, 50000, (2 * PACKET + 9,), generator=g, dtype=torch.int64).cuda(),
        torch.randint(0, 256, (3 * PACKET,), generator=g, dtype=torch.uint8).cuda(),
        torch.empty(0, dtype=torch.float32, device="cuda"),
        torch.randint(0, 256, (PACKET + 4097,), generator=g, dtype=torch.uint8).cuda(),      # odd lengths
        torch.randint(0, 256, (8191,), generator=g, dtype=torch.uint8).cuda(),
        normal(100).to(torch.bfloat16).cuda(),                                # less than a packet
        (torch.randn(1000, generator=g) + 1j * torch.randn(1000, generator=g)).to(torch.complex64).cuda(),      # 8 bytes, but complex: not split
    ]


def raw(t):
    """the tensor's bytes on the host"""
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1) if t.numel() else np.empty(0, dtype=np.uint8)


def test_compress_auto_codes_the_split_bytes_and_decompress_returns_the_bits(H, oracle):
    from gpuar_amd import batch
    ts = typed_tensors()
    before = [raw(t).copy() for t in ts]
    c = batch.compress(ts, planes="auto")
    assert c.planes == [2, 2, 4, 8, 1, 4, 1, 1, 2, 1]
    assert c.sizes == [b.size for b in before] and c.crc32 is None
    for t, b in zip(ts, before):
        assert (raw(t) == b).all(), "compress modified its input"
    for b, (host, w) in enumerate(zip(before, c.planes)):
        want = oracle.encode_stream(R.numpy_split(host, w)).tobytes() if host.size else b""
        assert c.payload(b).cpu().numpy().tobytes() == want, (b, w)
    outs = batch.decompress(c)
    for b, (o, host) in enumerate(zip(outs, before)):
        assert o.dtype == torch.uint8 and (o.cpu().numpy() == host).all(), b
    # into the caller's tensors, of the inputs' own types
    mine = [torch.empty_like(t) for t in ts]
    assert batch.decompress(c, out=mine) is mine
    for b, (o, t) in enumerate(zip(mine, ts)):
        assert (raw(o) == raw(t)).all(), b
    # it is smaller than the plain stream of the same tensors
    plain = batch.compress(ts)
    assert plain.planes is None and c.stream.numel() < 0.95 * plain.stream.numel()


def test_compress_with_explicit_widths_on_odd_lengths(H, oracle):
    from gpuar_amd import batch
    sizes = [PACKET + 4097, 3, 65537, 2 * 65536 + 4099, 8191]
    ts = [torch.from_numpy(data_for(n, 50 + i)).cuda() for i, n in enumerate(sizes)]
    for planes in (8, [2, 4, 8, 8, 4], [1, 1, 2, 1, 1]):
        c = batch.compress(ts, planes=planes)
        widths = [planes] * len(ts) if isinstance(planes, int) else planes
        assert c.planes == widths
        for b, (t, w) in enumerate(zip(ts, widths)):
            assert c.payload(b).cpu().numpy().tobytes() == oracle.encode_stream(R.numpy_split(t.cpu().numpy(), w)).tobytes(), (planes, b)
        for o, t in zip(batch.decompress(c), ts):
            assert torch.equal(o, t), planes


def test_planes_none_is_the_call_without_the_keyword(H):
    from gpuar_amd import batch
    ts = typed_tensors()
    a, b = batch.compress(ts), batch.compress(ts, planes=None)
    assert torch.equal(a.stream, b.stream) and torch.equal(a.offsets, b.offsets) and a.planes is None and b.planes is None
    ones = batch.compress(ts, planes=1)
    assert torch.equal(a.stream, ones.stream) and ones.planes == [1] * len(ts)
    assert ones.gip(0) == a.gip(0)


def test_a_width_of_3_raises_through_bad_batch(H):
    from gpuar_amd import batch
    ts = typed_tensors()[:3]
    with pytest.raises(H.GpuarError, match="BAD_BATCH"):
        batch.compress(ts, planes=[2, 3, 4])
    with pytest.raises(H.GpuarError):
        batch.compress(ts, planes=[2, 2])
    with pytest.raises(H.GpuarError):
        batch.compress(ts, planes="always")


# ---- checksums --------------------------------------------------------------------------------------------------------

def test_checksums_are_those_of_the_original_bytes_and_catch_a_flipped_bit(H):
    from gpuar_amd import batch
    ts = typed_tensors()
    c = batch.compress(ts, planes="auto", checksum=True)
    want = [zlib.crc32(raw(t)[p * PACKET:(p + 1) * PACKET].tobytes()) for t in ts for p in range((raw(t).size + PACKET - 1) // PACKET)]
    assert [v & 0xFFFFFFFF for v in c.crc32.cpu().tolist()] == want
    for o, t in zip(batch.decompress(c), ts):
        assert (o.cpu().numpy() == raw(t)).all()
    # one flipped bit in the stream of buffer 2 (fp32, width 4), split packet 5: a byte plane of the group of packets 4 .. 7
    b, j, w = 2, 5, 4
    off = c._offsets_host()
    p = c.first_packet[b] + j
    for at in range(off[p] + 12, off[p + 1] - 8, 41):
        bad = batch.Compressed(stream=c.stream.clone(), offsets=c.offsets, first_packet=c.first_packet, sizes=c.sizes, crc32=c.crc32, planes=c.planes)
        bad.stream[at] ^= 0x08
        try:
            out = batch.decompress(bad, verify=False)
        except H.GpuarError:
            continue
        if not (out[b].cpu().numpy() == raw(ts[b])).all():
            break
    else:
        pytest.fail("no flip decodes to wrong bytes")
    with pytest.raises(H.GpuarError, match=r"checksum mismatch: buffer 2, packet (\d+) ") as e:
        batch.decompress(bad)
    named = int(e.value.args[0].split("packet ")[1].split(" ")[0])
    assert j // w * w <= named < j // w * w + w, (named, e.value)


# ---- the command line on the GPU --------------------------------------------------------------------------------------

def _run(cli, *args):
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1")
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (args, r.stdout, r.stderr)


@pytest.mark.parametrize("w", [2, 8])
def test_cli_planes_on_the_gpu_writes_the_file_gpuar_host_writes(H, tmp_path, w):
    from gpuar_amd import batch
    n = 1000 * PACKET + 4099
    data = R.typed_input("bf16", n + 1, seed=w)[:n]
    src = tmp_path / "in.dat"
    data.tofile(src)
    _run(HOST_CLI, "c", "--host", "--checksum", f"--planes={w}", "--threads", "16", f"--in={src}", f"--out={tmp_path / 'h.gip'}")
    want = (tmp_path / "h.gip").read_bytes()
    end = struct.unpack_from("<Q", want, 12)[0]
    assert struct.unpack_from("<4sIQII", want, end) == (b"GIPX", 3, (n + PACKET - 1) // PACKET, w, 1)
    for extra in ((), ("--batch=100",), ("--batch", "64", "--index")):
        _run(CLI, "c", "--checksum", f"--planes={w}", *extra, f"--in={src}", f"--out={tmp_path / 'g.gip'}")
        assert (tmp_path / "g.gip").read_bytes() == want, extra
        for d_extra in ((), ("--batch=100",), ("--host",)):
            _run(CLI, "d", *d_extra, f"--in={tmp_path / 'g.gip'}", f"--out={tmp_path / 'back.dat'}")
            assert (tmp_path / "back.dat").read_bytes() == data.tobytes(), (extra, d_extra)
    # without CRCs: the same packets, a trailer without the CRC array
    _run(CLI, "c", f"--planes={w}", "--batch=100", f"--in={src}", f"--out={tmp_path / 'n.gip'}")
    plain = (tmp_path / "n.gip").read_bytes()
    assert plain[:end] == want[:end] and struct.unpack_from("<4sIQII", plain, end) == (b"GIPX", 3, (n + PACKET - 1) // PACKET, w, 0)
    _run(CLI, "d", f"--in={tmp_path / 'n.gip'}", f"--out={tmp_path / 'back.dat'}")
    assert (tmp_path / "back.dat").read_bytes() == data.tobytes()
    # Compressed.gip(b) is that file
    t = torch.from_numpy(data).cuda()
    assert batch.compress([t], planes=w, checksum=True).gip(0) == want
    assert batch.compress([t], planes=w).gip(0) == plain


@pytest.mark.parametrize("w", [2, 4, 8])
def test_cli_planes_on_the_gpu_at_small_sizes(H, tmp_path, w):
    """Nothing, less than an element, less than a packet, one group exactly and one byte more: one chunk, the tail paths."""
    for n in (0, 1, w - 1, 8191, w * PACKET, w * PACKET + 1, 70 * PACKET + 13):
        data = data_for(n, 31 * w + n % 101)
        src = tmp_path / "in.dat"
        data.tofile(src)
        _run(HOST_CLI, "c", "--host", "--checksum", f"--planes={w}", f"--in={src}", f"--out={tmp_path / 'h.gip'}")
        _run(CLI, "c", "--checksum", f"--planes={w}", f"--in={src}", f"--out={tmp_path / 'g.gip'}")
        assert (tmp_path / "g.gip").read_bytes() == (tmp_path / "h.gip").read_bytes(), (w, n)
        _run(CLI, "d", f"--in={tmp_path / 'g.gip'}", f"--out={tmp_path / 'back.dat'}")
        assert (tmp_path / "back.dat").read_bytes() == data.tobytes(), (w, n)


def test_gpu_decode_refuses_unusable_planes_trailers_and_catches_damage(H, tmp_path):
    n = 200 * PACKET + 100
    data = R.typed_input("fp32", n + 4, seed=9)[:n]
    src, gip = tmp_path / "in.dat", tmp_path / "g.gip"
    data.tofile(src)
    _run(CLI, "c", "--checksum", "--planes=4", "--batch=64", f"--in={src}", f"--out={gip}")
    good = gip.read_bytes()
    end = struct.unpack_from("<Q", good, 12)[0]
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1")

    def decode(blob):
        (tmp_path / "bad.gip").write_bytes(bytes(blob))
        return subprocess.run([CLI, "d", "--batch=64", f"--in={tmp_path / 'bad.gip'}", f"--out={tmp_path / 'bad.out'}"], capture_output=True, text=True,
                              timeout=300, env=env)
    for at, value in ((end + 16, 3), (end + 20, 3)):                          # the width, an unknown flag
        bad = bytearray(good)
        struct.pack_into("<I", bad, at, value)
        r = decode(bad)
        assert r.returncode == 1 and "byte planes" in r.stderr, (at, r.returncode, r.stderr)
        assert (tmp_path / "bad.out").read_bytes() == b""
    bad = bytearray(good)
    struct.pack_into("<H", bad, end + 24, struct.unpack_from("<H", bad, end + 24)[0] + 1)
    assert decode(bad).returncode == 1
    bad = bytearray(good)
    struct.pack_into("<H", bad, 20 + 2, 8191)                                 # packet 0 says it holds 8191 bytes
    r = decode(bad)
    assert r.returncode == 1 and "packet 0" in r.stderr, r.stderr
    # a flipped bit deep in the stream: caught by the CRCs of the merged bytes, named within the damaged packet's group
    clens = struct.unpack_from("<200H", good, end + 24)
    p = 133
    for shift in range(0, 400, 7):
        bad = bytearray(good)
        bad[20 + sum(clens[:p]) + clens[p] // 2 + shift] ^= 0x04
        r = decode(bad)
        if r.returncode == 1 and "Checksum mismatch" in r.stderr:
            named = int(r.stderr.split("Checksum mismatch: packet ")[1].split(" ")[0])
            assert p // 4 * 4 <= named < p // 4 * 4 + 4, r.stderr
            break
        assert r.returncode == 0 and (tmp_path / "bad.out").read_bytes() == data.tobytes(), r.stderr      # (a flip in bits nobody decodes)
    else:
        pytest.fail("no flip was caught")
