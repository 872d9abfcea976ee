"""The XOR-base kernels on the MI355X: gpuar_hip_split_xor / merge_xor and their batch forms against the host definitions of
gpuar_amd/csrc/xorbase.h (themselves checked against numpy in tests/test_xor_host.py).  Every device buffer has canary bytes
behind what a call may write -- and behind what it may read of buffer and base, which end mid-quad -- and every status word is
read."""
import numpy as np
import pytest

import xor_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
GUARD = 256


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


def guarded(host: np.ndarray, fill):
    t = torch.full((host.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    t[:host.size] = torch.from_numpy(host).cuda()
    return t


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def host_split(H, x, b, w):
    return np.frombuffer(H.split_xor_host(x.tobytes(), b.tobytes(), w), dtype=np.uint8)


# ---- one buffer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", X.WIDTHS)
def test_single_buffer_split_and_merge_against_the_host_definitions(H, w):
    """Every length of the grid: below a quad, across a packet, a group and with a tail; buffer and base both end mid-quad."""
    for n in X.lengths_for(w):
        x, b = X.pair(n, seed=1000 * w + n % 997)
        want = host_split(H, x, b, w)
        assert (want == X.numpy_split_xor(x, b, w)).all()
        d_in, d_base = guarded(x, 0xA5), guarded(b, 0xC3)
        d_out = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        H.split_xor(d_in, d_base, w, d_out=d_out, n_bytes=n)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:n] == want).all(), (w, n, int(np.flatnonzero(got[:n] != want)[0]))
        assert (got[n:] == 0x5A).all(), (w, n, "split wrote behind n")
        assert (d_in.cpu().numpy()[:n] == x).all() and (d_in[n:] == 0xA5).all(), (w, n, "split changed its input")
        assert (d_base.cpu().numpy()[:n] == b).all() and (d_base[n:] == 0xC3).all(), (w, n, "split changed its base")
        # merge, out of place
        d_back = torch.full((n + GUARD,), 0x3C, dtype=torch.uint8, device="cuda")
        H.merge_xor(d_out, d_base, w, d_out=d_back, n_bytes=n)
        torch.cuda.synchronize()
        back = d_back.cpu().numpy()
        assert (back[:n] == x).all(), (w, n, int(np.flatnonzero(back[:n] != x)[0]))
        assert (back[n:] == 0x3C).all(), (w, n, "merge wrote behind n")
        # merge and split, in place
        H.merge_xor(d_out, d_base, w, d_out=d_out, n_bytes=n)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:n] == x).all(), (w, n, "merge in place")
        assert (got[n:] == 0x5A).all(), (w, n, "merge in place wrote behind n")
        H.split_xor(d_out, d_base, w, d_out=d_out, n_bytes=n)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:n] == want).all() and (got[n:] == 0x5A).all(), (w, n, "split in place")
        assert (d_base.cpu().numpy()[:n] == b).all() and (d_base[n:] == 0xC3).all(), (w, n, "the base was changed")


def test_more_groups_than_resident_workgroups_and_a_tail(H):
    """1100 groups of w = 8 (8800 workgroups, more than the chip holds at once) and a tail of 3 packets and 5 bytes, one launch."""
    w, n = 8, 1100 * 8 * PACKET + 3 * PACKET + 5
    x, b = X.pair(n, seed=77)
    want = X.numpy_split_xor(x, b, w)
    d_in, d_base = guarded(x, 0xA5), guarded(b, 0xC3)
    d_out = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    H.split_xor(d_in, d_base, w, d_out=d_out, n_bytes=n)
    assert torch.equal(d_out[:n], torch.from_numpy(want).cuda()) and bool((d_out[n:] == 0x5A).all())
    H.merge_xor(d_out, d_base, w, d_out=d_out, n_bytes=n)
    assert torch.equal(d_out[:n], d_in[:n]) and bool((d_out[n:] == 0x5A).all())
    assert torch.equal(d_base[:n], torch.from_numpy(b).cuda()) and bool((d_base[n:] == 0xC3).all())
    assert H.status() == 0


def test_single_buffer_error_codes_write_nothing(H):
    lib = H.load()
    d = torch.zeros(8 * PACKET + 64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    base = p + 6 * PACKET
    for fn in (lib.gpuar_hip_split_xor, lib.gpuar_hip_merge_xor):
        assert fn(p + 4, base, PACKET, 2, p + 2 * PACKET, None) == -1          # GPUAR_ERR_ALIGNMENT
        assert fn(p, base, PACKET, 2, p + 2 * PACKET + 8, None) == -1
        assert fn(p, base + 8, PACKET, 2, p + 2 * PACKET, None) == -1          # a misaligned base
        assert fn(p, base, PACKET, 3, p + 2 * PACKET, None) == -2              # GPUAR_ERR_ARGUMENT: the width
        assert fn(p, None, PACKET, 2, p + 2 * PACKET, None) == -2              # a null base
        assert fn(p, base, 2 * PACKET, 2, p + PACKET, None) == -2              # partial overlap of in and out
        assert fn(p + PACKET, base, 2 * PACKET, 2, p, None) == -2
        assert fn(p, p + 3 * PACKET, 2 * PACKET, 2, p + 2 * PACKET, None) == -2      # the base overlaps the output
        assert fn(p, p, PACKET, 2, p, None) == -2
        assert fn(p, base, 0, 2, p, None) == 0
    torch.cuda.synchronize()
    assert int(d.count_nonzero().item()) == 0
    with pytest.raises(H.GpuarError):
        H.split_xor(d, d[6 * PACKET:], 3)
    with pytest.raises(H.GpuarError):
        H.split_xor(d, d[:100], 2)                                             # a base shorter than the buffer


# ---- batches ----------------------------------------------------------------------------------------------------------

def _layout(sizes):
    at, offs = 0, []
    for n in sizes:
        offs.append(at)
        at += (n + GUARD + 15) // 16 * 16
    return offs, at


def test_a_batch_gives_what_its_buffers_give_alone(H):
    """65 buffers (the sizes of the survey's batch test), widths 1, 2, 4, 8, every third with a base and the others with a null base
    pointer, in one call: each gives what it gives alone, those without a base what split_planes_batch gives; canaries behind
    every output; merge in place restores."""
    rng = np.random.default_rng(5)
    sizes = [0, 1, 17, 3000, 8192, 8193, 8191, 16384, 0, 3 * 8192 + 5] + [int(v) for v in rng.integers(0, 40000, 53)] + [65536, 65537]
    assert len(sizes) == 65
    n = len(sizes)
    based = [i % 3 == 0 for i in range(n)]
    widths = [(1, 2, 4, 8)[(i // 3 if f else i) % 4] for i, f in enumerate(based)]
    assert {w for w, f in zip(widths, based) if f} == {w for w, f in zip(widths, based) if not f} == {1, 2, 4, 8}
    pairs = [X.pair(size, seed=3 * i + 1) for i, size in enumerate(sizes)]
    offs, at = _layout(sizes)
    src = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    bases = torch.full((at,), 0xC3, dtype=torch.uint8, device="cuda")
    for o, (x, b) in zip(offs, pairs):
        src[o:o + x.size] = torch.from_numpy(x).cuda()
        bases[o:o + b.size] = torch.from_numpy(b).cuda()
    src_before, bases_before = src.clone(), bases.clone()
    dst = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    fp, npk = H.batch_packet_count(sizes)
    desc = torch.tensor([src.data_ptr() + o for o in offs] + [dst.data_ptr() + o for o in offs] + sizes + fp + widths +
                        [bases.data_ptr() + o if f else 0 for o, f in zip(offs, based)], dtype=torch.int64, device="cuda")
    d_in, d_out, d_bytes, d_fp = desc[:n], desc[n:2 * n], desc[2 * n:3 * n], desc[3 * n:4 * n + 1]
    d_w, d_base = desc[4 * n + 1:5 * n + 1], desc[5 * n + 1:6 * n + 1]
    status = _status()
    H.split_xor_batch(d_in, d_bytes, d_fp, d_w, d_base, n, npk, d_out, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    plain = torch.full((at,), 0x5A, dtype=torch.uint8, device="cuda")
    H.split_planes_batch(d_in, d_bytes, d_fp, d_w, n, npk, d_out - dst.data_ptr() + plain.data_ptr(), d_status=status)
    assert int(status.item()) == 0
    planes = plain.cpu().numpy()
    for i, (o, (x, b), w, f) in enumerate(zip(offs, pairs, widths, based)):
        want = host_split(H, x, b, w) if f else planes[o:o + x.size]
        assert (got[o:o + x.size] == want).all(), (i, x.size, w, f)
        end = offs[i + 1] if i + 1 < n else at
        assert (got[o + x.size:end] == 0x5A).all(), (i, x.size, w, f, "wrote behind the buffer")
        if f and x.size:
            alone = H.split_xor(src[o:o + x.size], bases[o:o + x.size], w)
            assert (alone.cpu().numpy() == want).all(), (i, x.size, w)
    H.merge_xor_batch(d_out, d_bytes, d_fp, d_w, d_base, n, npk, d_out, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    for i, (o, (x, b)) in enumerate(zip(offs, pairs)):
        assert (got[o:o + x.size] == x).all(), (i, x.size, widths[i], based[i])
        end = offs[i + 1] if i + 1 < n else at
        assert (got[o + x.size:end] == 0x5A).all(), (i, "merge wrote behind the buffer")
    assert torch.equal(src, src_before) and torch.equal(bases, bases_before), "an input or a base changed"
    assert H.status() == 0


def test_a_misaligned_base_pointer_is_bad_batch_and_the_buffer_keeps_its_canary(H):
    sizes = [3 * PACKET, 2 * PACKET + 5, 4 * PACKET]
    src = torch.arange(16 * PACKET, device="cuda").to(torch.uint8)
    bases = (torch.arange(16 * PACKET + 64, device="cuda") * 7 + 3).to(torch.uint8)
    dst = torch.full((16 * PACKET,), 0x5A, dtype=torch.uint8, device="cuda")
    offs = [0, 4 * PACKET, 8 * PACKET]
    fp, npk = H.batch_packet_count(sizes)
    host, hbase = src.cpu().numpy(), bases.cpu().numpy()

    def call(fn, widths, base_offs, out_offs=offs):
        dst.fill_(0x5A)
        desc = torch.tensor([src.data_ptr() + o for o in offs] + [dst.data_ptr() + o for o in out_offs] + sizes + fp + widths +
                            [0 if o is None else bases.data_ptr() + o for o in base_offs], dtype=torch.int64, device="cuda")
        status = _status()
        fn(desc[0:3], desc[6:9], desc[9:13], desc[13:16], desc[16:19], 3, npk, desc[3:6], d_status=status)
        return int(status.item()), dst.cpu().numpy()

    def want(i, w, base_off):
        x = host[offs[i]:offs[i] + sizes[i]]
        return host_split(H, x, hbase[base_off:base_off + sizes[i]], w) if base_off is not None else np.frombuffer(H.split_planes_host(x.tobytes(), w), dtype=np.uint8)

    for fn in (H.split_xor_batch, H.merge_xor_batch):
        flags, got = call(fn, [2, 2, 4], [offs[0], offs[1] + 8, None])              # a base pointer that is not 16-byte aligned
        assert flags == H.STATUS_BAD_BATCH
        assert (got[offs[1]:offs[2]] == 0x5A).all(), "the buffer with the misaligned base was written"
        assert (got[offs[2] + sizes[2]:] == 0x5A).all()
        if fn is H.split_xor_batch:
            assert (got[:sizes[0]] == want(0, 2, offs[0])).all() and (got[offs[2]:offs[2] + sizes[2]] == want(2, 4, None)).all()
    flags, got = call(H.split_xor_batch, [2, 3, 4], offs)                           # a width of 3
    assert flags == H.STATUS_BAD_BATCH and (got[offs[1]:offs[2]] == 0x5A).all()
    flags, got = call(H.split_xor_batch, [2, 2, 4], offs, [offs[0], offs[1] + 8, offs[2]])      # a misaligned output pointer
    assert flags == H.STATUS_BAD_BATCH and (got[offs[1]:offs[2]] == 0x5A).all()
    flags, got = call(H.split_xor_batch, [2, 2, 4], [offs[0], offs[1] + 16, None])  # aligned: fine, wherever the base lies
    assert flags == 0
    for i, (w, o) in enumerate(zip([2, 2, 4], [offs[0], offs[1] + 16, None])):
        assert (got[offs[i]:offs[i] + sizes[i]] == want(i, w, o)).all(), i
    assert (got[offs[1] + sizes[1]:offs[2]] == 0x5A).all()
    assert H.status() == 0
