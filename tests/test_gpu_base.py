"""batch.compress(base=...) / decompress / estimate and `gpuar c|d --base` on the MI355X.  The exact oracle: compressing tensors
against bases gives the stream and offsets of compressing the XORed tensors without one.  Every documented refusal is raised
before any launch; every status word is read by the calls under test."""
import os
import struct
import subprocess

import numpy as np
import pytest

import planes_ref as R
import xor_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")
HOST_CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar-host")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


def raw(t):
    """the tensor's bytes on the host"""
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1) if t.numel() else np.empty(0, dtype=np.uint8)


def close_pair(n_bytes, seed, step=1e-4):
    """(tensor, base) of n_bytes bytes each, uint8 views of bf16 weights a small step apart"""
    rng = np.random.default_rng(seed)
    weights = rng.standard_normal(n_bytes // 2 + 1).astype(np.float32) * np.float32(0.02)
    b = X.bf16(weights).view(np.uint8)[:n_bytes].copy()
    x = X.bf16(weights + rng.standard_normal(weights.size).astype(np.float32) * np.float32(step)).view(np.uint8)[:n_bytes].copy()
    return torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()


@pytest.fixture(scope="module")
def batch_of_pairs(H):
    """(tensors, bases): groups and tails, one tensor without a base, an empty one, one of 3000 bytes, a typed one"""
    sizes = [5 * PACKET + 333, 2 * 2 * PACKET, 0, 3000, 3 * PACKET + 1, 8191, 7 * PACKET + 16]
    pairs = [close_pair(n, seed=20 + i) for i, n in enumerate(sizes)]
    xs, bs = [p[0] for p in pairs], [p[1] for p in pairs]
    bs[4] = None                                                                    # coded as it is
    xs[6], bs[6] = xs[6].view(torch.bfloat16), bs[6].view(torch.bfloat16)         # a typed tensor and its typed base
    return xs, bs


def xored(xs, bs):
    return [x if b is None else (x.view(torch.uint8) ^ b.view(torch.uint8)) for x, b in zip(xs, bs)]


def same_compressed(a, b):
    assert torch.equal(a.stream, b.stream) and torch.equal(a.offsets, b.offsets)
    assert a.first_packet == b.first_packet and a.sizes == b.sizes and a.planes == b.planes
    for name in ("stored", "raw", "raw_offsets"):
        p, q = getattr(a, name), getattr(b, name)
        assert (p is None) == (q is None) and (p is None or torch.equal(p, q)), name


@pytest.mark.parametrize("planes", [None, 2, "survey"])
@pytest.mark.parametrize("extra", [{}, {"checksum": True}, {"stored": "auto"}, {"checksum": True, "stored": "auto"}], ids=["plain", "crc", "stored", "crc+stored"])
def test_compress_against_bases_is_compress_of_the_xored_tensors(H, batch_of_pairs, planes, extra):
    from gpuar_amd import batch
    xs, bs = batch_of_pairs
    before = [raw(t).copy() for t in xs]
    bases_before = [None if b is None else raw(b).copy() for b in bs]
    c = batch.compress(xs, planes=planes, base=bs, **extra)
    assert c.based == [True, True, False, True, False, True, True] and c.delta is None      # (an empty tensor has nothing to XOR)
    if planes == "survey":
        assert c.planes == batch.survey_widths(xs, extra.get("stored"))             # the survey sees the ORIGINAL bytes
    else:
        assert c.planes == [planes or 1] * len(xs)
    want = batch.compress(xored(xs, bs), planes=c.planes, **{k: v for k, v in extra.items() if k != "checksum"})
    same_compressed(c, want)
    for t, h in zip(xs, before):
        assert (raw(t) == h).all(), "compress modified an input"
    for t, h in zip(bs, bases_before):
        assert t is None or (raw(t) == h).all(), "compress modified a base"
    if "checksum" in extra:                                                          # the CRCs are those of the original bytes
        assert torch.equal(c.crc32, batch.compress(xs, checksum=True).crc32)
    else:
        assert c.crc32 is None
    outs = batch.decompress(c, base=bs)
    for o, h in zip(outs, before):
        assert o.dtype == torch.uint8 and (o.cpu().numpy() == h).all()
    mine = [torch.empty_like(t) for t in xs]                                         # into the caller's tensors
    assert batch.decompress(c, out=mine, base=bs) is mine
    for o, t in zip(mine, xs):
        assert torch.equal(o, t)
    for t, h in zip(bs, bases_before):
        assert t is None or (raw(t) == h).all(), "decompress modified a base"


def test_base_none_takes_the_path_of_the_call_without_the_keyword(H, batch_of_pairs):
    from gpuar_amd import batch
    xs, bs = batch_of_pairs
    for planes in (None, 2):
        a, b = batch.compress(xs, planes=planes), batch.compress(xs, planes=planes, base=None)
        same_compressed(a, b)
        assert a.based is None and b.based is None
        none = batch.compress(xs, planes=planes, base=[None] * len(xs))
        assert torch.equal(a.stream, none.stream) and none.based == [False] * len(xs)
        for o, t in zip(batch.decompress(none), xs):
            assert (o.cpu().numpy() == raw(t)).all()


def test_a_wrong_base_is_the_checksum_mismatch_that_names_buffer_and_packet(H, batch_of_pairs):
    from gpuar_amd import batch
    xs, bs = batch_of_pairs
    c = batch.compress(xs, planes=2, base=bs, checksum=True)
    wrong = list(bs)
    wrong[0] = bs[0].clone()
    wrong[0][3 * PACKET + 77] ^= 0x10                                                # buffer 0, packet 3
    with pytest.raises(H.GpuarError, match=r"checksum mismatch: buffer 0, packet 3 \(batch packet 3\)"):
        batch.decompress(c, base=wrong)
    wrong = list(bs)
    wrong[6] = bs[6].clone()
    wrong[6].view(torch.uint8)[6 * PACKET + 5] ^= 0x01                               # buffer 6, a packet of its tail
    with pytest.raises(H.GpuarError, match=r"checksum mismatch: buffer 6, packet 6 "):
        batch.decompress(c, base=wrong)
    batch.decompress(c, base=wrong, verify=False)                                    # (unverified, the damage goes unnoticed)
    for o, t in zip(batch.decompress(c, base=bs), xs):
        assert (o.cpu().numpy() == raw(t)).all()


@pytest.fixture(scope="module")
def table(H):
    """the four 1 MiB pairs of base_auto's test, in its order, as (tensors, bases, widths)"""
    pairs = X.table_pairs()
    names = ["step_1e-4", "one_percent", "unrelated", "uniform"]
    return ([torch.from_numpy(pairs[k][0].copy()).cuda() for k in names], [torch.from_numpy(pairs[k][1].copy()).cuda() for k in names],
            [pairs[k][2] for k in names])


def test_base_auto_keeps_the_bases_that_pay_and_compresses_as_the_fixed_choice(H, table, monkeypatch):
    from gpuar_amd import batch
    xs, bs, widths = table
    assert all(t.numel() == 1 << 20 for t in xs)
    calls = {}
    for name in ("split_xor_batch", "split_planes_batch", "estimate_batch"):
        def counted(*a, _fn=getattr(batch.H, name), _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(batch.H, name, counted)
    # one split and one estimate launch more than fixed bases with stored="auto" take, and nothing is split a third time
    def launches(**kwargs):
        calls.clear()
        got = batch.compress(xs, planes=widths, **kwargs)
        assert got.based == [True, True, False, False]
        return got, tuple(calls.get(k, 0) for k in ("split_xor_batch", "split_planes_batch", "estimate_batch"))
    fixed_stored, n = launches(base=[bs[0], bs[1], None, None], stored="auto")
    assert n == (1, 0, 1)
    auto_stored, n = launches(base=bs, base_auto=True, stored="auto")
    assert n == (1, 1, 2)
    same_compressed(auto_stored, fixed_stored)
    assert launches(base=bs, base_auto=True)[1] == (1, 1, 2)
    calls.clear()
    batch.estimate(xs, planes=widths, base=bs, base_auto=True)
    assert calls == {"split_xor_batch": 1, "split_planes_batch": 1, "estimate_batch": 2}
    monkeypatch.undo()
    c = batch.compress(xs, planes=widths, base=bs, base_auto=True, checksum=True)
    assert c.based == [True, True, False, False]
    fixed = batch.compress(xs, planes=widths, base=[bs[0], bs[1], None, None], checksum=True)
    same_compressed(c, fixed)
    assert fixed.based == c.based and torch.equal(c.crc32, fixed.crc32)
    for o, t in zip(batch.decompress(c, base=bs), xs):
        assert torch.equal(o, t)
    for o, t in zip(batch.decompress(c, base=[bs[0], bs[1], None, None]), xs):      # the bases that were dropped are not needed
        assert torch.equal(o, t)
    plain = batch.compress(xs, planes=widths)
    assert c.nbytes < 0.7 * plain.nbytes
    auto = batch.estimate(xs, planes=widths, base=bs, base_auto=True)
    assert auto == batch.estimate(xs, planes=widths, base=[bs[0], bs[1], None, None])
    assert all(a <= p for a, p in zip(auto, batch.estimate(xs, planes=widths)))


def test_estimate_is_the_host_composition(H, batch_of_pairs, table):
    from gpuar_amd import batch
    for xs, bs, widths in (batch_of_pairs + ([2] * 7,), table):
        got = batch.estimate(xs, planes=widths, base=bs)
        want = [sum(H.estimate_host(R.numpy_split(raw(x), w).tobytes() if b is None else H.split_xor_host(raw(x).tobytes(), raw(b).tobytes(), w)))
                for x, b, w in zip(xs, bs, widths)]
        assert got == want
    xs, bs = batch_of_pairs
    assert batch.estimate(xs, base=bs) == batch.estimate(xored(xs, bs))              # no planes: a width of 1
    assert batch.estimate(xs, planes=2, base=bs, stored="auto") == batch.estimate(xored(xs, bs), planes=2, stored="auto")


def test_every_refusal_comes_before_any_launch(H, batch_of_pairs, monkeypatch):
    from gpuar_amd import batch
    xs, bs = batch_of_pairs
    good = batch.compress(xs, planes=2, base=bs)                                    # (without CRCs)
    checked = batch.compress(xs, planes=2, base=bs, checksum=True)

    def launched(*_a, **_k):
        raise AssertionError("a launch")
    for name in ("split_xor_batch", "merge_xor_batch", "split_planes_batch", "split_delta_batch", "encode_batch", "estimate_batch",
                 "survey_planes_batch", "decode_stream_batch", "crc32_batch", "move_packets"):
        monkeypatch.setattr(batch.H, name, launched)

    def bases_with(i, t):
        out = list(bs)
        out[i] = t
        return out
    shorter = bs[0][:-16]
    longer = torch.zeros(bs[0].numel() + 16, dtype=torch.uint8, device="cuda")
    misaligned = torch.zeros(bs[0].numel() + 16, dtype=torch.uint8, device="cuda")[8:8 + bs[0].numel()]
    strided = torch.zeros(2 * bs[0].numel(), dtype=torch.uint8, device="cuda")[::2]
    elsewhere = [bs[0].cpu()] + ([bs[0].to("cuda:1")] if torch.cuda.device_count() > 1 else [])
    for planes in (None, 2, "survey"):
        for call in (batch.compress, batch.estimate):
            for bad in [shorter, longer, misaligned, strided, "a string", 7] + elsewhere:
                with pytest.raises(H.GpuarError):
                    call(xs, planes=planes, base=bases_with(0, bad))
            with pytest.raises(H.GpuarError):
                call(xs, planes=planes, base=bs[:-1])                                # one entry per tensor
            with pytest.raises(H.GpuarError):
                call(xs, planes=planes, base=bs[0])                                  # a tensor is no list
            for delta in (True, False, "auto", [True] * len(xs)):
                with pytest.raises(H.GpuarError, match="delta"):
                    call(xs, planes=planes, base=bs, delta=delta)
            with pytest.raises(H.GpuarError):
                call(xs, planes=planes, base_auto=True)                              # nothing to choose from
    # decompress: a base for every buffer that was compressed against one
    with pytest.raises(H.GpuarError, match="base"):
        batch.decompress(good)
    with pytest.raises(H.GpuarError, match="base"):
        batch.decompress(good, base=bs[:-1])
    for bad in [None, shorter, longer, misaligned, strided] + elsewhere:
        with pytest.raises(H.GpuarError, match="base"):
            batch.decompress(good, base=bases_with(0, bad))
    out = [torch.empty(t.numel() * t.element_size(), dtype=torch.uint8, device="cuda") for t in xs]
    with pytest.raises(H.GpuarError, match="overlaps"):
        batch.decompress(good, out=out, base=bases_with(0, out[0]))
    both = torch.empty(out[0].numel() + out[1].numel() + 64, dtype=torch.uint8, device="cuda")
    out[0] = both[:out[0].numel()]
    with pytest.raises(H.GpuarError, match=r"base\[1\] overlaps out\[0\]"):        # a base inside ANOTHER buffer's output
        batch.decompress(good, out=out, base=bases_with(1, both[16:16 + out[1].numel()]))
    for bad in elsewhere[:1]:
        with pytest.raises(H.GpuarError, match=r"base\[0\] is on cpu"):             # the device is compared first
            batch.compress(xs, base=bases_with(0, bad))
        with pytest.raises(H.GpuarError, match=r"base\[0\] is on cpu"):
            batch.decompress(good, base=bases_with(0, bad))
    # the .gip form of a based buffer needs the CRCs
    with pytest.raises(H.GpuarError, match="checksum=True"):
        good.gip(0)
    assert good.gip(4)[:3] == b"\x00\x01\x00"                                        # (buffer 4 has no base: version 3 as ever)
    assert struct.unpack_from("<I", checked.gip(4), struct.unpack_from("<Q", checked.gip(4), 12)[0] + 4)[0] == 3
    monkeypatch.undo()
    assert torch.equal(batch.decompress(good, base=bs)[0], xs[0])


# ---- the container and the command line on the GPU --------------------------------------------------------------------

def _run(cli, *args, env=None, ok=True):
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1", **(env or {}))
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=600, env=env)
    if ok:
        assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


@pytest.fixture(scope="module")
def cli_files(H, tmp_path_factory):
    """(directory, input path, base path, tensor, base tensor): 1 MiB and a tail, and the files gpuar-host writes at widths 1 and 2"""
    d = tmp_path_factory.mktemp("gpu_base")
    x, b = close_pair((1 << 20) + 3 * PACKET + 4099, seed=9)
    raw(x).tofile(d / "in.dat")
    raw(b).tofile(d / "base.dat")
    for w in (1, 2):
        _run(HOST_CLI, "c", "--host", "--threads", "16", f"--base={d / 'base.dat'}", f"--planes={w}", f"--in={d / 'in.dat'}", f"--out={d / f'host{w}.gip'}")
    return d, d / "in.dat", d / "base.dat", x, b


@pytest.mark.parametrize("w", [1, 2])
def test_gip_of_a_based_buffer_is_the_file_gpuar_host_writes(H, cli_files, w):
    from gpuar_amd import batch
    d, _src, _base, x, b = cli_files
    want = (d / f"host{w}.gip").read_bytes()
    end = struct.unpack_from("<Q", want, 12)[0]
    assert struct.unpack_from("<4sIQII", want, end) == (b"GIPX", 5, (x.numel() + PACKET - 1) // PACKET, w, 5)
    c = batch.compress([x, x], planes=w, base=[b, None], checksum=True)
    assert c.gip(0) == want
    plain = c.gip(1)                                                                 # the buffer without a base: version 2 or 3 as ever
    assert struct.unpack_from("<I", plain, struct.unpack_from("<Q", plain, 12)[0] + 4)[0] == (3 if w > 1 else 2)


@pytest.mark.parametrize("w", [1, 2])
def test_cli_base_on_the_gpu_writes_the_hosts_file_and_reads_it_back(H, cli_files, tmp_path, w):
    d, src, base, x, _b = cli_files
    want = (d / f"host{w}.gip").read_bytes()
    env = {"GPUAR_OVERSUBSCRIBE_DEVICES": "1"}
    for tag, flags in (("one", []), ("batch", ["--batch=64"]), ("gpus", ["--gpus=2"])):
        gip = tmp_path / f"{tag}.gip"
        r = _run(CLI, "c", f"--base={base}", f"--planes={w}", *flags, f"--in={src}", f"--out={gip}", env=env)
        assert "Attention" not in r.stdout
        assert gip.read_bytes() == want, (w, flags)
    for flags in ([], ["--batch=64"], ["--gpus=2"], ["--host"]):
        back = tmp_path / "back.dat"
        _run(CLI, "d", f"--base={base}", *flags, f"--in={tmp_path / 'batch.gip'}", f"--out={back}", env=env)
        assert back.read_bytes() == raw(x).tobytes(), (w, flags)


def test_cli_on_the_gpu_refuses_what_the_host_refuses(H, cli_files, tmp_path):
    d, src, base, x, b = cli_files
    gip, out = d / "host2.gip", tmp_path / "out.dat"
    out.write_bytes(b"left over")
    r = _run(CLI, "d", "--batch=64", f"--in={gip}", f"--out={out}", ok=False)        # no base for a version-5 file
    assert r.returncode == 1 and "--base" in r.stderr and out.read_bytes() == b"", (r.returncode, r.stderr)
    wrong = raw(b).copy()
    wrong[70 * PACKET + 9] ^= 0x20
    wrong.tofile(tmp_path / "wrong.dat")
    r = _run(CLI, "d", "--batch=64", f"--base={tmp_path / 'wrong.dat'}", f"--in={gip}", f"--out={out}", ok=False)
    assert r.returncode == 1 and "Checksum mismatch: packet 70 " in r.stderr and out.read_bytes() == b"", (r.returncode, r.stderr)
    _run(CLI, "c", "--planes=2", "--checksum", f"--in={src}", f"--out={tmp_path / 'plain.gip'}")
    out.write_bytes(b"left over")
    r = _run(CLI, "d", f"--base={base}", f"--in={tmp_path / 'plain.gip'}", f"--out={out}", ok=False)      # a base for a plain file
    assert r.returncode == 1 and "--base" in r.stderr and out.read_bytes() == b"", (r.returncode, r.stderr)
    raw(b)[:-1].tofile(tmp_path / "short.dat")
    r = _run(CLI, "c", f"--base={tmp_path / 'short.dat'}", f"--in={src}", f"--out={tmp_path / 'never.gip'}", ok=False)
    assert r.returncode == 1 and "base" in r.stderr and (tmp_path / "never.gip").read_bytes() == b"", (r.returncode, r.stderr)
    r = _run(CLI, "c", "--delta", f"--base={base}", f"--in={src}", f"--out={tmp_path / 'never2.gip'}", ok=False)
    assert r.returncode == 2 and not (tmp_path / "never2.gip").exists()
