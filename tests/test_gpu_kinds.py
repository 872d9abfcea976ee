"""Raw and sparse packets in a packet stream on the MI355X: kinds_store and kinds_expand against the host functions of
gpuar_amd/csrc/kinds.h on the packet families of tests/kinds_ref.py, with canaries in every slot beyond clen, behind the kinds and
behind every destination, inconsistent scan words, packets at every residue mod 16 and every damaged form; `gpuar c` / `gpuar d` on
the GPU against `gpuar-host --host` in both directions, with chunks that end inside the file; and batch's gip(b, kinds=True)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import kinds_ref as K
import sparse_ref as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gpuar_amd", "bin")
PACKET, SLOT = 8192, 8704
GUARD = 64
OPTIONS = [(False, False), (True, False), (False, True), (True, True)]        # (stored, sparse)
LAST = ("text_n4095", "uniform_n4095", "ends_n4095", "zeros_n1", "uniform_n5", "text_n17", "zeros_n127", "ends_n129", "fill80_k65_n8191",
        "uniform_n8192")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def packets():
    return dict(K.packets())


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _i32(values):
    return torch.tensor([v if v < (1 << 31) else v - (1 << 32) for v in values], dtype=torch.int32, device="cuda")


def _buffer(parts):
    """(the bytes, a device tensor of exactly those bytes inside an allocation that ends with the 16-byte piece of its last byte)"""
    data = np.concatenate(parts)
    full = torch.full(((data.size + 15) // 16 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    full[:data.size] = torch.from_numpy(data).cuda()
    return data, full[:data.size]


def _full_packets(packets):
    return [x for _name, x in sorted(packets.items()) if x.size == PACKET]


# ---- kinds_store ------------------------------------------------------------------------------------------------------

def _encoded(H, d_in, n_packets):
    """the encoder's slots with 0x5A in every slot beyond the packet's clen and behind the last slot"""
    buf = torch.full((n_packets * SLOT + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    status = _status()
    H.encode(d_in, buf[:n_packets * SLOT], d_status=status)
    assert int(status.item()) == 0
    slots = buf[:n_packets * SLOT].view(n_packets, SLOT)
    clen = slots[:, 0].to(torch.int64) | slots[:, 1].to(torch.int64) << 8
    slots[torch.arange(SLOT, device="cuda")[None, :] >= clen[:, None]] = 0x5A
    return buf


def _check_store(H, parts, stored, sparse, stream=None):
    data, d_in = _buffer(parts)
    n_packets = len(parts)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        buf = _encoded(H, d_in, n_packets)
        before = buf.cpu().numpy().copy()
        d_est = H.estimate(d_in, stream=stream)
        d_scan = H.sparse_scan(d_in, stream=stream) if sparse else None
        kinds = torch.full((n_packets + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        status = _status()
        H.kinds_store(d_in, d_est, d_scan, stored, buf[:n_packets * SLOT], d_kind=kinds[:n_packets], stream=stream, d_status=status)
        if stream is not None:
            stream.synchronize()
    assert int(status.item()) == 0
    after, got_kinds = buf.cpu().numpy(), kinds.cpu().numpy()
    assert (got_kinds[n_packets:] == 0x5A).all(), "wrote behind d_kind"
    assert (after[n_packets * SLOT:] == 0x5A).all(), "wrote behind the last slot"
    for p, x in enumerate(parts):
        kind, pkt = H.kinds_store_host(x.tobytes(), stored, sparse)
        slot, was = after[p * SLOT:(p + 1) * SLOT], before[p * SLOT:(p + 1) * SLOT]
        assert got_kinds[p] == kind == K.kind_of(x, stored, sparse), (p, x.size)
        if kind == K.CODED:
            assert (slot == was).all(), (p, "a coded packet's slot is the encoder's")
        else:
            assert slot[:len(pkt)].tobytes() == pkt, (p, x.size, kind)
            assert (slot[len(pkt):] == was[len(pkt):]).all(), (p, "wrote beyond slot + clen")
    assert (d_in.cpu().numpy() == data).all()
    return set(got_kinds[:n_packets].tolist())


@pytest.mark.parametrize("stored,sparse", OPTIONS)
def test_store_writes_the_hosts_packets_and_nothing_else(H, packets, stored, sparse):
    full = _full_packets(packets)
    assert len(full) > 25
    side = torch.cuda.Stream()
    seen = set()
    for i, last in enumerate(LAST):                          # one buffer per last packet: short, of every kind, and a full one
        seen |= _check_store(H, full[i % 3::3] + [packets[last]], stored, sparse, stream=side if i % 2 else None)
    assert seen == {K.CODED} | ({K.RAW} if stored else set()) | ({K.SPARSE} if sparse else set())


def test_an_inconsistent_scan_is_bad_batch_and_leaves_the_slot(H, packets):
    """The estimates say "anything is smaller than coded" (5000, and 20000 for the last but one), so a scan word decides alone."""
    most = np.zeros(PACKET, dtype=np.uint8)
    most[np.arange(4095) * 2 + 1] = 1 + np.arange(4095) % 255                 # 4095 exceptions: a record of 12 292 bytes, no slot holds it
    parts = [packets["zeros_n8192"], packets["fill80_k64_n8192"], packets["text_n8192"], packets["fill00_k1_n8192"], packets["zeros_n8192"],
             packets["fillff_k128_n8192"], most, S.GOOD]
    other = int(S.GOOD[5])
    scans = [(1 << 8) | 0x00,                                # one exception that is not there
             (64 << 8) | 0x81,                               # another fill: 8192 exceptions
             S.NONE,                                         # no majority: coded, and no complaint
             (1 << 8) | 0x00,                                # right
             0x00,                                           # right
             (127 << 8) | 0xFF,                              # one too few
             (4095 << 8) | 0x00,                             # right, and longer than a slot
             (299 << 8) | other]                             # the count is right, the fill is no majority
    want = [K.CODED, K.CODED, K.CODED, K.SPARSE, K.SPARSE, K.CODED, K.CODED, K.CODED]
    assert [S.scan(x) for x in parts][3:5] == scans[3:5] and S.scan(most) == scans[6]
    data, d_in = _buffer(parts)
    n = len(parts)
    buf = _encoded(H, d_in, n)
    before = buf.cpu().numpy().copy()
    kinds = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    status = _status()
    H.kinds_store(d_in, _i32([5000] * 6 + [20000, 5000]), _i32(scans), False, buf[:n * SLOT], d_kind=kinds[:n], d_status=status)
    assert int(status.item()) == H.STATUS_BAD_BATCH
    after, got = buf.cpu().numpy(), kinds.cpu().numpy()
    assert got[:n].tolist() == want and (got[n:] == 0x5A).all() and (after[n * SLOT:] == 0x5A).all()
    for p, x in enumerate(parts):
        slot, was = after[p * SLOT:(p + 1) * SLOT], before[p * SLOT:(p + 1) * SLOT]
        if want[p] == K.CODED:
            assert (slot == was).all(), p
        else:
            pkt = K.store(x, False, True)[1]
            assert slot[:len(pkt)].tobytes() == pkt and (slot[len(pkt):] == was[len(pkt):]).all(), p


# ---- kinds_expand -----------------------------------------------------------------------------------------------------

def _filler(length):
    """a coded packet of `length` bytes as far as anybody but the decoder can tell: its header and bytes nobody reads"""
    return struct.pack("<HH", length, PACKET) + bytes([0xC3]) * (length - 4)


def _expand(H, stream_packets, kinds, n_bytes, shift=0, stream=None):
    """one kinds_expand launch over the packets laid back to back from byte `shift` of a 0x5A buffer; returns (status, output with
    its guard on the host)"""
    blob = b"".join(stream_packets)
    offsets = [shift]
    for pkt in stream_packets:
        offsets.append(offsets[-1] + len(pkt))
    d_stream = torch.full((shift + len(blob) + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    d_stream[shift:shift + len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_offsets = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    d_kind = torch.tensor(kinds, dtype=torch.uint8, device="cuda")
    out = torch.full((n_bytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    status = _status()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    H.kinds_expand(d_stream, d_offsets, d_kind, len(kinds), out, n_bytes, stream=stream, d_status=status)
    if stream is not None:
        stream.synchronize()
    return int(status.item()), out.cpu().numpy(), offsets


def test_expand_at_every_residue_against_the_host(H, packets):
    raws = [packets[f"uniform_n{PACKET}"], np.random.default_rng(8).integers(0, 256, PACKET, dtype=np.uint8)]
    sparses = [x for name, x in sorted(packets.items()) if x.size == PACKET and K.kind_of(x, False, True) == K.SPARSE]
    assert len(sparses) > 20
    side = torch.cuda.Stream()
    for turn, last in enumerate(LAST):
        stream_packets, kinds, plain, at, starts = [], [], [], 0, {K.RAW: set(), K.SPARSE: set()}
        for i in range(32):                                  # a filler, then a raw or a sparse packet that starts at residue i % 16
            x = raws[(i + turn) % 2] if i < 16 else sparses[(i + 7 * turn) % len(sparses)]
            kind, pkt = K.store(x, i < 16, i >= 16)
            assert kind == (K.RAW if i < 16 else K.SPARSE)
            length = 4 + 13 * i + turn
            length += (i % 16 - (at + length)) % 16          # the next packet starts at residue i % 16
            stream_packets += [_filler(length), pkt]
            at += length
            starts[kind].add(at % 16)
            at += len(pkt)
            kinds += [K.CODED, kind]
            plain += [None, x]
        assert starts[K.RAW] == starts[K.SPARSE] == set(range(16))
        x = packets[last]                                    # the stream's last packet: short, not coded, nothing behind it
        kind, pkt = K.store(x, True, True)
        if kind == K.CODED:
            kind, pkt = K.RAW, struct.pack("<HH", 4 + x.size, x.size) + x.tobytes()
        stream_packets.append(pkt)
        kinds.append(kind)
        plain.append(x)
        n_bytes = (len(kinds) - 1) * PACKET + x.size
        flags, out, offsets = _expand(H, stream_packets, kinds, n_bytes, stream=side if turn % 2 else None)
        assert flags == 0, (last, flags)
        for p, x in enumerate(plain):
            got = out[p * PACKET:p * PACKET + (PACKET if x is None else x.size)]
            if x is None:
                assert (got == 0x5A).all(), (last, p, "a coded packet's bytes are the decoder's")
            else:
                pkt = stream_packets[p]
                assert H.kinds_expand_host(pkt, kinds[p], x.size) == x.tobytes()
                assert (got == x).all(), (last, p, kinds[p], offsets[p] % 16)
        assert (out[n_bytes:] == 0x5A).all(), (last, "wrote behind the last packet")


def _bad_cases():
    return [d for d in K.damaged() if d[0] != "kind_0"]      # (kind 0 is the decoder's packet: skipped, not refused)


@pytest.mark.parametrize("name,pkt,kind,n", _bad_cases(), ids=[d[0] for d in _bad_cases()])
def test_expand_refuses_damaged_packets(H, packets, name, pkt, kind, n):
    """[a good raw packet][the damaged one, last in the stream], at an odd offset"""
    good = packets[f"uniform_n{PACKET}"]
    first = K.store(good, True, False)[1]
    flags, out, _offsets = _expand(H, [first, pkt], [K.RAW, kind], PACKET + n, shift=3)
    assert flags == H.STATUS_BAD_PACKET, (name, flags)
    assert (out[:PACKET] == good).all(), "the neighbour in front"
    assert (out[PACKET + n:] == 0x5A).all(), "wrote outside the packet"
    if kind != K.SPARSE:
        assert (out[PACKET:] == 0x5A).all(), "a raw packet that is refused leaves its destination alone"


def test_expand_refuses_a_full_packet_between_good_ones(H, packets):
    a, b, c = packets["fill80_k127_n8192"], packets[f"uniform_n{PACKET}"], packets[f"text_n{PACKET}"]
    pa, pb = K.store(a, False, True)[1], K.store(b, True, False)[1]
    pc = struct.pack("<HH", 4 + PACKET, PACKET) + c.tobytes()
    for name, bad, kind in (("raw clen", struct.pack("<HH", 4 + PACKET - 1, PACKET) + b.tobytes()[:-1], K.RAW),
                            ("raw ulen", struct.pack("<HH", 4 + PACKET, PACKET - 1) + b.tobytes(), K.RAW),
                            ("kind 3", pb, 3), ("kind 255", pb, 255),
                            ("sparse position", pa[:8] + struct.pack("<H", 0xFFFF) + pa[10:], K.SPARSE),
                            ("sparse as raw", pa, K.RAW), ("raw as sparse", pb, K.SPARSE)):
        assert K.expand(bad, kind, PACKET) is None, name
        flags, out, _o = _expand(H, [pa, bad, pc], [K.SPARSE, kind, K.RAW], 3 * PACKET, shift=5)
        assert flags == H.STATUS_BAD_PACKET, (name, flags)
        assert (out[:PACKET] == a).all() and (out[2 * PACKET:3 * PACKET] == c).all() and (out[3 * PACKET:] == 0x5A).all(), name
        if kind != K.SPARSE:
            assert (out[PACKET:2 * PACKET] == 0x5A).all(), name
    flags, out, _o = _expand(H, [pa, pb, pc], [K.SPARSE, K.RAW, K.RAW], 3 * PACKET, shift=5)
    assert flags == 0 and (out[:3 * PACKET] == np.concatenate([a, b, c])).all()
    # offsets that do not hold a header, run backwards or span more than a slot: refused before anything of the stream is read
    d_stream = torch.zeros(4 * SLOT, dtype=torch.uint8, device="cuda")
    for offsets in ([0, 3], [16, 8], [0, SLOT + 1]):
        out = torch.full((PACKET + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        status = _status()
        H.kinds_expand(d_stream, torch.tensor(offsets, dtype=torch.int64, device="cuda"), torch.tensor([1], dtype=torch.uint8, device="cuda"), 1, out, PACKET,
                       d_status=status)
        assert int(status.item()) == H.STATUS_BAD_PACKET and (out.cpu().numpy() == 0x5A).all(), offsets


# ---- files ------------------------------------------------------------------------------------------------------------

N_FILE = 300 * PACKET + 4097           # --batch=64: chunks of 64 packets, the last ragged; --batch=128: 128, 128 and 45


def run(exe, *args):
    return subprocess.run([os.path.join(BIN, exe), *args], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("stored,sparse", K.CLI_OPTIONS)
@pytest.mark.parametrize("content", K.CLI_CONTENTS)
def test_the_gpu_writes_and_reads_the_hosts_files(H, tmp_path, content, stored, sparse):
    x, base, flags, _how = K.cli_input(content, N_FILE)
    src = tmp_path / "in"
    x.tofile(src)
    if base is not None:
        base.tofile(tmp_path / "base")
        flags = flags + [f"--base={tmp_path / 'base'}"]
    based = [f"--base={tmp_path / 'base'}"] if base is not None else []
    flags = flags + K.cli_flags(stored, sparse)
    for batch, extra in (("--batch=64", []), ("--batch=128", ["--checksum"])):
        host, gpu, back = tmp_path / "host.gip", tmp_path / "gpu.gip", tmp_path / "back"
        r = run("gpuar-host", "c", "--host", "--threads=0", *flags, *extra, f"--in={src}", f"--out={host}")
        assert r.returncode == 0, r.stderr
        r = run("gpuar", "c", batch, *flags, *extra, f"--in={src}", f"--out={gpu}")
        assert r.returncode == 0, r.stderr
        assert gpu.read_bytes() == host.read_bytes(), (content, stored, sparse, batch)
        r = run("gpuar", "d", batch, *based, f"--in={host}", f"--out={back}")
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == x.tobytes(), (content, stored, sparse, batch)
    r = run("gpuar-host", "d", "--host", "--threads=0", *based, f"--in={gpu}", f"--out={back}")
    assert r.returncode == 0 and back.read_bytes() == x.tobytes(), r.stderr


def test_the_small_files_of_the_host_matrix(H, tmp_path):
    """the two sizes of tests/test_cli_kinds_host.py (one chunk each) with both options, and a damaged raw packet on the GPU"""
    for content in ("sorted_int32", "zeros", "text"):
        for n in K.CLI_SIZES:
            x, _base, flags, _how = K.cli_input(content, n)
            x.tofile(tmp_path / "in")
            flags = flags + K.cli_flags(True, True)
            assert run("gpuar-host", "c", "--host", *flags, f"--in={tmp_path / 'in'}", f"--out={tmp_path / 'host.gip'}").returncode == 0
            r = run("gpuar", "c", *flags, f"--in={tmp_path / 'in'}", f"--out={tmp_path / 'gpu.gip'}")
            assert r.returncode == 0, r.stderr
            assert (tmp_path / "gpu.gip").read_bytes() == (tmp_path / "host.gip").read_bytes(), (content, n)
            r = run("gpuar", "d", f"--in={tmp_path / 'host.gip'}", f"--out={tmp_path / 'back'}")
            assert r.returncode == 0 and (tmp_path / "back").read_bytes() == x.tobytes(), (content, n, r.stderr)
    x, _base, flags, _how = K.cli_input("uniform", K.CLI_SIZES[0])
    x.tofile(tmp_path / "in")
    assert run("gpuar-host", "c", "--host", "--stored=auto", f"--in={tmp_path / 'in'}", f"--out={tmp_path / 'raw.gip'}").returncode == 0
    blob = bytearray((tmp_path / "raw.gip").read_bytes())
    at = K.HEADER + 4 + PACKET + 100                         # a byte inside the second raw packet: decodes, to other bytes
    blob[at] ^= 1
    (tmp_path / "flipped.gip").write_bytes(bytes(blob))
    r = run("gpuar", "d", f"--in={tmp_path / 'flipped.gip'}", f"--out={tmp_path / 'back'}")
    assert r.returncode == 0 and (tmp_path / "back").read_bytes() != x.tobytes()
    blob[at] ^= 1
    blob[K.HEADER + 4 + PACKET + 2:K.HEADER + 4 + PACKET + 4] = struct.pack("<H", PACKET - 1)         # its ulen
    (tmp_path / "bad.gip").write_bytes(bytes(blob))
    (tmp_path / "back").write_bytes(b"left over")
    r = run("gpuar", "d", f"--in={tmp_path / 'bad.gip'}", f"--out={tmp_path / 'back'}")
    assert r.returncode == 1 and "Incorrect file format" in r.stderr and (tmp_path / "back").read_bytes() == b"", (r.returncode, r.stderr)


# ---- batch ------------------------------------------------------------------------------------------------------------

def test_gip_with_kinds_is_the_hosts_file(H, tmp_path):
    from gpuar_amd import batch
    n = 20 * PACKET + 4096
    equal, base_bytes, _f, _h = K.cli_input("bf16_base_equal", n)
    near, near_base, _f, _h = K.cli_input("bf16_base_0.1%", n)
    plain, _b, _f, _h = K.cli_input("bf16", n)
    uniform, _b, _f, _h = K.cli_input("uniform", n)

    def bf16(a):
        return torch.from_numpy(a.copy()).cuda().view(torch.bfloat16)

    tensors = [bf16(equal), bf16(near), bf16(plain), torch.from_numpy(uniform.copy()).cuda()]
    bases = [bf16(base_bytes), bf16(near_base), None, None]
    c = batch.compress(tensors, planes="auto", base=bases, stored="auto", sparse="auto", checksum=True)
    assert c.planes == [2, 2, 2, 1] and c.based == [True, True, False, False]
    got = batch.decompress(c, base=bases)
    for b, (data, base) in enumerate(((equal, base_bytes), (near, near_base), (plain, None), (uniform, None))):
        assert (got[b].cpu().numpy() == data).all()
        data.tofile(tmp_path / "in")
        flags = [f"--planes={c.planes[b]}", "--stored=auto", "--sparse=auto", "--checksum"]
        if base is not None:
            base.tofile(tmp_path / "base")
            flags.append(f"--base={tmp_path / 'base'}")
        r = run("gpuar-host", "c", "--host", *flags, f"--in={tmp_path / 'in'}", f"--out={tmp_path / 'host.gip'}")
        assert r.returncode == 0, r.stderr
        assert c.gip(b, kinds=True) == (tmp_path / "host.gip").read_bytes(), b
        with pytest.raises(H.GpuarError):                    # every buffer here holds a raw or a sparse packet: no file without kinds
            c.gip(b)
    plain_batch = batch.compress(tensors[2:], planes="auto", checksum=True)
    with pytest.raises(H.GpuarError):
        plain_batch.gip(0, kinds=True)
    listed = batch.compress(tensors[3:], stored=[True] + [False] * 20)
    with pytest.raises(H.GpuarError):
        listed.gip(0, kinds=True)
    with pytest.raises(H.GpuarError):
        listed.gip(0)
    only_stored = batch.compress(tensors[2:3], planes=2, stored="auto")
    plain.tofile(tmp_path / "in")
    assert run("gpuar-host", "c", "--host", "--planes=2", "--stored=auto", f"--in={tmp_path / 'in'}", f"--out={tmp_path / 'host.gip'}").returncode == 0
    assert only_stored.gip(0, kinds=True) == (tmp_path / "host.gip").read_bytes()


# ---- one object, many jobs --------------------------------------------------------------------------------------------

def test_one_gpu_object_through_jobs_with_and_without_kinds(H, tmp_path):
    """tests/kinds_client.cpp: the lanes of one GPUCompressor are reused by a decompress behind a compress and the other way
    round, with the two options on and off"""
    import client_build as B
    B.ensure_products()
    host = os.path.join(ROOT, "gpuar_amd", "csrc", "host")
    exe = B._make("kinds_client", [os.path.join(ROOT, "tests", "kinds_client.cpp")] +
                  [os.path.join(host, f) for f in ("compressor.cpp", "cpu_compressor.cpp", "gpu_compressor.cpp")], B.GPUFLAGS, B.GPULIBS,
                  [os.path.join(ROOT, "gpuar_amd", "lib", "libgpuar_hip.so"), os.path.join(ROOT, "gpuar_amd", "csrc", "kinds.h")])
    parts = [K.cli_input(content, 50 * PACKET)[0] for content in ("zeros", "uniform", "text")] + [K.cli_input("zeros", 4097)[0]]
    np.concatenate(parts).tofile(tmp_path / "in")
    r = subprocess.run([exe, str(tmp_path / "in"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1] == "ok", (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert run("gpuar-host", "c", "--host", "--stored=auto", "--sparse=auto", f"--in={tmp_path / 'in'}", f"--out={tmp_path / 'host.gip'}").returncode == 0
    assert (tmp_path / "a.gip").read_bytes() == (tmp_path / "host.gip").read_bytes()
