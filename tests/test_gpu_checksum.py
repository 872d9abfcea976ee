"""Per-packet CRC-32 kernels on the MI355X (gpuar_hip_crc32 / verify_crc32 and their batch forms), batch.compress /
decompress with checksum=True, Compressed.gip's version-2 trailer and `gpuar c|d --checksum` on the GPU.  zlib.crc32 is
the oracle throughout.  Every device buffer gets a canary behind what a call may write, and every status word is read."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import damage_sweep as DS
import length_sweep as LS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


def zcrcs(data: bytes, n=None):
    n = len(data) if n is None else n
    return [zlib.crc32(data[p * PACKET:min((p + 1) * PACKET, n)]) for p in range((n + PACKET - 1) // PACKET)]


def crc_list(t, n):
    return [v & 0xFFFFFFFF for v in t[:n].cpu().tolist()]


def device_crcs(H, host: np.ndarray):
    """gpuar_hip_crc32 of `host`'s bytes; checks the canary behind the n_packets values."""
    d = torch.from_numpy(host).cuda()
    npk = H.packet_count(host.size)
    out = torch.full((npk + 4,), CANARY, dtype=torch.int32, device="cuda")
    H.crc32(d, d_crc=out)
    torch.cuda.synchronize()
    assert out[npk:].eq(CANARY).all(), "gpuar_hip_crc32 wrote past n_packets"
    return crc_list(out, npk)


def test_single_packets_of_every_length(H):
    """One launch per length would be 8192 launches: the lengths go as a BATCH of 8192 one-packet buffers (each buffer's
    packet is a tail packet of its own length), and the 8192-byte one also through the single-buffer call."""
    pkts = LS.packets()
    host = np.zeros(PACKET * PACKET, dtype=np.uint8)
    for i, p in enumerate(pkts):
        host[i * PACKET:i * PACKET + p.size] = p
    d = torch.from_numpy(host).cuda()
    sizes = [p.size for p in pkts]
    ptrs = [d.data_ptr() + i * PACKET for i in range(PACKET)]
    fp, npk = H.batch_packet_count(sizes)
    desc = torch.tensor(ptrs + sizes + fp, dtype=torch.int64, device="cuda")
    d_ptrs, d_bytes, d_fp = desc[:PACKET], desc[PACKET:2 * PACKET], desc[2 * PACKET:]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((npk + 4,), CANARY, dtype=torch.int32, device="cuda")
    H.crc32_batch(d_ptrs, d_bytes, d_fp, PACKET, npk, d_crc=out, d_status=status)
    assert int(status.item()) == 0
    got = crc_list(out, npk)
    want = [zlib.crc32(p.tobytes()) for p in pkts]
    bad = [i + 1 for i in range(PACKET) if got[i] != want[i]]
    assert not bad, f"wrong CRC at lengths {bad[:20]} ({len(bad)} in all)"
    assert out[npk:].eq(CANARY).all()
    assert device_crcs(H, pkts[-1]) == want[-1:]


@pytest.mark.parametrize("residue", range(64))
def test_multi_packet_inputs_with_every_tail_residue(H, residue):
    n = 5 * PACKET + 64 * (residue * 37 % 128) + residue     # every residue mod 64, tails of 0 .. 8191 bytes
    host = LS.packet(((residue * 977) % PACKET) + 1)
    host = np.resize(np.concatenate([host, np.arange(997, dtype=np.uint8)]), n)
    assert device_crcs(H, host) == zcrcs(host.tobytes())


@pytest.mark.parametrize("model", range(6))
def test_source_models(H, model):
    """Inputs of 2 ... 7 packets made of one source model of length_sweep each."""
    lengths = [PACKET - ((PACKET - 1 - model) % 6) - 6 * k for k in range(model + 2)]      # lengths of this model near 8192
    assert all(LS.MODELS[(n - 1) % 6] == LS.MODELS[model] for n in lengths)
    host = np.concatenate([LS.packet(n) for n in lengths])
    assert device_crcs(H, host) == zcrcs(host.tobytes()), lengths


def test_batch_mixed_sizes_and_zero_byte_buffers(H):
    sizes = [0, 1, 8192, 0, 8193, 3 * 8192 + 17, 100, 0, 64 * 8192 + 5]
    hosts = [np.random.default_rng(i).integers(0, 256, n, dtype=np.uint8) for i, n in enumerate(sizes)]
    ts = [torch.from_numpy(h).cuda() for h in hosts]
    fp, npk = H.batch_packet_count(sizes)
    desc = torch.tensor([t.data_ptr() if t.numel() else 0 for t in ts] + sizes + fp, dtype=torch.int64, device="cuda")
    nb = len(sizes)
    d_ptrs, d_bytes, d_fp = desc[:nb], desc[nb:2 * nb], desc[2 * nb:]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((npk + 4,), CANARY, dtype=torch.int32, device="cuda")
    H.crc32_batch(d_ptrs, d_bytes, d_fp, nb, npk, d_crc=out, d_status=status)
    assert int(status.item()) == 0
    want = [c for h in hosts for c in zcrcs(h.tobytes())]
    assert crc_list(out, npk) == want and out[npk:].eq(CANARY).all()
    # verify: clean, then one byte changed in buffer 5's packet 2 and in buffer 8's packet 40
    first_bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    H.verify_crc32_batch(d_ptrs, d_bytes, d_fp, nb, npk, out, first_bad, d_status=status)
    assert int(status.item()) == 0 and int(first_bad.item()) == -1
    ts[8][40 * PACKET + 7] ^= 1
    ts[5][2 * PACKET + 16] ^= 0x80
    H.verify_crc32_batch(d_ptrs, d_bytes, d_fp, nb, npk, out, first_bad, d_status=status)
    assert int(status.item()) == H.STATUS_CHECKSUM
    assert int(first_bad.item()) == fp[5] + 2


def test_batch_unusable_descriptors(H):
    """A misaligned buffer, and a first_packet that gives a buffer more packets than its bytes: BAD_BATCH, CRC untouched."""
    a = torch.arange(3 * PACKET, dtype=torch.int64, device="cuda").to(torch.uint8)
    sizes = [PACKET, 2 * PACKET]
    fp = [0, 1, 4]                                               # buffer 1 claims 3 packets, owns 2
    desc = torch.tensor([a.data_ptr() + 8, a.data_ptr() + PACKET] + sizes + fp, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    H.crc32_batch(desc[:2], desc[2:4], desc[4:], 2, 4, d_crc=out, d_status=status)
    assert int(status.item()) == H.STATUS_BAD_BATCH
    got = crc_list(out, 4)
    host = a.cpu().numpy().tobytes()
    assert got[0] == CANARY and got[3] == CANARY
    assert got[1:3] == [zlib.crc32(host[PACKET:2 * PACKET]), zlib.crc32(host[2 * PACKET:3 * PACKET])]


def test_verify_finds_exactly_the_packets_that_decode_wrong(H):
    """The damage_sweep packets decoded (slot form) into a pre-filled output, verified -- as a batch of one-packet buffers of
    the ORIGINAL lengths -- against the CRCs of the undamaged packets.  Which packets must fail is computed from the decoded
    bytes, not from "was damaged": a flip past the bits a packet uses can decode correctly."""
    from gpuar_amd import batch
    pkts = LS.packets()
    host = np.zeros(PACKET * PACKET, dtype=np.uint8)
    for i, p in enumerate(pkts):
        host[i * PACKET:i * PACKET + p.size] = p
    views = torch.from_numpy(host).cuda()
    ts = [views[i * PACKET:i * PACKET + p.size] for i, p in enumerate(pkts)]
    c = batch.compress(ts)                                       # every packet's clean encoding
    stream = c.stream.cpu().numpy()
    off = c._offsets_host()
    clean = {m: stream[off[m - 1]:off[m]] for m in range(1, PACKET + 1)}
    dpkts, _ = DS.sweep(lambda m: clean[m])
    slots = torch.from_numpy(DS.slot_form(dpkts)).cuda()
    out = torch.full((PACKET * PACKET,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    H.decode(slots, PACKET, d_out=out, d_status=status)
    torch.cuda.synchronize()
    sizes = [p.size for p in pkts]
    got = out.view(PACKET, PACKET).cpu().numpy()
    wrong = [i for i, p in enumerate(pkts) if not np.array_equal(got[i, :p.size], p)]
    fp, npk = H.batch_packet_count(sizes)
    desc = torch.tensor([out.data_ptr() + i * PACKET for i in range(PACKET)] + sizes + fp, dtype=torch.int64, device="cuda")
    want_crc = torch.tensor([zlib.crc32(p.tobytes()) - (1 << 32) * (zlib.crc32(p.tobytes()) >> 31) for p in pkts],
                            dtype=torch.int32, device="cuda")
    status.zero_()
    first_bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    H.verify_crc32_batch(desc[:PACKET], desc[PACKET:2 * PACKET], desc[2 * PACKET:], PACKET, npk, want_crc, first_bad, d_status=status)
    flags = int(status.item())
    assert 100 < len(wrong) < PACKET, len(wrong)
    assert flags == H.STATUS_CHECKSUM and int(first_bad.item()) == wrong[0], (flags, int(first_bad.item()), wrong[:5])
    # exactly those: each packet verified on its own
    recomputed = torch.empty(PACKET, dtype=torch.int32, device="cuda")
    H.crc32_batch(desc[:PACKET], desc[PACKET:2 * PACKET], desc[2 * PACKET:], PACKET, npk, d_crc=recomputed)
    mism = (recomputed != want_crc).nonzero().flatten().cpu().tolist()
    assert mism == wrong
    # a clean round trip reports nothing
    back = batch.decompress(c)
    assert all(torch.equal(b, t) for b, t in zip(back, ts))
    d_all = torch.from_numpy(np.concatenate(pkts[-3:])).cuda()
    crc = H.crc32(d_all)
    status.zero_()
    first_bad.fill_(-1)
    H.verify_crc32(d_all, crc, d_first_bad=first_bad, d_status=status)
    assert int(status.item()) == 0 and int(first_bad.item()) == -1


def test_batch_compress_checksum_round_trip_and_damage(H):
    from gpuar_amd import batch
    from gpuar_amd.hip import GpuarError
    sizes = [5 * PACKET + 3, 0, 777, 2 * PACKET]
    ts = [torch.from_numpy(LS.packet(PACKET)).cuda().repeat(6)[:n].clone() if n else torch.empty(0, dtype=torch.uint8, device="cuda")
          for n in sizes]
    ts[0][PACKET:] = torch.arange(ts[0].numel() - PACKET, device="cuda").to(torch.uint8)
    c = batch.compress(ts, checksum=True)
    assert c.crc32 is not None and c.crc32.numel() == c.n_packets
    assert crc_list(c.crc32, c.n_packets) == [v for t in ts for v in zcrcs(t.cpu().numpy().tobytes())]
    assert batch.compress(ts).crc32 is None
    back = batch.decompress(c)
    assert all(torch.equal(b, t) for b, t in zip(back, ts))
    # damage one body byte of buffer 3's packet 1 (batch packet 8): find a flip that decodes to wrong bytes
    off = c._offsets_host()
    p = c.first_packet[3] + 1
    for at in range(off[p] + 12, off[p + 1] - 8, 41):
        bad = batch.Compressed(stream=c.stream.clone(), offsets=c.offsets, first_packet=c.first_packet, sizes=c.sizes, crc32=c.crc32)
        bad.stream[at] ^= 0x08
        try:
            out = batch.decompress(bad, verify=False)
        except GpuarError:
            continue
        if not torch.equal(out[3], ts[3]):
            break
    else:
        pytest.fail("no flip decodes to wrong bytes")
    with pytest.raises(GpuarError, match=r"buffer 3, packet 1 \(batch packet 8\), bytes 8192 \.\. 16384 of 16384"):
        batch.decompress(bad)


def test_gip_with_trailer_decodes_with_gpuar_and_fails_once_damaged(H, tmp_path):
    from gpuar_amd import batch
    data = np.resize(LS.packet(4321), 3 * PACKET + 100)
    t = torch.from_numpy(data).cuda()
    c = batch.compress([t], checksum=True)
    blob = c.gip(0)
    gip = tmp_path / "a.gip"
    gip.write_bytes(blob)
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1")
    for extra in ((), ("--host",)):
        r = subprocess.run([CLI, "d", *extra, f"--in={gip}", f"--out={tmp_path / 'b.dat'}"], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "Warning" not in r.stderr, r.stderr
        assert (tmp_path / "b.dat").read_bytes() == data.tobytes()
    end = int.from_bytes(blob[12:20], "little")
    off = c._offsets_host()
    for at in range(20 + off[2] + 12, 20 + off[3] - 8, 29):
        bad = bytearray(blob)
        bad[at] ^= 0x20
        plain = tmp_path / "p.gip"
        plain.write_bytes(bytes(bad[:end]))
        r = subprocess.run([CLI, "d", "--host", f"--in={plain}", f"--out={tmp_path / 'p.dat'}"], capture_output=True, text=True, timeout=300)
        if r.returncode == 0 and (tmp_path / "p.dat").read_bytes() != data.tobytes():
            break
    else:
        pytest.fail("no flip decodes silently to wrong bytes")
    gip.write_bytes(bytes(bad))
    r = subprocess.run([CLI, "d", f"--in={gip}", f"--out={tmp_path / 'b.dat'}"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 1 and "Checksum mismatch: packet 2 (uncompressed bytes 16384 .. 24576)" in r.stderr, (r.stdout, r.stderr)


def test_cli_checksum_on_the_gpu_matches_the_host(H, tmp_path):
    rng = np.random.default_rng(9)
    data = np.concatenate([rng.integers(0, 256, 200 * PACKET, dtype=np.uint8), np.resize(LS.packet(8000), 300 * PACKET + 555)])
    src = tmp_path / "in.dat"
    data.tofile(src)
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1")

    def run(*args):
        r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (args, r.stdout, r.stderr)
    run("c", "--host", "--checksum", "--threads", "16", f"--in={src}", f"--out={tmp_path / 'h.gip'}")
    want = (tmp_path / "h.gip").read_bytes()
    for extra in (("--batch", "64"), ("--batch", "128", "--index"), ()):
        run("c", "--checksum", *extra, f"--in={src}", f"--out={tmp_path / 'g.gip'}")
        assert (tmp_path / "g.gip").read_bytes() == want, extra
        run("d", "--batch", "64", f"--in={tmp_path / 'g.gip'}", f"--out={tmp_path / 'back.dat'}")
        assert (tmp_path / "back.dat").read_bytes() == data.tobytes()
    # a damaged packet deep inside a multi-chunk decode
    end = int.from_bytes(want[12:20], "little")
    import struct
    n = struct.unpack_from("<Q", want, end + 8)[0]
    clens = struct.unpack_from(f"<{n}H", want, end + 16)
    p = 333
    at = 20 + sum(clens[:p]) + clens[p] // 2
    for shift in range(0, 200, 7):
        bad = bytearray(want)
        bad[at + shift] ^= 0x04
        (tmp_path / "p.gip").write_bytes(bytes(bad[:end]))
        r = subprocess.run([CLI, "d", "--batch", "64", f"--in={tmp_path / 'p.gip'}", f"--out={tmp_path / 'p.dat'}"], capture_output=True, text=True,
                           timeout=300, env=env)
        if r.returncode == 0 and (tmp_path / "p.dat").read_bytes() != data.tobytes():
            break
    else:
        pytest.fail("no flip decodes silently to wrong bytes")
    (tmp_path / "d.gip").write_bytes(bytes(bad))
    r = subprocess.run([CLI, "d", "--batch", "64", f"--in={tmp_path / 'd.gip'}", f"--out={tmp_path / 'd.dat'}"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 1 and f"Checksum mismatch: packet {p} (uncompressed bytes {p * PACKET} .. {(p + 1) * PACKET})" in r.stderr, r.stderr


def test_gip_is_what_the_cli_writes_with_checksum(H, tmp_path):
    """Compressed.gip(b) of a checksummed batch is byte for byte what `gpuar c --host --checksum` writes for buffer b's bytes
    (batch.trailer pinned to the C++ Trailer::save), for buffers of one packet, several and none."""
    from gpuar_amd import batch
    sizes = [3 * PACKET + 100, 0, 1, 2 * PACKET, 777]
    ts = [torch.from_numpy(np.resize(LS.packet(1000 + 7 * i), n)).cuda() if n else torch.empty(0, dtype=torch.uint8, device="cuda")
          for i, n in enumerate(sizes)]
    c = batch.compress(ts, checksum=True)
    for b, t in enumerate(ts):
        src, gip = tmp_path / f"in{b}.dat", tmp_path / f"out{b}.gip"
        src.write_bytes(t.cpu().numpy().tobytes())
        r = subprocess.run([CLI, "c", "--host", "--checksum", f"--in={src}", f"--out={gip}"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert c.gip(b) == gip.read_bytes(), b


@pytest.mark.parametrize("packets,batch_packets", [(3, None), (200, 64)])
def test_gpu_decode_catches_a_last_packet_ulen_flipped_to_zero(H, tmp_path, packets, batch_packets):
    """An input of whole packets: one flip (bit 5 of the last packet's header byte 3) turns its ulen 8192 into 0.  The GPU
    decode must not drop that packet from the verify: exit 1 naming it, as --host does."""
    data = np.resize(LS.packet(5000), packets * PACKET)
    src, gip = tmp_path / "in.dat", tmp_path / "out.gip"
    data.tofile(src)
    env = dict(os.environ, GPUAR_NO_FAST_EXIT="1")
    extra = ("--batch", str(batch_packets)) if batch_packets else ()
    r = subprocess.run([CLI, "c", "--checksum", *extra, f"--in={src}", f"--out={gip}"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    blob = bytearray(gip.read_bytes())
    end = int.from_bytes(blob[12:20], "little")
    import struct
    n = struct.unpack_from("<Q", blob, end + 8)[0]
    assert n == packets
    clens = struct.unpack_from(f"<{n}H", blob, end + 16)
    at = 20 + sum(clens[:-1]) + 3
    assert blob[at] == 0x20 and blob[at - 1] == 0
    blob[at] ^= 0x20
    gip.write_bytes(bytes(blob))
    want = f"Checksum mismatch: packet {packets - 1} (uncompressed bytes {(packets - 1) * PACKET} .. {(packets - 1) * PACKET})"
    for host in ((), ("--host",)):
        r = subprocess.run([CLI, "d", *host, *extra, f"--in={gip}", f"--out={tmp_path / 'back.dat'}"], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 1 and want in r.stderr, (host, r.stdout, r.stderr)
