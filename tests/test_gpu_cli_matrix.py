"""The GPU file pipeline (gpuar_amd/csrc/host/gpu_compressor.cpp) against `gpuar-host --host` over its option matrix and at its own
edges: every flag set under every way of cutting the file and dealing the chunks (tests/cli_matrix.py); file sizes around the packet,
the chunk and the number of lanes; the ramped first chunk and a chunk that needs a second 64 MiB piece; short packets in the middle
of a stream; and damaged packets.  The GPU writes the host's file byte for byte, each path reads the other's files, and both refuse
the same files with the same words.  One child at a time, each under its own time limit; nothing is started after a child that
ended badly (cli_matrix.run_cli)."""
import re
import struct
import time

import numpy as np
import pytest

import cli_matrix as M
import gip_files as G
import kinds_ref as K
import trailer_ref as T
import xor_ref as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PACKET = M.PACKET
IDS = [name for name, _flags, _says in M.FLAG_SETS]


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return M.matrix_input()


def _host_file(tmp, x, flags, base):
    """(the host's file, the --base argument both paths take)"""
    blob = G.write(tmp, x, flags, base)
    return blob, [f"--base={tmp / 'base.bin'}"] if base is not None else []


def _written(tmp, shape, flags, based, want, what):
    """`gpuar c` under `shape` writes `want`; returns the file's path"""
    out = tmp / f"gpu_{shape}.gip"
    r = M.gpu("c", tmp / "in.bin", out, shape, [*flags, *based])
    assert r.returncode == 0, (what, shape, r.stderr[-2000:])
    assert out.read_bytes() == want, (what, shape, "the GPU's file is not the host's")
    return out


def _read(tmp, shape, gip, based, want, what):
    back = tmp / "back.bin"
    back.write_bytes(b"left over")
    r = M.gpu("d", gip, back, shape, based)
    assert r.returncode == 0, (what, shape, r.stderr[-2000:])
    assert back.read_bytes() == want, (what, shape, "the GPU does not decode the input")


def _as_the_host(tmp, gip, based, shapes, what, cls=M.message_class):
    """`gpuar d` under every shape does with `gip` what `gpuar-host d --host` does: the same bytes, or the same exit status and
    class of message and an empty output; returns the host's verdict and what the GPU runs said"""
    out = tmp / "verdict.out"
    r = M.host("d", gip, out, based)
    want = (r.returncode, cls(r.returncode, r.stderr))
    assert want[0] in (0, 1), (what, r.returncode, r.stderr)
    held = out.read_bytes() if want[0] == 0 else b""
    said = []
    for shape in shapes:
        out.write_bytes(b"left over")
        g = M.gpu("d", gip, out, shape, based)
        assert (g.returncode, cls(g.returncode, g.stderr)) == want, (what, shape, g.stderr[-2000:], r.stderr[-2000:])
        assert out.read_bytes() == held, (what, shape)
        said.append(g.stderr)
    return want, held, said


# ---- 1. the matrix --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", IDS)
def test_every_shape_writes_and_reads_the_hosts_file(tmp_path, data, name):
    x, base = data
    flags, says = M.FLAGS[name]
    blob, based = _host_file(tmp_path, x, flags, base if says.get("base") else None)
    G.expected(blob, x, says, base)
    files = {}
    for shape, _argv, _env in M.SHAPES:
        files[shape] = _written(tmp_path, shape, flags, based, blob, name)
        _read(tmp_path, shape, tmp_path / "out.gip", based, x.tobytes(), name)
    r = M.host("d", files["gpus3"], tmp_path / "host_back.bin", based)
    assert r.returncode == 0 and (tmp_path / "host_back.bin").read_bytes() == x.tobytes(), (name, r.stderr)
    _read(tmp_path, "batch64", files["gpus3"], based, x.tobytes(), (name, "written under gpus3"))
    _read(tmp_path, "gpus3", files["batch64"], based, x.tobytes(), (name, "written under batch64"))
    # as a reference-written file has its header
    (tmp_path / "garbage.gip").write_bytes(G.garbage_header(blob))
    want, held, _said = _as_the_host(tmp_path, tmp_path / "garbage.gip", based, ("batch64",), (name, "garbage header bytes"))
    assert want == (0, "quiet") and held == x.tobytes(), (name, want)


# ---- 2. sizes -------------------------------------------------------------------------------------------------------------

SIZE_SETS = {
    "plain": M.FLAGS["plain"],
    "delta_planes8_checksum": (["--planes=8", "--delta", "--checksum"], dict(version=4, elem=8, delta=True, crcs=True)),
    "base_planes2_stored_sparse": M.FLAGS["base_planes2_stored_sparse"],
}
SIZES = (1, 7, 8, 9, 8191, 8192, 8193, 2 * 8192 + 3, 64 * 8192 - 1, 64 * 8192, 64 * 8192 + 1, 192 * 8192 - 1, 192 * 8192, 192 * 8192 + 1, 384 * 8192)
SIZE_SHAPES = ("default", "batch64", "gpus2_batch64")


def _size_input(data, n):
    """n bytes of the matrix input and of its base: from the segment that changes packet by packet where that holds them, else from
    the start"""
    x, base = data
    at = 4 * M.CHUNK * PACKET if n <= M.CHUNK * PACKET + 1 else 0
    return x[at:at + n].copy(), base[at:at + n].copy()


def _both_ways(tmp, x, base, flags, says, shapes, what):
    """the host's verdict on compressing x, and the same from the GPU under every shape: the same file and the round trip, or the same
    refusal"""
    (tmp / "in.bin").write_bytes(x.tobytes())
    based = []
    if says.get("base"):
        (tmp / "base.bin").write_bytes(base.tobytes())
        based = [f"--base={tmp / 'base.bin'}"]
    r = M.host("c", tmp / "in.bin", tmp / "out.gip", [*flags, *based])
    assert r.returncode in (0, 1), (what, r.returncode, r.stderr)
    verdict = (r.returncode, M.message_class(r.returncode, r.stderr))
    if r.returncode == 0:
        blob = (tmp / "out.gip").read_bytes()
        G.expected(blob, x, says, base)
    for shape in shapes:
        if verdict[0] == 0:
            _written(tmp, shape, flags, based, blob, what)
            _read(tmp, shape, tmp / "out.gip", based, x.tobytes(), what)
        else:
            g = M.gpu("c", tmp / "in.bin", tmp / "gpu.gip", shape, [*flags, *based])
            assert (g.returncode, M.message_class(g.returncode, g.stderr)) == verdict, (what, shape, g.stderr[-2000:])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_sizes_at_the_edges_of_packet_chunk_and_lanes(tmp_path, data, name, n):
    """192 packets are three lanes times one 64-packet chunk, 384 six lanes times one; 1 .. 9 bytes are less than, exactly and more
    than one element of 8 bytes"""
    flags, says = SIZE_SETS[name]
    x, base = _size_input(data, n)
    _both_ways(tmp_path, x, base, flags, says, SIZE_SHAPES, (name, n))


@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_fewer_packets_than_lanes(tmp_path, data, name):
    """three packets, nine lanes: the idle lanes never allocate"""
    flags, says = SIZE_SETS[name]
    x, base = _size_input(data, 2 * 8192 + 3)
    _both_ways(tmp_path, x, base, flags, says, ("gpus3",), (name, "gpus3"))


# ---- 3. the ramp and the second piece -------------------------------------------------------------------------------------

N_RAMP = (3 * 8192 + 64) * PACKET + 4097            # 24 641 packets: the smallest file a lane's share of which exceeds 8192 packets
RAMP_CHUNKS = [8192, 8256, 8193]                     # chunk 0 ramped down to 8192, so chunks 1 and 2 start off the grid of 8256


def _same(a, b):
    """two files hold the same bytes: compared in pieces of 64 MiB"""
    with open(a, "rb") as f, open(b, "rb") as g:
        while True:
            x, y = f.read(64 << 20), g.read(64 << 20)
            if x != y:
                return False
            if not x:
                return True


def _ramp(tmp, x, base, flags, gpus=(1, 2)):
    x.tofile(tmp / "in.bin")
    based = []
    if base is not None:
        base.tofile(tmp / "base.bin")
        based = [f"--base={tmp / 'base.bin'}"]
    del x, base
    r = M.host("c", tmp / "in.bin", tmp / "host.gip", [*flags, *based], timeout=600)
    assert r.returncode == 0, r.stderr
    for label, extra, env in (("default", [], {}), ("gpus2", ["--gpus=2"], M.OVERSUBSCRIBE))[:len(gpus)]:
        env = dict(env, GPUAR_TRACE="1")
        r = M.gpu("c", tmp / "in.bin", tmp / "gpu.gip", "default", [*extra, *flags, *based], timeout=300, env=env)
        assert r.returncode == 0, (label, r.stderr[-2000:])
        assert _same(tmp / "gpu.gip", tmp / "host.gip"), (label, "the GPU's file is not the host's")
        if label == "default":
            got = [int(float(v)) for v in re.findall(r"compress: packets in chunk \d+: ([0-9.]+)", r.stderr)]
            assert got == RAMP_CHUNKS, r.stderr[-3000:]
            assert f"device 0 coded {N_RAMP} bytes in 3 chunks of at most {8256 * PACKET} bytes" in r.stderr
        r = M.gpu("d", tmp / "host.gip", tmp / "back.bin", "default", [*extra, *based], timeout=300, env=env)
        assert r.returncode == 0, (label, r.stderr[-2000:])
        assert _same(tmp / "back.bin", tmp / "in.bin"), (label, "the GPU does not decode the input")
        if label == "default":
            got = sorted((int(c), int(float(v))) for c, v in re.findall(r"decompress: packets in chunk (\d+): ([0-9.]+)", r.stderr))
            assert [v for _c, v in got] == RAMP_CHUNKS, r.stderr[-3000:]
            assert f"device 0 decoded {N_RAMP} bytes in 3 chunks" in r.stderr


def _bf16_like(n):
    """(n bytes of bf16 weights, a base that differs in one element of a thousand): 2 MiB and a bit of normal x 0.02, over and over --
    the chunks start 64 packets off the grid, which no multiple of that period is"""
    block = X.bf16(np.random.default_rng(32).standard_normal((1 << 20) + 12345).astype(np.float32) * np.float32(0.02)).view(np.uint8)
    x = np.tile(block, n // block.size + 1)[:n].copy()
    base = x.copy()
    base[:n // 2 * 2].view(np.uint16)[7::1000] ^= 0x0130
    return x, base


def test_ramped_chunks_and_a_second_piece(tmp_path, data):
    """(a) uniform bytes, raw packets: a chunk of 8192 packets is 64 MiB + 32 KiB of stream, two pieces to drain; CRC and kind rows
    from chunks of unequal length; decoded, the 8256-packet chunk is more than a piece.  On one device (the ramp: with two, a lane's
    share is under 8192 packets and the chunks lie on the grid) and on two.  (b) bf16-like data against a base that differs in one
    element of a thousand: the base is read at first_packet * 8192 for chunks that start off the grid.  On one device only: measured
    on the MI355X next to test_gpu_cli_deals_equal_shares_to_eight_devices (256 MiB), this test took 6.97 s against 1.98 s with (b)
    on two devices as well; as it stands 3.08 s against 1.72 s -- (a) 2.1 s, (b) 1.0 s --, still more than half as long again."""
    t0 = time.time()
    block = np.random.default_rng(31).integers(0, 256, (8 << 20) + 4099, dtype=np.uint8)      # (a period no chunk or packet boundary keeps to)
    _ramp(tmp_path, np.tile(block, N_RAMP // block.size + 1)[:N_RAMP].copy(), None, ["--stored=auto", "--checksum", "--planes=4"])
    t1 = time.time()
    x, base = _bf16_like(N_RAMP)
    _ramp(tmp_path, x, base, ["--planes=2", "--stored=auto", "--sparse=auto"], gpus=(1,))
    print(f"ramp: (a) {t1 - t0:.1f} s, (b) {time.time() - t1:.1f} s")


# ---- 4. short packets in the middle of a stream ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def splices(data, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("splices")
    M.splice_ulens()
    files = {trailer: M.spliced(tmp, M.splice_parts(), trailer) for trailer in M.SPLICE_TRAILERS}
    return files, M.splice_verdicts(tmp, files)


@pytest.mark.parametrize("trailer", M.SPLICE_TRAILERS, ids=lambda t: t or "none")
def test_spliced_files_as_the_host_takes_them(tmp_path, splices, trailer):
    files, verdicts = splices
    code, cls, want = verdicts[trailer]
    assert code == (0 if trailer in (None, "index") else 1), (trailer, cls)
    (tmp_path / "s.gip").write_bytes(files[trailer][0])
    got, held, _said = _as_the_host(tmp_path, tmp_path / "s.gip", [], [shape for shape, _a, _e in M.SHAPES], trailer, cls=T.stderr_class)
    assert got == (code, cls) and held == (want if code == 0 else b"")


def test_a_spliced_file_whose_header_says_less(tmp_path, splices):
    """the index trailer is right, the header's uncompressed size is not (the reference keeps 32 bits of it): what is written is what
    the packets hold"""
    files, _verdicts = splices
    blob, want = files["index"]
    (tmp_path / "s.gip").write_bytes(G.patched(blob, 4, struct.pack("<Q", 12345)))
    r = M.host("d", tmp_path / "s.gip", tmp_path / "s.out")
    assert r.returncode == 0 and (tmp_path / "s.out").read_bytes() == want, r.stderr
    for shape, _argv, _env in M.SHAPES:
        _read(tmp_path, shape, tmp_path / "s.gip", [], want, ("header says less", shape))


# ---- 5. damage ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["stored_sparse_checksum", "base_planes2"])
def test_damaged_packets_are_refused_as_the_host_refuses_them(tmp_path, data, name):
    """one damaged packet in chunk 3 (chunk 4 where chunk 3 holds no packet of the kind): written by the test from the host's file,
    refused by paths the kernels are tested on elsewhere"""
    x, base = data
    flags, says = M.FLAGS[name]
    blob, based = _host_file(tmp_path, x, flags, base if says.get("base") else None)
    kinds = M.kinds_of(x, base, says) if says["version"] == 6 else None
    cases = M.damaged(blob, kinds, 3)
    cases += [c for c in M.damaged(blob, kinds, 4) if c[0] not in {what for what, *_rest in cases}]
    assert {what for what, *_rest in cases} == ({"coded_ulen", "raw_byte", "sparse_count"} if kinds else {"coded_ulen"})
    for what, bad, begin, end in cases:
        (tmp_path / "bad.gip").write_bytes(bad)
        want, _held, said = _as_the_host(tmp_path, tmp_path / "bad.gip", based, ("batch64", "gpus2_batch64"), (name, what))
        print(name, what, want)
        for stderr in said:
            if "between file offsets" in stderr:
                assert f"between file offsets {begin} and {end}" in stderr, (name, what, stderr)
