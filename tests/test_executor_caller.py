"""The three reference-named executors under the call sequence of a program written against the reference's header:
tests/executor_client.cpp (plain C++, no torch, no ctypes) keeps two device buffers for the whole process and never clears
them, uploads packet by packet over several blocking streams, launches on the NULL stream with the reference's numBlocks,
synchronises the device, and brings every packet down with a copy of its own -- many batches per job, several jobs per
process, the last batch short.  Its files must be the ones the host codec writes, whatever the batch size, whatever lay in
the buffers before.

One child process at a time, each under a time limit; after a child that ended by a signal nothing more is started."""
import hashlib

import numpy as np
import pytest

import client_build as B
from gpuar_amd import synth
from test_oracle_golden import SURVEY

pytestmark = pytest.mark.gpu
CHILDREN = B.Children()          # module-level: remembers a child that ended badly
CHILD_SECONDS = 600


@pytest.fixture(scope="module")
def client():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return B.executor_client()


def run_client(exe, *args, expect=0):
    r = CHILDREN.run([exe, *map(str, args)], CHILD_SECONDS)
    assert r.returncode == expect, (r.returncode, r.stderr[-3000:])
    return B.parse_results(r.stderr)


def host_file(src, gip):
    r = CHILDREN.run([B.CLI, "c", "--host", "--threads=0", f"--in={src}", f"--out={gip}"], CHILD_SECONDS)
    assert r.returncode == 0, r.stderr
    return gip


def same_stream(mine, theirs):
    a, b = open(mine, "rb").read(), open(theirs, "rb").read()
    assert a[0:3] == b"\x00\x01\x00"
    assert (int.from_bytes(a[4:12], "little"), int.from_bytes(a[12:20], "little")) == (int.from_bytes(b[4:12], "little"), len(a))
    assert len(a) == len(b) and a[20:] == b[20:]
    return True


@pytest.mark.parametrize("s", SURVEY["streams"], ids=lambda s: f"{s['kind']}-{s['seed']}-{s['n']}")
def test_executor_caller_writes_the_survey_files_at_the_default_batch(client, tmp_path, s):
    """T = 32 * multiProcessorCount * 8, the reference's own batch: every survey stream, the 64 MiB one included."""
    src, gip, back = tmp_path / "in.dat", tmp_path / "out.gip", tmp_path / "back.dat"
    synth.generate(s["kind"], s["seed"], s["n"]).tofile(src)
    lines = run_client(client, "c", src, gip, "d", gip, back)
    assert [l["status"] for l in lines] == ["ok", "ok"], lines
    blob = gip.read_bytes()
    assert len(blob) == s["gip_bytes"]
    assert int.from_bytes(blob[4:12], "little") == s["n"] and int.from_bytes(blob[12:20], "little") == s["gip_bytes"]
    assert hashlib.md5(blob[20:]).hexdigest() == s["stream_md5"]
    assert hashlib.md5(back.read_bytes()).hexdigest() == s["input_md5"]


@pytest.fixture(scope="module")
def text_base():
    return synth.text(31, 2 * 4096 * 8192)


@pytest.mark.parametrize("T", [32, 96, 160, 64, 4096])
def test_executor_caller_at_small_and_ragged_batches(client, tmp_path, text_base, T):
    """T = 32 is half a wavefront per launch, 96 and 160 one and a half and two and a half.  A 3 MiB + 12345 zipf file (385
    packets: at T = 32, 64 and 96 its last batch holds exactly one packet) and text files whose last batch holds exactly
    one packet, exactly T, T - 1, and one that is an exact multiple of 8192 * T -- ten jobs in one process, every batch after
    the first over whatever the batches and jobs before left in the two buffers.  Byte-equal to `gpuar c --host` from byte
    20 on, and back to the inputs."""
    k = 1 if T >= 4096 else 2                               # full batches in front of the last one
    sizes = {"one": k * T * 8192 + 777,                     # last batch: one packet, and that one short
             "full": ((k + 1) * T - 1) * 8192 + 4321,       # last batch: exactly T packets, the last one short
             "less": ((k + 1) * T - 2) * 8192 + 5000,       # last batch: T - 1 packets
             "exact": k * T * 8192}                         # nothing behind the last full batch
    inputs = {"zipf": synth.zipf(4, 3 * 1024 * 1024 + 12345)}
    inputs.update({name: text_base[:n] for name, n in sizes.items()})
    args = [f"--packets={T}"]
    for name, data in inputs.items():
        data.tofile(tmp_path / f"{name}.dat")
        args += ["c", tmp_path / f"{name}.dat", tmp_path / f"{name}.gip"]
    for name in inputs:
        args += ["d", tmp_path / f"{name}.gip", tmp_path / f"{name}.back"]
    lines = run_client(client, *args)
    assert [l["status"] for l in lines] == ["ok"] * 10, lines
    for (name, data), rec in zip(inputs.items(), lines):
        assert rec["packets"] == T and rec["batches"] == -(-data.size // (8192 * T)), (name, rec)
        assert same_stream(tmp_path / f"{name}.gip", host_file(tmp_path / f"{name}.dat", tmp_path / f"{name}.host.gip")), name
        assert (tmp_path / f"{name}.back").read_bytes() == data.tobytes(), name


def test_executor_caller_and_cli_read_each_others_files(client, tmp_path):
    src, mine, theirs = tmp_path / "in.dat", tmp_path / "client.gip", tmp_path / "cli.gip"
    data = synth.text(12, 300 * 8192 + 99)
    data.tofile(src)
    r = CHILDREN.run([B.CLI, "c", f"--in={src}", f"--out={theirs}", "--batch=64"], CHILD_SECONDS)
    assert r.returncode == 0, r.stderr
    lines = run_client(client, "--packets=96", "c", src, mine, "d", theirs, tmp_path / "back.client")
    assert [l["status"] for l in lines] == ["ok", "ok"], lines
    assert mine.read_bytes() == theirs.read_bytes()                 # header included: both write this repository's FileHeader
    assert (tmp_path / "back.client").read_bytes() == data.tobytes()
    for extra, out in ((["--batch=64"], tmp_path / "back.gpu"), (["--host"], tmp_path / "back.host")):
        r = CHILDREN.run([B.CLI, "d", *extra, f"--in={mine}", f"--out={out}"], CHILD_SECONDS)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == data.tobytes()


def test_executor_caller_is_blind_to_what_lay_in_its_buffers(client, tmp_path):
    """A high-entropy file (packets of ~8260 bytes) and then a short, highly compressible one (packets of ~210 bytes into
    slots that still hold the long ones; a batch of 5 packets in front of 59 stale slots), then the reverse, compressing
    and decompressing, in one process -- and the same with both device buffers filled with 0x00 and with 0xEE before the
    first job.  All three runs write the same files: the host codec's."""
    rng = np.random.default_rng(9)
    noisy = rng.integers(0, 256, 200 * 8192 + 4000, dtype=np.uint8)
    calm = np.zeros(4 * 8192 + 100, dtype=np.uint8)
    calm[::997] = 7
    (tmp_path / "noisy.dat").write_bytes(noisy.tobytes())
    (tmp_path / "calm.dat").write_bytes(calm.tobytes())
    want = {n: host_file(tmp_path / f"{n}.dat", tmp_path / f"{n}.host.gip").read_bytes() for n in ("noisy", "calm")}
    for tag, poison in (("none", []), ("zero", ["--poison=0x00"]), ("ee", ["--poison=0xEE"])):
        d = tmp_path / tag
        d.mkdir()
        order = ["noisy", "calm", "noisy", "calm"]
        args = ["--packets=64", *poison]
        for i, n in enumerate(order):
            args += ["c", tmp_path / f"{n}.dat", d / f"{i}.gip"]
        for i, n in enumerate(order):
            args += ["d", d / f"{i}.gip", d / f"{i}.back"]
        args += ["d", d / "1.gip", d / "again.back"]          # ... and calm once more right behind noisy
        lines = run_client(client, *args)
        assert [l["status"] for l in lines] == ["ok"] * 9, (tag, lines)
        for i, n in enumerate(order):
            assert (d / f"{i}.gip").read_bytes() == want[n], (tag, i, n)
            assert (d / f"{i}.back").read_bytes() == (tmp_path / f"{n}.dat").read_bytes(), (tag, i, n)
        assert (d / "again.back").read_bytes() == calm.tobytes(), tag


def test_executor_caller_size_that_ends_inside_the_last_slot(client, tmp_path):
    """The reference's caller passes packets * 8704, for which a ceiling and a floor of size / 8704 are the same number.
    include/gpuar_hip.h promises more: every packet whose slot STARTS in front of `size` is decoded.  With --tight-size the
    client ends `size` with the last live packet's own bytes; the last packet of every batch must still come out (over
    0xEE, where a packet that was skipped would show)."""
    src, gip = tmp_path / "in.dat", tmp_path / "in.gip"
    data = synth.zipf(6, 200 * 8192 + 3000)
    data.tofile(src)
    host_file(src, gip)
    for T in (32, 96):
        back = tmp_path / f"back{T}.dat"
        lines = run_client(client, f"--packets={T}", "--poison=0xEE", "--tight-size", "d", gip, back)
        assert [l["status"] for l in lines] == ["ok"], lines
        assert back.read_bytes() == data.tobytes(), T


def test_executor_caller_empty_input(client, tmp_path):
    src, gip, back = tmp_path / "empty.dat", tmp_path / "empty.gip", tmp_path / "empty.back"
    src.write_bytes(b"")
    lines = run_client(client, "--poison=0xEE", "c", src, gip, "d", gip, back)
    assert [(l["status"], l["batches"]) for l in lines] == [("ok", 0), ("ok", 0)], lines
    blob = gip.read_bytes()
    assert len(blob) == 20 and blob[:3] == b"\x00\x01\x00" and int.from_bytes(blob[4:12], "little") == 0 and int.from_bytes(blob[12:20], "little") == 20
    assert back.read_bytes() == b""
