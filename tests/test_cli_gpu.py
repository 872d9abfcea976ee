"""The `gpuar` CLI on the GPU path (C++ GPUCompressor over the C ABI): files must equal the
reference's --host outputs from byte 20 on, and round-trip."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from gpuar_amd import synth
from test_oracle_golden import SURVEY

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpuar_amd", "bin", "gpuar")


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("s", SURVEY["streams"], ids=lambda s: f"{s['kind']}-{s['seed']}-{s['n']}")
def test_gpu_cli_matches_reference_files(tmp_path, s):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, gip, back = tmp_path / "in.dat", tmp_path / "out.gip", tmp_path / "back.dat"
    data = synth.generate(s["kind"], s["seed"], s["n"])
    data.tofile(src)
    r = run("c", f"--in={src}", f"--out={gip}", "--gpus=1")
    assert r.returncode == 0, r.stderr
    assert "Attention" not in r.stdout                     # not the host path
    blob = open(gip, "rb").read()
    assert len(blob) == s["gip_bytes"]
    assert blob[0:3] == b"\x00\x01\x00"
    assert int.from_bytes(blob[4:12], "little") == s["n"]
    assert int.from_bytes(blob[12:20], "little") == s["gip_bytes"]
    assert hashlib.md5(blob[20:]).hexdigest() == s["stream_md5"]
    r = run("d", f"--in={gip}", f"--out={back}", "--device=0")
    assert r.returncode == 0, r.stderr
    assert hashlib.md5(open(back, "rb").read()).hexdigest() == s["input_md5"]


def test_gpu_cli_small_batches_and_cross_check_with_host(tmp_path):
    """Several rounds per file (the multi-round path of GPUCompressor) and host<->GPU interchange."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, g1, g2, back = tmp_path / "in.dat", tmp_path / "gpu.gip", tmp_path / "host.gip", tmp_path / "back.dat"
    data = synth.zipf(4, 3 * 1024 * 1024 + 12345)
    data.tofile(src)
    # 64 packets per round: 6 pipelined rounds for this file, the last one ragged
    assert run("c", f"--in={src}", f"--out={g1}", "--batch=64").returncode == 0
    assert run("c", "--host", "--threads=0", f"--in={src}", f"--out={g2}").returncode == 0
    assert open(g1, "rb").read() == open(g2, "rb").read()          # identical files, header included
    assert run("d", "--host", "--threads=0", f"--in={g1}", f"--out={back}").returncode == 0
    assert open(back, "rb").read() == data.tobytes()
    back2 = tmp_path / "back2.dat"
    assert run("d", f"--in={g2}", f"--out={back2}", "--batch", "128").returncode == 0     # GPU decode, 4 rounds
    assert open(back2, "rb").read() == data.tobytes()


def test_gpu_cli_shards_over_several_devices(tmp_path):
    """--gpus=3 on this box: three logical devices (oversubscribed onto the physical one) take contiguous
    packet ranges, run concurrently on their own host threads and streams, and the segments are concatenated
    in device order -- the file must equal the single-device file byte for byte, and decode back."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, g1, g3, back = tmp_path / "in.dat", tmp_path / "one.gip", tmp_path / "three.gip", tmp_path / "back.dat"
    data = synth.text(8, 1000 * 8192 + 4321)
    data.tofile(src)
    env = dict(os.environ, GPUAR_OVERSUBSCRIBE_DEVICES="1")
    assert run("c", f"--in={src}", f"--out={g1}").returncode == 0
    r = subprocess.run([CLI, "c", f"--in={src}", f"--out={g3}", "--gpus=3", "--batch=128"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert "Shard packets over 3 GPUs." in r.stdout
    assert open(g1, "rb").read() == open(g3, "rb").read()
    r = subprocess.run([CLI, "d", f"--in={g3}", f"--out={back}", "--gpus=3", "--batch=64"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert open(back, "rb").read() == data.tobytes()
    # without the test override, asking for more GPUs than exist is an error, not a silent clamp
    r = run("c", f"--in={src}", f"--out={g3}", "--gpus=64")
    assert r.returncode == 1 and "visible" in r.stderr


def test_gpu_cli_deals_equal_shares_to_eight_devices(tmp_path):
    """--gpus=8 (eight logical devices oversubscribed onto this box's one, ONE process): the file is cut into contiguous
    packet ranges sized so that every lane of every device gets one, dealt round-robin in file order;
    GPUAR_TRACE names what every device coded.  All eight devices work, their shares differ by one chunk at most, the
    bytes add up -- and the file equals the single-device file."""
    import re
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, g1, g8, back = tmp_path / "in.dat", tmp_path / "one.gip", tmp_path / "eight.gip", tmp_path / "back.dat"
    n = 256 * 1024 * 1024 + 12345                               # a quarter GiB: 32769 packets
    synth.uniform(17, n).tofile(src)
    assert run("c", f"--in={src}", f"--out={g1}").returncode == 0
    env = dict(os.environ, GPUAR_OVERSUBSCRIBE_DEVICES="1", GPUAR_TRACE="1")
    for mode, out, inp in (("c", g8, src), ("d", back, g8)):
        r = subprocess.run([CLI, mode, f"--in={inp}", f"--out={out}", "--gpus=8"], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        verb = "coded" if mode == "c" else "decoded"
        shares = [(int(d), int(b), int(k)) for d, b, k in re.findall(rf"device (\d+) {verb} (\d+) bytes in (\d+) chunks", r.stderr)]
        assert [d for d, _, _ in shares] == list(range(8)), r.stderr[-2000:]
        assert sum(b for _, b, _ in shares) == n
        assert all(b > 0 for _, b, _ in shares)                                  # every device works
        chunks = [k for _, _, k in shares]
        assert max(chunks) - min(chunks) <= 1                                    # the same number of chunks to within one
        if mode == "c":
            cap = int(re.search(r"chunks of at most (\d+) bytes", r.stderr).group(1))
            assert cap % (64 * 8192) == 0 and cap <= -(-n // (8 * 3 * 64 * 8192)) * 64 * 8192     # <= ceil(share of a lane), whole wavefronts
            assert max(b for _, b, _ in shares) - min(b for _, b, _ in shares) <= cap     # shares differ by one chunk at most
    assert g8.read_bytes() == g1.read_bytes()
    assert back.read_bytes() == src.read_bytes()


def test_gpu_cli_index_trailer_and_bulk_reads(tmp_path):
    """--index on the GPU path: same bytes as the host writes, trailer a pure suffix; decode with and
    without the index, in several rounds (read windows that cut packets), on 1 and on 3 (oversubscribed) devices."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, plain, gidx, hidx = tmp_path / "in.dat", tmp_path / "plain.gip", tmp_path / "gpu_idx.gip", tmp_path / "host_idx.gip"
    data = synth.text(9, 5 * 1024 * 1024 + 777)
    data.tofile(src)
    assert run("c", f"--in={src}", f"--out={plain}", "--batch=192").returncode == 0
    assert run("c", "--index", f"--in={src}", f"--out={gidx}", "--batch=192").returncode == 0
    assert run("c", "--index", "--host", "--threads=0", f"--in={src}", f"--out={hidx}").returncode == 0
    a, b = plain.read_bytes(), gidx.read_bytes()
    assert b == hidx.read_bytes()                                  # GPU and host write the same indexed file
    assert b[:len(a)] == a and b[len(a):len(a) + 4] == b"GIPX" and int.from_bytes(b[12:20], "little") == len(a)
    env = dict(os.environ, GPUAR_OVERSUBSCRIBE_DEVICES="1")
    for gip, extra in ((gidx, ["--batch=64"]), (plain, ["--batch=64"]), (gidx, ["--gpus=3", "--batch=128"]), (plain, ["--gpus=3", "--batch=128"]), (gidx, [])):
        back = tmp_path / "back.dat"
        r = subprocess.run([CLI, "d", f"--in={gip}", f"--out={back}", *extra], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data.tobytes(), (gip, extra)
    # a truncated stream is an error, not a crash
    (tmp_path / "cut.gip").write_bytes(a[:len(a) - 100])
    r = run("d", f"--in={tmp_path / 'cut.gip'}", f"--out={tmp_path / 'cut.out'}")
    assert r.returncode == 1 and "file" in r.stderr.lower()


def test_gpu_cli_file_over_4gib(tmp_path):
    """a > 4 GiB file through `gpuar c` / `gpuar d` on the GPU path.  The input
    is a sparse file of zeros with a few islands of data (so it costs no disk on the way in): the header must
    carry the size as a u64 (the reference's u32 at src/file_header.hpp:50-51,63-71 would wrap), the stream
    must be the concatenation of the per-packet oracle outputs at the islands, and the file must decode back."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = (4 << 30) + (64 << 20) + 4321                    # ragged, > 2^32
    src, gip, back = tmp_path / "big.dat", tmp_path / "big.gip", tmp_path / "big.back"
    islands = {0: synth.text(1, 3 * 8192), (1 << 32) - 8192: synth.uniform(2, 3 * 8192), n - 4321 - 8192: synth.zipf(3, 8192 + 4321)}
    with open(src, "wb") as f:
        f.truncate(n)
        for at, data in islands.items():
            f.seek(at)
            f.write(data.tobytes())
    r = run("c", f"--in={src}", f"--out={gip}")
    assert r.returncode == 0, r.stderr
    blob = gip.read_bytes()
    assert int.from_bytes(blob[4:12], "little") == n and n > 0xFFFFFFFF          # u64 size field in use
    assert int.from_bytes(blob[12:20], "little") == len(blob)
    npk = (n + 8191) // 8192
    from oracle import oracle as O
    zero_pkt = O.require_best().encode_packet(bytes(8192))
    assert len(zero_pkt) == 210
    # first packets = the text island, then zero packets
    want_head = O.require_best().encode_stream(islands[0]).tobytes()
    assert blob[20:20 + len(want_head)] == want_head
    assert blob[20 + len(want_head):20 + len(want_head) + 210] == zero_pkt
    # the tail island (last two packets, the very last one short) closes the file
    want_tail = O.require_best().encode_stream(islands[n - 4321 - 8192]).tobytes()
    assert blob[-len(want_tail):] == want_tail
    assert len(blob) > 20 + (npk - 8) * 210
    # The mapped input is registered for DMA in 256 MiB windows; windows nobody copies from any more are unregistered
    # once more than GPUAR_MAX_WINDOWS (default 16 = 4 GiB) are registered, so the pinned footprint does not grow with
    # the file.  With a cap of two the 17 windows of this file are recycled again and again: same bytes out.
    import re
    gip2 = tmp_path / "big2.gip"
    env = dict(os.environ, GPUAR_MAX_WINDOWS="2", GPUAR_TRACE="1")
    r = subprocess.run([CLI, "c", f"--in={src}", f"--out={gip2}"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "every window registered" in r.stderr
    trimmed = float(re.search(r"input windows unregistered while the job ran: ([0-9.]+)", r.stderr).group(1))
    assert trimmed >= 12, r.stderr[-2000:]
    assert gip2.read_bytes() == blob
    gip2.unlink()
    del blob
    r = run("d", f"--in={gip}", f"--out={back}")
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(back) == n
    with open(back, "rb") as f:
        for at, data in islands.items():
            f.seek(at)
            assert f.read(data.size) == data.tobytes(), at
        f.seek(1 << 31)
        assert f.read(1 << 20) == bytes(1 << 20)
    # whole-file check without holding 4 GiB in memory: md5 in 64 MiB pieces against the sparse source
    ha, hb = hashlib.md5(), hashlib.md5()
    with open(src, "rb") as a, open(back, "rb") as b:
        while True:
            x, y = a.read(64 << 20), b.read(64 << 20)
            if not x and not y:
                break
            ha.update(x)
            hb.update(y)
    assert ha.hexdigest() == hb.hexdigest()


def test_gpu_cli_batch_that_is_not_a_multiple_of_64(tmp_path):
    """--gpus=2 --batch=100: per-device shares are whole wavefronts (multiples of 64 packets), so the batch is
    rounded down to 64 and nothing outgrows its buffers; output identical to the default run."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, g1, g2, back = tmp_path / "in.dat", tmp_path / "one.gip", tmp_path / "two.gip", tmp_path / "back.dat"
    data = synth.uniform(15, 777 * 8192 + 55)
    data.tofile(src)
    env = dict(os.environ, GPUAR_OVERSUBSCRIBE_DEVICES="1")
    assert run("c", f"--in={src}", f"--out={g1}").returncode == 0
    r = subprocess.run([CLI, "c", f"--in={src}", f"--out={g2}", "--gpus=2", "--batch=100"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr
    assert g1.read_bytes() == g2.read_bytes()
    r = subprocess.run([CLI, "d", f"--in={g2}", f"--out={back}", "--gpus=2", "--batch=100"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == data.tobytes()


def test_gpu_cli_decodes_files_with_the_references_uninitialised_header_bytes(tmp_path):
    """A .gip written by the reference has garbage in header bytes 3, 8-11, 16-19; the GPU path must write
    exactly the bytes the packets hold (last packet short), as --host does."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_cli_host import reference_style_header
    src, gip, ref_gip, back = tmp_path / "in.dat", tmp_path / "a.gip", tmp_path / "ref.gip", tmp_path / "back.dat"
    data = synth.text(12, 70 * 8192 + 777)
    data.tofile(src)
    assert run("c", f"--in={src}", f"--out={gip}").returncode == 0
    ref_gip.write_bytes(reference_style_header(gip.read_bytes()))
    r = run("d", f"--in={ref_gip}", f"--out={back}")
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == data.tobytes()
    assert f"Uncompressed file size {data.size} bytes" in r.stdout


def test_gpu_cli_names_the_chunk_of_a_corrupted_packet(tmp_path):
    """A multi-chunk .gip with one damaged packet: the lane that decodes that chunk reports it through its own
    status word (no device-wide flag shared between the three lanes of a device), the CLI fails with the
    reference's message and says which chunk it was -- and the same file with the damage undone decodes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, gip, back = tmp_path / "in.dat", tmp_path / "out.gip", tmp_path / "back.dat"
    data = synth.text(21, 64 * 30 * 8192 + 777)              # 30 chunks of 64 packets, last one ragged
    data.tofile(src)
    assert run("c", f"--in={src}", f"--out={gip}", "--batch=64").returncode == 0
    blob = bytearray(open(gip, "rb").read())
    # walk to packet 64 * 17 + 5 (chunk 17 at --batch=64) and claim an impossible ulen
    at = 20
    for _ in range(64 * 17 + 5):
        at += blob[at] | (blob[at + 1] << 8)
    chunk_begin = 20
    for _ in range(64 * 17):
        chunk_begin += blob[chunk_begin] | (blob[chunk_begin + 1] << 8)
    saved = bytes(blob[at + 2:at + 4])
    blob[at + 2:at + 4] = b"\xff\xff"
    open(gip, "wb").write(blob)
    for attempt in range(3):                                  # lanes race differently every time: always chunk 17
        r = run("d", f"--in={gip}", f"--out={back}", "--batch=64")
        assert r.returncode == 1 and "Incorrect file format" in r.stderr, r.stderr
        assert f"between file offsets {chunk_begin} and" in r.stderr, r.stderr
    blob[at + 2:at + 4] = saved
    open(gip, "wb").write(blob)
    assert run("d", f"--in={gip}", f"--out={back}", "--batch=64").returncode == 0
    assert open(back, "rb").read() == data.tobytes()


def test_gpu_cli_overwrites_a_longer_file_and_leaves_nothing_behind_on_failure(tmp_path):
    """The GPU path opens its output WITHOUT truncating it (dropping the page cache of a large old file costs most of
    a second) and sets the length itself at the end: over an older, longer file the result must still be exactly the
    fresh one -- in both directions -- and a job that fails must not leave a half-written file that looks like a result."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, fresh, reused, back = tmp_path / "in.dat", tmp_path / "fresh.gip", tmp_path / "reused.gip", tmp_path / "back.dat"
    data = synth.text(33, 200 * 8192 + 17)
    data.tofile(src)
    junk = np.random.default_rng(1).integers(0, 256, 5 << 20, dtype=np.uint8).tobytes()     # longer than any output here
    assert run("c", f"--in={src}", f"--out={fresh}").returncode == 0
    reused.write_bytes(junk)
    assert run("c", f"--in={src}", f"--out={reused}").returncode == 0
    assert reused.read_bytes() == fresh.read_bytes()
    back.write_bytes(junk)
    assert run("d", f"--in={reused}", f"--out={back}").returncode == 0
    assert back.read_bytes() == data.tobytes()
    # failure: a stream cut in the middle of a packet
    cut = tmp_path / "cut.gip"
    cut.write_bytes(fresh.read_bytes()[:-100])
    back.write_bytes(junk)
    r = run("d", f"--in={cut}", f"--out={back}")
    assert r.returncode == 1
    assert back.stat().st_size == 0


def test_gpu_cli_empty_input_and_input_without_a_mapping(tmp_path):
    """Edge cases of the pipeline: an empty file (no chunk, no packet: header only, and it decodes to an empty file),
    and the pread path of an input that cannot be mapped (GPUAR_NO_MMAP=1) -- same bytes as the mapped path, both ways."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    empty, gip, back = tmp_path / "empty.dat", tmp_path / "empty.gip", tmp_path / "empty.back"
    empty.write_bytes(b"")
    r = run("c", f"--in={empty}", f"--out={gip}")
    assert r.returncode == 0, r.stderr
    blob = gip.read_bytes()
    assert len(blob) == 20 and int.from_bytes(blob[4:12], "little") == 0 and int.from_bytes(blob[12:20], "little") == 20
    r = run("d", f"--in={gip}", f"--out={back}")
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == b""
    src, a, b, back2 = tmp_path / "in.dat", tmp_path / "mapped.gip", tmp_path / "pread.gip", tmp_path / "back2.dat"
    data = synth.zipf(44, 300 * 8192 + 5)
    data.tofile(src)
    assert run("c", f"--in={src}", f"--out={a}", "--batch=128").returncode == 0
    env = dict(os.environ, GPUAR_NO_MMAP="1")
    r = subprocess.run([CLI, "c", f"--in={src}", f"--out={b}", "--batch=128"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes()
    r = subprocess.run([CLI, "d", f"--in={b}", f"--out={back2}", "--batch=64"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr
    assert back2.read_bytes() == data.tobytes()


def test_gpu_cli_survives_an_input_cut_short_under_its_mapping(tmp_path):
    """A MAP_SHARED input truncated while the job runs: accesses behind the new end of the file
    raise SIGBUS -- in the decoder's header walk, or inside a HIP runtime thread -- and the default action would kill the
    process.  host/input_guard.hpp turns them into zeros and a mark; the job must end with the reference's message for a
    short read (src/gpu_compressor.cpp:146-150: "Read input file failed"; decoding: "Invalid file length", :299-307), exit
    code 1, and an empty output file.  GPUAR_TEST_HOLD_AFTER_MAP_MS makes the race deterministic: the CLI sleeps between
    mapping its input and reading it, and the file is cut in that window."""
    import threading
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src, gip, out = tmp_path / "in.dat", tmp_path / "whole.gip", tmp_path / "out.bin"
    data = synth.text(77, 96 << 20)
    data.tofile(src)
    assert run("c", f"--in={src}", f"--out={gip}", "--batch=2048").returncode == 0
    whole = gip.stat().st_size
    env = dict(os.environ, GPUAR_TEST_HOLD_AFTER_MAP_MS="1500")
    for mode, victim, keep, message in (("c", src, 5 << 20, "Read input file failed"), ("d", gip, whole // 3, "Invalid file length")):
        out.write_bytes(b"stale")
        # stdout goes to a file (nobody reads it while the job runs: a pipe could fill), stderr is read on a helper thread,
        # and every wait has a deadline after which the child is killed
        with open(tmp_path / f"stdout.{mode}", "w+") as stdout_file:
            p = subprocess.Popen([CLI, mode, f"--in={victim}", f"--out={out}", "--batch=2048"], stdout=stdout_file, stderr=subprocess.PIPE,
                                 text=True, env=env)
            # the CLI says "[gpuar] input mapped" once it has sized and mapped the file, then holds: cut the file THEN, however long
            # ROCm's start-up took on this box (a fixed sleep raced it)
            seen, mapped = [], threading.Event()

            def read_stderr():
                for line in p.stderr:                        # (the HIP runtime or libdrm may say something of their own first)
                    seen.append(line)
                    if "input mapped" in line:
                        mapped.set()
                mapped.set()                                 # end of file: the child is gone, nobody need wait any longer

            reader = threading.Thread(target=read_stderr, daemon=True)
            reader.start()
            try:
                if not mapped.wait(timeout=600):
                    raise AssertionError((mode, "no word from the child in 600 s", seen))
                assert any("input mapped" in line for line in seen), (mode, seen)
                os.truncate(victim, keep)
                p.wait(timeout=600)
            finally:
                if p.poll() is None:
                    p.kill()
                    p.wait()
                reader.join(timeout=60)
            stdout_file.seek(0)
            stdout, stderr = stdout_file.read(), "".join(seen)
        assert p.returncode == 1, (mode, p.returncode, stdout[-500:], stderr[-500:])       # not -SIGBUS
        assert message in stdout + stderr, (mode, stdout[-500:], stderr[-500:])
        assert out.stat().st_size == 0


def test_gpu_cli_takes_damaged_trailers_as_the_host_path_does(tmp_path):
    """Twelve files of the trailer sweep (test_trailer_damage.py) -- every trailer version undamaged, cut off, malformed,
    unusable and with a CRC that does not match, for a plain and for a planes file of 3 packets -- decoded on the GPU and by
    --host: the same exit status, the same kind of message and, where the file decodes, the same bytes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trailer_ref as T
    x = T.sweep_input()
    src, gip = tmp_path / "in.dat", tmp_path / "case.gip"
    src.write_bytes(x)
    goods = []
    for flags in T.FLAGS:
        r = run("c", "--host", *flags, f"--in={src}", f"--out={gip}")
        assert r.returncode == 0, r.stderr
        goods.append(gip.read_bytes())
    cases = T.cross_cases(x, goods)
    assert len(cases) == 12
    assert {T.classify(blob)[0] for _, blob, _ in cases} == {"none", "ok", "malformed", "unusable"}
    assert {cls.split()[0] for _, _, (_, cls, _) in cases} == {"quiet", "warning", "planes", "checksum"}
    for what, blob, (code, cls, want) in cases:
        gip.write_bytes(blob)
        got = {}
        for path in (["--host"], []):
            out = tmp_path / "case.out"
            out.unlink(missing_ok=True)
            r = run("d", *path, f"--in={gip}", f"--out={out}")
            assert r.returncode in (0, 1), (what, path, r.returncode, r.stderr)
            got[len(path)] = (r.returncode, T.stderr_class(r.returncode, r.stderr), out.read_bytes() if want is not None else None)
        assert got[0] == got[1] == (code, cls, want), (what, got[0][:2], got[1][:2])
