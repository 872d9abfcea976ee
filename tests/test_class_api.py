"""The C++ classes as a LIBRARY: tests/class_client.cpp holds gip::Compressor objects and runs many jobs per object and
per process -- what host/main.cpp, one job per process and out through _Exit, never does.  Every file an object writes is
compared byte for byte with what the CLI writes in a fresh process with the same flags, every error text with the CLI's.

The CPU class runs wherever g++ does; the GPU class needs the device (`-m gpu`): one child process per test, one at a
time, each under a time limit, and after a child that ended by a signal nothing more is started (client_build.Children)."""
import hashlib
import os

import pytest

import client_build as B
from gpuar_amd import synth
from test_oracle_golden import SURVEY

CHILDREN = B.Children()          # module-level: remembers a child that ended badly
CHILD_SECONDS = 300


def survey(kind, seed, n):
    (s,) = [s for s in SURVEY["streams"] if (s["kind"], s["seed"], s["n"]) == (kind, seed, n)]
    return s


def header_sizes(blob):
    return int.from_bytes(blob[4:12], "little"), int.from_bytes(blob[12:20], "little")


def cli(exe, *args, env=None):
    return CHILDREN.run([exe, *args], CHILD_SECONDS, env=env)


def run_script(exe, words, env=None, through_stdin=False):
    """-> (completed process, parsed result lines); exactly one line per command"""
    words = [str(w) for w in words]
    r = CHILDREN.run([exe] if through_stdin else [exe, *words], CHILD_SECONDS, env=env, stdin_text=" ".join(words) + "\n" if through_stdin else None)
    return r, B.parse_results(r.stderr)


def check_ok_line(rec, src, dst):
    """an `ok` line of a job against the two files on disk: sizes, and times that a clock could have measured"""
    assert rec["status"] == "ok", rec
    blob = open(src if rec["command"] == "d" else dst, "rb").read(20)
    plain = dst if rec["command"] == "d" else src
    assert rec["uncompressedFileSize"] == os.path.getsize(plain), rec
    assert rec["compressedFileSize"] == header_sizes(blob)[1], rec
    assert rec["processedUncompressedSize"] == os.path.getsize(plain), rec
    assert 0 <= rec["processTime"] and 0 <= rec["ioTime"], rec
    assert rec["processTime"] <= rec["wall_ms"], rec


# ---------------------------------------------------------------------------------------------------------------- CPU


@pytest.fixture(scope="module")
def host_client():
    B.ensure_products()
    return B.class_client_host()


def test_one_cpu_object_through_failing_and_succeeding_jobs(host_client, tmp_path):
    """One CPUCompressor, nine jobs: a missing input, compress, decompress, another size with the index, checksums both
    ways, another thread count, a damaged checksum, and a plain compress again.  Each file equals what `gpuar-host` writes
    in a fresh process with the same flags (and the golden survey vectors), each `ok` line's sizes are the files', each
    error text is the CLI's, a failed job leaves an empty output (or none) and the object goes on working -- and with
    setQuiet(true) not one progress mark reaches stdout in any of the jobs."""
    t = tmp_path
    sa, sb = survey("text", 1, 65539), survey("text", 3, 100000)
    a, b = t / "a.dat", t / "b.dat"
    synth.generate(sa["kind"], sa["seed"], sa["n"]).tofile(a)
    synth.generate(sb["kind"], sb["seed"], sb["n"]).tofile(b)
    # the damaged file: the CLI's own --checksum file with one stored CRC changed (packet 3 of 9)
    ck_cli = t / "ck_cli.gip"
    assert cli(B.CLI_HOST, "c", "--host", "--checksum", f"--in={a}", f"--out={ck_cli}").returncode == 0
    blob = bytearray(ck_cli.read_bytes())
    stream_end = header_sizes(blob)[1]
    npk = (sa["n"] + 8191) // 8192
    assert blob[stream_end:stream_end + 4] == b"GIPX" and int.from_bytes(blob[stream_end + 4:stream_end + 8], "little") == 2
    crc_at = stream_end + 16 + (2 * npk + 3) // 4 * 4      # behind "GIPX", version, count and the u16 lengths padded to 4 (packet_index.hpp)
    blob[crc_at + 4 * 3] ^= 0x10
    damaged = t / "damaged.gip"
    damaged.write_bytes(blob)

    jobs = [   # (settings before the job, command, in, out, the CLI's flags for the same job)
        ([], "c", t / "missing.dat", t / "j1.gip", []),
        ([], "c", a, t / "j2.gip", []),
        ([], "d", t / "j2.gip", t / "j3.back", []),
        (["index", 1], "c", b, t / "j4.gip", ["--index"]),
        (["index", 0, "checksum", 1], "c", a, t / "j5.gip", ["--checksum"]),
        ([], "d", t / "j5.gip", t / "j6.back", ["--checksum"]),
        (["threads", 4], "c", b, t / "j7.gip", ["--checksum", "--threads=4"]),
        (["threads", 0], "d", damaged, t / "j8.back", ["--threads=0"]),
        (["checksum", 0], "c", a, t / "j9.gip", ["--threads=0"]),
    ]
    words = ["new", "cpu", "x"]
    for settings, command, src, dst, _ in jobs:
        words += [*settings, command, src, dst]
    (t / "j8.back").write_bytes(b"stale")
    r, lines = run_script(host_client, words)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "", r.stdout                      # quiet stays on from job to job
    assert [l["command"] for l in lines] == [w for w in map(str, words) if w in ("new", "index", "checksum", "threads", "c", "d")], r.stderr
    results = [l for l in lines if l["command"] in ("c", "d")]
    assert all(l["status"] == "ok" for l in lines if l["command"] not in ("c", "d")), r.stderr
    assert [l["status"] for l in results] == ["error", "ok", "ok", "ok", "ok", "ok", "ok", "error", "ok"], r.stderr

    for k, ((_, command, src, dst, flags), rec) in enumerate(zip(jobs, results), 1):
        want = t / f"cli{k}.out"
        c = cli(B.CLI_HOST, command, "--host", *flags, f"--in={src}", f"--out={want}")
        if rec["status"] == "error":
            assert c.returncode == 1
            assert rec["what"] == c.stderr.strip(), (k, rec, c.stderr)            # the same text, file names included
            assert not dst.exists() or dst.stat().st_size == 0, k
            continue
        assert c.returncode == 0, (k, c.stderr)
        assert dst.read_bytes() == want.read_bytes(), k
        check_ok_line(rec, src, dst)
    assert "Can not open input file" in results[0]["what"]
    assert "Checksum mismatch: packet 3 " in results[7]["what"]

    # against the golden survey vectors: the plain files whole, the others up to their trailer
    for dst, s in ((t / "j2.gip", sa), (t / "j9.gip", sa), (t / "j5.gip", sa), (t / "j4.gip", sb), (t / "j7.gip", sb)):
        blob = dst.read_bytes()
        assert header_sizes(blob) == (s["n"], s["gip_bytes"])
        assert hashlib.md5(blob[20:s["gip_bytes"]]).hexdigest() == s["stream_md5"]
        assert len(blob) == s["gip_bytes"] or blob[s["gip_bytes"]:s["gip_bytes"] + 4] == b"GIPX"
    assert len((t / "j2.gip").read_bytes()) == sa["gip_bytes"] and (t / "j9.gip").read_bytes() == (t / "j2.gip").read_bytes()
    for back, s in ((t / "j3.back", sa), (t / "j6.back", sa)):
        assert hashlib.md5(back.read_bytes()).hexdigest() == s["input_md5"]


def test_cpu_client_progress_line_script_on_stdin_and_malformed_scripts(host_client, tmp_path):
    """`quiet 0` brings the decile line back for that object only; the script may come on stdin; a malformed script is
    exit code 2, and a command without an object an `error` line."""
    src = tmp_path / "in.dat"
    synth.text(2, 30000).tofile(src)
    words = ["new", "cpu", "loud", "quiet", 0, "c", src, tmp_path / "a.gip", "new", "cpu", "silent", "c", src, tmp_path / "b.gip",
             "use", "loud", "d", tmp_path / "b.gip", tmp_path / "back", "delete", "loud", "c", src, tmp_path / "c.gip"]
    r, lines = run_script(host_client, words, through_stdin=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("100%..") == 2, r.stdout                           # the two jobs of `loud`, not the one of `silent`
    assert [l["status"] for l in lines] == ["ok"] * 8 + ["error"], r.stderr
    assert lines[-1]["what"] == "no current object"
    assert (tmp_path / "a.gip").read_bytes() == (tmp_path / "b.gip").read_bytes() and (tmp_path / "back").read_bytes() == src.read_bytes()
    for bad in (["frobnicate"], ["new", "cpu"], ["new", "tpu", "x"], ["use", "nobody"], ["new", "cpu", "x", "threads", "many"]):
        r, _ = run_script(host_client, bad)
        assert r.returncode == 2 and "class_client:" in r.stderr, (bad, r.stderr)


def test_gpu_clients_compile_and_link_and_say_so_without_a_device(tmp_path):
    """Both GPU clients build from the tree with the Makefile's flags for $(BIN)/gpuar, without host/main.cpp.  Where no
    device is visible each ends with a message, not a crash (where one is, the GPU tests below do the rest)."""
    torch = pytest.importorskip("torch")
    exe, exe2 = B.class_client_gpu(), B.executor_client()
    assert os.access(exe, os.X_OK) and os.access(exe2, os.X_OK)
    if torch.cuda.is_available():
        return
    r, lines = run_script(exe, ["new", "gpu", "g"])
    assert r.returncode == 0 and [l["status"] for l in lines] == ["error"] and "No HIP device" in lines[0]["what"], r.stderr
    src = tmp_path / "in.dat"
    src.write_bytes(b"hello")
    r = CHILDREN.run([exe2, "c", str(src), str(tmp_path / "out.gip")], CHILD_SECONDS)
    assert r.returncode == 1 and "error" in r.stderr, r.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def gpu_client():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return B.class_client_gpu()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two inputs of a few MiB (385 and 641 packets: at `batch 64` seven and eleven chunks, the last one ragged) and what
    `gpuar --host --threads=0` makes of them, plain and with checksums."""
    d = tmp_path_factory.mktemp("class_api")
    out = {"dir": d}
    for name, data in (("a", synth.zipf(4, 3 * 1024 * 1024 + 12345)), ("b", synth.text(9, 5 * 1024 * 1024 + 777))):
        src = d / f"{name}.dat"
        data.tofile(src)
        out[name] = src
        for tag, flags in (("", []), ("_ck", ["--checksum"])):
            gip = d / f"{name}{tag}.gip"
            r = cli(B.CLI, "c", "--host", "--threads=0", *flags, f"--in={src}", f"--out={gip}")
            assert r.returncode == 0, r.stderr
            out[name + tag + "_gip"] = gip
    empty = d / "empty.dat"
    empty.write_bytes(b"")
    r = cli(B.CLI, "c", "--host", f"--in={empty}", f"--out={d / 'empty.gip'}")
    assert r.returncode == 0 and (d / "empty.gip").stat().st_size == 20
    out["empty"], out["empty_gip"] = empty, d / "empty.gip"
    return out


def same(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def run_jobs(exe, words, jobs_expected, env=None):
    r, lines = run_script(exe, words, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    jobs = [l for l in lines if l["command"] in ("c", "d")]
    assert all(l["status"] == "ok" for l in lines if l["command"] not in ("c", "d")), r.stderr[-3000:]
    assert [l["status"] for l in jobs] == jobs_expected, r.stderr[-3000:]
    return jobs


@pytest.mark.gpu
def test_gpu_object_reuses_its_lanes_at_the_same_chunk_size(gpu_client, files, tmp_path):
    """compress, compress another file, decompress, decompress: the second job on finds the lanes' buffers, pinned pieces,
    streams and the device's epoch as the first left them (ensureBuffers' reuse branch)."""
    t, f = tmp_path, files
    jobs = run_jobs(gpu_client, ["new", "gpu", "g", "batch", 64, "c", f["a"], t / "a.gip", "c", f["b"], t / "b.gip",
                                 "d", t / "a.gip", t / "a.back", "d", t / "b.gip", t / "b.back"], ["ok"] * 4)
    assert same(t / "a.gip", f["a_gip"]) and same(t / "b.gip", f["b_gip"])          # header included
    assert same(t / "a.back", f["a"]) and same(t / "b.back", f["b"])
    for rec, (src, dst) in zip(jobs, ((f["a"], t / "a.gip"), (f["b"], t / "b.gip"), (t / "a.gip", t / "a.back"), (t / "b.gip", t / "b.back"))):
        check_ok_line(rec, src, dst)
        assert rec["processTime"] > 0, rec


@pytest.mark.gpu
def test_gpu_object_that_decompressed_first_can_compress(gpu_client, files, tmp_path):
    """Lanes allocated by a decompress have no slot buffer: a compress at the same chunk size must replace them, not launch
    into a null pointer.  Then the chunk size changes between jobs (everything released and allocated again), and back."""
    t, f = tmp_path, files
    jobs = run_jobs(gpu_client, ["new", "gpu", "g", "batch", 64, "d", f["a_gip"], t / "a.back", "c", f["a"], t / "a.gip",
                                 "batch", 128, "c", f["b"], t / "b.gip", "d", t / "b.gip", t / "b.back",
                                 "batch", 64, "d", f["b_gip"], t / "b.back2", "c", f["b"], t / "b2.gip"], ["ok"] * 6)
    assert same(t / "a.back", f["a"]) and same(t / "a.gip", f["a_gip"])
    assert same(t / "b.gip", f["b_gip"]) and same(t / "b.back", f["b"])
    assert same(t / "b.back2", f["b"]) and same(t / "b2.gip", f["b_gip"])
    for rec, (src, dst) in zip(jobs, ((f["a_gip"], t / "a.back"), (f["a"], t / "a.gip"), (f["b"], t / "b.gip"), (t / "b.gip", t / "b.back"),
                                      (f["b_gip"], t / "b.back2"), (f["b"], t / "b2.gip"))):
        check_ok_line(rec, src, dst)


@pytest.mark.gpu
def test_gpu_object_after_a_failed_job(gpu_client, files, tmp_path):
    """A decompress that fails in a late chunk (packet 64 * 17 + 5 claims ulen = 0xFFFF: refused by the decoder, no
    output), then good jobs on the same object.  The message is the CLI's, chunk offsets included; the lanes the failure
    stopped work again; and the kernel spans the failed job recorded are not billed to the next job: a job that runs no
    kernel (an empty file, either direction) reports processTime 0, as it does on a fresh object in the same process."""
    t, f = tmp_path, files
    src, good, bad = t / "in.dat", t / "good.gip", t / "bad.gip"
    data = synth.text(21, 64 * 30 * 8192 + 777)              # 30 chunks of 64 packets, the last one ragged
    data.tofile(src)
    assert cli(B.CLI, "c", "--host", "--threads=0", f"--in={src}", f"--out={good}").returncode == 0
    blob = bytearray(good.read_bytes())
    at = 20
    for _ in range(64 * 17 + 5):
        at += blob[at] | (blob[at + 1] << 8)
    blob[at + 2:at + 4] = b"\xff\xff"
    bad.write_bytes(blob)
    c = cli(B.CLI, "d", f"--in={bad}", f"--out={t / 'cli.back'}", "--batch=64")
    assert c.returncode == 1 and "Incorrect file format (malformed packet between file offsets" in c.stderr, c.stderr

    (t / "bad.back").write_bytes(b"stale")
    words = ["new", "gpu", "fresh", "batch", 64, "c", f["empty"], t / "e0.gip", "d", f["empty_gip"], t / "e0.back",
             "new", "gpu", "g", "batch", 64,
             "d", bad, t / "bad.back", "d", good, t / "good.back", "c", f["empty"], t / "e1.gip",
             "d", bad, t / "bad.back2", "d", f["empty_gip"], t / "e1.back", "d", good, t / "good.back2"]
    jobs = run_jobs(gpu_client, words, ["ok", "ok", "error", "ok", "ok", "error", "ok", "ok"])
    fresh_c, fresh_d, fail1, ok1, empty_c, fail2, empty_d, ok2 = jobs
    assert fail1["what"] == c.stderr.strip() and fail2["what"] == c.stderr.strip()
    assert (t / "bad.back").stat().st_size == 0 and (t / "bad.back2").stat().st_size == 0
    assert same(t / "good.back", src) and same(t / "good.back2", src)
    assert same(t / "e0.gip", f["empty_gip"]) and same(t / "e1.gip", f["empty_gip"])
    assert (t / "e0.back").stat().st_size == 0 and (t / "e1.back").stat().st_size == 0
    print("processTime of the empty jobs: fresh object", fresh_c["processTime"], fresh_d["processTime"],
          "-- after a failed job", empty_c["processTime"], empty_d["processTime"])
    print("decompress after the failed job: processTime", ok1["processTime"], ok2["processTime"], "wall", ok1["wall_ms"], ok2["wall_ms"])
    assert fresh_c["processTime"] == 0 and fresh_d["processTime"] == 0
    assert empty_c["processTime"] == fresh_c["processTime"]
    assert empty_d["processTime"] == fresh_d["processTime"]
    for rec, (a, b) in ((fresh_c, (f["empty"], t / "e0.gip")), (fresh_d, (f["empty_gip"], t / "e0.back")), (ok1, (good, t / "good.back")),
                        (empty_c, (f["empty"], t / "e1.gip")), (empty_d, (f["empty_gip"], t / "e1.back")), (ok2, (good, t / "good.back2"))):
        check_ok_line(rec, a, b)


@pytest.mark.gpu
def test_gpu_object_turns_checksums_on_and_off_on_reused_lanes(gpu_client, files, tmp_path):
    """A plain job allocates the lanes without room for CRCs; `checksum 1` jobs on the same lanes then need it (compress
    and the verifying decompress), a flipped data bit is named by packet as the CLI names it, and `checksum 0` afterwards
    writes the plain file again."""
    t, f = tmp_path, files
    blob = bytearray(f["a_ck_gip"].read_bytes())
    at, packet = 20, 64 * 4 + 9                             # a packet of the fifth chunk
    for _ in range(packet):
        at += blob[at] | (blob[at + 1] << 8)
    blob[at + (blob[at] | (blob[at + 1] << 8)) // 2] ^= 0x04          # one data bit in the middle of it
    flipped = t / "flipped.gip"
    flipped.write_bytes(blob)
    c = cli(B.CLI, "d", f"--in={flipped}", f"--out={t / 'cli.back'}", "--batch=64")
    assert c.returncode == 1 and f"Checksum mismatch: packet {packet} " in c.stderr, c.stderr

    jobs = run_jobs(gpu_client, ["new", "gpu", "g", "batch", 64, "c", f["a"], t / "plain.gip", "checksum", 1, "c", f["a"], t / "ck.gip",
                                 "d", t / "ck.gip", t / "ck.back", "d", flipped, t / "flipped.back",
                                 "checksum", 0, "c", f["a"], t / "plain2.gip", "d", t / "ck.gip", t / "ck.back2"],
                    ["ok", "ok", "ok", "error", "ok", "ok"])
    assert jobs[3]["what"] == c.stderr.strip(), (jobs[3], c.stderr)
    assert (t / "flipped.back").stat().st_size == 0
    assert same(t / "plain.gip", f["a_gip"]) and same(t / "plain2.gip", f["a_gip"])
    assert same(t / "ck.gip", f["a_ck_gip"])
    assert same(t / "ck.back", f["a"]) and same(t / "ck.back2", f["a"])
    for rec, (a, b) in zip([j for j in jobs if j["status"] == "ok"],
                           ((f["a"], t / "plain.gip"), (f["a"], t / "ck.gip"), (t / "ck.gip", t / "ck.back"), (f["a"], t / "plain2.gip"), (t / "ck.gip", t / "ck.back2"))):
        check_ok_line(rec, a, b)


@pytest.mark.gpu
def test_gpu_object_changes_its_devices_between_jobs(gpu_client, files, tmp_path):
    """gpus 3, device 0, gpus 2, gpus 8 on one object (logical devices oversubscribed onto the one card, all in the one
    child): every change releases the lanes and the per-device epochs of the job before; every file equals the
    single-device file."""
    t, f = tmp_path, files
    env = dict(os.environ, GPUAR_OVERSUBSCRIBE_DEVICES="1")
    jobs = run_jobs(gpu_client, ["new", "gpu", "g", "batch", 64, "gpus", 3, "c", f["a"], t / "g3.gip", "device", 0, "c", f["b"], t / "d0.gip",
                                 "gpus", 2, "d", t / "g3.gip", t / "g2.back", "gpus", 8, "c", f["a"], t / "g8.gip", "d", t / "d0.gip", t / "g8.back"],
                    ["ok"] * 5, env=env)
    assert same(t / "g3.gip", f["a_gip"]) and same(t / "d0.gip", f["b_gip"]) and same(t / "g8.gip", f["a_gip"])
    assert same(t / "g2.back", f["a"]) and same(t / "g8.back", f["b"])
    for rec, (a, b) in zip(jobs, ((f["a"], t / "g3.gip"), (f["b"], t / "d0.gip"), (t / "g3.gip", t / "g2.back"), (f["a"], t / "g8.gip"), (t / "d0.gip", t / "g8.back"))):
        check_ok_line(rec, a, b)


@pytest.mark.gpu
def test_gpu_objects_are_deleted_created_and_used_side_by_side(gpu_client, files, tmp_path):
    """The class, unlike the CLI, must survive its own teardown in mid-process: delete after a job, new, a job; then two
    GPU objects alive at once and used in turn; and the client returns from main() with both alive, exit code 0."""
    t, f = tmp_path, files
    jobs = run_jobs(gpu_client, ["new", "gpu", "one", "batch", 64, "c", f["a"], t / "x1.gip", "delete", "one",
                                 "new", "gpu", "one", "batch", 64, "c", f["a"], t / "x2.gip",
                                 "new", "gpu", "two", "batch", 64, "c", f["b"], t / "y1.gip",
                                 "use", "one", "d", t / "y1.gip", t / "y1.back", "use", "two", "d", t / "x2.gip", t / "x2.back",
                                 "use", "one", "c", f["b"], t / "y2.gip", "use", "two", "c", f["a"], t / "x3.gip"], ["ok"] * 7)
    assert same(t / "x1.gip", f["a_gip"]) and same(t / "x2.gip", f["a_gip"]) and same(t / "x3.gip", f["a_gip"])
    assert same(t / "y1.gip", f["b_gip"]) and same(t / "y2.gip", f["b_gip"])
    assert same(t / "y1.back", f["b"]) and same(t / "x2.back", f["a"])
    for rec, (a, b) in zip(jobs, ((f["a"], t / "x1.gip"), (f["a"], t / "x2.gip"), (f["b"], t / "y1.gip"), (t / "y1.gip", t / "y1.back"),
                                  (t / "x2.gip", t / "x2.back"), (f["b"], t / "y2.gip"), (f["a"], t / "x3.gip"))):
        check_ok_line(rec, a, b)
