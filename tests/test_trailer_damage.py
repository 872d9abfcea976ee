"""What `gpuar d --host` makes of a damaged trailer (no GPU needed): four small files -- `--index`, `--checksum`, `--planes=2`,
`--planes=2 --checksum` -- cut at every length behind the stream and with every trailer byte flipped, each decoded and held
against trailer_ref's restatement of the format: which damage is silence, which a warning, which a checksum error and which
a refusal.  And the three writers of the trailer -- the C++ one, batch.trailer and trailer_ref.write -- against each other."""
import os
import subprocess

import pytest

import trailer_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gpuar_amd", "bin")


@pytest.fixture(scope="module")
def host_cli():
    if not os.path.exists(os.path.join(BIN, "gpuar-host")):
        import __graft_entry__ as g
        g.build()
    return os.path.join(BIN, "gpuar-host")


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def files(host_cli, tmp_path_factory):
    """(the input, the four files `gpuar-host c` writes for it)"""
    d = tmp_path_factory.mktemp("trailers")
    x = T.sweep_input()
    (d / "in").write_bytes(x)
    out = []
    for i, flags in enumerate(T.FLAGS):
        r = run(host_cli, "c", "--host", *flags, f"--in={d / 'in'}", f"--out={d / f'{i}.gip'}")
        assert r.returncode == 0, r.stderr
        out.append((d / f"{i}.gip").read_bytes())
    return x, out


def test_every_cut_and_every_flipped_byte_of_every_trailer(host_cli, files, tmp_path):
    """(A trailer that says version 2 and does not fit leaves the stream as it is: for a planes file whose version byte became
    2 that is the split bytes, with the warning.)"""
    x, goods = files
    seen, checked, runs = set(), set(), 0
    gip, out = tmp_path / "case.gip", tmp_path / "case.out"
    for i, good in enumerate(goods):
        assert len(good) - T.stream_end(good) == T.TRAILER_BYTES[i]
        assert T.classify(good)[:2] == ("ok", (1, 2, 3, 3)[i]) and len(T.classify(good)[2]) == 3
        for what, blob in T.damaged(good):
            case = (T.FLAGS[i], what)
            status = T.classify(blob)[0]
            code, cls, want = T.expected(blob, x, split=i >= 2)
            gip.write_bytes(blob)
            out.unlink(missing_ok=True)
            r = run(host_cli, "d", "--host", f"--in={gip}", f"--out={out}")
            runs += 1
            assert r.returncode in (0, 1), (case, r.returncode, r.stderr)
            assert (r.returncode, T.stderr_class(r.returncode, r.stderr)) == (code, cls), (case, status, r.stderr)
            if want is not None:
                assert out.read_bytes() == want, (case, status)
            if status == "ok" and i >= 1 and code == 0:
                assert want == x, case
            seen.add(status)
            if cls.startswith("checksum"):
                checked.add("mismatch")
            elif status == "ok" and T.classify(blob)[3] is not None:
                checked.add("match")
    assert runs == sum(1 + 3 * n for n in T.TRAILER_BYTES)
    assert seen == {"none", "ok", "malformed", "unusable"} and checked == {"match", "mismatch"}


def test_the_three_writers_agree(files):
    from gpuar_amd import batch
    _, goods = files
    for i, good in enumerate(goods):
        status, version, clens, crcs, elem_bytes = T.classify(good)
        assert status == "ok" and (crcs is not None) == (i in (1, 3)) and elem_bytes == (1, 1, 2, 2)[i]
        trailer = good[T.stream_end(good):]
        assert T.write(clens, elem_bytes, crcs) == trailer, T.FLAGS[i]
        assert batch.trailer(clens, elem_bytes, crcs) == trailer, T.FLAGS[i]


def test_a_packet_count_whose_doubling_wraps_is_a_damaged_trailer(host_cli, files, tmp_path):
    """n = 2^63 + 3 in the `--index` file: 2 n is 6 again in 64 bits, so sizes computed from it would fit the file.  The count
    is bounded by the room behind the stream first: a damaged version 1, dropped silently."""
    x, goods = files
    blob = bytearray(goods[0])
    blob[T.stream_end(goods[0]) + 15] ^= 0x80
    assert T.classify(bytes(blob))[0] == "none"
    gip, out = tmp_path / "wrap.gip", tmp_path / "wrap.out"
    gip.write_bytes(bytes(blob))
    r = run(host_cli, "d", "--host", f"--in={gip}", f"--out={out}")
    assert (r.returncode, r.stderr) == (0, "") and out.read_bytes() == x
