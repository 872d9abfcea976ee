"""The reference of the file-pipeline tests, without a GPU: what `gpuar-host --host` makes of the matrix input under every flag set
is the file gip_files.expected restates, and decodes; the packet kinds of that input -- from kinds_ref alone -- reach every branch
the GPU test is there for; and the spliced files (short packets in the middle of a stream) decode to their parts or are refused, and
their short packets sit where the pipeline's paths part."""
import pytest

import cli_matrix as M
import gip_files as G
import kinds_ref as K
import trailer_ref as T

IDS = [name for name, _flags, _says in M.FLAG_SETS]


@pytest.fixture(scope="module")
def data():
    return M.matrix_input()


def test_the_flag_sets_and_shapes_are_the_ones_named():
    assert len(M.FLAG_SETS) == 21 and len(set(IDS)) == 21 and M.FLAG_SETS[:15] == G.FLAG_SETS
    assert [name for name, _a, _e in M.SHAPES] == ["default", "batch64", "batch100", "gpus2_batch64", "gpus3", "batch128_no_mmap"]


def test_the_input_is_whole_segments_and_its_base_differs(data):
    x, base = data
    assert x.size == (6 * 64 + 17) * M.PACKET + 4097 and base.size == x.size
    seg = 64 * M.PACKET
    assert not x[seg:2 * seg].any() and (x[:seg] != base[:seg]).mean() > 0.99
    differs = (x[seg:3 * seg] != base[seg:3 * seg]).nonzero()[0]
    assert differs.size == len(range(-seg % 977, 2 * seg, 977)) and (x[seg:3 * seg][differs] ^ base[seg:3 * seg][differs] == 0x11).all()


@pytest.mark.parametrize("name", IDS)
def test_the_host_file_is_its_restatement_and_decodes(tmp_path, data, name):
    x, base = data
    flags, says = M.FLAGS[name]
    blob = G.write(tmp_path, x, flags, base if says.get("base") else None)
    G.expected(blob, x, says, base)
    based = [f"--base={tmp_path / 'base.bin'}"] if says.get("base") else []
    r = M.host("d", tmp_path / "out.gip", tmp_path / "back", based)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "back").read_bytes() == x.tobytes()


@pytest.mark.parametrize("name", [n for n, _f, says in M.FLAG_SETS if says.get("stored") or says.get("sparse")])
def test_the_kinds_reach_every_branch(data, name):
    x, base = data
    _flags, says = M.FLAGS[name]
    kinds = M.kinds_of(x, base, says)
    allowed = {K.CODED} | ({K.RAW} if says.get("stored") else set()) | ({K.SPARSE} if says.get("sparse") else set())
    chunks = [set(kinds[at:at + M.CHUNK]) for at in range(0, len(kinds), M.CHUNK)]
    print(name, [sorted(c) for c in chunks])
    assert set(kinds) == allowed
    assert any(K.CODED not in c for c in chunks), "a chunk that launches no decoder"
    if says.get("stored"):
        assert any(c == {K.RAW} for c in chunks), "a chunk of raw packets alone"
    assert any(len(c) >= 2 for c in chunks), "a chunk of two kinds or more"


@pytest.fixture(scope="module")
def splices(tmp_path_factory):
    parts = M.splice_parts()
    return {trailer: M.spliced(tmp_path_factory.mktemp("splice"), parts, trailer) for trailer in M.SPLICE_TRAILERS}


def test_the_short_packets_sit_where_the_paths_part():
    ulens, short = M.splice_ulens()
    assert len(ulens) == 164 and short == [63, 64, 66, 67, 162]


def test_spliced_files_decode_to_their_parts_or_are_refused(tmp_path, splices):
    _ulens, short = M.splice_ulens()
    verdicts = M.splice_verdicts(tmp_path, splices)
    for trailer in (None, "index"):
        assert verdicts[trailer] == (0, "quiet", splices[trailer][1]), (trailer, verdicts[trailer][:2])
    assert T.classify(splices["index"][0])[:2] == ("ok", 1) and T.classify(splices["crcs"][0])[:2] == ("ok", 2)
    assert T.classify(splices["planes"][0])[:2] == ("ok", 3)
    assert verdicts["crcs"][:2] == (1, f"checksum {short[0]}")
    code, cls, _out = verdicts["planes"]
    assert code == 1 and f"packet {short[0]} of a file of byte planes is not the last one" in cls
