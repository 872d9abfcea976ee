"""The last, partial quad of a packet at every size on the MI355X: move_packets, sparse_pack, sparse_unpack, kinds_store and
kinds_expand share one store for it (store_partial_quad; kinds_expand's raw path keeps a copy that loads as it stores), so each
of the five is driven with packets whose last quad holds r bytes for every r = 1 .. 15, at the lengths r, 16 + r and 8176 + r:
the only quad of a packet, the second, and the last quad of the last lane.  Every output is compared byte for byte with the
host twin (a plain copy for move_packets), behind every destination stands a 0x5A canary, and the status word is 0.  The raw
path gets random bytes; the sparse path zeros with byte 0 = 0x11 and the last byte = 0xA5, so that an exception lands in the
partial quad (at 3 and 4 bytes, where two exceptions leave no majority byte, the last byte alone; the region kernels take no
shorter packet, a record needing 2 k < n, and the kinds kernels the sparse lengths above 16, where the rule says sparse).  No damaged packets here: tests/test_gpu_sparse.py and tests/test_gpu_kinds.py have them for both callers of the
shared builder."""
import numpy as np
import pytest

from test_gpu_kinds import H, _check_store, _expand  # noqa: F401  (H: the module-scoped fixture)
from test_gpu_sparse import _i64, _pack, _status, _unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
RAW, SPARSE = 1, 2
LENGTHS = [base + r for base in (0, 16, PACKET - 16) for r in range(1, 16)]
RESIDUES = set(range(1, 16))


def _ends(n):
    """zeros with the last byte 0xA5 and, where zero then still is the majority byte (n >= 5), byte 0 = 0x11"""
    x = np.zeros(n, dtype=np.uint8)
    x[-1] = 0xA5
    if n >= 5:
        x[0] = 0x11
    return x


@pytest.fixture(scope="module")
def ragged(H):  # noqa: F811
    """(the raw packets, the sparse packets of the kinds kernels, the sparse packets of the region kernels), each {length: bytes},
    after the host functions alone have said that every residue occurs in each: a changed rule cannot empty the tests below"""
    rng = np.random.default_rng(20251)
    raws = {n: rng.integers(0, 256, n, dtype=np.uint8) for n in LENGTHS}
    sparses = {n: _ends(n) for n in LENGTHS if n > 16}
    regions = {n: _ends(n) for n in LENGTHS if n >= 3}          # a record needs 2 k < n
    assert all(H.kinds_store_host(x.tobytes(), True, True)[0] == RAW for x in raws.values())
    assert all(H.kinds_store_host(x.tobytes(), True, True)[0] == SPARSE for x in sparses.values())
    for n, x in regions.items():
        scan = H.sparse_scan_host(x.tobytes())[0]
        assert scan == ((2 if n >= 5 else 1) << 8), (n, scan)
    assert {n % 16 for n in raws} == {n % 16 for n in sparses} == {n % 16 for n in regions} == RESIDUES
    assert len(raws) == 45 and len(sparses) == 30 and len(regions) == 43
    return raws, sparses, regions


def _device(x):
    """the packet in an allocation of its own that ends with the 16-byte piece that holds its last byte"""
    t = torch.full(((x.size + 15) // 16 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    t[:x.size] = torch.from_numpy(x).cuda()
    return t


def _front():
    """a full packet that holds every byte value 32 times: raw"""
    return (np.arange(PACKET) % 256).astype(np.uint8)


def test_move_packets_at_every_residue(H, ragged):  # noqa: F811
    parts = list(ragged[0].values())
    srcs = [_device(x) for x in parts]
    n, room = len(parts), PACKET + 64
    dst = torch.full((n * room,), 0x5A, dtype=torch.uint8, device="cuda")
    status = _status()
    H.move_packets(_i64([t.data_ptr() for t in srcs]), _i64([dst.data_ptr() + r * room for r in range(n)]), _i64([x.size for x in parts]), n,
                   d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    for r, x in enumerate(parts):
        assert (got[r * room:r * room + x.size] == x).all(), x.size
        assert (got[r * room + x.size:(r + 1) * room] == 0x5A).all(), (x.size, "wrote behind the packet")


def test_sparse_pack_at_every_residue(H, ragged):  # noqa: F811
    parts = list(ragged[2].values())
    recs = [H.sparse_pack_host(x.tobytes()) for x in parts]
    flags, got, offs = _pack(H, [_device(x) for x in parts], [x.size for x in parts], [H.sparse_scan_host(x.tobytes())[0] for x in parts],
                             [len(r) for r in recs])
    assert flags == 0
    assert (got[:4] == 0x5A).all()
    for r, (x, rec) in enumerate(zip(parts, recs)):
        assert got[offs[r]:offs[r] + len(rec)].tobytes() == rec, x.size
        assert (got[offs[r] + len(rec):offs[r + 1]] == 0x5A).all(), (x.size, "wrote behind the record")


def test_sparse_unpack_at_every_residue(H, ragged):  # noqa: F811
    parts = list(ragged[2].values())
    recs = [H.sparse_pack_host(x.tobytes()) for x in parts]
    flags, got, offs = _unpack(H, recs, [len(r) for r in recs], [x.size for x in parts])
    assert flags == 0
    for r, (x, rec) in enumerate(zip(parts, recs)):
        assert got[offs[r]:offs[r] + x.size].tobytes() == H.sparse_unpack_host(rec, x.size) == x.tobytes(), x.size
        assert (got[offs[r] + x.size:offs[r + 1]] == 0x5A).all(), (x.size, "wrote behind the packet")


def test_kinds_store_at_every_residue(H, ragged):  # noqa: F811
    """the partial packet is its buffer's last, behind one full raw packet; _check_store compares every slot with kinds_store_host
    and the bytes beyond clen, behind the last slot and behind the kinds with what stood there"""
    front = _front()
    for want, family in ((RAW, ragged[0]), (SPARSE, ragged[1])):
        for n, x in family.items():
            assert H.kinds_store_host(x.tobytes(), True, True)[0] == want
            assert _check_store(H, [front, x], True, True) == {RAW, want}, n


def test_kinds_expand_at_every_residue(H, ragged):  # noqa: F811
    """[a full raw packet][the partial packet, last in the stream: nothing of the buffer is behind its last byte but the guard],
    the stream starting at byte 1 .. 16 of its buffer"""
    front = _front()
    first = H.kinds_store_host(front.tobytes(), True, True)
    assert first[0] == RAW
    for want, family in ((RAW, ragged[0]), (SPARSE, ragged[1])):
        for n, x in family.items():
            kind, pkt = H.kinds_store_host(x.tobytes(), True, True)
            assert kind == want
            flags, out, _offsets = _expand(H, [first[1], pkt], [RAW, kind], PACKET + n, shift=1 + n % 16)
            assert flags == 0, (n, flags)
            assert out[:PACKET].tobytes() == front.tobytes(), n
            assert out[PACKET:PACKET + n].tobytes() == H.kinds_expand_host(pkt, kind, n) == x.tobytes(), (n, kind)
            assert (out[PACKET + n:] == 0x5A).all(), (n, "wrote behind the packet")
