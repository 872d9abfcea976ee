"""What tests/test_capi_codes_host.py cannot see without a device: the checks gpuar_hip_kinds_store makes once it has its status
word, and one well-formed call of every per-packet and per-region entry point at the smallest sizes where a launch's grid and its
tail can go wrong -- 1 byte, 5 packets less 3 bytes (one packet past a 4-wavefront workgroup), 9 packets (one past a survey
window), 17 packets (one past a 16-wavefront workgroup), and a batch of 0, 1, 8192 and 8193 bytes.  Every call returns 0 (the
bindings raise otherwise), leaves its status word 0 and gives what its *_host twin gives (zlib.crc32 for the CRCs)."""
import numpy as np
import pytest

import kinds_ref as K
import sparse_ref as S
from test_gpu_checksum import crc_list, zcrcs
from test_gpu_kinds import _check_store, _expand, _filler
from test_gpu_sparse import _i32, _i64, _pack, _status, _u32, _unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET, SLOT = 8192, 8704
SIZES = [1, 5 * PACKET - 3, 9 * PACKET, 17 * PACKET]
BATCH = [0, 1, PACKET, PACKET + 1]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def full():
    """the 8192-byte packets of kinds_ref: (a mix of coded, raw and sparse ones, the ones that have a majority byte)"""
    packets = dict(K.packets())
    names = sorted(n for n, x in packets.items() if x.size == PACKET)
    mixed = [packets[n] for n in names if n.startswith(("text", "uniform", "zeros", "fill80_k64", "ends"))]
    return mixed, [packets[n] for n in names if S.scan(packets[n]) != S.NONE]


def parts_of(source, n_bytes):
    """n_bytes as packets taken in turn from `source`, the last one cut short"""
    count = (n_bytes + PACKET - 1) // PACKET
    parts = [source[i % len(source)] for i in range(count)]
    parts[-1] = parts[-1][:n_bytes - (count - 1) * PACKET]
    return parts


def _descriptors(H, hosts):
    ts = [torch.from_numpy(h).cuda() for h in hosts]
    sizes = [h.size for h in hosts]
    first_packet, n_packets = H.batch_packet_count(sizes)
    return ts, (_i64([t.data_ptr() if t.numel() else 0 for t in ts]), _i64(sizes), _i64(first_packet), len(hosts), n_packets)


def _survey_rows(d_est):
    return [_u32(row) for row in d_est]


@pytest.mark.parametrize("n_bytes", SIZES)
def test_one_buffer_gives_what_the_host_gives(H, full, n_bytes):
    host = np.concatenate(parts_of(full[0], n_bytes))
    data, d_in = host.tobytes(), torch.from_numpy(host).cuda()
    npk = H.packet_count(n_bytes)
    d_crc = H.crc32(d_in)
    assert crc_list(d_crc, npk) == zcrcs(data)
    status, first_bad = _status(), torch.full((1,), -1, dtype=torch.int64, device="cuda")
    H.verify_crc32(d_in, d_crc, d_first_bad=first_bad, d_status=status)
    assert int(status.item()) == 0 and int(first_bad.item()) == -1
    assert _u32(H.estimate(d_in)) == H.estimate_host(data)
    assert _u32(H.sparse_scan(d_in)) == H.sparse_scan_host(data)
    assert _survey_rows(H.survey_planes(d_in)) == H.survey_planes_host(data)
    assert _survey_rows(H.survey_delta(d_in)) == H.survey_delta_host(data)
    assert H.status() == 0                                     # the word of the calls that take none of their own


def test_a_batch_gives_what_the_host_gives(H, full):
    hosts = [np.concatenate(parts_of(full[0][b:], n)) if n else np.empty(0, dtype=np.uint8) for b, n in enumerate(BATCH)]
    _ts, desc = _descriptors(H, hosts)
    status = _status()
    d_crc = H.crc32_batch(*desc, d_status=status)
    assert crc_list(d_crc, desc[-1]) == [c for h in hosts for c in zcrcs(h.tobytes())]
    first_bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    H.verify_crc32_batch(*desc, d_crc, first_bad, d_status=status)
    assert int(first_bad.item()) == -1
    assert _u32(H.estimate_batch(*desc, d_status=status)) == [e for h in hosts for e in H.estimate_host(h.tobytes())]
    assert _u32(H.sparse_scan_batch(*desc, d_status=status)) == [s for h in hosts for s in H.sparse_scan_host(h.tobytes())]
    for device, on_host in ((H.survey_planes_batch, H.survey_planes_host), (H.survey_delta_batch, H.survey_delta_host)):
        want = [on_host(h.tobytes()) for h in hosts]
        assert _survey_rows(device(*desc, d_status=status)) == [[e for w in want for e in w[j]] for j in range(4)]
    assert int(status.item()) == 0


@pytest.mark.parametrize("n_bytes", SIZES)
def test_regions_give_what_the_host_gives(H, full, n_bytes):
    """the packets of a buffer of n_bytes as the regions of move_packets, sparse_pack and sparse_unpack"""
    parts = parts_of(full[1], n_bytes)
    sizes = [x.size for x in parts]
    srcs = [torch.from_numpy(np.resize(x, (x.size + 15) // 16 * 16)).cuda() for x in parts]
    n = len(parts)
    dst = torch.full((n * PACKET + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    status = _status()
    H.move_packets(_i64([t.data_ptr() for t in srcs]), _i64([dst.data_ptr() + r * PACKET for r in range(n)]), _i64(sizes), n, d_status=status)
    assert int(status.item()) == 0
    got = dst.cpu().numpy()
    for r, x in enumerate(parts):
        assert (got[r * PACKET:r * PACKET + x.size] == x).all() and (got[r * PACKET + x.size:(r + 1) * PACKET] == 0x5A).all(), r
    assert (got[n * PACKET:] == 0x5A).all()
    recs = [H.sparse_pack_host(x.tobytes()) for x in parts]
    flags, got, offs = _pack(H, srcs, sizes, H.sparse_scan_host(np.concatenate(parts).tobytes()), [len(r) for r in recs])
    assert flags == 0
    for r, rec in enumerate(recs):
        assert got[offs[r]:offs[r] + len(rec)].tobytes() == rec and (got[offs[r] + len(rec):offs[r + 1]] == 0x5A).all(), r
    flags, got, offs = _unpack(H, recs, [len(r) for r in recs], sizes)
    assert flags == 0
    for r, (rec, x) in enumerate(zip(recs, parts)):
        assert got[offs[r]:offs[r] + x.size].tobytes() == H.sparse_unpack_host(rec, x.size) == x.tobytes(), r
        assert (got[offs[r] + x.size:offs[r + 1]] == 0x5A).all(), r


@pytest.mark.parametrize("n_bytes", SIZES)
def test_kinds_give_what_the_host_gives(H, full, n_bytes):
    parts = parts_of(full[0], n_bytes)
    _check_store(H, parts, True, True)                         # status 0, kinds and slots against gpuar_hip_kinds_store_host
    stored = [H.kinds_store_host(x.tobytes(), True, True) for x in parts]
    assert any(kind != K.CODED for kind, _pkt in stored)       # something to expand
    stream_packets = [pkt if kind != K.CODED else _filler(100) for kind, pkt in stored]
    kinds = [kind for kind, _pkt in stored]
    flags, out, _offsets = _expand(H, stream_packets, kinds, n_bytes)
    assert flags == 0
    for p, (x, (kind, pkt)) in enumerate(zip(parts, stored)):
        got = out[p * PACKET:p * PACKET + x.size]
        if kind == K.CODED:
            assert (got == 0x5A).all(), p
        else:
            assert got.tobytes() == H.kinds_expand_host(pkt, kind, x.size) == x.tobytes(), p
    assert (out[n_bytes:] == 0x5A).all()


def test_kinds_store_checks_behind_the_status_word(H, full):
    """d_slots and d_kind null: GPUAR_ERR_ARGUMENT; d_slots (16) and d_scan (4) misaligned: GPUAR_ERR_ALIGNMENT; and nothing ran."""
    lib = H.load()
    host = np.concatenate(parts_of(full[0], 2 * PACKET))
    d_in = torch.from_numpy(host).cuda()
    d_est, d_scan = _i32([5000, 5000]), _i32([S.NONE, S.NONE])
    slots = torch.full((2 * SLOT + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    kinds = torch.full((16,), 0x5A, dtype=torch.uint8, device="cuda")
    status = _status()
    i, e, c, s, k, w = d_in.data_ptr(), d_est.data_ptr(), d_scan.data_ptr(), slots.data_ptr(), kinds.data_ptr(), status.data_ptr()
    for w_or_none in (w, None):
        assert lib.gpuar_hip_kinds_store(i, host.size, e, c, 1, None, k, w_or_none, None) == -2
        assert lib.gpuar_hip_kinds_store(i, host.size, e, c, 1, s, None, w_or_none, None) == -2
        assert lib.gpuar_hip_kinds_store(i, host.size, e, c, 1, s + 8, k, w_or_none, None) == -1
        assert lib.gpuar_hip_kinds_store(i, host.size, e, c + 2, 1, s, k, w_or_none, None) == -1
        assert lib.gpuar_hip_kinds_store(i, host.size, e, c + 2, 1, None, k, w_or_none, None) == -2       # null and misaligned: the null
    torch.cuda.synchronize()
    assert slots.eq(0x5A).all() and kinds.eq(0x5A).all() and int(status.item()) == 0 and H.status() == 0
