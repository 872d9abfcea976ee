"""Helpers of the XOR-survey tests (not a test module): a numpy restatement of gpuar_amd/csrc/xor_survey.h -- XOR, planes_ref's
split, the exact-integer estimate and the majority scan --, the inputs the issue names and the scan-edge pairs per width."""
import numpy as np

import planes_ref as PR
import sparse_ref as SR
import xor_ref as XR
from test_estimate_host import COUNTS, PACKET, lg16

WIDTHS = (1, 2, 4, 8)
SG = 8 * PACKET
NONE = 0xFFFFFFFF

_LF = [0, 0]
for _c in range(2, COUNTS):
    _LF.append(_LF[-1] + lg16(_c))
_LF = np.array(_LF, dtype=np.int64)


def packet_values(packet):
    """(estimate, scan word) of one packet from its histogram, in exact integers"""
    h = np.bincount(packet, minlength=256)
    cost16 = int(_LF[packet.size + 255] - _LF[255] - _LF[h].sum())
    top = int(h.argmax())
    scan = ((packet.size - int(h[top])) << 8 | top) if 2 * int(h[top]) > packet.size else NONE
    return 4 + ((cost16 + (1 << 19) - 1) >> 19), scan


def survey_xor(x, b):
    """(est rows, scan rows): four lists each, one entry per packet, by the definition -- supergroup by supergroup, each split as
    a buffer of its own"""
    x, b = np.frombuffer(bytes(x), dtype=np.uint8), np.frombuffer(bytes(b), dtype=np.uint8)
    assert x.size == b.size
    y = x ^ b
    est, scan = [[] for _ in WIDTHS], [[] for _ in WIDTHS]
    for j, w in enumerate(WIDTHS):
        for at in range(0, y.size, SG):
            s = PR.numpy_split(y[at:at + SG], w)
            for p in range(0, s.size, PACKET):
                e, k = packet_values(s[p:p + PACKET])
                est[j].append(e)
                scan[j].append(k)
    return est, scan


def int64_pair():
    """1 MiB of int64 indices below 50 000 as the base, 1 % of them replaced as the tensor: (tensor bytes, base bytes)"""
    rng = np.random.default_rng(1)
    idx = rng.integers(0, 50000, 131072).astype('<i8')
    m = rng.random(131072) < 0.01
    x = idx.copy()
    x[m] = rng.integers(0, 50000, m.sum())
    return x.view(np.uint8).copy(), idx.view(np.uint8).copy()


def table_pairs():
    """DESIGN.md 4.10's table pairs: {name: (tensor bytes, base bytes)}"""
    return {name: (np.ascontiguousarray(x), np.ascontiguousarray(b)) for name, (x, b, _w) in XR.table_pairs().items()}


def plane_with(n, w, k, equal, fill_xor, seed):
    """(x, b) of n bytes (one supergroup or less) such that plane packet k of split_planes(x ^ b, w) holds exactly `equal` bytes of
    the value fill_xor and no other value more than once over that often: the rest of the packet cycles through other values"""
    rng = np.random.default_rng(seed)
    split = rng.integers(0, 256, n, dtype=np.uint8)
    lo, hi = k * PACKET, min(n, (k + 1) * PACKET)
    packet = np.empty(hi - lo, dtype=np.uint8)
    packet[:equal] = fill_xor
    others = np.array([v for v in range(256) if v != fill_xor], dtype=np.uint8)
    packet[equal:] = others[np.arange(hi - lo - equal) % 255]
    split[lo:hi] = rng.permutation(packet)
    y = PR.numpy_merge(split, w)
    b = rng.integers(0, 256, n, dtype=np.uint8)
    return (y ^ b), b


def scan_edges(w):
    """[(tag, x, b, packet, scan word wanted at width w in that packet)]: exactly half equal (none), half + 1 (k = n/2 - 1), an odd
    short packet, a fill that is not 0, x equal to its base"""
    out = []
    n, k = SG, w - 1 if w > 1 else 3
    x, b = plane_with(n, w, k, PACKET // 2, 0, 10 + w)
    out.append(("half", x, b, k, NONE))
    x, b = plane_with(n, w, k, PACKET // 2 + 1, 0, 20 + w)
    out.append(("half+1", x, b, k, (PACKET // 2 - 1) << 8))
    n = 2 * PACKET + 4099 if w <= 2 else w * PACKET + 4099        # a last packet of 4099 bytes: odd
    last = (n - 1) // PACKET
    m = n - last * PACKET
    x, b = plane_with(n, w, last, m // 2 + 1, 0x5A, 30 + w)
    out.append(("odd short, fill 0x5A", x, b, last, (m - m // 2 - 1) << 8 | 0x5A))
    x, b = plane_with(n, w, last, m // 2, 0x5A, 40 + w)
    out.append(("odd short, one below", x, b, last, NONE))
    x = np.random.default_rng(50 + w).integers(0, 256, SG + 777, dtype=np.uint8)
    out.append(("equal to its base", x, x.copy(), 0, 0))
    out.append(("fill 0x5A everywhere", x, x ^ np.uint8(0x5A), 8, 0x5A))
    return out


def kinds_total(est_row, scan_row, n, stored, sparse):
    """The total of one width's row under batch._kinds' rule (sparse_ref.rule): a sparse packet counts its record, a raw one its
    bytes, a coded one its estimate"""
    total = 0
    for p, (e, s) in enumerate(zip(est_row, scan_row)):
        ulen = min(PACKET, n - p * PACKET)
        kind = SR.rule(s if sparse else NONE, e, ulen, stored)
        total += SR.sparse_len(s >> 8) if kind == 2 else ulen if kind == 1 else e
    return total
