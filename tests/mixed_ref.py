"""What tests/test_mixed_host.py and tests/test_gpu_mixed.py share (not a test module): the lengths, the mode patterns, the
constructed buffer of DESIGN.md 4.16 and the per-supergroup choice written out in Python over hip.choose_filter / choose_planes."""
import numpy as np

PACKET = 8192
SUPER = 8 * PACKET
MODES = tuple(range(12))
INVALID = (12, 13, 14, 15, 16, 255)
# every edge of a packet and of a supergroup; a long tail at width 8 behind two supergroups; and a short last supergroup that
# holds full groups at widths 1, 2 and 4 and a pure tail at width 8
LENGTHS = (0, 1, 8191, 8192, 65535, 65536, 65537, 2 * SUPER + 8 * PACKET - 1, 3 * SUPER + 5 * PACKET + 7)


def parts(mode):
    """(width, kind) of a mode: kind 0 planes, 1 delta, 2 base"""
    return 1 << (mode & 3), mode >> 2


def mode_count(n):
    return (n + SUPER - 1) // SUPER


def uniform(mode, n):
    return bytes([mode]) * mode_count(n)


def cyclic(n, start=0):
    return bytes((start + s) % 12 for s in range(mode_count(n)))


def random_modes(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 12, mode_count(n), dtype=np.uint8).tolist())


def pair(n, seed):
    """(buffer, base) of n bytes: typed-looking data, so that a wrong width or filter shows in every plane"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    x[1::2] &= 0x3F
    b = x.copy()
    flip = rng.integers(0, max(n, 1), max(n // 50, 1))
    if n:
        b[flip % n] ^= rng.integers(1, 256, flip.size, dtype=np.uint8)
    return x, b


def dedicated(H, x, b, mode):
    """split_planes_host / split_delta_host / split_xor_host of the whole buffer at the mode's width"""
    w, kind = parts(mode)
    if kind == 2:
        return H.split_xor_host(x, b, w)
    return H.split_delta_host(x, w) if kind == 1 else H.split_planes_host(x, w)


def by_supergroup(H, x, b, modes):
    """split_mixed by its definition, in Python: every supergroup through the dedicated host call of its mode"""
    return b"".join(dedicated(H, x[at:at + SUPER], b[at:at + SUPER], modes[at // SUPER]) for at in range(0, len(x), SUPER))


# ---- the constructed buffer: 8 supergroups of bf16 weights, 4 of sorted int64 offsets, 3 of fp32, 1 supergroup + 12345 bytes of
# uniform bytes; the base is the bf16 part with one element in a thousand changed and unrelated bytes elsewhere ----

SHAPE = (("bf16", 8 * SUPER), ("int64", 4 * SUPER), ("fp32", 3 * SUPER), ("bytes", SUPER + 12345))
TOTAL = sum(n for _kind, n in SHAPE)             # 1 060 921


def _bf16(rng, count):
    return (rng.normal(0.0, 0.02, count).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def constructed(seed=2024, scale=1):
    """(buffer, base, [(kind, first supergroup, supergroups)]) as uint8 arrays; scale: every part that many times as long"""
    rng = np.random.default_rng(seed)
    xs, bs, where, at = [], [], [], 0
    for kind, n in SHAPE:
        n *= scale
        if kind == "bf16":
            x = _bf16(rng, n // 2)
            b = x.copy()
            moved = rng.choice(x.size, x.size // 1000, replace=False)
            b[moved] = _bf16(rng, moved.size)
            x, b = x.view(np.uint8), b.view(np.uint8)
        else:
            if kind == "int64":
                x = np.cumsum(rng.integers(1, 1000, n // 8, dtype=np.int64)).view(np.uint8)
            elif kind == "fp32":
                x = rng.normal(0.0, 1.0, n // 4).astype(np.float32).view(np.uint8)
            else:
                x = rng.integers(0, 256, n, dtype=np.uint8)
            b = rng.integers(0, 256, n, dtype=np.uint8)
        xs.append(x), bs.append(b)
        where.append((kind, at // SUPER, mode_count(n)))
        at += n
    return np.concatenate(xs), np.concatenate(bs), where


def surveys(H, x, b=None, delta=True):
    """(plain, delta or None, xored or None): the three host surveys' rows of the buffer"""
    x = bytes(x)
    return H.survey_planes_host(x), (H.survey_delta_host(x) if delta else None), (H.survey_xor_host(x, bytes(b), scan=False)[0] if b is not None else None)


def supergroup_totals(rows, n):
    """[[four totals] per supergroup] of one survey's rows"""
    npk = (n + PACKET - 1) // PACKET
    return [[sum(row[p] for p in range(8 * s, min(npk, 8 * s + 8))) for row in rows] for s in range(mode_count(n))]


def python_choice(H, plain, delta, xored, n):
    """(modes, totals) by the rules written out: choose_filter (without a delta row: choose_planes), then the base at its own
    best width iff that total + packets <= the total so far"""
    npk = (n + PACKET - 1) // PACKET
    sums = [supergroup_totals(r, n) if r is not None else None for r in (plain, delta, xored)]
    modes, totals = [], []
    for s in range(mode_count(n)):
        packets = min(8, npk - 8 * s)
        p = sums[0][s]
        w, filtered = H.choose_filter(p, sums[1][s], packets) if delta is not None else (H.choose_planes(p, packets), False)
        total = (sums[1][s] if filtered else p)[H.SURVEY_WIDTHS.index(w)]
        mode = H.SURVEY_WIDTHS.index(w) | (4 if filtered else 0)
        if xored is not None:
            wx = H.choose_planes(sums[2][s], packets)
            tx = sums[2][s][H.SURVEY_WIDTHS.index(wx)]
            if tx + packets <= total:
                mode, total = H.SURVEY_WIDTHS.index(wx) | 8, tx
        modes.append(mode), totals.append(total)
    return bytes(modes), totals


def best_single_total(plain, delta, xored):
    """the smallest whole-buffer total over every (width, filter) offered"""
    return min(sum(row) for rows in (plain, delta, xored) if rows is not None for row in rows)
