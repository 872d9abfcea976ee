"""The placement arithmetic of tests/address_edges.py, swept over a few hundred seeded fake arena addresses on the CPU: the
alignment is exactly the minimum, the 2^32 line is strictly inside what is said to straddle it, and everything stays inside the
arena.  (tests/test_gpu_address_edges.py asserts the same of every real pointer before it launches.)"""
import numpy as np
import pytest

import address_edges as AE

LINE = AE.LINE
MARGIN = 64 << 20
SIZE = LINE + 2 * MARGIN
ALIGNS = (4, 8, 16)


def _bases():
    rng = np.random.default_rng(20261018)
    bases = [hi * LINE + lo for hi in (0, 1, 0x7F3A) for lo in (0, 16, LINE - 16, MARGIN, MARGIN - 16, LINE - MARGIN, LINE - MARGIN + 16)]
    bases += [int(rng.integers(1, 1 << 47)) // 16 * 16 for _ in range(300)]
    return bases


BASES = _bases()


def test_the_sweep_covers_the_edges_of_base():
    assert len(BASES) >= 300 and {0, 16, LINE - 16} <= {b % LINE for b in BASES}


def test_weak_is_the_smallest_offset_at_the_minimum_alignment():
    for align in ALIGNS:
        for off in range(0, 4 * align + 3):
            o = AE.weak(off, align)
            assert o >= off and o % (2 * align) == align
            assert not any(c % (2 * align) == align for c in range(off, o))
    for base in BASES:
        for align in ALIGNS:
            o = AE.weak(base + 257, align) - base
            assert 257 <= o < 257 + 2 * align and (base + o) % align == 0 and (base + o) % (2 * align) == align


def test_line_in_is_strictly_inside_with_its_margin():
    for base in BASES:
        L = AE.line_in(base, SIZE, MARGIN)
        assert (base + L) % LINE == 0
        assert MARGIN <= L <= SIZE - MARGIN and 0 < L < SIZE
    with pytest.raises(AssertionError):
        AE.line_in(16, SIZE - 1, MARGIN)


@pytest.mark.parametrize("nbytes", [12, 24, 40, 77, 8192, 8704, 200710, 131 * 8704])
def test_straddle_puts_the_line_inside_at_the_minimum_alignment(nbytes):
    for base in BASES[::3]:
        L = AE.line_in(base, SIZE, MARGIN)
        for align in ALIGNS:
            if nbytes <= align:
                continue
            for frac in (0.0, 0.01, 0.37, 0.5, 0.99, 1.0):
                start = AE.straddle(L, nbytes, frac, align)
                ptr = base + start
                assert ptr % (2 * align) == align
                assert ptr < base + L < ptr + nbytes
                assert 0 <= start and start + nbytes <= SIZE
                assert abs((L - start) - frac * nbytes) <= 2 * align + 1 or nbytes < 4 * align


@pytest.mark.parametrize("join", [None, (3, 5)])
def test_scattered_buffers_are_weak_disjoint_and_inside(join):
    sizes = [0, 1, 15, 48, 8191, 8192, 8193, 77, 3 * 8192 + 5, 16]
    for seed in range(40):
        for align in (8, 16):
            if join is not None and sizes[join[0]] % (2 * align) != align:
                continue
            offs, total = AE.scattered(sizes, seed, align=align, gap=16, join=join)
            assert total % (2 * align) == 0
            spans = sorted((o, o + n) for o, n in zip(offs, sizes))
            assert spans[0][0] >= 16 and spans[-1][1] + 16 <= total
            for (_a0, a1), (b0, _b1) in zip(spans, spans[1:]):
                assert a1 <= b0
            for i, o in enumerate(offs):
                if join is not None and i == join[1]:
                    assert o == offs[join[0]] + sizes[join[0]] and o % (2 * align) == 0
                else:
                    assert o % (2 * align) == align
