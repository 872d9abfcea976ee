"""Where a buffer lies: the placement arithmetic of tests/test_gpu_address_edges.py as plain integer functions (no device, no
codec), so that tests/test_address_edges_host.py can check it without a GPU.

An offset counts bytes from the start of an arena whose device address is `base`; "aligned to `align` and to nothing coarser"
means address % (2 * align) == align, the weakest alignment a contract of `align` bytes allows.  LINE = 2^32: an address that
is a multiple of it is where a pointer's low word carries into its high word.
"""
import numpy as np

LINE = 1 << 32


def weak(off: int, align: int) -> int:
    """The smallest o >= off with o % (2 * align) == align."""
    return off + (align - off) % (2 * align)


def line_in(base: int, size: int, margin: int) -> int:
    """The offset L of a multiple of 2^32 in [base, base + size) with at least `margin` bytes of the arena on both sides."""
    assert size >= LINE + 2 * margin, f"an arena of {size} bytes need not hold an address line with {margin} bytes on both sides"
    L = (-base) % LINE
    if L < margin:
        L += LINE
    assert margin <= L and L + margin <= size and (base + L) % LINE == 0
    return L


def straddle(L: int, nbytes: int, frac: float, align: int) -> int:
    """The start offset of `nbytes` bytes that have the line at offset L about `frac` of the way through them and start at
    the weakest alignment: start = L - k with k % (2 * align) == align (the line is a multiple of every alignment), k the such
    value next to frac * nbytes with 0 < k < nbytes."""
    assert nbytes > align, f"{nbytes} bytes aligned to {align} cannot hold the line"
    k = weak(max(int(frac * nbytes) - align, 0), align)
    while k >= nbytes:
        k -= 2 * align
    assert 0 < k < nbytes and k % (2 * align) == align
    return L - k


def scattered(sizes, seed: int, align: int = 16, gap: int = 16, join=None):
    """Buffers of sizes[i] bytes in one block, in a seeded permuted address order (so batch order is not address order), at
    least `gap` bytes apart, every start aligned to `align` and to nothing coarser relative to the block -- which the caller
    puts at a multiple of 2 * align.  join = (a, b): buffer b begins exactly where buffer a ends (sizes[a] % (2 * align) must be
    `align`, so b's start is a multiple of 2 * align: the one start that is not weak).  Returns (offsets, block bytes)."""
    rng = np.random.default_rng([20261018, seed])
    order = [int(i) for i in rng.permutation(len(sizes))]
    if join is not None:
        a, b = join
        assert sizes[a] % (2 * align) == align
        order.remove(b)
        order.insert(order.index(a) + 1, b)
    offs = [0] * len(sizes)
    at = gap
    for i in order:
        if join is not None and i == join[1]:
            offs[i] = offs[join[0]] + sizes[join[0]]
        else:
            offs[i] = weak(at, align)
        at = offs[i] + int(sizes[i]) + gap
    return offs, weak(at, align) + align
