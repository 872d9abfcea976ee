"""Batch descriptors for the length and damage sweeps through the batch kernels (tests/test_gpu_lengths.py,
tests/test_gpu_damaged.py): which buffer owns which lanes, where each buffer lies in the caller's arena and how many bytes it
has.  Data only: plain integers, no device and no codec here.

A buffer is (offset, bytes, packets): its byte offset in the arena (None for a zero-byte buffer, whose pointer is 0), its
d_in_bytes / d_out_bytes, and how many batch packets it owns (its step in first_packet).  Zero-byte buffers sit at the
front, at the end and in seeded runs in the middle, so batch_lane's upper-bound search meets repeated first_packet entries.
"""
import numpy as np

import length_sweep as LS

PACKET = 8192
SEED = LS.SEED + 501
EMPTY = (None, 0, 0)


def with_empty(bufs, rng):
    """`bufs` in order, with two zero-byte buffers in front, three behind, and runs of 1-4 after about every tenth one."""
    out = [EMPTY] * 2
    for k, b in enumerate(bufs):
        out.append(b)
        if k + 1 < len(bufs) and rng.random() < 0.1:
            out += [EMPTY] * int(rng.integers(1, 5))
    return out + [EMPTY] * 3


def scattered_inputs(sizes, seed, gap=16):
    """Lane i's own one-packet input buffer of sizes[i] bytes, placed in one arena in a seeded permuted address order (so
    batch order is not address order), each 16-byte aligned with at least `gap` bytes behind it: (buffers, arena bytes)."""
    rng = np.random.default_rng([SEED, seed])
    starts = np.zeros(len(sizes), dtype=np.int64)
    at = gap
    for i in rng.permutation(len(sizes)):
        starts[i] = at
        at = (at + int(sizes[i]) + gap + 15) // 16 * 16
    return with_empty([(int(s), int(n), 1) for s, n in zip(starts, sizes)], rng), at + gap


def one_packet_outputs(rooms, seed, permute=True):
    """Lane i's own output buffer of rooms[i] bytes (rooms may be 0: that packet is then BAD_BATCH) at row rows[i] of an
    arena of 8192-byte rows, the rows a seeded permutation of the lanes (or in lane order): (buffers, rows)."""
    n = len(rooms)
    rng = np.random.default_rng([SEED, seed])
    rows = rng.permutation(n) if permute else np.arange(n)
    return with_empty([(int(rows[i]) * PACKET, int(rooms[i]), 1) for i in range(n)], rng), rows


def grouped_outputs(ulens, seed):
    """Consecutive lanes in output buffers of 1-5 packets, lane i at row i: a buffer of k packets has (k - 1) * 8192 +
    the last packet's ulen bytes, so each of its other packets has a room of 8192 behind a shorter ulen."""
    rng = np.random.default_rng([SEED, seed])
    bufs, i = [], 0
    while i < len(ulens):
        k = min(int(rng.integers(1, 6)), len(ulens) - i)
        bufs.append((i * PACKET, (k - 1) * PACKET + int(ulens[i + k - 1]), k))
        i += k
    return with_empty(bufs, rng)


def columns(bufs, base: int):
    """The descriptor rows for buffers in an arena at device address `base`: (pointers, bytes, first_packet)."""
    ptrs = [0 if off is None else base + off for off, _, _ in bufs]
    nbytes = [n for _, n, _ in bufs]
    first = np.zeros(len(bufs) + 1, dtype=np.int64)
    first[1:] = np.cumsum([k for _, _, k in bufs])
    return ptrs, nbytes, first.tolist()


def lane_rooms(bufs):
    """Each batch packet's room, in batch order: its buffer's bytes from the packet's start on, at most 8192."""
    rooms = []
    for _, n, k in bufs:
        rooms += [max(0, min(PACKET, n - j * PACKET)) for j in range(k)]
    return np.asarray(rooms, dtype=np.int64)
