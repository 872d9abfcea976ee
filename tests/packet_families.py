"""Adversarial packet families shared by the GPU parity tests (tests/test_gpu_parity.py) and the host emulation of the table
walk (tests/test_encode_table.py): the generators, seeds and formulas are those of the parity tests, so both halves see the
same bytes.  Every generator draws its packets in order from one seeded stream: a call with fewer packets gives the packets a
call with more begins with (but for the cut of the last one).  Data only: no codec here."""
import numpy as np

PACKET = 8192


def keep_carrying(npk=512):
    """The coder's rare path (a leaving dword of 32 ones that has to wait for its carry): packets of two symbols either side of
    the interval's midpoint, few-symbol alphabets at every skew, and long constant stretches; the last packet is a short one."""
    rng = np.random.default_rng(2904)
    data = np.zeros(npk * 8192, dtype=np.uint8)
    for p in range(npk):
        view = data[p * 8192:(p + 1) * 8192]
        kind = p % 4
        if kind == 0:
            view[:] = np.where(rng.random(8192) < 0.5, 0x7F, 0x80).astype(np.uint8)
        elif kind == 1:
            view[:] = rng.choice(np.array([0x7F, 0x80, 0x00, 0xFF], dtype=np.uint8), 8192, p=[0.45, 0.45, 0.05, 0.05])
        elif kind == 2:
            view[:] = rng.choice(rng.integers(0, 256, int(rng.integers(2, 6))).astype(np.uint8), 8192)
        else:
            view[:] = np.repeat(rng.integers(0, 256, 8192 // 64).astype(np.uint8), 64)
    n = npk * 8192 - 3001                               # the last packet is a short one
    return data[:n]


def drain_the_window(npk=192):
    """A model trained on one byte (or on a few) and then fed bytes it has never seen -- 12-13 bits a symbol --, switch points
    and lengths ragged, next to constant packets (0.2 bits a symbol) and uniform ones (8); the last packet is a short one."""
    rng = np.random.default_rng(6006)
    data = np.zeros(npk * 8192, dtype=np.uint8)
    for p in range(npk):
        view = data[p * 8192:(p + 1) * 8192]
        kind = p % 6
        if kind == 0:                                       # one byte for a while, then every other byte in turn
            cut = int(rng.integers(512, 7000))
            view[:cut] = rng.integers(0, 256)
            view[cut:] = (np.arange(8192 - cut) * 37 + int(rng.integers(0, 256))).astype(np.uint8)
        elif kind == 1:                                     # a few bytes, then bytes drawn from the unseen rest, then back
            few = rng.integers(0, 256, 3).astype(np.uint8)
            a, b = sorted(int(v) for v in rng.integers(256, 7900, 2))
            view[:] = rng.choice(few, 8192)
            rest = np.setdiff1d(np.arange(256, dtype=np.uint8), few)
            view[a:b] = rng.choice(rest, b - a)
        elif kind == 2:
            view[:] = rng.integers(0, 256)                  # constant: the slowest reader
        elif kind == 3:
            view[:] = rng.integers(0, 256, 8192)            # uniform
        elif kind == 4:                                     # bursts of rare bytes in a constant packet
            view[:] = 0x20
            for _ in range(int(rng.integers(1, 40))):
                at = int(rng.integers(0, 8100))
                view[at:at + int(rng.integers(1, 90))] = rng.integers(0, 256, 1)
        else:                                               # a ramp over all byte values, then a constant tail
            cut = int(rng.integers(300, 8000))
            view[:cut] = (np.arange(cut) % 256).astype(np.uint8)
            view[cut:] = 0xFF
    n = npk * 8192 - 777
    return data[:n]


def ten_source_models(seed, npk=4096):
    """Packets from ten source models in turn -- uniform, few symbols, geometric, runs, ramps, midpoint pairs, a constant with
    1-40 strangers late in the packet (intervals of width 1-3), sorted, one dominant symbol, zipf."""
    rng = np.random.default_rng(seed)
    data = np.empty(npk * 8192, dtype=np.uint8)
    for p in range(npk):
        v = data[p * 8192:(p + 1) * 8192]
        m = p % 10
        if m == 0:
            v[:] = rng.integers(0, 256, 8192, dtype=np.uint8)
        elif m == 1:
            v[:] = rng.integers(0, int(rng.integers(1, 9)), 8192, dtype=np.uint8) * int(rng.integers(1, 32))
        elif m == 2:
            v[:] = (rng.geometric(float(rng.uniform(0.02, 0.5)), 8192) % 256).astype(np.uint8)
        elif m == 3:
            v[:] = np.repeat(rng.integers(0, 256, 8192 // 32, dtype=np.uint8), 32)
        elif m == 4:
            v[:] = (np.arange(8192) * int(rng.integers(1, 255))) % 256
        elif m == 5:
            v[:] = rng.choice(np.array([0x7F, 0x80], dtype=np.uint8), 8192)
        elif m == 6:
            v[:] = int(rng.integers(0, 256))
            late = rng.integers(4000, 8192, int(rng.integers(1, 40)))
            v[late] = rng.integers(0, 256, late.size, dtype=np.uint8)
        elif m == 7:
            v[:] = np.sort(rng.integers(0, 256, 8192, dtype=np.uint8))
        elif m == 8:
            k = int(rng.integers(2, 6))
            v[:] = rng.choice(rng.integers(0, 256, k, dtype=np.uint8), 8192, p=np.array([0.97] + [0.03 / (k - 1)] * (k - 1)))
        else:
            v[:] = (rng.zipf(1.3, 8192) % 256).astype(np.uint8)
    return data
