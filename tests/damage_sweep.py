"""Damaged packets for the decoders' tests (tests/test_gpu_damaged.py on the GPU; tests/test_lane_emulation.py and
tests/test_host_codec.py on the host): one damaged packet per length 1 ... 8192, made from length_sweep.packet(n)'s
encoding, so every source model and every residue mod 64 meets every damage class.  Data only: the caller encodes.

A damaged packet is ordinary input: what comes out is what the reference's arDecompress makes of it, which reads only
ulen from the header and reads its bit stream without a bound (zeros behind its input, as oracle/ref_driver.cpp stages
it).  The classes, in turn (CLASSES[((n - 1) // 6) % 8], so each class meets all six source models):

  flip       1-3 bit flips in the body
  burst      1-64 body bytes overwritten by random bytes, 0x00 or 0xFF
  cut        the body truncated at k >= 4 bytes, clen = k
  ulen_up    ulen raised to a value in (n, 8192]: n + 1, 8192 or a draw  (n = 8192: left at 8192)
  ulen_down  ulen lowered to a value in [0, n): 0, n - 1 or a draw; the output is then packet(n)[:ulen]
  random     a random body behind a valid header: ulen 1 ... 8192, clen 4 ... 8688
  empty      clen = 4, no body, ulen in {1, 63, 64, 65, 8192}
  splice     the header of packet n on the body of packet m (clen = the bytes there are)

INVALID lists headers the decoders must refuse (flag GPUAR_STATUS_BAD_PACKET, write nothing): ulen 8193 or 0xFFFF,
clen 0 ... 3.

Two layouts (see slot_form, stream_form):
  slot form    packet p at p * 8704, zeros to the end of its slot; every clen is <= 8688, so the slot's last 16-byte
               piece is zero and a reader that repeats it past the slot's end reads zeros, as the reference does;
  stream form  arbitrary offsets, ending in a zero tail of STREAM_TAIL bytes inside offsets[n]: a packet consumes at
               most 16 bits a symbol, 8192 symbols <= 16 386 body bytes, so no packet reaches the stream's end.
"""
import numpy as np

import length_sweep as LS

PACKET, SLOT, HDR = 8192, 8704, 4
MAX_CLEN = SLOT - 16                     # 8688: the slot's last 16-byte piece stays zero
STREAM_TAIL = 2 * SLOT                   # 17408: more than any packet's reader can consume behind its start
SEED = LS.SEED + 77
CLASSES = ("flip", "burst", "cut", "ulen_up", "ulen_down", "random", "empty", "splice")


def header(clen: int, ulen: int) -> np.ndarray:
    return np.array([clen & 0xFF, clen >> 8, ulen & 0xFF, ulen >> 8], dtype=np.uint8)


def fields(pkt: np.ndarray):
    """(clen, ulen) as the header says."""
    return int(pkt[0]) | (int(pkt[1]) << 8), int(pkt[2]) | (int(pkt[3]) << 8)


def damage_class(n: int) -> str:
    return CLASSES[((n - 1) // 6) % len(CLASSES)]


def damaged(n: int, encode) -> tuple:
    """(damaged packet bytes, class) for length n.  encode(m) returns the clean encoding of length_sweep.packet(m)
    (a uint8 array holding its whole packet); `splice` asks for a second one."""
    cls = damage_class(n)
    rng = np.random.default_rng([SEED, n])
    clean = np.asarray(encode(n), dtype=np.uint8)
    pkt = clean.copy()
    clen = clean.size
    body = clen - HDR
    if cls == "flip":
        for _ in range(int(rng.integers(1, 4))):
            pkt[int(rng.integers(HDR, clen))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    elif cls == "burst":
        k = int(rng.integers(1, min(64, body) + 1))
        at = int(rng.integers(HDR, clen - k + 1))
        fill = int(rng.integers(0, 3))
        pkt[at:at + k] = rng.integers(0, 256, k, dtype=np.uint8) if fill == 0 else (0x00 if fill == 1 else 0xFF)
    elif cls == "cut":
        k = int(rng.integers(HDR, clen))             # 4 ... clen - 1 (every clean packet has a body of >= 2 bytes)
        pkt = pkt[:k].copy()
        pkt[:2] = header(k, 0)[:2]
    elif cls == "ulen_up":
        pick = int(rng.integers(0, 3))
        ulen = PACKET if n == PACKET else (n + 1 if pick == 0 else PACKET if pick == 1 else int(rng.integers(n + 1, PACKET + 1)))
        pkt[2:4] = header(0, ulen)[2:]
    elif cls == "ulen_down":
        pick = int(rng.integers(0, 3))
        ulen = 0 if pick == 0 else n - 1 if pick == 1 else int(rng.integers(0, n))
        pkt[2:4] = header(0, ulen)[2:]
    elif cls == "random":
        k = int(rng.integers(HDR, MAX_CLEN + 1))
        pkt = np.concatenate([header(k, int(rng.integers(1, PACKET + 1))), rng.integers(0, 256, k - HDR, dtype=np.uint8)])
    elif cls == "empty":
        pkt = header(HDR, (1, 63, 64, 65, PACKET)[(n // 48) % 5])
    else:                                            # splice
        m = int(rng.integers(1, PACKET + 1))
        other = np.asarray(encode(m), dtype=np.uint8)
        k = other.size
        pkt = np.concatenate([header(k, n), other[HDR:]])
    assert HDR <= pkt.size <= MAX_CLEN and fields(pkt)[0] == pkt.size, (n, cls)
    return pkt, cls


def sweep(encode):
    """[damaged(n) for n = 1 ... 8192]: (list of packets, list of classes); index i holds length i + 1."""
    pkts, classes = [], []
    for n in range(1, PACKET + 1):
        p, c = damaged(n, encode)
        pkts.append(p)
        classes.append(c)
    return pkts, classes


def invalid(encode):
    """Packets whose header the decoders refuse: [(packet, what)].  Their bodies are real encoded data, so a decoder
    that took them would write something."""
    body = np.asarray(encode(PACKET), dtype=np.uint8)[HDR:]
    out = []
    for ulen in (PACKET + 1, 0xFFFF):
        out.append((np.concatenate([header(HDR + body.size, ulen), body]), f"ulen {ulen}"))
    for clen in (0, 1, 2, 3):
        out.append((np.concatenate([header(clen, 1000 + clen), body]), f"clen {clen}"))
    return out


def slot_form(pkts) -> np.ndarray:
    """Packets in 8704-byte slots (slot p = pkts[p], then zeros)."""
    slots = np.zeros((len(pkts), SLOT), dtype=np.uint8)
    for p, b in enumerate(pkts):
        slots[p, :b.size] = b
    return slots.reshape(-1)


def stream_form(pkts, spacing=None):
    """(stream, offsets): the packets back to back (spacing None) or every `spacing` bytes apart (zeros between),
    then a zero tail of STREAM_TAIL bytes; offsets[n] = stream.size."""
    n = len(pkts)
    offs = np.zeros(n + 1, dtype=np.int64)
    for p, b in enumerate(pkts):
        assert spacing is None or b.size <= spacing
        offs[p + 1] = offs[p] + (b.size if spacing is None else spacing)
    offs[n] += STREAM_TAIL
    stream = np.zeros(int(offs[n]), dtype=np.uint8)
    for p, b in enumerate(pkts):
        stream[offs[p]:offs[p] + b.size] = b
    return stream, offs


def reference_view(stream: np.ndarray, off: int, end: int) -> bytes:
    """What the reference must be handed to see packet `off` as a decoder of `stream` does: the bytes that really
    follow it, up to STREAM_TAIL or the stream's end, with the clen field rewritten to that length (arDecompress never
    reads bytes 0-1; the staging in oracle/ref_driver.cpp copies clen bytes and zero-pads)."""
    view = stream[off:min(off + STREAM_TAIL, end)].copy()
    view[:2] = header(view.size, 0)[:2]
    return view.tobytes()
