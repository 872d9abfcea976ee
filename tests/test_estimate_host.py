"""The packet size estimate on the CPU (gpuar_amd/csrc/estimate.h through gpuar_hip_estimate_host; no device is touched): the
integer logarithm table against its pinned sums and math.log2, the host function against an independent Python restatement
(bincount + table), the estimate against the reference codec's recorded packet lengths (tests/golden/ref_vectors.json: within
+-1 byte on every packet, the range measured when the estimate was defined), and the stored rule on the typed inputs of
planes_ref.py."""
import math

import numpy as np
import pytest

import planes_ref as R

PACKET = 8192
FRACTION_BITS = 16
COUNTS = PACKET + 256                 # LF has an entry for every count 0 .. 8447


def lg16(k):
    """floor(2^16 log2 k), restated: 16 squarings of a Q62 mantissa, each giving one fraction bit."""
    e = k.bit_length() - 1
    m, r = k << (62 - e), e
    for _ in range(FRACTION_BITS):
        m = (m * m) >> 62
        r <<= 1
        if m >> 63:
            m >>= 1
            r |= 1
    return r


@pytest.fixture(scope="module")
def LF():
    lf = [0, 0]
    for c in range(2, COUNTS):
        lf.append(lf[-1] + lg16(c))
    return lf


@pytest.fixture(scope="module")
def H():
    import os

    from gpuar_amd import hip
    if not os.path.exists(hip.LIB_PATH):                  # the library is built when it is missing
        import __graft_entry__ as g
        g.build()
    hip.load()
    return hip


def python_estimate(LF, data):
    data = np.asarray(data, dtype=np.uint8).reshape(-1)
    out = []
    for at in range(0, data.size, PACKET):
        packet = data[at:at + PACKET]
        cost16 = LF[packet.size + 255] - LF[255] - sum(LF[int(c)] for c in np.bincount(packet, minlength=256))
        out.append(4 + ((cost16 + (1 << 19) - 1) >> 19))
    return out


def test_the_table_has_its_pinned_sums(LF):
    assert len(LF) == COUNTS and LF[0] == 0 and LF[1] == 0
    assert LF[255] == 109837967
    assert LF[8447] == 6422914120
    assert sum(LF) % (1 << 32) == 2225061214


def test_lg16_is_the_floor_of_the_scaled_logarithm():
    for k in range(1, COUNTS):
        x = math.log2(k) * (1 << FRACTION_BITS)
        if abs(x - round(x)) > 1e-6:                      # (a double cannot decide a fraction that close to an integer)
            assert lg16(k) == math.floor(x), k
        else:
            assert abs(lg16(k) - round(x)) <= 1, k
    for e in range(14):
        assert lg16(1 << e) == e << FRACTION_BITS


@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 127, 128, 129, 4096, 8191, 8192, 8193, 3 * 8192 + 5])
def test_the_host_function_is_the_python_restatement(H, LF, n):
    rng = np.random.default_rng(n)
    for alphabet in (256, 2, 17):
        data = rng.integers(0, alphabet, n, dtype=np.uint8)
        got = H.estimate_host(data.tobytes())
        assert len(got) == (n + PACKET - 1) // PACKET
        assert got == python_estimate(LF, data), (n, alphabet)
    for byte in (0x00, 0xFF):
        data = np.full(n, byte, dtype=np.uint8)
        assert H.estimate_host(data.tobytes()) == python_estimate(LF, data), (n, byte)
    assert H.estimate_host(b"") == []


def test_the_estimate_does_not_depend_on_the_order_of_the_bytes(H):
    from gpuar_amd import synth
    rng = np.random.default_rng(3)
    for n in (5, 129, 8191, 8192):
        data = synth.text(7, n)
        assert H.estimate_host(rng.permutation(data).tobytes()) == H.estimate_host(data.tobytes())
        assert H.estimate_host(np.sort(data).tobytes()) == H.estimate_host(data.tobytes())


def test_within_one_byte_of_the_reference_codecs_lengths_on_every_golden_packet(H):
    from oracle import oracle as O
    cases = O.golden_cases()
    assert len(cases) == 40
    low, high, packets = 0, 0, 0
    for c in cases:
        assert "clens" in c, c["name"]
        est = H.estimate_host(O.golden_case_input(c).tobytes())
        assert len(est) == len(c["clens"]), c["name"]
        for p, (e, clen) in enumerate(zip(est, c["clens"])):
            assert abs(clen - e) <= 1, (c["name"], p, clen, e)
            low, high, packets = min(low, clen - e), max(high, clen - e), packets + 1
    print(f"clen - est over {packets} packets: {low} .. {high}")


TYPED = [("bf16", 2, [0]), ("fp32", 4, [1, 2]), ("uniform", 1, [0])]


def packet_lengths_of(oracle, data):
    return R.packet_lengths(oracle.encode_stream(data).tobytes())


@pytest.fixture(scope="module")
def port_oracle():
    from oracle import oracle as O
    O.build()
    return O.PortOracle()


@pytest.mark.parametrize("kind,w,planes", TYPED)
def test_the_incompressible_planes_of_typed_inputs_are_stored(H, port_oracle, kind, w, planes):
    """1 MiB, seed 1, split: exactly the packets of the mantissa planes (bf16: plane 0; fp32: planes 1 and 2; every packet of
    uniform bytes); each of them really codes to at least 3 bytes more than it holds, and storing them makes the total smaller."""
    split = R.numpy_split(R.typed_input(kind, 1 << 20, seed=1), w)
    est = H.estimate_host(split.tobytes())
    assert len(est) == 128
    stored = [H.stored_rule(e, PACKET) for e in est]
    assert stored == [p % w in planes for p in range(128)]
    assert sum(stored) == (128 if w == 1 else 64)
    clens = packet_lengths_of(port_oracle, split)
    assert len(clens) == 128
    for p, (flag, clen, e) in enumerate(zip(stored, clens, est)):
        assert abs(clen - e) <= 1, (p, clen, e)
        if flag:
            assert clen >= PACKET + 3, (p, clen)
    assert sum(PACKET if flag else clen for flag, clen in zip(stored, clens)) < sum(clens)


def test_compressible_inputs_have_no_raw_packets(H):
    from gpuar_amd import synth
    for data in (np.zeros(1 << 20, dtype=np.uint8), synth.text(1, 1 << 20)):
        est = H.estimate_host(data.tobytes())
        assert len(est) == 128 and not any(H.stored_rule(e, PACKET) for e in est)


def test_the_host_call_checks_its_arguments(H):
    import ctypes as C
    lib = H.load()
    est = (C.c_uint32 * 2)(7, 7)
    assert lib.gpuar_hip_estimate_host(None, 0, None) == 0
    assert lib.gpuar_hip_estimate_host(None, 5, est) == -2 and lib.gpuar_hip_estimate_host(b"abcde", 5, None) == -2
    assert list(est) == [7, 7]
    assert lib.gpuar_hip_estimate_host(b"abcde", 5, est) == 0 and est[0] == 10 and est[1] == 7      # 40.06 bits: 6 bytes and the header
