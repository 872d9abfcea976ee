"""The host-callable packet codec (include/gpuar_host.h, libgpuar_host.so and
the same three symbols in libgpuar_hip.so) against the reference's own
arCompress / arDecompress / initializeAdaptiveProbabilityRangeList
(/root/reference/src/gpuar.h:73,75,76).

Anchors: the tiny vectors of SURVEY.md section 8(b), tests/golden/ref_vectors.json,
tests/golden/model_vectors.json (caller-owned model carried across calls, from
oracle/_ref), the C restatement in oracle/, and tests/golden/seeded_vectors.json
(oracle/_ref on seeded inputs, including corrupted packets).  No GPU.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from gpuar_amd import host as HC
from gpuar_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")
with open(os.path.join(GOLD, "model_vectors.json")) as f:
    MODELV = json.load(f)
with open(os.path.join(GOLD, "ref_vectors.json")) as f:
    REFV = json.load(f)["cases"]
with open(os.path.join(GOLD, "seeded_vectors.json")) as f:
    SEEDED = json.load(f)


def md5(b):
    return hashlib.md5(bytes(b)).hexdigest()


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(HC.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def ranges_of(hexstr):
    return np.frombuffer(bytes.fromhex(hexstr), dtype="<u2").astype(np.uint16)


def test_initial_model_is_the_references():
    m = HC.Model()
    assert m.total == MODELV["initial_total"] == 256
    assert np.array_equal(m.ranges, ranges_of(MODELV["initial_ranges_hex"]))
    assert m.ranges[0] == 0 and m.ranges[256] == 256 and m.ranges[1] == 1 and m.ranges[192] == 64


def test_survey_tiny_vectors():
    assert HC.encode_packet(b"hello").hex() == "0900050068650823e3"
    assert HC.encode_packet(b"\xd7").hex() == "06000100d740"
    zeros = HC.encode_packet(bytes(8192))
    assert len(zeros) == 210 and zeros[:4].hex() == "d2000020" and zeros[-1] == 0x04
    assert HC.decode_packet(bytes.fromhex("0900050068650823e3")) == b"hello"
    assert HC.decode_packet(zeros) == bytes(8192)


@pytest.mark.parametrize("case", MODELV["cases"], ids=lambda c: f"{c['kind']}_s{c['seed']}")
def test_model_carried_across_calls(case):
    enc, dec = HC.Model(), HC.Model()
    for seg in case["segments"]:
        data = synth.generate(case["kind"], case["seed"], seg["n"], offset=seg["offset"]).tobytes()
        pkt = HC.encode_packet(data, enc)
        assert len(pkt) == seg["clen"]
        assert hashlib.md5(pkt).hexdigest() == seg["packet_md5"]
        if "packet_hex" in seg:
            assert pkt.hex() == seg["packet_hex"]
        assert enc.total == seg["total_after"]
        assert np.array_equal(enc.ranges, ranges_of(seg["ranges_after_hex"]))
        assert HC.decode_packet(pkt, dec) == data
        assert dec.total == enc.total and np.array_equal(dec.ranges, enc.ranges)


def test_single_packet_golden_cases():
    for c in REFV:
        if c["kind"] not in synth.KINDS or c["n"] > 8192:
            continue
        data = synth.generate(c["kind"], c["seed"], c["n"]).tobytes()
        pkt = HC.encode_packet(data)
        assert len(pkt) == c["stream_len"] and hashlib.md5(pkt).hexdigest() == c["stream_md5"], c["name"]
        assert HC.decode_packet(pkt) == data


def test_fixture_streams_packet_by_packet(port_oracle):
    data = np.fromfile(os.path.join(GOLD, "adversarial_midpoint.in.bin"), dtype=np.uint8).tobytes()
    want = open(os.path.join(GOLD, "adversarial_midpoint.stream.bin"), "rb").read()
    assert HC.encode_packet(data) == want            # the long pending-run packet
    assert HC.decode_packet(want) == data
    stream = open(os.path.join(GOLD, "uniform_s1_n65539_keep.stream.bin"), "rb").read()
    src = synth.uniform(1, 65539).tobytes()
    off = 0
    for p in range(9):
        clen = int.from_bytes(stream[off:off + 2], "little")
        chunk = src[p * 8192:(p + 1) * 8192]
        assert HC.encode_packet(chunk) == stream[off:off + clen]
        assert HC.decode_packet(stream[off:off + clen]) == chunk
        off += clen
    assert off == len(stream)


def test_matches_c_restatement_on_ragged_sizes(port_oracle):
    for kind in synth.KINDS:
        for seed, n in [(21, 0), (22, 1), (23, 2), (24, 15), (25, 16), (26, 17), (27, 255), (28, 4095), (29, 8191), (30, 8192)]:
            data = synth.generate(kind, seed, n).tobytes()
            pkt = HC.encode_packet(data)
            assert pkt == port_oracle.encode_packet(data), (kind, seed, n)
            assert HC.decode_packet(pkt) == data
    for b in (0, 0x41, 0xFF):
        data = bytes([b]) * 8192
        assert HC.encode_packet(data) == port_oracle.encode_packet(data)


def test_reads_exactly_size_bytes_and_writes_exactly_clen():
    # input sits at the very end of a buffer, output is guarded by sentinels
    lib = HC.load()
    data = synth.text(9, 1000)
    out = np.full(8704 + 64, 0xA5, dtype=np.uint8)
    m = HC.Model()
    n = lib.arCompress(data.ctypes.data_as(C.POINTER(C.c_uint8)), data.size, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                       m.ranges.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(m._total))
    assert 4 < n < 1000 and (out[n:] == 0xA5).all()
    assert int(out[0]) | (int(out[1]) << 8) == n and int(out[2]) | (int(out[3]) << 8) == 1000


def test_same_symbols_in_both_libraries():
    from gpuar_amd import hip as H
    if not os.path.exists(H.LIB_PATH):
        pytest.skip("libgpuar_hip.so not built")
    big = C.CDLL(H.LIB_PATH)
    for name in HC.EXPORTS:
        assert hasattr(big, name), name
    u16p, u8p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
    big.arCompress.restype = C.c_uint16
    big.arCompress.argtypes = [u8p, C.c_uint16, u8p, u16p, u16p]
    big.initializeAdaptiveProbabilityRangeList.argtypes = [u16p, u16p]
    ranges = np.zeros(257, dtype=np.uint16)
    total = C.c_uint16(0)
    big.initializeAdaptiveProbabilityRangeList(ranges.ctypes.data_as(u16p), C.byref(total))
    src = np.frombuffer(b"hello", dtype=np.uint8).copy()
    out = np.zeros(64, dtype=np.uint8)
    n = big.arCompress(src.ctypes.data_as(u8p), 5, out.ctypes.data_as(u8p), ranges.ctypes.data_as(u16p), C.byref(total))
    assert out[:n].tobytes().hex() == "0900050068650823e3" and total.value == 261


def test_carried_models_match_reference_seeded_chains():
    """40 chains of 2-4 segments, the model carried from call to call, against the reference's packets and model state after
    every call (tests/golden/seeded_vectors.json; the reference's own decoder left the same state and bytes there)."""
    chains = SEEDED["carried_models"]
    assert len(chains) == 40
    for trial, chain in enumerate(chains):
        enc, dec = HC.Model(), HC.Model()
        for seg in chain["segments"]:
            data = synth.generate(chain["kind"], chain["seed"], seg["n"], offset=seg["offset"]).tobytes()
            pkt = HC.encode_packet(data, enc)
            assert len(pkt) == seg["clen"] and md5(pkt) == seg["packet_md5"], (trial, seg["offset"])
            assert enc.total == seg["total_after"] and md5(enc.ranges.astype("<u2").tobytes()) == seg["ranges_after_md5"]
            assert HC.decode_packet(pkt, dec) == data
            assert dec.total == seg["total_after"] and md5(dec.ranges.astype("<u2").tobytes()) == seg["ranges_after_md5"]


def test_corrupted_packets_decode_like_the_reference():
    # a damaged packet must decode to the same bytes (and stop at the same place) as the reference
    cases = SEEDED["corrupted_packets"]
    assert len(cases) == 200
    for trial, c in enumerate(cases):
        data = synth.generate(c["kind"], c["seed"], c["n"]).tobytes()
        pkt = bytearray(HC.encode_packet(data))
        assert md5(pkt) == c["packet_md5"], trial
        for byte, bit in c["flips"]:
            pkt[byte] ^= 1 << bit
        back = HC.decode_packet(bytes(pkt))
        assert len(back) == c["decoded_len"] and md5(back) == c["decoded_md5"], trial


def test_damaged_packets_decode_like_the_reference():
    """The 1024 damaged packets of tests/golden/damaged_vectors.json (tests/damage_sweep.py: bit flips, bursts, cuts,
    raised and lowered ulen, random bodies, empty bodies, spliced headers) through arDecompress: the reference's
    decoded length and md5.  The packets are rebuilt from this codec's own encodings and pinned by their md5."""
    import damage_sweep as DS
    import length_sweep as LS
    with open(os.path.join(GOLD, "damaged_vectors.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 1024 and {c["class"] for c in cases} == set(DS.CLASSES)
    encode = lambda m: np.frombuffer(HC.encode_packet(LS.packet(m).tobytes()), dtype=np.uint8)  # noqa: E731
    for c in cases:
        pkt, cls = DS.damaged(c["n"], encode)
        assert md5(pkt.tobytes()) == c["packet_md5"] and cls == c["class"], c["n"]
        back = HC.decode_packet(pkt.tobytes())
        assert len(back) == c["decoded_len"] and md5(back) == c["decoded_md5"], f"packet {c['n']} ({cls})"
