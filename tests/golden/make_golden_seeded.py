#!/usr/bin/env python3
"""Regenerates tests/golden/seeded_vectors.json: the reference's outputs on the
seeded inputs of three CPU tests, so that those tests run where the reference
is not present.

Run where oracle/_ref can be built (the reference's sources are needed):

    python tests/golden/make_golden_seeded.py

  packets            60 packets of seeded random bytes (four shapes: uniform,
                     a small alphabet, geometric, runs of 64) through arCompress
                     (tests/test_oracle_golden.py)
  carried_models     40 chains of synthetic segments coded WITHOUT re-initialising
                     the caller's model in between (tests/test_host_codec.py)
  corrupted_packets  200 packets with 1-3 flipped bits, decoded by arDecompress
                     (tests/test_host_codec.py)

The file is data: inputs (generator parameters, sizes, bit positions; the
md5 of the seeded random bytes) and the reference's outputs for them, all
through the checker whose sha256 tests/golden/ref_vectors.json pins.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gpuar_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def md5(b) -> str:
    return hashlib.md5(bytes(b)).hexdigest()


def seeded_packet_inputs():
    """The 60 inputs of tests/test_oracle_golden.py::test_port_matches_reference_seeded_packets, in order."""
    rng = np.random.default_rng(20261003)
    for trial in range(60):
        n = int(rng.integers(1, 8193))
        mode = trial % 4
        if mode == 0:
            data = rng.integers(0, 256, n, dtype=np.uint8)
        elif mode == 1:
            data = rng.integers(0, int(rng.integers(1, 8)), n, dtype=np.uint8)
        elif mode == 2:
            data = (rng.geometric(0.08, n) % 256).astype(np.uint8)
        else:
            data = np.repeat(rng.integers(0, 256, (n + 63) // 64, dtype=np.uint8), 64)[:n]
        yield data


def packets(ref):
    out = []
    for data in seeded_packet_inputs():
        pkt = ref.encode_packet(data)
        assert ref.decode_packet(pkt) == data.tobytes()
        out.append({"n": int(data.size), "input_md5": md5(data.tobytes()), "clen": len(pkt), "packet_md5": md5(pkt)})
    return out


def carried_models(ref):
    rng = np.random.default_rng(5)
    out = []
    for trial in range(40):
        kind = synth.KINDS[trial % 3]
        sizes = [int(x) for x in rng.integers(0, 4000, size=int(rng.integers(2, 5)))]
        r, t = ref.model_init()
        r2, t2 = ref.model_init()
        segs, off = [], 0
        for n in sizes:
            data = synth.generate(kind, trial + 1, n, offset=off).tobytes()
            pkt, r, t = ref.encode_packet_model(data, r, t)
            back, r2, t2 = ref.decode_packet_model(pkt, r2, t2)
            assert back == data and t2 == t and np.array_equal(r2, r)
            segs.append({"n": n, "offset": off, "clen": len(pkt), "packet_md5": md5(pkt),
                         "total_after": t, "ranges_after_md5": md5(r.astype("<u2").tobytes())})
            off += n
        out.append({"kind": kind, "seed": trial + 1, "segments": segs})
    return out


def corrupted_packets(ref):
    rng = np.random.default_rng(9)
    out = []
    for trial in range(200):
        kind = synth.KINDS[trial % 3]
        n = int(rng.integers(1, 3000))
        data = synth.generate(kind, trial + 3, n).tobytes()
        clean = ref.encode_packet(data)
        pkt = bytearray(clean)
        flips = []
        for _ in range(int(rng.integers(1, 4))):
            flips.append([int(rng.integers(4, len(pkt))), int(rng.integers(0, 8))])
            pkt[flips[-1][0]] ^= 1 << flips[-1][1]
        back = ref.decode_packet(bytes(pkt))
        out.append({"kind": kind, "seed": trial + 3, "n": n, "packet_md5": md5(clean), "flips": flips,
                    "decoded_len": len(back), "decoded_md5": md5(back)})
    return out


def main():
    ref = O.ReferenceOracle()
    doc = {"_provenance": "expected outputs produced by oracle/_ref (the reference's unmodified "
                          "initializeAdaptiveProbabilityRangeList / arCompress / arDecompress) on seeded inputs; "
                          "regenerate with tests/golden/make_golden_seeded.py",
           "checker_sha256": O.file_sha256(O.REF_LIB_PATH),
           "packets": packets(ref), "carried_models": carried_models(ref), "corrupted_packets": corrupted_packets(ref)}
    with open(os.path.join(HERE, "seeded_vectors.json"), "w") as f:
        json.dump(doc, f, indent=0)
    print(f"wrote {len(doc['packets'])} packets, {len(doc['carried_models'])} chains, "
          f"{len(doc['corrupted_packets'])} corrupted packets")


if __name__ == "__main__":
    main()
