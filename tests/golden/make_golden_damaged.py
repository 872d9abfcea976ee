#!/usr/bin/env python3
"""Regenerates tests/golden/damaged_vectors.json: the reference's decode of 1024 of the damaged packets of
tests/damage_sweep.py, so that the host decoders are held to it where the reference is not present.

Run where oracle/_ref can be built (the reference's sources are needed):

    python tests/golden/make_golden_damaged.py

Per case: the packet length n it was made from (damage_sweep.damaged(n) rebuilds the packet from that alone), its
damage class, the md5 of the damaged packet, and what arDecompress made of it staged as oracle/ref_driver.cpp stages
a packet (clen bytes, then zeros): the decoded length and md5.  Every decoded length equals the header's ulen: the
reference never stopped decoding early on these packets (its exit for a code value no symbol owns was never taken).
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import damage_sweep as DS  # noqa: E402
import length_sweep as LS  # noqa: E402
from oracle import oracle as O  # noqa: E402


def md5(b) -> str:
    return hashlib.md5(bytes(b)).hexdigest()


def lengths():
    """The 1024 sweep lengths the file keeps (1 and 8192 among them); every class is reached."""
    pick = np.random.default_rng([DS.SEED, 5]).choice(np.arange(2, DS.PACKET), 1022, replace=False)
    return sorted({1, DS.PACKET, *(int(n) for n in pick)})


def main():
    ref = O.ReferenceOracle()
    cases = []
    for n in lengths():
        pkt, cls = DS.damaged(n, lambda m: ref.encode_stream(LS.packet(m)))
        back = ref.decode_packet(pkt.tobytes())
        assert len(back) == DS.fields(pkt)[1], (n, cls, len(back))
        cases.append({"n": n, "class": cls, "packet_md5": md5(pkt), "decoded_len": len(back), "decoded_md5": md5(back)})
    assert {c["class"] for c in cases} == set(DS.CLASSES)
    doc = {"_provenance": "arDecompress of oracle/_ref (the reference's unmodified codec) on damaged packets of "
                          "tests/damage_sweep.py; regenerate with tests/golden/make_golden_damaged.py",
           "checker_sha256": O.file_sha256(O.REF_LIB_PATH),
           "cases": cases}
    with open(os.path.join(HERE, "damaged_vectors.json"), "w") as f:
        json.dump(doc, f, indent=0)
    print(f"wrote {len(cases)} damaged packets")


if __name__ == "__main__":
    main()
