"""The host model of batch.py (tests/batch_model.py) on the CPU, over the whole option matrix: planes x filter x stored x sparse, 240
combinations of which 40 are refused by contract.  Every valid combination goes through model_compress and back through
model_decompress; the conditions that keep tests/test_gpu_batch_matrix.py from being vacuous -- every kind of packet, every choice
taken both ways, an empty kind -- are asserted on the model alone; the model's restatements of choose_planes and choose_filter are
pinned against the C functions; and the parts of batch.py that are device-free torch (_kinds, _partition, the counting rule
_counts_as with the per-buffer sum _per_buffer, and the decisions of _auto_delta and _auto_base with the launches replaced by the
model's estimates) run on CPU tensors against the model.

Wall time of the module: 7 s on one core (22 tests), 3 s of it importing torch in the first test that needs it.  The 400
model_compress / model_decompress pairs (with and without CRCs) take under 2 s: 124 layouts are split, estimated, scanned and encoded
once each for all of them.

base_auto="survey" is the eighth value of the filter axis.  At fixed widths its model is base_auto=True's, field by field; beside
planes="survey" it is a rule of its own -- width and base together, on totals that count raw and sparse packets -- whose totals
and choices for the three tensors with a base are written out here (CODED_TOTALS, KEPT_TOTALS) and differ from base_auto=True's in
the widths of two of them."""
import itertools
import os

import numpy as np
import pytest

import sparse_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpuar_amd", "lib", "libgpuar_hip.so")
PACKET = 8192


@pytest.fixture(scope="module")
def H():
    if not os.path.exists(LIB):
        pytest.skip("libgpuar_hip.so not built")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def M(H):
    import batch_model
    batch_model.codec()                                        # (the oracle: the reference's codec wherever the golden vectors pin it)
    return batch_model


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def kinds_of(m, b):
    return m.stored[m.first_packet[b]:m.first_packet[b + 1]]


def valid(M):
    return [c for c in M.combinations() if not M.is_refused(c)]


# ---- the matrix --------------------------------------------------------------------------------------------------------

def test_the_matrix_is_200_valid_combinations_and_40_refused_ones(M):
    combos = M.combinations()
    assert len(combos) == len(set(combos)) == 5 * 8 * 3 * 2 == 240
    refused = [c for c in combos if M.is_refused(c)]
    assert len(refused) == 40 and len(valid(M)) == 200
    assert {(p, f) for p, f, _s, _q in refused} == set(itertools.product(M.PLANES_AXIS, M.FILTER_AXIS))
    for c in refused:
        with pytest.raises(M.Refused):
            M.model_compress(M.ARRAYS, M.DTYPES, **M.keywords(c))
    for c in valid(M):
        M.model(c, False)                                      # (raises for none of them)
    with pytest.raises(M.Refused):
        M.model_compress(M.ARRAYS, M.DTYPES, base_auto=True)
    for base_auto in ("survey", "auto"):                       # without a base; a string other than "survey", as batch.py refuses it
        with pytest.raises(M.Refused):
            M.model_compress(M.ARRAYS, M.DTYPES, base_auto=base_auto)
    with pytest.raises(M.Refused):
        M.model_compress(M.ARRAYS, M.DTYPES, base=M.BASES, base_auto="auto")
    for base_auto in (True, "survey"):
        with pytest.raises(M.Refused):
            M.model_compress(M.ARRAYS, M.DTYPES, base=M.BASES, base_auto=base_auto, delta=True)
    for delta in (True, False, M.DELTA_LIST, "auto", "survey"):
        with pytest.raises(M.Refused):
            M.model_compress(M.ARRAYS, M.DTYPES, base=M.BASES, delta=delta)


def test_the_batch_has_every_packet_and_group_edge(M):
    assert {n % PACKET for n in M.SIZES} >= {1, 2, 3} and PACKET + 1 in M.SIZES and 3 * PACKET in M.SIZES and 0 in M.SIZES
    assert M.N_PACKETS == 51 and sum(M.SIZES) < 340 * 1024
    by_width = {8: M.SIZES[0], 4: M.SIZES[1], 2: M.SIZES[2]}
    for w, n in by_width.items():                              # whole groups and a tail that is no whole packet
        assert n >= w * PACKET and n % (w * PACKET) and n % PACKET and n % w == 0
    assert all(by_width[w] % (w * PACKET) > PACKET for w in (8, 4))              # ... of whole packets and a partial one
    assert M.SIZES[7] % 2 == 1 and M.SIZES[7] > 4 * PACKET     # a length that is a multiple of no width, behind a whole group of 4
    # a partial group at every width: buffers shorter than a group, whose elements are spread over fewer than w packets
    assert all(any(PACKET < n < w * PACKET for n in M.SIZES) for w in (2, 4, 8))


@pytest.mark.parametrize("planes", ["none", "auto", "2", "list", "survey"])
def test_every_valid_combination_goes_there_and_back(M, planes):
    n = 0
    for c in valid(M):
        if c[0] != planes:
            continue
        for checksum in (False, True):
            m = M.model(c, checksum)
            back = M.model_decompress(m, M.BASES)
            assert len(back) == len(M.ARRAYS)
            for b, (x, a) in enumerate(zip(back, M.ARRAYS)):
                assert x.dtype == np.uint8 and x.size == M.SIZES[b] and (x == raw(a)).all(), (c, b)
            assert (m.crc32 is None) == (not checksum)
            if checksum:
                assert M.first_wrong_packet(m, back) is None
            assert m.nbytes == len(m.stream) + len(m.raw or b"") + len(m.sparse or b"")
            assert m.offsets[-1] == len(m.stream)
            assert (m.stored is None) == (c[2] == "none" and c[3] == "none") and (m.sparse is None) == (c[3] == "none")
            assert (m.raw is None) == (m.stored is None) and (m.stored is None or len(m.stored) == M.N_PACKETS)
        n += 1
    assert n == 40


def test_estimate_is_the_size_where_no_packet_is_coded_and_bounds_it_elsewhere(M):
    """model_estimate counts a raw packet as its bytes and a sparse one as its record: those parts of the total are exact."""
    for c in valid(M):
        if c[2] == "list":
            continue
        m = M.model(c, False)
        est = M.model_estimate(M.ARRAYS, M.DTYPES, **M.keywords(c))
        assert len(est) == len(M.ARRAYS) and est[9] == 0
        for b in range(len(M.ARRAYS)):
            if m.stored is not None and M.SIZES[b] and S.CODED not in kinds_of(m, b):
                lens = [min(PACKET, M.SIZES[b] - j * PACKET) for j in range(len(kinds_of(m, b)))]
                sparse = [S.sparse_len(s >> 8) for s in m.layouts[b].scan]
                assert est[b] == sum(s if k == S.SPARSE else n for k, n, s in zip(kinds_of(m, b), lens, sparse)), (c, b)


# ---- the conditions that keep the GPU tests from being vacuous -----------------------------------------------------------

def test_every_kind_of_packet_occurs(M):
    for p in M.PLANES_AXIS:
        for f in ("delta", "base"):
            if p == "none" and f == "delta":
                continue                                       # (bytes: position ids and offsets are no runs of one value)
            both = set(M.model((p, f, "auto", "auto"), False).stored)
            assert both == {S.CODED, S.RAW, S.SPARSE}, (p, f, both)
            assert set(M.model((p, f, "none", "auto"), False).stored) == {S.CODED, S.SPARSE}, (p, f)
    for f in ("delta", "base"):
        assert set(M.model(("auto", f, "auto", "auto"), False).stored) == {S.CODED, S.RAW, S.SPARSE}
    m = M.model(("auto", "delta", "auto", "auto"), False)
    assert m.planes[1] == 4 and S.SPARSE in kinds_of(m, 1)     # position ids: the filter makes packets of one byte value
    m = M.model(("auto", "delta", "none", "auto"), False)
    assert m.planes[1] == 4 and S.SPARSE in kinds_of(m, 1)
    m = M.model(("auto", "base", "auto", "auto"), False)
    assert set(kinds_of(m, 3)) == {S.SPARSE} and len(m.sparse) >= 4 * 3          # the tensor equal to its base: 4 bytes a packet
    assert S.RAW in kinds_of(M.model(("auto", "base", "auto", "none"), False), 4)             # an unrelated base: the mantissa plane
    assert set(kinds_of(M.model(("none", "none", "auto", "none"), False), 5)) == {S.RAW}      # uniform bytes
    assert set(kinds_of(M.model(("none", "none", "auto", "auto"), False), 8)) == {S.SPARSE}   # zeros: sparse without a base
    assert set(kinds_of(M.model(("none", "none", "auto", "none"), False), 6)) == {S.CODED}    # text


def test_the_delta_choices_go_both_ways_and_the_survey_agrees_with_auto(M):
    for p in M.PLANES_AXIS:
        for s in M.STORED_AXIS:
            auto, survey = M.model((p, "delta_auto", s, "none"), False), M.model((p, "delta_survey", s, "none"), False)
            assert len(set(auto.delta)) == 2, (p, s, auto.delta)
            assert survey.delta == auto.delta, (p, s)
            assert not auto.delta[9] and all(isinstance(f, bool) for f in auto.delta)
    m = M.model(("auto", "delta_auto", "none", "none"), False)
    assert m.delta[0] and m.delta[1] and m.delta[13] and not m.delta[2] and not m.delta[5] and not m.delta[7]
    m = M.model(("survey", "delta_survey", "none", "none"), False)
    assert True in m.delta and False in m.delta and m.planes[1] == 4 and m.delta[1]


def test_base_auto_keeps_the_bases_that_pay(M):
    for p in M.PLANES_AXIS:
        for s in M.STORED_AXIS:
            m = M.model((p, "base_auto", s, "none"), False)
            assert m.based == [b in (2, 3) for b in range(len(M.ARRAYS))], (p, s)
            assert M.model((p, "base", s, "none"), False).based == [b in (2, 3, 4) for b in range(len(M.ARRAYS))]


def test_base_survey_at_fixed_widths_is_base_auto_field_by_field(M):
    """base_auto="survey" beside None, "auto", a width or a list of widths keeps the bases base_auto=True keeps, by the same rule on
    coded estimates: the two models are equal in every field and coded from the same layouts."""
    n = 0
    for c in valid(M):
        if c[1] != "base_survey" or c[0] == "survey":
            continue
        for checksum in (False, True):
            m, a = M.model(c, checksum), M.model((c[0], "base_auto") + c[2:], checksum)
            assert sorted(vars(m)) == sorted(vars(a))
            for field in vars(a):
                if field == "layouts":
                    assert all(x is y for x, y in zip(m.layouts, a.layouts)), c
                else:
                    assert getattr(m, field) == getattr(a, field), (c, field)
        assert m.based == [b in (2, 3) for b in range(len(M.ARRAYS))], c
        n += 1
    assert n == 4 * 5


# base_auto="survey" beside planes="survey", for the three tensors of the batch that have a base: the totals [T1, T2, T4, T8] of
# the bytes as they are and XORed, 7, 3 and 3 packets, and what choose_filter makes of them.  Coded totals (no stored, no sparse;
# a list of stored packets counts as None): tensors 2 and 3 are within one byte a packet of their lowest XORed total at every
# width, so the smallest width wins, where the plain bytes alone (and so planes="survey" beside base_auto=True) say 2.
CODED_TOTALS = {
    2: ([38795, 33646, 35366, 38115], [1372, 1370, 1370, 1371], (1, True)),
    3: ([12976, 11267, 12982, 12986], [462, 462, 462, 462], (1, True)),
    4: ([19337, 17620, 18986, 19255], [19905, 18254, 19572, 19829], (2, False)),
}
# Counting moves totals and no choice.  stored="auto": the raw packets are low-byte planes at widths 2 and 4, plain and against
# the unrelated base.  sparse="auto": an unchanged packet is a 4-byte record and one with a few changed elements a short one, so
# the XORed side falls to 160 .. 164 bytes for tensor 2 (7 packets: all within the margin, width 1) and 12 for tensor 3; no
# packet of the plain side or of tensor 4 is sparse.  (stored, sparse): (plain, xored) where they differ from CODED_TOTALS.
KEPT_TOTALS = {
    ("auto", "none"): {2: ([38795, 33530, 35284, 38115], None), 3: ([12976, 11226, 12982, 12986], None),
                       4: ([19337, 17583, 18986, 19255], [19905, 18192, 19572, 19829])},
    ("none", "auto"): {2: (None, [164, 160, 164, 160]), 3: (None, [12, 12, 12, 12]), 4: (None, None)},
    ("auto", "auto"): {2: ([38795, 33530, 35284, 38115], [164, 160, 164, 160]), 3: ([12976, 11226, 12982, 12986], [12, 12, 12, 12]),
                       4: ([19337, 17583, 18986, 19255], [19905, 18192, 19572, 19829])},
}


def test_base_survey_beside_the_plane_survey_chooses_width_and_base_together(H, M):
    for b, (plain, xored, choice) in CODED_TOTALS.items():
        packets = M.packets_of(M.SIZES[b])
        assert M.survey_base_totals(M.ARRAYS, M.BASES, b) == (plain, xored), b
        assert M.choose_filter(plain, xored, packets) == H.choose_filter(plain, xored, packets) == choice, b
        # the survey the device decides from gives the same coded totals: its est rows are the layouts' estimates
        est, _scan = H.survey_xor_host(M._raw(M.ARRAYS[b]).tobytes(), M.BASES[b].tobytes())
        assert [sum(row) for row in est] == xored, b
    assert [M.choose_planes(CODED_TOTALS[b][0], M.packets_of(M.SIZES[b])) for b in (2, 3, 4)] == [2, 2, 2]
    n = 0
    for s in M.STORED_AXIS:
        for q in M.SPARSE_AXIS:
            c = ("survey", "base_survey", s, q)
            if M.is_refused(c):
                continue
            for b, (plain, xored, choice) in CODED_TOTALS.items():
                moved = KEPT_TOTALS.get((s, q), {}).get(b, (None, None))
                want = (moved[0] or plain, moved[1] or xored)
                got = M.survey_base_totals(M.ARRAYS, M.BASES, b, s == "auto", q == "auto")
                packets = M.packets_of(M.SIZES[b])
                assert got == want, (c, b)
                assert M.choose_filter(*got, packets) == H.choose_filter(*got, packets) == choice, (c, b)
            m, a = M.model(c, False), M.model(("survey", "base_auto", s, q), False)
            assert [(m.planes[b], m.based[b]) for b in (2, 3, 4)] == [(1, True), (1, True), (2, False)], c
            assert [(a.planes[b], a.based[b]) for b in (2, 3, 4)] == [(2, True), (2, True), (2, False)], c
            # a tensor without a base: choose_planes of plain totals that count sparse packets too, which planes="survey" alone
            # does not; on this batch that moves no width
            others = [b for b in range(len(M.ARRAYS)) if b not in CODED_TOTALS]
            assert [m.planes[b] for b in others] == [a.planes[b] for b in others] and not any(m.based[b] for b in others), c
            assert m.layouts[2] is M.layout(M.ARRAYS[2], 1, "base", M.BASES[2]) and m.layouts[4] is M.layout(M.ARRAYS[4], 2, "none")
            n += 1
    assert n == 5
    # the whole joint rule once more by hand: no base, no packets
    assert M.survey_base_totals(M.ARRAYS, M.BASES, 9) == ([0] * 4, None) and M.survey_base_totals(M.ARRAYS, M.BASES, 0)[1] is None


def test_the_plane_survey_finds_widths_that_auto_cannot_see(M):
    for s in M.STORED_AXIS:
        m = M.model(("survey", "none", s, "none"), False)
        assert len(set(m.planes)) >= 3 and m.planes[7] == 4 and m.planes[0] == 8 and m.planes[9] == 1, (s, m.planes)
    assert M.model(("auto", "none", "none", "none"), False).planes[7] == 1
    # the stored rule reaches the choice: uniform bytes are within noise at every width, raw at every width they are all equal
    assert M.model(("survey", "none", "auto", "none"), False).planes[5] == 1


def test_some_kind_is_empty_somewhere(M):
    assert any(m.stored is not None and M.SIZES[b] and S.CODED not in kinds_of(m, b)
               for c in valid(M) for m in [M.model(c, False)] for b in range(len(M.ARRAYS)))
    # over the whole batch the 1-, 2- and 3-byte tensors and the uniform bytes are raw under stored="auto": the parts of the batch
    calm = [M.model(c, False, "calm") for c in M.SUBSET_COMBOS]
    assert all(m.stored is None or S.RAW not in m.stored for m in calm)
    assert any(m.stored is not None and m.raw == b"" and m.raw_offsets == [0] and c[2] == "auto" for c, m in zip(M.SUBSET_COMBOS, calm))
    still = {c: M.model(c, False, "still") for c in M.SUBSET_COMBOS}
    m = still["auto", "base", "auto", "auto"]
    assert set(m.stored) == {S.SPARSE} and m.stream == b"" and m.offsets == [0] and m.raw == b"" and m.nbytes == 4 * 6
    m = still["auto", "base", "auto", "none"]
    assert set(m.stored) == {S.CODED} and m.raw == b"" and m.raw_offsets == [0] and m.sparse is None
    rough = [M.model(c, False, "rough") for c in M.SUBSET_COMBOS]
    assert all(m.stored is None or S.SPARSE not in m.stored for m in rough) and any(m.sparse == b"" and m.sparse_offsets == [0] for m in rough)
    for c in M.SUBSET_COMBOS:
        for part in M.SUBSETS:
            m = M.model(c, True, part)
            back = M.model_decompress(m, [M.BASES[b] for b in M.SUBSETS[part]])
            assert all((x == raw(M.ARRAYS[b])).all() for x, b in zip(back, M.SUBSETS[part]))


def test_gip_forms(M):
    """A buffer has a .gip form iff none of its packets is raw or sparse and, where it was XORed with a base, the CRCs are there."""
    import trailer_ref as T
    seen = set()
    for c in valid(M):
        for checksum in (False, True):
            m = M.model(c, checksum)
            for b, blob in enumerate(m.gips):
                stored = m.stored is not None and any(kinds_of(m, b))
                xored = m.based is not None and m.based[b]
                assert (blob is None) == (stored or (xored and not checksum)), (c, b)
                if blob is not None:
                    end = T.stream_end(blob)
                    assert blob[4:12] == M.SIZES[b].to_bytes(8, "little")
                    version = int.from_bytes(blob[end + 4:end + 8], "little") if len(blob) > end else 0
                    seen.add(version)
                    filtered = m.delta is not None and m.delta[b]
                    w = m.planes[b] if m.planes is not None else 1
                    assert version == (5 if xored else 4 if filtered else 3 if w > 1 else 2 if checksum else 0), (c, b)
    assert seen == {0, 2, 3, 4, 5}


# ---- the restated rules against the C functions --------------------------------------------------------------------------

def survey_totals(M, b, how, replace):
    out = []
    for w in M.WIDTHS:
        lay = M.layout(M.ARRAYS[b], w, how)
        out.append(sum(n if replace and e >= 4 + n else e for e, n in zip(lay.est, lay.lens)))
    return out


def test_choose_planes_and_choose_filter_equal_the_c_functions(H, M):
    n = 0
    for b in range(len(M.ARRAYS)):
        packets = M.packets_of(M.SIZES[b])
        for replace in (False, True):
            plain, filtered = survey_totals(M, b, "none", replace), survey_totals(M, b, "delta", replace)
            assert M.choose_planes(plain, packets) == H.choose_planes(plain, packets), (b, plain)
            assert M.choose_planes(filtered, packets) == H.choose_planes(filtered, packets), (b, filtered)
            assert M.choose_filter(plain, filtered, packets) == H.choose_filter(plain, filtered, packets), (b, plain, filtered)
            n += 1
    assert n == 28
    # ties and one off a tie, by hand: the margin is n_packets, a tie with the margin wins, the smallest width wins among equals
    for p in (0, 1, 7):
        for low_at in range(4):
            for other_at in range(4):
                for step in (p - 1, p, p + 1):
                    if step < 0:
                        continue
                    totals = [5000] * 4
                    totals[low_at], totals[other_at] = 1000, 1000 + step
                    totals[low_at] = 1000                      # (other_at == low_at: the minimum stays)
                    assert M.choose_planes(totals, p) == H.choose_planes(totals, p), (totals, p)
    assert M.choose_planes([1007, 5000, 5000, 1000], 7) == 1 and M.choose_planes([1008, 5000, 5000, 1000], 7) == 8
    plain = [5000, 4000, 3000, 3000]
    for p in (0, 1, 7):
        for gain in (p - 1, p, p + 1):
            for at in range(4):
                filtered = [9000] * 4
                filtered[at] = 3000 - gain
                assert M.choose_filter(plain, filtered, p) == H.choose_filter(plain, filtered, p), (filtered, p)
    assert M.choose_filter(plain, [9000, 9000, 2993, 9000], 7) == (4, True) and M.choose_filter(plain, [9000, 9000, 2994, 9000], 7) == (4, False)
    assert M.choose_filter([0] * 4, [0] * 4, 0) == H.choose_filter([0] * 4, [0] * 4, 0) == (1, False)
    assert M.choose_filter([0] * 4, [0] * 4, 5) == H.choose_filter([0] * 4, [0] * 4, 5) == (1, False)
    assert M.choose_filter(plain, [100, 9000, 9000, 100], 7) == H.choose_filter(plain, [100, 9000, 9000, 100], 7) == (1, True)


def test_the_models_estimates_and_scans_are_the_host_librarys(H, M):
    """sparse_ref.scan (which the model uses) against sparse_scan_host, sparse_ref.rule against sparse_rule, on every packet of every
    layout the matrix made."""
    for c in valid(M):
        M.model(c, False)
    layouts = M.layouts_made()
    assert len(layouts) >= 100
    for lay in layouts:
        assert lay.scan == H.sparse_scan_host(lay.data.tobytes())
        for s, e, n in zip(lay.scan, lay.est, lay.lens):
            for on in (False, True):
                assert S.rule(s, e, n, on) == H.sparse_rule(s, e, n, on)


# ---- batch.py's device-free torch on CPU tensors -------------------------------------------------------------------------

def _i32(values):
    import torch
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32).copy())


def _i64(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int64)


def test_kinds_is_the_rule_on_the_table_and_on_every_packet_of_the_matrix(H, M):
    torch = pytest.importorskip("torch")
    from gpuar_amd import batch
    for on in (False, True):
        rows = [r for r in S.RULE_TABLE if r[3] == on]
        kind, slen = batch._kinds(_i32([r[0] for r in rows]), _i64([r[1] for r in rows]), _i64([r[2] for r in rows]), on)
        assert kind.dtype == torch.int64 and kind.tolist() == [r[4] for r in rows], on
        assert [v for v, r in zip(slen.tolist(), rows) if r[0] != S.NONE] == [S.sparse_len(r[0] >> 8) for r in rows if r[0] != S.NONE]
    n = 0
    for c in valid(M):
        if c[3] != "auto":
            continue
        m = M.model(c, False)
        scan = [s for lay in m.layouts for s in lay.scan]
        est = [e for lay in m.layouts for e in lay.est]
        lens = [v for lay in m.layouts for v in lay.lens]
        kind, slen = batch._kinds(_i32(scan), _i64(est), _i64(lens), c[2] == "auto")
        assert kind.tolist() == m.stored, c
        assert all(v == S.sparse_len(s >> 8) for v, s in zip(slen.tolist(), scan) if s != S.NONE), c
        n += len(scan)
    assert n == 80 * M.N_PACKETS


def _check_partition(batch, m, lens, scan):
    kinds = m.stored
    len16 = [(v + 15) // 16 * 16 for v in lens]
    slen = _i64([S.sparse_len(s >> 8) for s in scan]) if m.sparse is not None else None             # (as _kinds: of every scan word)
    n_stored, raw_bytes, coded, kept, n_sparse, sparse_bytes, packed = batch._partition(_i64(kinds), _i64(len16), slen)
    assert (n_stored, raw_bytes) == (len(m.raw_offsets) - 1, len(m.raw))
    assert (n_sparse, sparse_bytes) == ((len(m.sparse_offsets) - 1, len(m.sparse)) if m.sparse is not None else (0, 0))
    for got, kind in ((coded, S.CODED), (kept, S.RAW), (packed, S.SPARSE)):
        assert got.tolist() == [p for p, k in enumerate(kinds) if k == kind]
    assert coded.numel() == len(m.offsets) - 1


def test_partition_gives_the_models_ranks(H, M):
    pytest.importorskip("torch")
    from gpuar_amd import batch
    n = 0
    for c in valid(M):
        m = M.model(c, False)
        if m.stored is not None:
            _check_partition(batch, m, [v for lay in m.layouts for v in lay.lens], [s for lay in m.layouts for s in lay.scan])
            n += 1
    assert n == 160
    empty = set()
    for part in M.SUBSETS:
        for c in M.SUBSET_COMBOS:
            m = M.model(c, False, part)
            if m.stored is not None:
                _check_partition(batch, m, [v for lay in m.layouts for v in lay.lens], [s for lay in m.layouts for s in lay.scan])
                empty |= {kind for kind in (S.CODED, S.RAW, S.SPARSE) if kind not in m.stored and (kind != S.SPARSE or m.sparse is not None)}
    assert empty == {S.CODED, S.RAW, S.SPARSE}                 # every kind was the empty one once


class _FakeLaunches:
    """batch._split and hip.estimate_batch without a device: the descriptors as CPU tensors, and per-packet estimates given by the
    test for the plain and for the filtered (or XORed) copy."""

    def __init__(self, sizes, first_packet, plain, other):
        self.sizes, self.first_packet, self.est = sizes, first_packet, (plain, other)

    def split(self, a, stream):
        other = int(bool((a.flags is not None and any(a.flags)) or (a.bases is not None and any(a.bases))))
        d_coded = _i64([2 * b + other for b in range(len(a.sizes))])             # (which copy: the estimate below looks at it)
        from gpuar_amd import batch
        return batch._Split(_i64(a.ptrs), _i64(a.sizes), _i64(a.first_packet), d_coded, None)

    def estimate_batch(self, d_coded, d_bytes, d_fp, n, n_packets, stream=None, d_status=None, device=None):
        import torch
        return torch.tensor(self.est[int(d_coded[0].item()) & 1], dtype=torch.int32)


def _tied_estimates(M):
    """the estimates of the batch at planes="auto" without and with the delta filter, as they are -- and moved, buffer by buffer, to
    a tie (filtered + packets == plain), to one byte either side of it, and left alone"""
    m_plain, m_delta = M.model(("auto", "none", "none", "none"), False), M.model(("auto", "delta", "none", "none"), False)
    plain = [list(lay.est) for lay in m_plain.layouts]
    other = [list(lay.est) for lay in m_delta.layouts]
    for b, (p, o) in enumerate(zip(plain, other)):
        if not p or b % 4 == 3:
            continue
        level = max(sum(p[:-1]), sum(o[:-1])) + 100
        p[-1] = level + len(p) - sum(p[:-1])
        o[-1] = level + (b % 4 - 1) - sum(o[:-1])              # b % 4: 0 pays by one byte, 1 the tie (pays), 2 one byte short
    return m_plain, plain, other


def test_auto_delta_and_auto_base_decide_by_the_models_rule_at_ties(H, M, monkeypatch):
    """_auto_delta and _auto_base with their launches replaced: the decision from the totals, `<=` and the margin of one byte per
    packet, and _auto_base's per-packet estimates of the chosen copy."""
    torch = pytest.importorskip("torch")
    from gpuar_amd import batch
    m, plain, other = _tied_estimates(M)
    fake = _FakeLaunches(m.sizes, m.first_packet, [e for p in plain for e in p], [e for o in other for e in o])
    monkeypatch.setattr(batch, "_split", fake.split)
    monkeypatch.setattr(batch.H, "estimate_batch", fake.estimate_batch)
    n, counts = len(m.sizes), [len(p) for p in plain]
    want = [M.filter_pays(sum(o), sum(p), c) for o, p, c in zip(other, plain, counts)]
    margins = {sum(p) - sum(o) - c for o, p, c in zip(other, plain, counts) if c}
    assert {-1, 0, 1} <= margins and True in want and False in want
    status = torch.zeros(1, dtype=torch.int32)
    ptrs = [0x10000 * (b + 1) if size else 0 for b, size in enumerate(m.sizes)]
    a = batch._Batch(torch.device("cpu"), ptrs, m.sizes, m.first_packet, m.first_packet[-1], widths=m.planes, d_status=status)
    got = batch._auto_delta(a, None)
    assert got == want
    bases = [0x9000000 + 0x10000 * b if size else 0 for b, size in enumerate(m.sizes)]
    bases[1] = 0                                               # a buffer without a base keeps none, whatever the totals say
    keep, chosen, d_est = batch._auto_base(a._replace(bases=bases), None)
    want_keep = [bool(q) and w for q, w in zip(bases, want)]
    assert keep == want_keep and want[1] and not keep[1]
    assert d_est.tolist() == [e for b in range(n) for e in (other[b] if want_keep[b] else plain[b])]
    assert chosen[3].tolist() == [2 * b + int(k) for b, k in enumerate(want_keep)]           # every buffer is coded from the copy of its choice
    assert chosen.d_coded is chosen[3]
    assert batch._auto_delta(batch._Batch(torch.device("cpu"), [], [], [0], 0, widths=[], d_status=status), None) == []
    assert batch._auto_base(a._replace(bases=[0] * n), None) == ([False] * n, None, None)


def test_the_counting_rule_and_the_per_buffer_sum_give_model_estimate(H, M):
    """batch._counts_as on the model's per-packet estimates, lengths and scan words, summed by batch._per_buffer: model_estimate for every
    valid combination of the matrix that estimate takes (the 160 without a list of stored packets) and for the parts of the batch, where
    each branch of the rule is taken and not taken; and the per-buffer sum, on one row and on four rows, against a loop."""
    torch = pytest.importorskip("torch")
    from gpuar_amd import batch
    cases = [(c, None) for c in valid(M) if c[2] != "list"] + [(c, part) for part in M.SUBSETS for c in M.SUBSET_COMBOS]
    kinds_seen = {part: set() for part in list(M.SUBSETS) + [None]}
    for c, part in cases:
        m = M.model(c, False, part)
        which = range(len(M.ARRAYS)) if part is None else M.SUBSETS[part]
        want = M.model_estimate([M.ARRAYS[b] for b in which], [M.DTYPES[b] for b in which], **M.keywords(c, part))
        est = _i64([e for lay in m.layouts for e in lay.est])
        lens = _i64([v for lay in m.layouts for v in lay.lens])
        scan = _i32([s for lay in m.layouts for s in lay.scan]) if c[3] == "auto" else None
        buf = _i64([b for b, lay in enumerate(m.layouts) for _ in lay.lens])
        counted = batch._counts_as(est, lens, c[2] == "auto", scan)
        assert counted.shape == est.shape and counted.dtype == est.dtype
        assert batch._per_buffer(counted, buf, len(m.layouts)).tolist() == want, (c, part)
        loop = [0] * len(m.layouts)
        for b, v in zip(buf.tolist(), counted.tolist()):
            loop[b] += v
        assert batch._per_buffer(counted, buf, len(m.layouts)).tolist() == loop, (c, part)
        # the surveys' shape: the same packets four times over, one row unchanged and three moved -- every row sums on its own
        rows = torch.stack([counted, counted + 1, counted * 2, torch.zeros_like(counted)])
        assert batch._per_buffer(rows, buf, len(m.layouts)).tolist() == [loop, [t + len(lay.lens) for t, lay in zip(loop, m.layouts)],
                                                                         [2 * t for t in loop], [0] * len(loop)], (c, part)
        four = batch._counts_as(est.expand(4, -1), lens, c[2] == "auto", scan.expand(4, -1) if scan is not None else None)
        assert four.tolist() == [counted.tolist()] * 4, (c, part)
        if m.stored is not None:
            kinds_seen[part] |= set(m.stored)
            moved = [v != e for v, e in zip(counted.tolist(), est.tolist())]
            assert all(k != S.CODED or not mv for k, mv in zip(m.stored, moved)), (c, part)    # a coded packet counts as its estimate
    assert len(cases) == 160 + 36
    # every branch both ways: over the whole batch every kind, and a part without each of them
    assert kinds_seen[None] == {S.CODED, S.RAW, S.SPARSE}
    assert S.SPARSE not in kinds_seen["rough"] and S.RAW not in kinds_seen["calm"] and kinds_seen["rough"] >= {S.CODED, S.RAW}
    assert any(set(M.model(c, False, "still").stored or [S.CODED]) == {S.SPARSE} for c in M.SUBSET_COMBOS)
