"""batch.compress / estimate / decompress on the MI355X over the whole option matrix, against the host model of
tests/batch_model.py: planes x filter (40 tests) x the five valid (stored, sparse) pairs inside each -- the 200 valid combinations
tests/test_batch_model_host.py counts, on the batch of 14 tensors it describes, uploaded once.  Every comparison is byte for byte.

For every combination: every field of Compressed against model_compress (the None-ness too: `stored`, `raw`, `sparse` and their
offsets follow the dataclass's docstring); batch.estimate against model_estimate (not for a list of stored packets, which estimate
does not take); decompress twice, into fresh tensors and into caller tensors that are 16, 32 or 48 bytes too long and full of a
canary, one of the two with verify=False, and every byte behind sizes[b] still the canary; Compressed.gip(b) of every buffer equal
to the model's file, or GpuarError where the model says the buffer has none (a raw or sparse packet, or a base without the CRCs);
the inputs and bases unchanged; the fallback status word 0 at the end of the test.

The other keywords rotate with the combination (ROTATION, from the positions p, f, s, q of the combination on its four axes):
    checksum   (p + q) % 2                      False, True
    stream     (p + f + q + 1) % 2              the default stream, one side stream (compress and both decompress calls on it,
                                                synchronised once after each group of calls)
    mode       (2 p + f + 2 s + q + 2) % 3      None, "latency", "throughput"
    out        (f + q + 1) % 2                  which decompress call comes first and verifies: into fresh tensors, into the caller's
so that every value of each of them meets every value of every axis and of each other at least once
(test_the_rotation_covers_every_pair).  Three parts of the batch (batch_model.SUBSETS) add what the whole batch cannot have: a call
with stored="auto" and no raw packet, one with no coded packet at all, one with sparse="auto" and no sparse packet.

The filter axis ends at base_auto="survey" (base_survey).  At fixed widths it must give what base_auto=True gives from other
launches; beside planes="survey" it is a decision of its own (width and base together, batch.survey_base_choice), which the model
makes by definition and which codes tensors 2 and 3 of the batch from another layout than base_auto=True does
(tests/test_batch_model_host.py has the totals).

compress calls compared against the model, field by field: 200 (the matrix) + 36 (the parts) + 52 (the valid call behind every
refused one: 40 + 9 + 1 + 2) + 1 (damage) = 289.

Time, pytest --durations=0 on an MI355X, with tests/test_gpu_batch_trace.py and tests/test_gpu_xor_survey_batch.py behind it: 65
passed in 9.5 s (of which 2 s import torch and collect, and 3.6 s the trace module's child process); this module's 53 tests:
    1.00 s  test_every_field_estimate_decompress_and_gip_equal_the_model[none-none] (the first launches of the process and the
            first layouts of the model), 0.34 s its setup (the upload)
    0.04 .. 0.06 s  each of the other 39 tests of the matrix (5 compress, 4 estimate, 10 decompress and 70 gip calls each, and
            the model of its five combinations), the five base_survey ones at 0.04 s among them
    0.06 .. 0.08 s  each of the three parts of the batch (12 combinations each)
    0.03 s  test_damage_is_reported_at_the_packet_the_model_gets_wrong_first
    0.01 .. 0.02 s  each of the six older refusal tests and test_base_survey_beside_a_width_the_surveys_do_not_have;
            test_base_auto_of_another_string_is_refused_before_any_launch and everything else is under 0.005 s.
"""
import dataclasses

import numpy as np
import pytest

import batch_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PACKET = 8192
CANARY = 0xA5
MODES = (None, "latency", "throughput")


def rotation(combo):
    """(checksum, side stream, mode, caller tensors first) for a combination"""
    p, f, s, q = (list(axis).index(name) for axis, name in zip((M.PLANES_AXIS, M.FILTER_AXIS, M.STORED_AXIS, M.SPARSE_AXIS), combo))
    return bool((p + q) % 2), bool((p + f + q + 1) % 2), MODES[(2 * p + f + 2 * s + q + 2) % 3], bool((f + q + 1) % 2)


VALID = [c for c in M.combinations() if not M.is_refused(c)]
ROTATION = {c: rotation(c) for c in VALID}
PAIRS = [(p, f) for p in M.PLANES_AXIS for f in M.FILTER_AXIS]
COMPARED = []                                                  # every compress call that was compared against the model


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


class Uploaded:
    """the batch on the device, uploaded once and never modified"""

    def __init__(self):
        types = {"uint8": torch.uint8, "int32": torch.int32, "int64": torch.int64, "float32": torch.float32}
        self.tensors = []
        for a, name in zip(M.ARRAYS, M.DTYPES):
            if a.size == 0:
                self.tensors.append(torch.empty(0, dtype=types[name], device="cuda"))
            elif name == "bfloat16":
                self.tensors.append(torch.from_numpy(a.view(np.int16).copy()).cuda().view(torch.bfloat16))
            else:
                self.tensors.append(torch.from_numpy(a.copy()).cuda())
            assert self.tensors[-1].dtype == (torch.bfloat16 if name == "bfloat16" else types[name])
        self.bases = [None if b is None else torch.from_numpy(b.copy()).cuda() for b in M.BASES]
        self.side = torch.cuda.Stream()
        torch.cuda.synchronize()

    def keywords(self, combo, subset=None):
        kw = M.keywords(combo, subset)
        if "base" in kw:
            kw["base"] = self.part(self.bases, subset)
        return kw

    @staticmethod
    def part(items, subset):
        return list(items) if subset is None else [items[b] for b in M.SUBSETS[subset]]

    def unchanged(self):
        for t, a in zip(self.tensors, M.ARRAYS):
            assert on_host(t) == M._raw(a).tobytes()
        for t, a in zip(self.bases, M.BASES):
            assert t is None or on_host(t) == a.tobytes()


@pytest.fixture(scope="module")
def T(H):
    return Uploaded()


def on_host(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""


def compare(c, m, what):
    """every field of the Compressed `c` against the model `m`"""
    assert c.sizes == m.sizes and c.first_packet == m.first_packet, what
    assert c.planes == m.planes and c.delta == m.delta and c.based == m.based, (what, c.planes, c.delta, c.based)
    assert c.delta is None or all(isinstance(f, bool) for f in c.delta), what
    assert c.based is None or all(isinstance(f, bool) for f in c.based), what
    assert c.stream.dtype == torch.uint8 and c.offsets.dtype == torch.int64
    assert c.offsets.cpu().tolist() == m.offsets, what
    assert on_host(c.stream) == m.stream, what
    if m.stored is None:
        assert c.stored is None and c.raw is None and c.raw_offsets is None, what
    else:
        assert c.stored.dtype == torch.uint8 and c.stored.cpu().tolist() == m.stored, what
        assert c.raw.dtype == torch.uint8 and c.raw_offsets.dtype == torch.int64
        assert c.raw_offsets.cpu().tolist() == m.raw_offsets, what
        assert on_host(c.raw) == m.raw, what
    if m.sparse is None:
        assert c.sparse is None and c.sparse_offsets is None, what
    else:
        assert c.sparse.dtype == torch.uint8 and c.sparse_offsets.dtype == torch.int64
        assert c.sparse_offsets.cpu().tolist() == m.sparse_offsets, what
        assert on_host(c.sparse) == m.sparse, what
    if m.crc32 is None:
        assert c.crc32 is None, what
    else:
        assert [v & 0xFFFFFFFF for v in c.crc32.cpu().tolist()] == m.crc32, what
    assert c.nbytes == m.nbytes and c.n_packets == m.first_packet[-1] and c.n_buffers == len(m.sizes), what
    COMPARED.append(what)


def check_gips(H, c, m, what):
    for b, want in enumerate(m.gips):
        if want is None:
            with pytest.raises(H.GpuarError):
                c.gip(b)
        else:
            assert c.gip(b) == want, (what, b)


def check_decompress(batch, c, arrays, bases, stream, caller_first, what):
    """two decompress calls, into fresh tensors and into caller tensors with a canary behind every buffer; the first verifies"""
    results = []
    for nth, into_caller in enumerate((caller_first, not caller_first)):
        out = None
        if into_caller:
            out = [torch.full((n + 16 + 16 * (b % 3),), CANARY, dtype=torch.uint8, device="cuda") for b, n in enumerate(c.sizes)]
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
        got = batch.decompress(c, out=out, stream=stream, verify=nth == 0, base=bases)
        assert out is None or all(g is o for g, o in zip(got, out))
        results.append(got)
    if stream is not None:
        stream.synchronize()
    for got in results:
        assert len(got) == len(arrays)
        for b, (t, a) in enumerate(zip(got, arrays)):
            have, want = on_host(t), M._raw(a).tobytes()
            assert t.dtype == torch.uint8 and have[:len(want)] == want, (what, b)
            assert have[len(want):] == bytes([CANARY]) * (len(have) - len(want)), (what, b, "wrote behind the buffer")
    assert any(t.numel() > n for got in results for t, n in zip(got, c.sizes))


def run(H, T, combo, subset=None):
    from gpuar_amd import batch
    checksum, side, mode, caller_first = ROTATION[combo]
    what = (combo, subset)
    stream = T.side if side else None
    tensors, bases = T.part(T.tensors, subset), T.part(T.bases, subset)
    kw = T.keywords(combo, subset)
    c = batch.compress(tensors, mode=mode, stream=stream, checksum=checksum, **kw)
    if stream is not None:
        stream.synchronize()
    m = M.model(combo, checksum, subset)
    compare(c, m, what)
    if combo[2] != "list":
        names = T.part(M.DTYPES, subset)
        arrays = T.part(M.ARRAYS, subset)
        assert batch.estimate(tensors, **kw) == M.model_estimate(arrays, names, **M.keywords(combo, subset)), what
    check_decompress(batch, c, T.part(M.ARRAYS, subset), bases if "base" in kw else None, stream, caller_first, what)
    check_gips(H, c, m, what)
    return c, m


# ---- the matrix --------------------------------------------------------------------------------------------------------

def test_the_rotation_covers_every_pair():
    assert len(VALID) == 200 and len(PAIRS) == 40
    rows = [c + tuple(str(v) for v in ROTATION[c]) for c in VALID]
    values = [sorted({r[i] for r in rows}) for i in range(8)]
    assert [len(v) for v in values] == [5, 8, 3, 2, 2, 2, 3, 2]
    for i in range(4, 8):                                      # a rotating keyword ...
        for j in range(8):                                     # ... against every axis and every other rotating keyword
            if i != j:
                assert {(r[i], r[j]) for r in rows} == {(x, y) for x in values[i] for y in values[j]}, (i, j)


@pytest.mark.parametrize("planes,filter_", PAIRS, ids=[f"{p}-{f}" for p, f in PAIRS])
def test_every_field_estimate_decompress_and_gip_equal_the_model(H, T, planes, filter_):
    n = 0
    for stored in M.STORED_AXIS:
        for sparse in M.SPARSE_AXIS:
            combo = (planes, filter_, stored, sparse)
            if not M.is_refused(combo):
                run(H, T, combo)
                n += 1
    assert n == 5
    T.unchanged()
    assert H.status() == 0


@pytest.mark.parametrize("subset", sorted(M.SUBSETS))
def test_a_part_of_the_batch_with_an_empty_kind(H, T, subset):
    empty = set()
    for combo in M.SUBSET_COMBOS:
        c, m = run(H, T, combo, subset)
        if m.stored is not None:
            empty |= {kind for kind in (M.CODED, M.RAW, M.SPARSE) if kind not in m.stored and (kind != M.SPARSE or m.sparse is not None)}
            assert c.offsets.numel() - 1 == m.stored.count(M.CODED) and c.raw_offsets.numel() - 1 == m.stored.count(M.RAW)
    assert empty >= {"calm": {M.RAW}, "still": {M.CODED, M.RAW}, "rough": {M.SPARSE}}[subset]
    T.unchanged()
    assert H.status() == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planes", list(M.PLANES_AXIS))
def test_sparse_beside_a_stored_list_is_refused_and_the_next_call_is_right(H, T, planes):
    from gpuar_amd import batch
    for n, filter_ in enumerate(M.FILTER_AXIS):
        refused = (planes, filter_, "list", "auto")
        assert M.is_refused(refused)
        with pytest.raises(H.GpuarError, match="sparse"):
            batch.compress(T.tensors, **T.keywords(refused))
        follow = (planes, filter_, ("list", "auto", "none")[n % 3], "none" if n % 3 == 0 else "auto")
        checksum = ROTATION[follow][0]
        compare(batch.compress(T.tensors, checksum=checksum, **T.keywords(follow)), M.model(follow, checksum), ("after", refused))
    T.unchanged()
    assert H.status() == 0


def test_base_beside_delta_and_base_auto_without_base_are_refused(H, T):
    from gpuar_amd import batch
    calls = [dict(base=T.bases, delta=delta) for delta in (True, False, M.DELTA_LIST, "auto", "survey")] + [dict(base_auto=True)]
    calls += [dict(base=T.bases, delta=True, base_auto="survey"), dict(base=T.bases, delta="survey", base_auto="survey"), dict(base_auto="survey")]
    follows = [("auto", "base", "auto", "auto"), ("auto", "delta", "auto", "auto"), ("survey", "base_auto", "auto", "none"),
               ("list", "delta_auto", "none", "auto"), ("2", "delta_survey", "list", "none"), ("none", "none", "none", "none"),
               ("survey", "base_survey", "auto", "auto"), ("2", "base_survey", "none", "auto"), ("survey", "base_survey", "list", "none")]
    assert len(calls) == len(follows) == 9
    for kw, follow in zip(calls, follows):
        with pytest.raises(H.GpuarError, match="base"):
            batch.compress(T.tensors, planes="auto", **kw)
        with pytest.raises(H.GpuarError, match="base"):
            batch.estimate(T.tensors, planes="auto", **kw)
        checksum = ROTATION[follow][0]
        compare(batch.compress(T.tensors, checksum=checksum, **T.keywords(follow)), M.model(follow, checksum), ("after", sorted(kw)))
    T.unchanged()
    assert H.status() == 0


def launches_of(monkeypatch, batch):
    """the names of the functions of batch.H that take a stream -- the ones that launch or copy -- as they are called from here on"""
    import inspect
    seen = []
    for name, fn in sorted(vars(batch.H).items()):
        if inspect.isfunction(fn) and not name.startswith("_") and "stream" in inspect.signature(fn).parameters:
            def wrapped(*args, _name=name, _fn=fn, **kwargs):
                seen.append(_name)
                return _fn(*args, **kwargs)
            monkeypatch.setattr(batch.H, name, wrapped)
    return seen


def test_base_auto_of_another_string_is_refused_before_any_launch(H, T, monkeypatch):
    """base_auto="auto" is no spelling of anything (delta="auto" is): GpuarError that names the values, from compress and estimate,
    beside every value of `planes` -- planes="survey", which would launch first, too -- and with nothing launched."""
    from gpuar_amd import batch
    seen = launches_of(monkeypatch, batch)
    for planes in M.PLANES_AXIS.values():
        for call in (batch.compress, batch.estimate):
            with pytest.raises(H.GpuarError, match=r'base_auto=\'auto\': False, True or "survey"'):
                call(T.tensors, planes=planes, base=T.bases, base_auto="auto", stored="auto", sparse="auto")
    with pytest.raises(H.GpuarError, match="base_auto"):
        batch.compress(T.tensors, planes="survey", base_auto="auto")              # (without a base: that refusal comes first)
    assert seen == [], seen
    follow = ("survey", "base_survey", "none", "auto")
    checksum = ROTATION[follow][0]
    compare(batch.compress(T.tensors, checksum=checksum, **T.keywords(follow)), M.model(follow, checksum), ("after", "base_auto='auto'"))
    assert "survey_xor_batch" in seen and "encode_batch" in seen
    T.unchanged()
    assert H.status() == 0


def test_base_survey_beside_a_width_the_surveys_do_not_have(H, T, monkeypatch):
    """base_auto="survey" decides from the surveys' rows, which are those of widths 1, 2, 4 and 8: beside planes=3, or a list with a
    3 in it, compress and estimate raise GpuarError that names the width, before any launch -- where base_auto=True, which splits,
    gets BAD_BATCH from the device for the same width.  The call behind each is right."""
    from gpuar_amd import batch
    seen = launches_of(monkeypatch, batch)
    listed = [3 if b == 3 else w for b, w in enumerate(M.PLANES_AXIS["list"])]
    for planes in (3, listed):
        for call in (batch.compress, batch.estimate):
            with pytest.raises(H.GpuarError, match=r'base_auto="survey": the widths are \(1, 2, 4, 8\), not \[3\]'):
                call(T.tensors, planes=planes, base=T.bases, base_auto="survey")
    assert seen == [], seen
    follow = ("list", "base_survey", "auto", "none")
    checksum = ROTATION[follow][0]
    compare(batch.compress(T.tensors, checksum=checksum, **T.keywords(follow)), M.model(follow, checksum), ("after", "planes=3"))
    assert seen.count("survey_planes_batch") == 1 and seen.count("survey_xor_batch") == 1 and seen.count("split_xor_batch") == 1, seen
    with pytest.raises(H.GpuarError, match="BAD_BATCH"):
        batch.compress(T.tensors, planes=3, base=T.bases, base_auto=True)
    follow = ("survey", "base_survey", "auto", "auto")
    checksum = ROTATION[follow][0]
    compare(batch.compress(T.tensors, checksum=checksum, **T.keywords(follow)), M.model(follow, checksum), ("after", "BAD_BATCH"))
    T.unchanged()
    assert H.status() == 0


# ---- damage ------------------------------------------------------------------------------------------------------------

def host_view(c):
    """a Compressed as the model's object: every field on the host"""
    m = M.Model()
    m.sizes, m.first_packet, m.planes, m.delta, m.based = c.sizes, c.first_packet, c.planes, c.delta, c.based
    m.stored = c.stored.cpu().tolist() if c.stored is not None else None
    m.stream, m.offsets = on_host(c.stream), c.offsets.cpu().tolist()
    m.raw, m.raw_offsets = (on_host(c.raw), c.raw_offsets.cpu().tolist()) if c.raw is not None else (None, None)
    m.sparse, m.sparse_offsets = (on_host(c.sparse), c.sparse_offsets.cpu().tolist()) if c.sparse is not None else (None, None)
    m.crc32 = [v & 0xFFFFFFFF for v in c.crc32.cpu().tolist()] if c.crc32 is not None else None
    return m


def test_damage_is_reported_at_the_packet_the_model_gets_wrong_first(H, T):
    """One byte of a raw packet and the fill byte of a sparse record, under planes and the delta filter: the packet that comes back
    wrong first is in general not the one that was damaged -- the filter carries the error to the end of the group, the planes
    spread a plane's packet over the group's packets."""
    from gpuar_amd import batch
    combo = ("auto", "delta", "auto", "auto")
    c = batch.compress(T.tensors, checksum=True, **T.keywords(combo))
    m = M.model(combo, True)
    compare(c, m, ("damage", combo))
    # raw: the low-byte plane of the bf16 tensor's first group, at element 6000 of 8192 -- bytes 12000 and on of the buffer
    p_raw = m.first_packet[2]
    assert m.stored[p_raw] == M.RAW and m.planes[2] == 2
    at = m.raw_offsets[m.stored[:p_raw].count(M.RAW)] + 6000
    # sparse: plane 1 of the position ids' first group -- byte 1 of every difference, so every element of the group
    p_sparse = m.first_packet[1] + 1
    assert m.stored[p_sparse] == M.SPARSE and m.planes[1] == 4
    fill_at = m.sparse_offsets[m.stored[:p_sparse].count(M.SPARSE)]
    damaged_raw, damaged_sparse = c.raw.clone(), c.sparse.clone()
    damaged_raw[at] ^= 0x10
    damaged_sparse[fill_at] ^= 0x01
    for what, bad, p_damaged in (("raw", dataclasses.replace(c, raw=damaged_raw), p_raw), ("sparse", dataclasses.replace(c, sparse=damaged_sparse), p_sparse)):
        view = host_view(bad)
        assert (view.raw, view.sparse) != (m.raw, m.sparse)
        first = M.first_wrong_packet(view, M.model_decompress(view))
        assert first is not None and view.first_packet[first[0]] + first[1] != p_damaged, (what, first)
        b, j = first
        with pytest.raises(H.GpuarError, match=rf"checksum mismatch: buffer {b}, packet {j} \(batch packet {view.first_packet[b] + j}\)"):
            batch.decompress(bad)
        got = batch.decompress(bad, verify=False)               # without the check the damage goes through, as the model has it
        assert [on_host(t) for t in got] == [x.tobytes() for x in M.model_decompress(view)], what
    back = batch.decompress(c)
    assert [on_host(t) for t in back] == [M._raw(a).tobytes() for a in M.ARRAYS]
    T.unchanged()
    assert H.status() == 0
