"""The XOR-base survey in the batch API on the MI355X: batch.survey_xor against batch.estimate, base_auto="survey"
against base_auto=True, the joint choice of width and base, and the temporary memory the survey saves."""
import numpy as np
import pytest

import xor_ref as X
import xor_survey_ref as XS
from test_survey_host import WIDTHS, one_mib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MIB = 1 << 20
PACKET = 8192


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def pairs(H):
    """DESIGN.md 4.10's six table pairs and the int64 pair, 1 MiB each: (names, tensors, bases)"""
    table = XS.table_pairs()
    names = list(X.TABLE_BASE_WINS) + list(X.TABLE_BASE_LOSES) + ["int64"]
    table["int64"] = XS.int64_pair()
    assert all(table[k][0].size == MIB for k in names)
    return names, [torch.from_numpy(table[k][0].copy()).cuda() for k in names], [torch.from_numpy(table[k][1].copy()).cuda() for k in names]


@pytest.mark.parametrize("sparse", [None, "auto"])
@pytest.mark.parametrize("stored", [None, "auto"])
def test_survey_xor_is_the_estimate_against_the_base_at_every_width(H, pairs, stored, sparse, monkeypatch):
    from gpuar_amd import batch
    names, xs, bs = pairs
    calls = []
    for name in ("survey_xor_batch", "survey_planes_batch", "split_xor_batch", "estimate_batch"):
        def counted(*a, _fn=getattr(batch.H, name), _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(batch.H, name, counted)
    got = batch.survey_xor(xs, bs, stored=stored, sparse=sparse)
    assert calls == ["survey_xor_batch"]                                              # one launch, nothing split
    monkeypatch.undo()
    per_width = [batch.estimate(xs, planes=w, base=bs, stored=stored, sparse=sparse) for w in WIDTHS]
    assert got == [[per_width[j][b] for j in range(4)] for b in range(len(xs))], (stored, sparse)
    # a tensor without a base gets its plain totals
    some = [b if i % 2 else None for i, b in enumerate(bs)]
    got = batch.survey_xor(xs, some, stored=stored, sparse=sparse)
    per_width = [batch.estimate(xs, planes=w, base=some, stored=stored, sparse=sparse) for w in WIDTHS]
    assert got == [[per_width[j][b] for j in range(4)] for b in range(len(xs))], (stored, sparse)
    widths = batch.survey_xor_widths(xs, bs, stored=stored, sparse=sparse)
    assert widths == [H.choose_planes(t, MIB // PACKET) for t in batch.survey_xor(xs, bs, stored=stored, sparse=sparse)]
    assert widths[names.index("int64")] == 1


def test_survey_xor_counts_what_the_host_twin_counts_and_refuses_what_it_cannot_take(H, pairs):
    from gpuar_amd import batch
    names, xs, bs = pairs
    i = names.index("int64")
    x, b = xs[i].cpu().numpy(), bs[i].cpu().numpy()
    est, scan = H.survey_xor_host(x.tobytes(), b.tobytes())
    assert batch.survey_xor([xs[i]], [bs[i]]) == [[sum(row) for row in est]] == [[31062, 31063, 31045, 31021]]
    assert batch.survey_xor([xs[i]], [bs[i]], sparse="auto") == [[XS.kinds_total(est[j], scan[j], MIB, False, True) for j in range(4)]]
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert batch.survey_xor([empty], [None]) == [[0, 0, 0, 0]] and batch.survey_xor_widths([empty], [empty]) == [1]
    for bad in (dict(base=None), dict(base=bs[:1] * 2), dict(base=[bs[i][:-8]]), dict(base=[bs[i]], stored=[True]), dict(base=[bs[i]], sparse="on")):
        with pytest.raises(H.GpuarError):
            batch.survey_xor([xs[i]], **bad)


def _same(a, b):
    assert torch.equal(a.stream, b.stream) and torch.equal(a.offsets, b.offsets)
    assert a.first_packet == b.first_packet and a.sizes == b.sizes and a.planes == b.planes and a.based == b.based
    for name in ("stored", "raw", "raw_offsets", "sparse", "sparse_offsets", "crc32"):
        p, q = getattr(a, name), getattr(b, name)
        assert (p is None) == (q is None) and (p is None or torch.equal(p, q)), name


@pytest.mark.parametrize("w", WIDTHS)
def test_base_auto_survey_is_base_auto_true(H, pairs, w, monkeypatch):
    from gpuar_amd import batch
    names, xs, bs = pairs
    calls = []
    for name in ("survey_xor_batch", "survey_planes_batch", "split_xor_batch", "split_planes_batch", "estimate_batch"):
        def counted(*a, _fn=getattr(batch.H, name), _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(batch.H, name, counted)
    fast = batch.compress(xs, planes=w, base=bs, base_auto="survey", checksum=True)
    assert calls == ["survey_planes_batch", "survey_xor_batch", "split_xor_batch"]    # two surveys, then ONE split and no estimate
    monkeypatch.undo()
    slow = batch.compress(xs, planes=w, base=bs, base_auto=True, checksum=True)
    assert slow.based == [k in X.TABLE_BASE_WINS or k == "int64" for k in names]
    _same(fast, slow)
    for o, t in zip(batch.decompress(fast, base=bs), xs):
        assert torch.equal(o, t)
    for kwargs in (dict(stored="auto"), dict(stored="auto", sparse="auto")):
        _same(batch.compress(xs, planes=w, base=bs, base_auto="survey", **kwargs), batch.compress(xs, planes=w, base=bs, base_auto=True, **kwargs))
    assert batch.estimate(xs, planes=w, base=bs, base_auto="survey") == batch.estimate(xs, planes=w, base=bs, base_auto=True)
    # nothing to choose from, and what base_auto=True refuses
    none = batch.compress(xs[:2], planes=w, base=[None, None], base_auto="survey")
    _same(none, batch.compress(xs[:2], planes=w, base=[None, None], base_auto=True))
    for bad in (dict(base_auto="survey"), dict(base=bs, base_auto="auto"), dict(base=bs, base_auto="survey", delta=True)):
        with pytest.raises(H.GpuarError):
            batch.compress(xs, planes=w, **bad)


def test_width_and_base_are_chosen_together(H, pairs):
    from gpuar_amd import batch
    names, xs, bs = pairs
    i = names.index("int64")
    fp32 = torch.from_numpy(np.ascontiguousarray(one_mib("fp32"))).cuda()
    unrelated = torch.from_numpy(np.random.default_rng(77).integers(0, 256, MIB, dtype=np.uint8)).cuda()
    tensors, bases = [xs[i], fp32, xs[0]], [bs[i], unrelated, None]
    assert batch.compress(tensors, planes="survey").planes[:2] == [8, 4]              # the original bytes pick 8 for the indices
    assert batch.compress(tensors, planes="survey", base=bases).planes[:2] == [8, 4]  # ... and still do beside a fixed base
    for kwargs in ({}, dict(stored="auto"), dict(sparse="auto"), dict(stored="auto", sparse="auto", checksum=True)):
        c = batch.compress(tensors, planes="survey", base=bases, base_auto="survey", **kwargs)
        assert (c.planes[0], c.based[0]) == (1, True) and (c.planes[1], c.based[1]) == (4, False) and c.based[2] is False, kwargs
        widths, kept = batch.survey_base_choice(tensors, bases, kwargs.get("stored"), kwargs.get("sparse"))
        assert (c.planes, c.based) == (widths, kept)
        fixed = batch.compress(tensors, planes=c.planes, base=[bs[i], None, None], **kwargs)
        _same(c, fixed)
        for o, t in zip(batch.decompress(c, base=bases), tensors):
            assert torch.equal(o.view(torch.uint8), t.view(torch.uint8)), kwargs
        est = batch.estimate(tensors, planes="survey", base=bases, base_auto="survey", **{k: v for k, v in kwargs.items() if k != "checksum"})
        assert est == batch.estimate(tensors, planes=c.planes, base=[bs[i], None, None], **{k: v for k, v in kwargs.items() if k != "checksum"})
    # the totals behind the choice are those of survey and survey_xor
    plain, xored = batch.survey(tensors), batch.survey_xor(tensors, bases)
    assert batch.survey_base_choice(tensors, bases) == (
        [H.choose_filter(p, x, MIB // PACKET)[0] if b is not None else H.choose_planes(p, MIB // PACKET) for p, x, b in zip(plain, xored, bases)],
        [b is not None and H.choose_filter(p, x, MIB // PACKET)[1] for p, x, b in zip(plain, xored, bases)])


def test_the_survey_needs_one_temporary_of_the_batch_where_base_auto_true_needs_two(H):
    """64 MiB of bf16 a small step from its base: base_auto=True keeps two split copies of the batch until the slots are freed,
    base_auto="survey" one.  The bound: one temporary of the batch's size less the survey rows (32 bytes a packet), so 0.9 of it."""
    from gpuar_amd import batch
    g = torch.Generator(device="cuda").manual_seed(6)
    n_tensors, elements = 8, 4 * MIB
    base = [(torch.randn(elements, device="cuda", generator=g) * 0.02).bfloat16() for _ in range(n_tensors)]
    xs = [(b.float() + torch.randn(elements, device="cuda", generator=g) * 1e-4).bfloat16() for b in base]
    total = sum(t.numel() * 2 for t in xs)
    assert total == 64 * MIB
    peaks = {}
    for how in ("survey", True):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        c = batch.compress(xs, planes=2, base=base, base_auto=how)
        torch.cuda.synchronize()
        peaks[how] = torch.cuda.max_memory_allocated() - before
        assert c.based == [True] * n_tensors
        del c
    print(peaks, total)
    assert peaks[True] - peaks["survey"] >= 0.9 * total, (peaks, total)
