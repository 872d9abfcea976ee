"""The sequence of launches, staged uploads and synchronising reads that batch.py makes, pinned for every one of the 200 valid option
combinations of tests/test_gpu_batch_matrix.py: the speed of that layer is this sequence, so a change of batch.py that keeps it keeps
the speed, and one that adds a launch, a pinned upload or a wait shows up here and not in a timing.

On the batch of 14 tensors of tests/batch_model.py (test_gpu_batch_matrix's Uploaded; no new inputs), with checksum, stream and mode
as ROTATION gives them, the test records what is called inside
    compress
    estimate                          (not for a list of stored packets, which estimate does not take)
    decompress(verify=True)
    from_gip of the buffers' gip(b, kinds=...) files, where every buffer has a file (kinds: where the kinds came from the rule)
in order: every call of a function of batch.H that takes a stream -- the ones that launch or copy -- as its name and its n_buffers /
n_packets / n_regions; every torch.Tensor.item, .tolist and .cpu on a CUDA tensor (the synchronising reads); every
torch.Tensor.pin_memory (the staged uploads).  What the test itself calls between those four is not recorded.

The expected traces are tests/golden/batch_call_trace.json, every distinct trace once with the (combination, call) pairs that have it.
The file was written by this module run as a script,
    python tests/test_gpu_batch_trace.py --write
against the batch.py of the commit in front of the one that made batch.py one split, one upload, one partition and one prepare step:
it is the record of that commit's behaviour and is never rewritten from later code (its first key says so).  It holds the 175
combinations that commit had.  base_auto="survey" came later (the 25 combinations of the filter value base_survey): their traces
are held to what batch.py's docstring says of the keyword instead (SURVEY_PREFIX) -- with the widths fixed one plane-survey
launch, one XOR-survey launch, one synchronising read and ONE split; beside planes="survey" the two survey launches in front (with
sparse="auto" both of them the XOR survey, the plain side with base pointers of 0), the same read and one split --, and behind
the split to the trace of base_auto=True behind its second split and estimate, launch for launch by name.

Two things came later still and are held byte for byte by a second file, tests/golden/batch_call_trace_later.json, written by
    python tests/test_gpu_batch_trace.py --write-later
against the batch.py of the commit in front of the one that made batch.py one batch description, one filter plan and one counting
rule, and never rewritten from later code either: the full traces of the 25 base_survey combinations (beside check_base_survey, which
stays), and planes="mixed", which is on no axis of the matrix -- the 20 combinations of MIXED on the same batch, with checksum, stream
and mode from mixed_rotation: per combination the traces of compress, estimate and decompress(verify=True), what estimate returned,
Compressed.modes, based and kinds_rule, and a sha256 of every device field of the Compressed (read outside the recording).  The
recording process also checks that decompress gives the input bytes back.

The recording runs in a process of its own (this module as a script, --record FILE) and the test compares what it wrote: a process
that has wrapped torch.Tensor's methods, uploaded the batch a second time and driven 665 calls over one more stream leaves the
streams of the pool in another state than it found them, and the stream-order tests of tests/test_gpu_packet_forms_concurrency.py,
which run later in the same pytest process, then find their control launch serialised behind their producer.  The child starts,
imports torch and records in about 5 s."""
import contextlib
import hashlib
import inspect
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import batch_model as M  # noqa: E402
from test_gpu_batch_matrix import MODES, ROTATION, VALID, Uploaded, on_host  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_call_trace.json")
WRITTEN_FROM = ("the batch.py of the commit in front of 'batch.py: one split, one upload, one partition, one prepare step' "
                "(python tests/test_gpu_batch_trace.py --write); never from later code")
LATER = os.path.join(ROOT, "tests", "golden", "batch_call_trace_later.json")
WRITTEN_FROM_LATER = ("the batch.py of the commit in front of 'batch.py: one batch description, one filter plan, one counting rule' "
                      "(python tests/test_gpu_batch_trace.py --write-later); never from later code")
COUNTS = ("n_buffers", "n_packets", "n_regions")
RECORDED = [c for c in VALID if c[1] != "base_survey"]         # the combinations of the golden file
# base_auto="survey" by batch.py's docstring: (planes="survey", sparse packets counted) -> the launches and the one synchronising
# read up to and including the one split
SURVEY_PREFIX = {
    (False, False): ["survey_planes_batch", "survey_xor_batch", ".tolist", "split_xor_batch"],
    (True, False): ["survey_planes_batch", "survey_xor_batch", ".tolist", "split_xor_batch"],
    (True, True): ["survey_xor_batch", "survey_xor_batch", ".tolist", "split_xor_batch"],
}
READS = ("item", "tolist", "cpu")
# planes="mixed": (delta, base, stored, sparse) by name -- delta None or "mixed", no base or the batch's bases, the five valid pairs
MIXED = [(d, b, s, q) for d in ("none", "mixed") for b in ("none", "base") for s in M.STORED_AXIS for q in M.SPARSE_AXIS
         if not (s == "list" and q == "auto")]
DEVICE_FIELDS = ("stream", "offsets", "crc32", "stored", "raw", "raw_offsets", "sparse", "sparse_offsets")


def mixed_rotation(combo):
    """(checksum, side stream, mode) for a mixed combination, from its position i among the 20"""
    i = MIXED.index(combo)
    return bool(i % 2), bool((i // 2 + i // 5) % 2), MODES[(i + i // 3) % 3]


class Recorder:
    """the calls made while `during` is open, in order"""

    def __init__(self):
        self.trace = None

    @contextlib.contextmanager
    def during(self):
        self.trace = []
        try:
            yield self.trace
        finally:
            self.trace = None

    def launch(self, name, fn):
        signature = inspect.signature(fn)

        def wrapped(*args, **kwargs):
            if self.trace is not None:
                given = signature.bind(*args, **kwargs).arguments
                self.trace.append(" ".join([name] + [str(int(given[k])) for k in COUNTS if k in given]))
            return fn(*args, **kwargs)
        return wrapped

    def method(self, name, fn, cuda_only):
        def wrapped(tensor, *args, **kwargs):
            if self.trace is not None and (tensor.is_cuda or not cuda_only):
                self.trace.append("." + name)
            return fn(tensor, *args, **kwargs)
        return wrapped


def install(monkeypatch, batch):
    """every function of batch.H that takes a stream, and the four tensor methods, wrapped until `monkeypatch` undoes it"""
    rec = Recorder()
    for name, fn in sorted(vars(batch.H).items()):
        if inspect.isfunction(fn) and not name.startswith("_") and "stream" in inspect.signature(fn).parameters:
            monkeypatch.setattr(batch.H, name, rec.launch(name, fn))
    for name in READS:
        monkeypatch.setattr(torch.Tensor, name, rec.method(name, getattr(torch.Tensor, name), True))
    monkeypatch.setattr(torch.Tensor, "pin_memory", rec.method("pin_memory", torch.Tensor.pin_memory, False))
    return rec


def traces_of(batch, rec, T, combo):
    """{call: trace} of one combination"""
    checksum, side, mode, _caller_first = ROTATION[combo]
    stream = T.side if side else None
    kw = T.keywords(combo)
    out = {}
    with rec.during() as trace:
        c = batch.compress(T.tensors, mode=mode, stream=stream, checksum=checksum, **kw)
    out["compress"] = trace
    if stream is not None:
        stream.synchronize()
    if combo[2] != "list":
        with rec.during() as trace:
            batch.estimate(T.tensors, **kw)
        out["estimate"] = trace
    with rec.during() as trace:
        batch.decompress(c, stream=stream, verify=True, base=T.bases if "base" in kw else None)
    out["decompress"] = trace
    if stream is not None:
        stream.synchronize()
    try:
        files = [c.gip(b, kinds=c.kinds_rule is not None) for b in range(c.n_buffers)]
    except batch.GpuarError:
        files = None                                           # (a list of stored packets, or a base without the CRCs)
    if files is not None:
        with rec.during() as trace:
            batch.from_gip(files, stream=stream)
        out["from_gip"] = trace
        if stream is not None:
            stream.synchronize()
    return out


def mixed_record(batch, rec, T, combo):
    """what one mixed combination does and gives: its traces, and -- read outside the recording -- its results"""
    checksum, side, mode = mixed_rotation(combo)
    stream = T.side if side else None
    d, b, s, q = combo
    kw = dict(planes="mixed", delta=None if d == "none" else "mixed", stored=M.STORED_AXIS[s], sparse=M.SPARSE_AXIS[q])
    if b == "base":
        kw["base"] = T.bases
    out = {"traces": {}}
    with rec.during() as trace:
        c = batch.compress(T.tensors, mode=mode, stream=stream, checksum=checksum, **kw)
    out["traces"]["compress"] = trace
    if stream is not None:
        stream.synchronize()
    if s != "list":
        with rec.during() as trace:
            estimate = batch.estimate(T.tensors, **kw)
        out["traces"]["estimate"], out["estimate"] = trace, estimate
    with rec.during() as trace:
        back = batch.decompress(c, stream=stream, verify=True, base=kw.get("base"))
    out["traces"]["decompress"] = trace
    if stream is not None:
        stream.synchronize()
    assert [on_host(x) for x in back] == [on_host(t) for t in T.tensors], combo
    out["modes"] = [m.hex() for m in c.modes]
    out["based"], out["kinds_rule"] = c.based, list(c.kinds_rule) if c.kinds_rule is not None else None
    for name in DEVICE_FIELDS:
        field = getattr(c, name)
        out[name] = None if field is None else hashlib.sha256(field.cpu().numpy().tobytes()).hexdigest()
    return out


def all_traces(monkeypatch):
    """({"planes-filter-stored-sparse:call": trace} over the 200 combinations, {"delta-base-stored-sparse": mixed_record} over the 20
    of MIXED)"""
    from gpuar_amd import batch
    batch.H.load()
    T = Uploaded()
    rec = install(monkeypatch, batch)
    got = {}
    for combo in VALID:
        for call, trace in traces_of(batch, rec, T, combo).items():
            got["-".join(combo) + ":" + call] = trace
    mixed = {"-".join(combo): mixed_record(batch, rec, T, combo) for combo in MIXED}
    T.unchanged()
    assert batch.H.status() == 0
    return got, mixed


def grouped(got):
    """every distinct trace once, with the calls that have it"""
    by_trace = {}
    for key, trace in got.items():
        by_trace.setdefault(";".join(trace), []).append(key)
    return [{"calls": keys, "trace": trace} for trace, keys in sorted(by_trace.items(), key=lambda kv: kv[1][0])]


def test_every_combination_makes_the_recorded_launches_uploads_and_reads(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert list(golden)[0] == "written from" and golden["written from"] == WRITTEN_FROM
    want = {key: entry["trace"].split(";") if entry["trace"] else [] for entry in golden["traces"] for key in entry["calls"]}
    assert len(want) == sum(len(entry["calls"]) for entry in golden["traces"])
    assert len({key.split(":")[0] for key in want}) == len(RECORDED) == 175 and len(VALID) == 200
    recorded = tmp_path / "traces.json"
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--record", str(recorded)], capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, (child.returncode, child.stdout[-2000:], child.stderr[-4000:])
    with open(recorded) as f:
        got, mixed = json.load(f)
    later = {key: trace for key, trace in got.items() if key.split("-")[1] == "base_survey"}
    got = {key: trace for key, trace in got.items() if key not in later}
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # the recording is not vacuous: every kind of event is there; estimate for all but the 35 combinations with a stored list; a file
    # of every buffer for all but those 35 and the 20 of the other 140 that have a base and, by the rotation, no CRCs
    events = {e.split()[0] for trace in got.values() for e in trace}
    assert {".item", ".tolist", ".pin_memory", "encode_batch", "decode_stream_batch", "move_bytes", "estimate_batch"} <= events
    assert sum(key.endswith(":estimate") for key in got) == 140 and sum(key.endswith(":from_gip") for key in got) == 120
    check_base_survey(later, got)
    check_later(later, mixed)


def check_later(later, mixed):
    """the base_survey traces and everything recorded of the mixed combinations against the second golden file, exactly"""
    with open(LATER) as f:
        golden = json.load(f)
    assert list(golden)[0] == "written from" and golden["written from"] == WRITTEN_FROM_LATER
    want = {key: entry["trace"].split(";") if entry["trace"] else [] for entry in golden["base_survey"] for key in entry["calls"]}
    assert len(want) == sum(len(entry["calls"]) for entry in golden["base_survey"]) == 25 + 20 + 25 + 10
    assert sorted(later) == sorted(want)
    for key in want:
        assert later[key] == want[key], key
    assert len(MIXED) == 20 and sorted(mixed) == sorted(golden["mixed"]) == sorted("-".join(c) for c in MIXED)
    turns = [mixed_rotation(c) for c in MIXED]
    assert {t[0] for t in turns} == {False, True} and {t[1] for t in turns} == {False, True} and {t[2] for t in turns} == set(MODES)
    for key, record in golden["mixed"].items():
        assert sorted(mixed[key]) == sorted(record), key
        for name in record:
            assert mixed[key][name] == record[name], (key, name)
        assert sorted(record["traces"]) == (["compress", "decompress"] if "-list-" in key else ["compress", "decompress", "estimate"]), key
        assert ("estimate" in record) == ("estimate" in record["traces"]), key
        assert [len(m) for m in record["modes"]] == [2 * ((size + 65535) // 65536) for size in M.SIZES], key    # a mode per supergroup
    # not vacuous: the mixed split and merge are launched once each per compress and decompress, and some supergroup takes each offer
    for key, record in golden["mixed"].items():
        assert sum(e.startswith("split_mixed_batch ") for e in record["traces"]["compress"]) == 1, key
        assert sum(e.startswith("merge_mixed_batch ") for e in record["traces"]["decompress"]) == 1, key
        assert (record["based"] is None) == ("-base-" not in "-" + key), key
    assert any(record["based"] is not None and any(record["based"]) for record in golden["mixed"].values())
    assert len({tuple(record["modes"]) for record in golden["mixed"].values()}) > 1


def names_of(trace):
    """the launches of a trace by name, and between them the synchronising reads"""
    return [e.split()[0] for e in trace if e != ".pin_memory"]


def check_base_survey(later, got):
    """the traces of base_auto="survey" against batch.py's docstring; `got`: the recorded traces of the other filter values"""
    combos = [c for c in VALID if c[1] == "base_survey"]
    assert len(combos) == 25 and sorted({key.split(":")[0] for key in later}) == sorted("-".join(c) for c in combos)
    assert sum(key.endswith(":estimate") for key in later) == 20 and sum(key.endswith(":from_gip") for key in later) == 10
    for c in combos:
        for call in ("compress", "estimate"):
            key = "-".join(c) + ":" + call
            if key not in later:
                assert call == "estimate" and c[2] == "list"
                continue
            trace, names = later[key], names_of(later[key])
            prefix = SURVEY_PREFIX[c[0] == "survey", c[0] == "survey" and c[3] == "auto"]
            assert names[:len(prefix)] == prefix, (key, names[:8])
            assert [e for e in trace if e.split()[0].startswith("survey_")] == [f"{name} 14 51" for name in prefix[:2]], key
            assert sum(name.startswith("split_") for name in names) == 1, (key, names)
            # behind the split: what base_auto=True does behind its two splits and estimates -- but for the estimate launch, which
            # _auto_base has made already and this path makes behind the split where stored or sparse (or estimate itself) needs one
            rest = names[len(prefix):]
            other = names_of(got["-".join((c[0], "base_auto") + c[2:]) + ":" + call])
            tail = other[len(other) - other[::-1].index("split_xor_batch"):]
            assert tail[:3] == ["estimate_batch", ".tolist", ".item"] and "estimate_batch" not in tail[3:], (key, tail)   # (_auto_base's own reads)
            assert [n for n in rest if n != "estimate_batch"] == tail[3:], (key, rest, tail)
            assert rest.count("estimate_batch") == (1 if call == "estimate" or c[2] == "auto" or c[3] == "auto" else 0), (key, rest)


if __name__ == "__main__":
    if sys.argv[1:] not in (["--write"], ["--write-later"]) and not (len(sys.argv) == 3 and sys.argv[1] == "--record"):
        sys.exit("usage: python tests/test_gpu_batch_trace.py --record FILE   (what the test compares), or --write / --write-later   (a "
                 "golden file, against the commit it records; see the docstring)")
    with pytest.MonkeyPatch.context() as patch:
        traces, mixed = all_traces(patch)
    if sys.argv[1] == "--record":
        with open(sys.argv[2], "w") as f:
            json.dump([traces, mixed], f)
    elif sys.argv[1] == "--write-later":
        later = {key: trace for key, trace in traces.items() if key.split("-")[1] == "base_survey"}
        with open(LATER, "w") as f:
            json.dump({"written from": WRITTEN_FROM_LATER, "base_survey": grouped(later), "mixed": mixed}, f, separators=(",", ":"))
            f.write("\n")
        print(f"{LATER}: {len(later)} base_survey calls, {len(mixed)} mixed combinations, {os.path.getsize(LATER)} bytes")
    else:
        traces = {key: trace for key, trace in traces.items() if key.split("-")[1] != "base_survey"}
        with open(GOLDEN, "w") as f:
            json.dump({"written from": WRITTEN_FROM, "traces": grouped(traces)}, f, separators=(",", ":"))
            f.write("\n")
        print(f"{GOLDEN}: {len(traces)} calls, {len({';'.join(t) for t in traces.values()})} distinct traces, {os.path.getsize(GOLDEN)} bytes")
