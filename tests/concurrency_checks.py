"""Verdict helpers of the concurrency tests (tests/test_gpu_concurrency.py, tests/test_gpu_filter_concurrency.py,
tests/test_gpu_packet_forms_concurrency.py; not a test module): comparisons that stay on the device, one copy to the host per
test that names every check that did not hold, status words against what each launch should report, and the non-blocking streams the launches go to.  torch is imported where it
is used, so that importing this module needs no GPU."""


def _status(k=1):
    """k zeroed status words on the device."""
    import torch
    return torch.zeros(k, dtype=torch.int32, device="cuda")


def _same(a, b):
    """Device verdict: a and b have the same shape and bytes."""
    import torch
    if a.shape != b.shape:
        return torch.zeros((), dtype=torch.bool, device="cuda")
    return a.eq(b).all()


def _fail_on(verdicts):
    """verdicts: [(description, device bool)]: one copy to the host; fails naming every check that did not hold."""
    import torch
    if not verdicts:
        return
    ok = torch.stack([v for _, v in verdicts]).cpu().numpy()
    wrong = [what for (what, _), good in zip(verdicts, ok) if not good]
    assert not wrong, f"{len(wrong)} of {len(verdicts)} checks failed: " + "; ".join(wrong[:12])


def _words(verdicts, words, expected, what):
    """Status words against what each launch should report (one verdict each)."""
    import torch
    want = torch.tensor(expected, dtype=torch.int32, device=words.device)
    for j, w in enumerate(what):
        verdicts.append((f"{w}: status word is not {expected[j]:#x}", words[j].eq(want[j])))


def _streams(k):
    import torch
    return [torch.cuda.Stream() for _ in range(k)]
