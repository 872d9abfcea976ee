"""The host-side contract of include/gpuar_hip_xsurvey.h, the header of the XOR-base survey: its names
are exactly those of hip.XSURVEY_SIGNATURES, with the header's arities, the library exports them, and the two device calls return
the documented code for each defect, in the documented order -- called with made-up addresses and rejected (or a no-op) before the
library touches a device, as tests/test_capi_codes_host.py does for the others.  (The host call's codes: test_xor_survey_host.py.)"""
import pytest

from test_capi_codes_host import ALIGNMENT, ARGUMENT, MANY, MANY_BYTES, OK, A, B, C, D, E, F, G, pointer_cases
from test_capi_symbols import declared_arity, declared_symbols

HEADER = "gpuar_hip_xsurvey.h"


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from gpuar_amd import hip as H
    if not os.path.exists(H.LIB_PATH):
        g.build()
    return H.load()


def test_the_header_declares_exactly_the_third_binding_table(lib):
    from gpuar_amd import hip as H
    names = declared_symbols(HEADER)
    assert set(names) == set(H.XSURVEY_SIGNATURES) and len(names) == 3, (names, list(H.XSURVEY_SIGNATURES))
    for other in (set(H.EXPORTS), set(H.GIP_SIGNATURES), set(declared_symbols()), set(declared_symbols("gpuar_hip_gip.h"))):
        assert not set(names) & other                      # a name is declared in one header and bound from one table
    for name, arity in declared_arity(HEADER).items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity == len(H.XSURVEY_SIGNATURES[name][1]), (name, arity, fn.argtypes)
    assert declared_arity(HEADER) == {"gpuar_hip_survey_xor": 7, "gpuar_hip_survey_xor_batch": 11, "gpuar_hip_survey_xor_host": 6}
    assert H.ABI_VERSION == 2 == lib.gpuar_hip_abi_version() and lib.gpuar_hip_version() == b"gpuar-hip 0.2 gfx950"


def test_a_library_without_the_new_calls_is_refused_with_the_rebuild_message(monkeypatch):
    from gpuar_amd import hip as H
    monkeypatch.setattr(H, "_lib", None)
    monkeypatch.setattr(H, "XSURVEY_SIGNATURES", {**H.XSURVEY_SIGNATURES, "gpuar_hip_no_such_survey": H.XSURVEY_SIGNATURES["gpuar_hip_survey_xor"]})
    with pytest.raises(H.GpuarError, match=r"lacks \['gpuar_hip_no_such_survey'\].*rebuild the library"):
        H.load()


def xsurvey_cases():
    cases = []
    good = (A, B, 5 * 8192, C, D, 5, None)                 # d_in, d_base, n_bytes, d_est, d_scan, stride, stream
    ptrs = {0: ("d_in", 16, False), 1: ("d_base", 16, False), 3: ("d_est", 4, True), 4: ("d_scan", 4, True)}
    cases += pointer_cases("gpuar_hip_survey_xor", good, ptrs, nothing=(2, (0, 1, 3, 4)), tail=[
        ("both outputs null", {3: None, 4: None}, ARGUMENT),
        ("both outputs null and a misaligned d_in", {0: A + 8, 3: None, 4: None}, ARGUMENT),
        ("stride below the packet count", {5: 4}, ARGUMENT),
        ("too many packets", {2: MANY_BYTES, 5: MANY}, ARGUMENT),
        ("a short stride with a misaligned d_base", {1: B + 8, 5: 4}, ARGUMENT),            # every ARGUMENT before any ALIGNMENT
        ("a null d_base with a misaligned d_est", {1: None, 3: C + 2}, ARGUMENT),
        ("a null d_in with a misaligned d_base", {0: None, 1: B + 8}, ARGUMENT),
        ("no d_est and a misaligned d_scan", {3: None, 4: D + 2}, ALIGNMENT),               # the scan rows stand in for the est rows
        ("no d_scan and a misaligned d_est", {3: C + 2, 4: None}, ALIGNMENT),
        ("no d_scan and a misaligned d_base", {1: B + 4, 4: None}, ALIGNMENT),
        ("nothing to do with every pointer misaligned", {0: A + 1, 1: B + 1, 2: 0, 3: C + 1, 4: D + 1, 5: 0}, OK),
    ])
    # d_in_ptrs, d_in_bytes, d_first_packet, d_base_ptrs, n_buffers, n_packets, d_est, d_scan, stride, d_status, stream
    good = (A, B, C, D, 3, 5, E, F, 5, G, None)
    ptrs = {0: ("d_in_ptrs", 8, False), 1: ("d_in_bytes", 8, False), 2: ("d_first_packet", 8, False), 3: ("d_base_ptrs", 8, False),
            6: ("d_est", 4, True), 7: ("d_scan", 4, True), 9: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_survey_xor_batch", good, ptrs, nothing=(5, (0, 1, 2, 3, 6, 7, 9)), tail=[
        ("both outputs null", {6: None, 7: None}, ARGUMENT),
        ("too many buffers", {4: MANY}, ARGUMENT),
        ("too many packets", {5: MANY, 8: MANY}, ARGUMENT),
        ("stride below the packet count", {8: 4}, ARGUMENT),
        ("a short stride with a misaligned d_base_ptrs", {3: D + 4, 8: 4}, ARGUMENT),
        ("a null d_base_ptrs with a misaligned d_status", {3: None, 9: G + 2}, ARGUMENT),
        ("no d_est and a misaligned d_scan", {6: None, 7: F + 2}, ALIGNMENT),
        ("no d_scan and a misaligned d_base_ptrs", {3: D + 4, 7: None}, ALIGNMENT),
        ("nothing to do with every pointer misaligned", {0: A + 1, 1: B + 1, 2: C + 1, 3: D + 1, 5: 0, 6: E + 1, 7: F + 1, 9: G + 1}, OK),
    ])
    return cases


CASES = xsurvey_cases()


def test_the_table_covers_every_device_call_of_the_header():
    from gpuar_amd import hip as H
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))
    assert {c[1] for c in CASES} == set(H.XSURVEY_SIGNATURES) - {"gpuar_hip_survey_xor_host"}


@pytest.mark.parametrize("what,name,args,want", CASES, ids=[c[0] for c in CASES])
def test_code(lib, what, name, args, want):
    assert getattr(lib, name)(*args) == want
