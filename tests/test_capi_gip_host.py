"""The host-side contract of include/gpuar_hip_gip.h, the header of the device calls that came after the closed tables of
gpuar_hip.h: its names are exactly those of hip.GIP_SIGNATURES, with the header's arities, the library
exports them, and gpuar_hip_move_bytes returns the documented code for each defect, in the documented order -- called with made-up
addresses and rejected (or a no-op) before the library touches a device, as tests/test_capi_codes_host.py does for the others."""
import pytest

from test_capi_codes_host import ALIGNMENT, ARGUMENT, MANY, OK, A, B, C, G, pointer_cases
from test_capi_symbols import declared_arity, declared_symbols

HEADER = "gpuar_hip_gip.h"


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from gpuar_amd import hip as H
    if not os.path.exists(H.LIB_PATH):
        g.build()
    return H.load()


def test_the_header_declares_exactly_the_second_binding_table(lib):
    from gpuar_amd import hip as H
    names = declared_symbols(HEADER)
    assert set(names) == set(H.GIP_SIGNATURES) and names, (names, list(H.GIP_SIGNATURES))
    assert not set(names) & set(H.EXPORTS)                  # a name is declared in one header and bound from one table
    assert not set(names) & set(declared_symbols())
    for name, arity in declared_arity(HEADER).items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity == len(H.GIP_SIGNATURES[name][1]), (name, arity, fn.argtypes)
    assert H.ABI_VERSION == 2 == lib.gpuar_hip_abi_version() and lib.gpuar_hip_version() == b"gpuar-hip 0.2 gfx950"


def test_a_library_without_the_new_call_is_refused_with_the_rebuild_message(monkeypatch):
    from gpuar_amd import hip as H
    monkeypatch.setattr(H, "_lib", None)
    monkeypatch.setattr(H, "GIP_SIGNATURES", {**H.GIP_SIGNATURES, "gpuar_hip_no_such_call": H.GIP_SIGNATURES["gpuar_hip_move_bytes"]})
    with pytest.raises(H.GpuarError, match=r"lacks \['gpuar_hip_no_such_call'\].*rebuild the library"):
        H.load()


def move_bytes_cases():
    good = (A, B, C, 3, G, None)                         # d_src_ptrs, d_dst_ptrs, d_bytes, n_regions, d_status, stream
    ptrs = {0: ("d_src_ptrs", 8, False), 1: ("d_dst_ptrs", 8, False), 2: ("d_bytes", 8, False), 4: ("d_status", 4, True)}
    return pointer_cases("gpuar_hip_move_bytes", good, ptrs, nothing=(3, (0, 1, 2, 4)), tail=[
        ("too many regions", {3: MANY}, ARGUMENT),
        ("nothing to do with every pointer misaligned", {0: A + 1, 1: B + 1, 2: C + 1, 3: 0, 4: G + 1}, OK),
        ("every array misaligned", {0: A + 4, 1: B + 4, 2: C + 4}, ALIGNMENT),
        ("a null d_bytes with a misaligned d_status", {2: None, 4: G + 2}, ARGUMENT),       # ARGUMENT before ALIGNMENT
    ])


CASES = move_bytes_cases()


def test_the_table_covers_every_call_of_the_header():
    from gpuar_amd import hip as H
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) and {c[1] for c in CASES} == set(H.GIP_SIGNATURES)
    # each array null, each array and d_status misaligned, each of those with another pointer null, nothing to do
    assert len(CASES) == 3 + 4 + 4 + 1 + 4


@pytest.mark.parametrize("what,name,args,want", CASES, ids=[c[0] for c in CASES])
def test_code(lib, what, name, args, want):
    assert getattr(lib, name)(*args) == want
