"""The host-side contract of the device entry points of include/gpuar_hip.h: which code a call returns for each documented
defect, what it does when there is nothing to do, and which defect wins when a call has two.  Every case is called through
hip.load() with made-up addresses and is rejected (or is a no-op) before the library touches a device: nothing is dereferenced,
nothing is launched, and the answer is the same with and without a GPU.  A well-formed call has no place here (without a device
it cannot succeed): tests/test_gpu_capi_codes.py makes those.

The three filters' own checks are pinned in test_planes_host.py / test_delta_host.py / test_xor_host.py and their GPU files; here
only the order inside their batch forms."""
import pytest

OK, ALIGNMENT, ARGUMENT = 0, -1, -2
A, B, C, D, E, F, G = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000      # "16-byte aligned device pointers"
MANY = 1 << 32                          # a packet, buffer or region count above 0xFFFFFFFF
MANY_BYTES = MANY * 8192                # the bytes of that many packets


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from gpuar_amd import hip as H
    if not os.path.exists(H.LIB_PATH):
        g.build()
    return H.load()


def pointer_cases(name, good, pointers, tail=(), nothing=None):
    """The cases every call has.  `good`: a well-formed argument list; `pointers`: {index: (what, alignment, nullable)} for its
    pointer arguments.  Each pointer null (ARGUMENT unless nullable), each pointer misaligned by half its alignment (ALIGNMENT),
    and -- the precedence -- every misaligned pointer together with another, null one: ARGUMENT wins."""
    out = []
    required = [i for i, (_w, _a, nullable) in pointers.items() if not nullable]
    for i, (what, align, nullable) in pointers.items():
        if not nullable:
            out.append((f"{name}: null {what}", name, _with(good, {i: None}), ARGUMENT))
        if align == 1:                                   # a pointer of any alignment
            continue
        out.append((f"{name}: {what} not {align}-byte aligned", name, _with(good, {i: good[i] + align // 2}), ALIGNMENT))
        other = next(j for j in required if j != i)
        out.append((f"{name}: {what} misaligned and {pointers[other][0]} null", name,
                    _with(good, {i: good[i] + align // 2, other: None}), ARGUMENT))
    if nothing is not None:
        index, nulls = nothing
        out.append((f"{name}: nothing to do", name, _with(good, {index: 0, **{i: None for i in nulls}}), OK))
    return out + [(f"{name}: {what}", name, _with(good, changes), code) for what, changes, code in tail]


def _with(args, changes):
    args = list(args)
    for i, v in changes.items():
        args[i] = v
    return tuple(args)


def all_cases():
    cases = []

    # ---- encode / decode of one buffer ----------------------------------------------------------------------------------
    good = (A, 8192, B, G, None, 0)                      # d_in, n_bytes, d_slots, d_status, stream, mode
    ptrs = {0: ("d_in", 16, False), 2: ("d_slots", 16, False), 3: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_encode_mode", good, ptrs, nothing=(1, (0, 2, 3)), tail=[
        ("unknown mode", {5: 7}, ARGUMENT),
        ("negative mode", {5: -1}, ARGUMENT),
        ("unknown mode with nothing to do", {1: 0, 5: 7}, ARGUMENT),                       # the mode comes before everything
        ("unknown mode with a misaligned d_in", {0: A + 8, 5: 7}, ARGUMENT),
        # this count is checked behind the status word: with a word of the caller's own the library still asks no device for one
        ("too many packets", {1: MANY_BYTES}, ARGUMENT),
    ])
    cases += pointer_cases("gpuar_hip_encode", good[:5], ptrs, nothing=(1, (0, 2, 3)))
    good = (A, 5, B, G, None)                            # d_slots, n_packets, d_out, d_status, stream
    ptrs = {0: ("d_slots", 16, False), 2: ("d_out", 16, False), 3: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_decode", good, ptrs, nothing=(1, (0, 2, 3)), tail=[("too many packets", {1: MANY}, ARGUMENT)])
    good = (A, 5, B, C, None)                            # d_slots, n_packets, d_stream, d_offsets, stream
    ptrs = {0: ("d_slots", 16, False), 2: ("d_stream", 8, False), 3: ("d_offsets", 8, False)}
    cases += pointer_cases("gpuar_hip_compact", good, ptrs, tail=[
        ("no packets and a null d_offsets", {1: 0, 3: None}, ARGUMENT),
        ("more packets than one gather launch", {1: 1 << 24}, ARGUMENT),
    ])
    good = (A, B, 5, C, G, None)                         # d_stream, d_offsets, n_packets, d_out, d_status, stream
    ptrs = {0: ("d_stream", 4, False), 1: ("d_offsets", 8, False), 3: ("d_out", 16, False), 4: ("d_status", 4, True)}
    del ptrs[1]                                          # decode_stream makes no alignment test of d_offsets: only its null test
    cases += pointer_cases("gpuar_hip_decode_stream", good, ptrs, nothing=(2, (0, 1, 3, 4)), tail=[
        ("null d_offsets", {1: None}, ARGUMENT),
        ("too many packets", {2: MANY}, ARGUMENT),
    ])

    # ---- the batch coders -----------------------------------------------------------------------------------------------
    counts = lambda nb, npk: [("too many buffers", {nb: MANY}, ARGUMENT), ("too many packets", {npk: MANY}, ARGUMENT)]
    good = (A, B, C, 2, 5, D, G, None, 0)                # d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, d_slots, d_status, stream, mode
    ptrs = {0: ("d_in_ptrs", 8, False), 1: ("d_in_bytes", 8, False), 2: ("d_first_packet", 8, False), 5: ("d_slots", 16, False),
            6: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_encode_batch", good, ptrs, nothing=(4, (0, 1, 2, 5, 6)), tail=counts(3, 4) + [
        ("unknown mode", {8: 7}, ARGUMENT),
        ("GPUAR_MODE_TABLE", {8: 3}, ARGUMENT),
        ("GPUAR_MODE_TABLE with nothing to do", {4: 0, 8: 3}, ARGUMENT),
        ("unknown mode with a misaligned d_slots", {5: D + 8, 8: 7}, ARGUMENT),
    ])
    good = (A, B, 2, 5, C, D, G, None)                   # d_slots, d_first_packet, n_buffers, n_packets, d_out_ptrs, d_out_bytes, d_status, stream
    ptrs = {0: ("d_slots", 16, False), 1: ("d_first_packet", 8, False), 4: ("d_out_ptrs", 8, False), 5: ("d_out_bytes", 8, False),
            6: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_decode_batch", good, ptrs, nothing=(3, (0, 1, 4, 5, 6)), tail=counts(2, 3))
    # d_stream, d_offsets, d_first_packet, n_buffers, n_packets, d_out_ptrs, d_out_bytes, d_status, stream
    good = (A, B, C, 2, 5, D, E, G, None)
    ptrs = {0: ("d_stream", 4, False), 2: ("d_first_packet", 8, False), 5: ("d_out_ptrs", 8, False), 6: ("d_out_bytes", 8, False),
            7: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_decode_stream_batch", good, ptrs, nothing=(4, (0, 1, 2, 5, 6, 7)), tail=counts(3, 4) + [
        ("null d_offsets", {1: None}, ARGUMENT),
        ("d_offsets not 8-byte aligned", {1: B + 4}, ALIGNMENT),
        ("d_offsets misaligned and d_stream null", {0: None, 1: B + 4}, ALIGNMENT),        # d_offsets is looked at before the rest
    ])

    # ---- per-packet calls with one 32-bit array: CRC, estimate, sparse scan ----------------------------------------------
    for name, word in (("gpuar_hip_crc32", "d_crc"), ("gpuar_hip_estimate", "d_est"), ("gpuar_hip_sparse_scan", "d_scan")):
        good = (A, 8192, B, None)                        # d_in, n_bytes, the array, stream
        ptrs = {0: ("d_in", 16, False), 2: (word, 4, False)}
        cases += pointer_cases(name, good, ptrs, nothing=(1, (0, 2)), tail=[("too many packets", {1: MANY_BYTES}, ARGUMENT)])
        good = (A, B, C, 2, 5, D, G, None)               # d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, the array, d_status, stream
        ptrs = {0: ("d_in_ptrs", 8, False), 1: ("d_in_bytes", 8, False), 2: ("d_first_packet", 8, False), 5: (word, 4, False),
                6: ("d_status", 4, True)}
        cases += pointer_cases(name + "_batch", good, ptrs, nothing=(4, (0, 1, 2, 5, 6)), tail=counts(3, 4))
    good = (A, 8192, B, C, G, None)                      # d_out, n_bytes, d_crc, d_first_bad, d_status, stream
    ptrs = {0: ("d_out", 16, False), 2: ("d_crc", 4, False), 3: ("d_first_bad", 8, True), 4: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_verify_crc32", good, ptrs, nothing=(1, (0, 2, 3, 4)), tail=[("too many packets", {1: MANY_BYTES}, ARGUMENT)])
    good = (A, B, C, 2, 5, D, E, G, None)                # d_out_ptrs, d_out_bytes, d_first_packet, n_buffers, n_packets, d_crc, d_first_bad, d_status, stream
    ptrs = {0: ("d_out_ptrs", 8, False), 1: ("d_out_bytes", 8, False), 2: ("d_first_packet", 8, False), 5: ("d_crc", 4, False),
            6: ("d_first_bad", 8, True), 7: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_verify_crc32_batch", good, ptrs, nothing=(4, (0, 1, 2, 5, 6, 7)), tail=counts(3, 4))

    # ---- the surveys: est_stride and widths_mask come first ---------------------------------------------------------------
    good = (A, 3 * 8192, B, 3, None)                     # d_in, n_bytes, d_est, est_stride, stream
    ptrs = {0: ("d_in", 16, False), 2: ("d_est", 4, False)}
    cases += pointer_cases("gpuar_hip_survey_planes", good, ptrs, nothing=(1, (0, 2)), tail=[
        ("est_stride below the packet count", {3: 2}, ARGUMENT),
        ("too many packets", {1: MANY_BYTES, 3: MANY}, ARGUMENT),
        ("a short est_stride with a null d_in", {0: None, 3: 2}, ARGUMENT),
        ("a short est_stride with a misaligned d_est", {2: B + 2, 3: 2}, ARGUMENT),       # the stride comes before the pointers
        ("a short est_stride with nothing to do", {1: 0, 3: 0}, OK),
    ])
    good = (A, B, C, 2, 5, D, 5, G, None)                # d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, d_est, est_stride, d_status, stream
    ptrs = {0: ("d_in_ptrs", 8, False), 1: ("d_in_bytes", 8, False), 2: ("d_first_packet", 8, False), 5: ("d_est", 4, False),
            7: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_survey_planes_batch", good, ptrs, nothing=(4, (0, 1, 2, 5, 7)), tail=[
        ("too many buffers", {3: MANY}, ARGUMENT),
        ("too many packets", {4: MANY, 6: MANY}, ARGUMENT),
        ("est_stride below the packet count", {6: 4}, ARGUMENT),
        ("a short est_stride with a null d_est", {5: None, 6: 4}, ARGUMENT),
        ("a short est_stride with a misaligned d_in_ptrs", {0: A + 4, 6: 4}, ARGUMENT),
    ])
    good = (A, 3 * 8192, 15, B, 3, None)                 # d_in, n_bytes, widths_mask, d_est, est_stride, stream
    ptrs = {0: ("d_in", 16, False), 3: ("d_est", 4, False)}
    cases += pointer_cases("gpuar_hip_survey_delta", good, ptrs, nothing=(1, (0, 3)), tail=[
        ("est_stride below the packet count", {4: 2}, ARGUMENT),
        ("widths_mask 0", {2: 0}, ARGUMENT),
        ("widths_mask with a bit above 8", {2: 16}, ARGUMENT),
        ("widths_mask with a wanted bit and one above 8", {2: 17}, ARGUMENT),
        ("too many packets", {1: MANY_BYTES, 4: MANY}, ARGUMENT),
        ("widths_mask 0 with a null d_est", {2: 0, 3: None}, ARGUMENT),
        ("widths_mask 0 with a misaligned d_in", {0: A + 8, 2: 0}, ARGUMENT),             # the mask comes before the pointers
        ("a short est_stride with a misaligned d_est", {3: B + 2, 4: 2}, ARGUMENT),
        ("widths_mask 0 with nothing to do", {1: 0, 2: 0}, OK),
    ])
    # d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, widths_mask, d_est, est_stride, d_status, stream
    good = (A, B, C, 2, 5, 1, D, 5, G, None)
    ptrs = {0: ("d_in_ptrs", 8, False), 1: ("d_in_bytes", 8, False), 2: ("d_first_packet", 8, False), 6: ("d_est", 4, False),
            8: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_survey_delta_batch", good, ptrs, nothing=(4, (0, 1, 2, 6, 8)), tail=[
        ("too many buffers", {3: MANY}, ARGUMENT),
        ("too many packets", {4: MANY, 7: MANY}, ARGUMENT),
        ("est_stride below the packet count", {7: 4}, ARGUMENT),
        ("widths_mask 0", {5: 0}, ARGUMENT),
        ("widths_mask with a bit above 8", {5: 16}, ARGUMENT),
        ("widths_mask 0 with a null d_first_packet", {2: None, 5: 0}, ARGUMENT),
        ("widths_mask 0 with a misaligned d_status", {5: 0, 8: G + 2}, ARGUMENT),
        ("widths_mask 0 with nothing to do", {4: 0, 5: 0}, OK),
    ])

    # ---- region calls -----------------------------------------------------------------------------------------------------
    good = (A, B, C, 3, G, None)                         # d_src_ptrs, d_dst_ptrs, d_bytes, n_regions, d_status, stream
    ptrs = {0: ("d_src_ptrs", 8, False), 1: ("d_dst_ptrs", 8, False), 2: ("d_bytes", 8, False), 4: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_move_packets", good, ptrs, nothing=(3, (0, 1, 2, 4)), tail=[("too many regions", {3: MANY}, ARGUMENT)])
    good = (A, B, C, D, 3, G, None)                      # d_src_ptrs, d_bytes, d_scan, d_dst_ptrs, n_regions, d_status, stream
    ptrs = {0: ("d_src_ptrs", 8, False), 1: ("d_bytes", 8, False), 2: ("d_scan", 4, False), 3: ("d_dst_ptrs", 8, False), 5: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_sparse_pack", good, ptrs, nothing=(4, (0, 1, 2, 3, 5)), tail=[("too many regions", {4: MANY}, ARGUMENT)])
    good = (A, B, C, D, 3, G, None)                      # d_rec_ptrs, d_rec_bytes, d_dst_ptrs, d_bytes, n_regions, d_status, stream
    ptrs = {0: ("d_rec_ptrs", 8, False), 1: ("d_rec_bytes", 8, False), 2: ("d_dst_ptrs", 8, False), 3: ("d_bytes", 8, False), 5: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_sparse_unpack", good, ptrs, nothing=(4, (0, 1, 2, 3, 5)), tail=[("too many regions", {4: MANY}, ARGUMENT)])

    # ---- raw and sparse packets in a stream -------------------------------------------------------------------------------
    # kinds_store: what it checks before it has the status word (d_slots, d_kind and d_scan come behind it: the GPU file)
    good = (A, 8192, B, C, 1, D, E, G, None)             # d_in, n_bytes, d_est, d_scan, stored_on, d_slots, d_kind, d_status, stream
    ptrs = {0: ("d_in", 16, False), 2: ("d_est", 4, False), 7: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_kinds_store", good, ptrs, nothing=(1, (0, 2, 3, 5, 6, 7)), tail=[("too many packets", {1: MANY_BYTES}, ARGUMENT)])
    good = (A, B, C, 2, D, 8192 + 5, G, None)            # d_stream, d_offsets, d_kind, n_packets, d_out, n_bytes, d_status, stream
    ptrs = {0: ("d_stream", 1, False), 1: ("d_offsets", 8, False), 2: ("d_kind", 1, False), 4: ("d_out", 16, False), 6: ("d_status", 4, True)}
    cases += pointer_cases("gpuar_hip_kinds_expand", good, ptrs, nothing=(3, (0, 1, 2, 4, 6)), tail=[
        ("too many packets", {3: MANY, 5: MANY_BYTES}, ARGUMENT),
        ("n_bytes of one packet fewer", {5: 8192}, ARGUMENT),
        ("n_bytes of one packet more", {5: 2 * 8192 + 1}, ARGUMENT),
        ("n_bytes 0", {5: 0}, ARGUMENT),
        ("the wrong n_bytes with a misaligned d_out", {4: D + 8, 5: 8192}, ARGUMENT),
    ])

    # ---- measurement support ----------------------------------------------------------------------------------------------
    good = (A, B, 4096, None)                            # d_src, d_dst, n_bytes, stream
    ptrs = {0: ("d_src", 16, False), 1: ("d_dst", 16, False)}
    cases += pointer_cases("gpuar_hip_copy", good, ptrs, nothing=(2, (0, 1)), tail=[
        ("n_bytes no multiple of 16", {2: 4096 + 8}, ARGUMENT),
        ("n_bytes no multiple of 16 with a misaligned d_src", {0: A + 8, 2: 4100}, ARGUMENT),
        ("64 GiB", {2: 1 << 36}, ARGUMENT),
    ])
    good = (0, 1, 0, 4096, A, None)                      # kind, seed, offset, n, d_out, stream
    cases += [(f"gpuar_hip_generate: {what}", "gpuar_hip_generate", _with(good, changes), code) for what, changes, code in [
        ("null d_out", {4: None}, ARGUMENT),
        ("d_out not 8-byte aligned", {4: A + 4}, ALIGNMENT),
        ("kind -1", {0: -1}, ARGUMENT),
        ("kind 3", {0: 3}, ARGUMENT),
        ("offset no multiple of 8", {2: 4}, ARGUMENT),
        ("a bad offset with a misaligned d_out", {2: 4, 4: A + 4}, ARGUMENT),
        ("nothing to do", {3: 0, 4: None}, OK),
        ("nothing to do, of a bad kind", {0: 9, 3: 0}, OK),
    ]]
    cases += [("gpuar_hip_status: null flags", "gpuar_hip_status", (None,), ARGUMENT),
              ("gpuar_hip_clock_samples: null ticks", "gpuar_hip_clock_samples", (0, None, 0), ARGUMENT)]

    # ---- the batch filters: their own descriptors' alignment is looked at before the shared descriptors' null test -------
    for kind, extra in (("planes", ()), ("delta", (E,)), ("xor", (E,))):
        for way in ("split", "merge"):
            name = f"gpuar_hip_{way}_{kind}_batch"
            # d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, [d_filter | d_base_ptrs,] n_buffers, n_packets, d_out_ptrs, d_status, stream
            cases.append((f"{name}: d_elem_bytes misaligned and d_in_ptrs null", name, (None, B, C, D + 4, *extra, 2, 5, F, G, None), ALIGNMENT))
            cases.append((f"{name}: d_elem_bytes null and d_in_ptrs misaligned", name, (A + 4, B, C, None, *extra, 2, 5, F, G, None), ARGUMENT))
    return cases


CASES = all_cases()


def test_the_table_names_every_case_once_and_every_device_entry_point():
    from gpuar_amd import hip as H
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))
    pure = {"gpuar_hip_packet_count", "gpuar_hip_batch_packet_count", "gpuar_hip_last_error", "gpuar_hip_error_string", "gpuar_hip_version",
            "gpuar_hip_abi_version", "gpuar_hip_choose_planes", "gpuar_hip_choose_filter", "gpuar_hip_sparse_len", "gpuar_hip_sparse_rule",
            "gpuar_hip_delta_block_host", "initConstantRange", "garCompressExecutor", "garDecompressExecutor"}
    filters = {f"gpuar_hip_{way}_{kind}" for way in ("split", "merge") for kind in ("planes", "delta", "xor")}       # pinned in their own files
    device = {n for n in H.EXPORTS if not n.endswith("_host")} - pure - filters
    assert device == {c[1] for c in CASES}


@pytest.mark.parametrize("what,name,args,want", CASES, ids=[c[0] for c in CASES])
def test_code(lib, what, name, args, want):
    assert getattr(lib, name)(*args) == want


def test_the_executors_record_the_code_of_their_call(lib, capfd):
    """garCompressExecutor / garDecompressExecutor return nothing: the code of the encode / decode call inside them is what
    gpuar_hip_last_error gives, once."""
    lib.gpuar_hip_last_error()
    for fn, word in ((lib.garCompressExecutor, b"garCompressExecutor"), (lib.garDecompressExecutor, b"garDecompressExecutor")):
        for args, want in (((None, 8192, A, 0), ARGUMENT), ((A, 8192, None, 0), ARGUMENT), ((A + 8, 8192, B, 0), ALIGNMENT),
                           ((A, 8192, B + 8, 0), ALIGNMENT), ((None, 8192, B + 8, 0), ARGUMENT), ((None, 0, None, 0), OK)):
            fn(*args)
            assert lib.gpuar_hip_last_error() == want, (word, args)
            assert lib.gpuar_hip_last_error() == OK
    assert "garCompressExecutor: invalid argument" in capfd.readouterr().err
