"""The mixed-filter kernels on the MI355X: gpuar_hip_split_mixed / merge_mixed, their batch forms and gpuar_hip_choose_modes_batch
against the host definitions of gpuar_amd/csrc/mixed.h (themselves checked in tests/test_mixed_host.py), the later grid-stride
passes on the build capped at 3 workgroups, and batch.compress(planes="mixed").  Every output has sentinel bytes in front of it
and behind it, and every status word is read."""
import numpy as np
import pytest

import grid_cap_build as G
import mixed_ref as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 256
BAD_BATCH = 0x4
FILL = 0x5A


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def B(H):
    from gpuar_amd import batch
    return batch


@pytest.fixture(scope="module")
def pairs():
    """(buffer, base) per length, made once"""
    return {n: M.pair(n, seed=40 + n % 733) for n in M.LENGTHS}


@pytest.fixture(scope="module")
def built(H):
    """the constructed buffer cut into three tensors at 16-byte offsets that are no supergroup's edge, with its bases, on the device"""
    x, b, _where = M.constructed()
    cuts = (0, 5 * M.SUPER + 4096 + 16, 12 * M.SUPER - 32, x.size)
    hosts = [(x[lo:hi].copy(), b[lo:hi].copy()) for lo, hi in zip(cuts, cuts[1:])]
    tensors = [torch.from_numpy(h).cuda() for h, _b in hosts]
    bases = [torch.from_numpy(hb).cuda() for _h, hb in hosts]
    return hosts, tensors, bases


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _i64(values):
    return torch.tensor(np.asarray(values, dtype=np.uint64).view(np.int64), dtype=torch.int64, device="cuda")


def _u8(data):
    return torch.from_numpy(np.frombuffer(bytes(data) or b"\0", dtype=np.uint8).copy()).cuda()


def _host(H, x, b, modes):
    return np.frombuffer(H.split_mixed_host(x.tobytes(), modes, b.tobytes()), dtype=np.uint8)


class Arena:
    """one device allocation that holds outputs of `sizes` bytes, each 16-byte aligned with GUARD sentinel bytes on both sides"""

    def __init__(self, sizes, fill=FILL):
        self.sizes, self.fill = list(sizes), fill
        self.offs, at = [], GUARD
        for n in self.sizes:
            self.offs.append(at)
            at += (n + 15) // 16 * 16 + GUARD
        self.d = torch.full((at,), fill, dtype=torch.uint8, device="cuda")
        assert self.d.data_ptr() % 16 == 0

    def view(self, i):
        return self.d[self.offs[i]:self.offs[i] + self.sizes[i]]

    def ptrs(self):
        return [self.d.data_ptr() + off if n else 0 for off, n in zip(self.offs, self.sizes)]

    def put(self, i, host):
        self.view(i).copy_(torch.from_numpy(np.array(host, dtype=np.uint8)).cuda())

    def check(self, wants, what):
        """output i holds wants[i] (None: untouched) and every byte outside the outputs is the sentinel"""
        got = self.d.cpu().numpy()
        mask = np.ones(got.size, dtype=bool)
        for i, (off, n) in enumerate(zip(self.offs, self.sizes)):
            mask[off:off + n] = False
            if wants[i] is None:
                assert (got[off:off + n] == self.fill).all(), (what, i, "a refused output was written")
            else:
                bad = np.flatnonzero(got[off:off + n] != wants[i])
                assert bad.size == 0, (what, i, int(bad[0]), bad.size)
        assert (got[mask] == self.fill).all(), (what, "a sentinel byte was written")


def _mode_sets(n):
    return [M.uniform(m, n) for m in M.MODES] + [M.cyclic(n), M.cyclic(n, 7), M.random_modes(n, 3 + n % 101)]


# ---- one buffer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [n for n in M.LENGTHS if n])
def test_single_buffer_split_and_merge_against_the_host(H, pairs, n):
    x, b = pairs[n]
    d_in, d_base = _u8(x), _u8(b)
    status = _status()
    for modes in _mode_sets(n):
        want = _host(H, x, b, modes)
        d_modes = _u8(modes)
        out = Arena([n])
        H.split_mixed(d_in, d_modes, d_base, d_out=out.view(0), d_status=status)
        out.check([want], (n, modes, "split"))
        back = Arena([n], 0x3C)
        H.merge_mixed(out.view(0), d_modes, d_base, d_out=back.view(0), d_status=status)
        back.check([x], (n, modes, "merge"))
        H.merge_mixed(out.view(0), d_modes, d_base, d_out=out.view(0), d_status=status)          # in place
        out.check([x], (n, modes, "merge in place"))
        H.split_mixed(out.view(0), d_modes, d_base, d_out=out.view(0), d_status=status)
        out.check([want], (n, modes, "split in place"))
    assert int(status.item()) == 0
    assert torch.equal(d_in, _u8(x)) and torch.equal(d_base, _u8(b)), "an input or a base was changed"


def test_uniform_modes_give_what_the_dedicated_kernels_give(H, pairs):
    for n in (65537, 3 * M.SUPER + 5 * M.PACKET + 7):
        x, b = pairs[n]
        d_in, d_base = _u8(x), _u8(b)
        for mode in M.MODES:
            w, kind = M.parts(mode)
            got = H.split_mixed(d_in, _u8(M.uniform(mode, n)), d_base)
            want = H.split_xor(d_in, d_base, w) if kind == 2 else H.split_delta(d_in, w) if kind == 1 else H.split_planes(d_in, w)
            assert torch.equal(got, want), (n, mode)
    assert H.status() == 0


def test_a_mode_without_its_base_and_an_invalid_mode_leave_their_supergroup_alone(H, pairs):
    n = 3 * M.SUPER + 5 * M.PACKET + 7
    x, b = pairs[n]
    d_in, d_base = _u8(x), _u8(b)
    for modes, bad, base in ((bytes([1, 13, 6, 3]), 1, d_base), (bytes([5, 2, 200, 0]), 2, d_base), (bytes([4, 7, 1, 12]), 3, d_base),
                             (bytes([1, 9, 6, 3]), 1, None), (bytes([1, 2, 6, 11]), 3, None)):
        good = bytes(0 if s == bad else m for s, m in enumerate(modes))
        want = _host(H, x, b, good).copy()
        want[bad * M.SUPER:(bad + 1) * M.SUPER] = FILL
        for fn in (H.split_mixed, H.merge_mixed):
            status, out = _status(), Arena([n])
            src = d_in if fn is H.split_mixed else _u8(_host(H, x, b, good))
            fn(src, _u8(modes), base, d_out=out.view(0), d_status=status)
            assert int(status.item()) == BAD_BATCH, (modes, base is None)
            if fn is H.split_mixed:
                out.check([want], (modes, "split"))
            else:
                back = x.copy()
                back[bad * M.SUPER:(bad + 1) * M.SUPER] = FILL
                out.check([back], (modes, "merge"))


# ---- a batch ----------------------------------------------------------------------------------------------------------

def _batch(H, hosts, modes, based=None):
    """the descriptors of a batch of (buffer, base) host pairs with their modes: a dict of device tensors and host lists"""
    sizes = [x.size for x, _b in hosts]
    first_packet, n_packets = H.batch_packet_count(sizes)
    first_mode, n_modes = H.batch_mode_count(sizes)
    d_in = [_u8(x) for x, _b in hosts]
    d_base = [_u8(b) for _x, b in hosts]
    based = [True] * len(hosts) if based is None else based
    return dict(sizes=sizes, n=len(hosts), n_packets=n_packets, n_modes=n_modes, d_in=d_in, d_base=d_base,
                in_ptrs=_i64([t.data_ptr() if n else 0 for t, n in zip(d_in, sizes)]), bytes=_i64(sizes), fp=_i64(first_packet), fm=_i64(first_mode),
                modes=_u8(b"".join(modes)), base_ptrs=_i64([t.data_ptr() if n and on else 0 for t, n, on in zip(d_base, sizes, based)]))


def _call(H, fn, d, in_ptrs, out_ptrs, status):
    fn(in_ptrs, d["bytes"], d["fp"], d["fm"], d["modes"], d["base_ptrs"], d["n"], d["n_packets"], out_ptrs, d_status=status)


def test_batch_split_and_merge_against_the_host(H, pairs):
    """an empty buffer, a one-byte buffer, buffers that end on and just off a supergroup's edge, and the two long ones"""
    lengths = (65536, 0, 1, 65537, 3 * M.SUPER + 5 * M.PACKET + 7, 65535, 0, 2 * M.SUPER + 8 * M.PACKET - 1, 8192)
    hosts = [pairs[n] for n in lengths]
    for k, pattern in enumerate((lambda n, i: M.cyclic(n, i), lambda n, i: M.random_modes(n, 17 + i), lambda n, i: M.uniform((5 * i + 3) % 12, n))):
        modes = [pattern(n, i) for i, n in enumerate(lengths)]
        d = _batch(H, hosts, modes)
        wants = [_host(H, x, b, m) for (x, b), m in zip(hosts, modes)]
        status, out = _status(), Arena(lengths)
        _call(H, H.split_mixed_batch, d, d["in_ptrs"], _i64(out.ptrs()), status)
        out.check(wants, (k, "split"))
        back = Arena(lengths, 0x3C)
        _call(H, H.merge_mixed_batch, d, _i64(out.ptrs()), _i64(back.ptrs()), status)
        back.check([x for x, _b in hosts], (k, "merge"))
        _call(H, H.merge_mixed_batch, d, _i64(out.ptrs()), _i64(out.ptrs()), status)              # in place
        out.check([x for x, _b in hosts], (k, "merge in place"))
        _call(H, H.split_mixed_batch, d, _i64(out.ptrs()), _i64(out.ptrs()), status)
        out.check(wants, (k, "split in place"))
        assert int(status.item()) == 0
        for t, (x, _b) in zip(d["d_in"], hosts):
            assert x.size == 0 or torch.equal(t, _u8(x))


@pytest.mark.parametrize("defect", ("invalid_mode", "base_mode_without_a_base"))
def test_batch_a_bad_supergroup_is_flagged_and_left_alone(H, pairs, defect):
    lengths = (65537, 3 * M.SUPER + 5 * M.PACKET + 7, 2 * M.SUPER + 8 * M.PACKET - 1)
    hosts = [pairs[n] for n in lengths]
    modes = [bytes([9, 4]), bytes([6, 14 if defect == "invalid_mode" else 10, 11 if defect == "invalid_mode" else 3, 1]), bytes([2, 8, 7])]
    based = [True, defect == "invalid_mode", True]
    good = [modes[0], bytes([6, 0, modes[1][2], 1]), modes[2]]
    wants = [_host(H, x, b, m).copy() for (x, b), m in zip(hosts, good)]
    wants[1][M.SUPER:2 * M.SUPER] = FILL
    d = _batch(H, hosts, modes, based)
    status, out = _status(), Arena(lengths)
    _call(H, H.split_mixed_batch, d, d["in_ptrs"], _i64(out.ptrs()), status)
    assert int(status.item()) == BAD_BATCH
    out.check(wants, (defect, "split"))
    # the merge: the same supergroup stays as it is, the others come back
    src = Arena(lengths)
    for i, ((x, b), m) in enumerate(zip(hosts, good)):
        src.put(i, _host(H, x, b, m))
    backs = [x.copy() for x, _b in hosts]
    backs[1][M.SUPER:2 * M.SUPER] = FILL
    status, out = _status(), Arena(lengths)
    _call(H, H.merge_mixed_batch, d, _i64(src.ptrs()), _i64(out.ptrs()), status)
    assert int(status.item()) == BAD_BATCH
    out.check(backs, (defect, "merge"))


def test_batch_a_misaligned_pointer_or_a_buffer_that_does_not_own_its_packets_is_left_alone(H, pairs):
    lengths = (65537, 2 * M.SUPER + 8 * M.PACKET - 1, 8192)
    hosts = [pairs[n] for n in lengths]
    modes = [M.cyclic(n, 3 + i) for i, n in enumerate(lengths)]
    wants = [_host(H, x, b, m) for (x, b), m in zip(hosts, modes)]
    for defect in ("input", "output", "base", "packets"):
        d = _batch(H, hosts, modes)
        out = Arena(lengths)
        in_ptrs, out_ptrs, expect = d["in_ptrs"].clone(), _i64(out.ptrs()), list(wants)
        if defect == "input":
            in_ptrs[1] += 4
        elif defect == "output":
            out_ptrs[1] += 8
        elif defect == "base":
            d["base_ptrs"][1] += 4
        else:
            d["bytes"][1] -= M.PACKET                          # the buffer now owns one packet more than its bytes make
        expect[1] = None
        status = _status()
        _call(H, H.split_mixed_batch, d, in_ptrs, out_ptrs, status)
        assert int(status.item()) == BAD_BATCH, defect
        out.check(expect, defect)


# ---- the choice -------------------------------------------------------------------------------------------------------

def test_choose_modes_batch_equals_the_host(H, B, built):
    hosts, tensors, bases = built
    for delta, base in ((True, bases), (False, None), (True, None), (False, [bases[0], None, bases[2]])):
        got = B.survey_mixed(tensors, delta=delta, base=base)
        for i, (x, b) in enumerate(hosts):
            with_base = base is not None and base[i] is not None
            plain, drows, xrows = M.surveys(H, x, b if with_base else None, delta)
            modes, totals = H.choose_modes_host(plain, drows, xrows, x.size)
            assert got[i] == (modes, sum(totals)), (delta, with_base, i)
    assert B.survey_mixed([torch.empty(0, dtype=torch.uint8, device="cuda")]) == [(b"", 0)]


def test_choose_modes_single_buffer_and_totals(H, built):
    hosts, tensors, bases = built
    (x, b), t, tb = hosts[1], tensors[1], bases[1]
    status = _status()
    d_plain, d_delta = H.survey_planes(t), H.survey_delta(t)
    d_xored, _scan = H.survey_xor(t, tb, d_scan=False)
    d_modes, d_totals = H.choose_modes(d_plain, d_delta, d_xored, x.size, d_status=status)
    modes, totals = H.choose_modes_host(*M.surveys(H, x, b), x.size)
    assert bytes(d_modes.cpu().tolist()) == modes and d_totals.cpu().tolist() == totals and int(status.item()) == 0


# ---- the later grid-stride passes -------------------------------------------------------------------------------------

WALK_MODES = bytes([7, 4, 11, 5, 2, 9])       # delta 8, delta 1, XOR 8, delta 2, planes 4, XOR 2: one supergroup each


def _walks(modes, cap=G.CAP):
    """per workgroup the (kind, width) of the groups it moves, in its order: packet p is workgroup p % cap's"""
    walks = [[] for _ in range(cap)]
    for s, m in enumerate(modes):
        w, kind = M.parts(m)
        for p in range(8 * s, 8 * s + 8, w):
            walks[p % cap].append(("planes", "delta", "xor")[kind] + str(w))
    return walks


def test_the_walks_of_the_capped_grid_cross_every_change_of_kind():
    """With 3 workgroups a group of width 8 is workgroup (2 s) % 3's, so no single workgroup leads the groups of supergroups 0 and
    2 both; between them the three walks go through every change the kernel's comment argues: delta to delta at another width
    (the alternating slots), delta to XOR and back (the slots beside the base's LDS), delta to planes, planes to XOR and XOR to XOR
    (the trailing barrier)."""
    walks = _walks(WALK_MODES)
    assert walks[0] == ["delta8", "delta1", "delta1", "delta1", "delta2", "delta2", "planes4", "xor2"]
    assert walks[1] == ["delta1", "delta1", "xor8", "delta2", "xor2", "xor2"]
    assert walks[2] == ["delta1", "delta1", "delta1", "delta2", "planes4", "xor2"]
    steps = {(a, b) for walk in walks for a, b in zip(walk, walk[1:])}
    assert {("delta8", "delta1"), ("delta1", "delta2"), ("delta1", "xor8"), ("xor8", "delta2"), ("delta2", "planes4"), ("planes4", "xor2"),
            ("delta2", "xor2"), ("xor2", "xor2")} <= steps


def test_three_workgroups_walk_from_kind_to_kind(H):
    capped_lib = G.load()
    for name, (restype, argtypes) in H.MIXED_SIGNATURES.items():
        getattr(capped_lib, name).restype, getattr(capped_lib, name).argtypes = restype, argtypes
    n = 6 * M.SUPER
    x, b = M.pair(n, seed=99)
    want = _host(H, x, b, WALK_MODES)
    d_in, d_base, d_modes = _u8(x), _u8(b), _u8(WALK_MODES)
    with G.capped():
        assert H.load() is capped_lib
        status, out = _status(), Arena([n])
        H.split_mixed(d_in, d_modes, d_base, d_out=out.view(0), d_status=status)
        out.check([want], "split")
        H.merge_mixed(out.view(0), d_modes, d_base, d_out=out.view(0), d_status=status)           # in place
        out.check([x], "merge in place")
        H.split_mixed(out.view(0), d_modes, d_base, d_out=out.view(0), d_status=status)
        out.check([want], "split in place")
        # the same as the one buffer of a batch, and a second buffer behind it whose walk begins on another workgroup
        hosts = [(x, b), M.pair(M.SUPER + 5 * M.PACKET + 9, seed=98)]
        modes = [WALK_MODES, bytes([6, 3])]
        d = _batch(H, hosts, modes)
        wants = [want, _host(H, hosts[1][0], hosts[1][1], modes[1])]
        both = Arena([h.size for h, _b in hosts])
        _call(H, H.split_mixed_batch, d, d["in_ptrs"], _i64(both.ptrs()), status)
        both.check(wants, "batch split")
        _call(H, H.merge_mixed_batch, d, _i64(both.ptrs()), _i64(both.ptrs()), status)
        both.check([h for h, _b in hosts], "batch merge in place")
        assert int(status.item()) == 0
    assert H.load() is not capped_lib


# ---- batch.compress ---------------------------------------------------------------------------------------------------

def test_compress_mixed_round_trips_and_keeps_its_bound(H, B, built):
    hosts, tensors, bases = built
    n_packets = sum(H.packet_count(x.size) for x, _b in hosts)
    chosen = B.survey_mixed(tensors, delta=True, base=bases)
    c = B.compress(tensors, planes="mixed", delta="mixed", base=bases, checksum=True)
    assert c.modes == [m for m, _t in chosen] and c.planes is None and c.delta is None
    assert c.based == [any(m >> 2 == 2 for m in modes) for modes in c.modes] and c.based[0]
    outs = B.decompress(c, base=bases)
    for out, (x, _b) in zip(outs, hosts):
        assert np.array_equal(out.cpu().numpy(), x)
    # against the best single choice per tensor, and against the estimate
    whole = min(B.compress(tensors, planes="survey", base=bases, base_auto="survey").nbytes, B.compress(tensors, planes="survey", delta="survey").nbytes)
    est = B.estimate(tensors, planes="mixed", delta="mixed", base=bases)
    print(f"mixed {c.nbytes} bytes, best single choice per tensor {whole}, estimate {sum(est)}, predicted {sum(t for _m, t in chosen)}, {n_packets} packets")
    assert c.nbytes <= whole + 2 * n_packets + n_packets
    assert abs(sum(est) - c.nbytes) <= n_packets
    assert abs(sum(t for _m, t in chosen) - c.nbytes) <= n_packets
    with pytest.raises(B.GpuarError, match="version 7"):
        c.gip(0)
    with pytest.raises(B.GpuarError):
        B.decompress(c)                                   # the bases are needed again
    # a wrong base is a checksum mismatch
    with pytest.raises(B.GpuarError, match="checksum"):
        B.decompress(c, base=[bases[0] ^ 1, bases[1], bases[2]])


def test_compress_mixed_with_raw_and_sparse_packets_and_without_a_base(H, B, built):
    hosts, tensors, bases = built
    c = B.compress(tensors, planes="mixed", delta="mixed", base=bases, checksum=True, stored="auto", sparse="auto")
    kinds = c.stored.cpu().numpy()
    assert (kinds == H.KIND_RAW).any() and (kinds == H.KIND_SPARSE).any()          # the uniform bytes; the unchanged bf16 packets
    for out, (x, _b) in zip(B.decompress(c, base=bases), hosts):
        assert np.array_equal(out.cpu().numpy(), x)
    plain = B.compress(tensors, planes="mixed")
    assert plain.based is None and all(m < 4 for modes in plain.modes for m in modes)
    assert plain.modes == [m for m, _t in B.survey_mixed(tensors)]
    for out, (x, _b) in zip(B.decompress(plain), hosts):
        assert np.array_equal(out.cpu().numpy(), x)
    empty = B.compress([torch.empty(0, dtype=torch.uint8, device="cuda"), tensors[2]], planes="mixed", delta="mixed")
    assert empty.modes[0] == b"" and np.array_equal(B.decompress(empty)[1].cpu().numpy(), hosts[2][0])


def test_what_compress_refuses_beside_mixed(B, built):
    _hosts, tensors, bases = built
    launches = torch.cuda.memory_allocated()
    for kwargs in (dict(delta="mixed"), dict(planes="survey", delta="mixed"), dict(planes="mixed", delta=True), dict(planes="mixed", delta="survey"),
                   dict(planes="mixed", delta="auto"), dict(planes="mixed", base=bases, base_auto=True),
                   dict(planes="mixed", base=bases, base_auto="survey")):
        with pytest.raises(B.GpuarError):
            B.compress(tensors, **kwargs)
        with pytest.raises(B.GpuarError):
            B.estimate(tensors, **kwargs)
    assert torch.cuda.memory_allocated() == launches      # nothing was allocated: the refusals come before the device step
