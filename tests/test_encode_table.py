"""The table walk of the throughput encoder (encode_kernel_t16, GPUAR_MODE_TABLE): the path operands of
tree depths 4-7 come from a 256-byte table instead of a shift and a mask per level.  Same integers, so every check here is
byte for byte:

  * CPU: the table itself against the shift-and-mask form for every symbol; the host build of the table-walk modelers
    (tests/encode_table_emulation.cpp) against the modelers the host CLI runs today, the oracle and the golden streams -- in
    the three forms a lane of the kernel can be in: whole phases, the ragged form (a group that is not full, a packet's
    tail) and the hand-off between them inside a packet, at every packet length, every shortest length of the wavefront
    and on the adversarial packet families of tests/test_gpu_parity.py (tests/packet_families.py);
  * code object: the new kernel's resources and per-phase instruction counts, read out of the shipped library the way
    tests/test_codeobj_contract.py reads the pinned kernels';
  * GPU (-m gpu): slots through GPUAR_MODE_TABLE against GPUAR_MODE_THROUGHPUT and the oracle at the shapes where a table
    index, a carry out of the low four bits or a ragged phase can go wrong.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import length_sweep as LS
import packet_families as PF
from test_codeobj_contract import VEC, code_object, phase_segments          # noqa: F401  (code_object: the fixture)
from test_oracle_golden import REFV, case_input, md5

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
u8p = C.POINTER(C.c_uint8)
PACKET, SLOT = 8192, 8704
MODE_TABLE = 3                  # GPUAR_MODE_TABLE


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.fixture(scope="module")
def emu():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libencode_table_emulation.so")
    srcs = [os.path.join(HERE, "encode_table_emulation.cpp"), os.path.join(ROOT, "gpuar_amd", "csrc", "lane_codec.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-fconstexpr-ops-limit=100000000",
                               "-fconstexpr-loop-limit=1000000", "-Wno-unknown-pragmas",
                               "-I", os.path.join(ROOT, "include"), "-o", so, srcs[0]])
    lib = C.CDLL(so)
    for name in ("emu_table_pick", "emu_shift_pick_of_symbol", "emu_shift_pick_of_tag"):
        getattr(lib, name).restype = C.c_uint32
        getattr(lib, name).argtypes = [C.c_uint32, C.c_uint32]
    lib.emu_table_row_offset.restype = C.c_uint32
    lib.emu_table_row_offset.argtypes = [C.c_uint32]
    for name in ("emu_current_encode_slots", "emu_table_encode_slots"):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [u8p, C.c_size_t, u8p]
    for name in ("emu_table_encode_slots_phased", "emu_table_encode_slots_ragged"):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [u8p, C.c_size_t, u8p, C.c_uint32]
    lib.emu_table_encode_slots_handoff.restype = C.c_int
    lib.emu_table_encode_slots_handoff.argtypes = [u8p, C.c_size_t, u8p, C.c_uint32, C.c_uint32]
    return lib


def test_every_table_entry_is_the_shifted_and_masked_path_word(emu):
    """All 256 symbols, depths 4-7: table[x & 15][depth - 4] == (z >> s) & 0x10001 as account() forms it from the symbol
    (paths_of_symbol) and from the GPU's row tag (paths_of_tag), and is bit 7 - depth of x | the same bit of x + 1 << 16 --
    the rows with x & 15 == 15, whose x + 1 carries out of the low four bits, and x = 255, whose x + 1 wraps, included."""
    for x in range(256):
        assert emu.emu_table_row_offset(x) == (x & 15) * 16
        for depth in (4, 5, 6, 7):
            bit = 7 - depth
            want = ((x >> bit) & 1) | ((((x + 1) >> bit) & 1) << 16)
            got = emu.emu_table_pick(x, depth)
            assert got == want == emu.emu_shift_pick_of_symbol(x, depth) == emu.emu_shift_pick_of_tag(x, depth), (x, depth)


def emu_slots(fn, data, *more):
    data = np.ascontiguousarray(data)
    npk = (data.size + PACKET - 1) // PACKET
    slots = np.zeros(max(npk, 1) * SLOT, dtype=np.uint8)
    ov = fn(data.ctypes.data_as(u8p), data.size, slots.ctypes.data_as(u8p), *more)
    return slots, npk, ov


def slots_to_stream(slots, npk):
    parts = []
    for p in range(npk):
        clen = int(slots[p * SLOT]) | (int(slots[p * SLOT + 1]) << 8)
        parts.append(slots[p * SLOT:p * SLOT + clen])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


@pytest.mark.parametrize("c", REFV, ids=lambda c: c["name"])
def test_table_walk_on_the_host_gives_the_golden_streams(emu, port_oracle, c):
    """The table-walk modelers chained with the existing coder, straight, in the kernel's whole phases (row tags, a lane's
    column, the low modeler a phase behind) and in its ragged form (every symbol by the top modeler's symbol form and the low
    one's prime_tag + step_last_tag: a lane of a group that is not full): the slots of today's host modelers byte for byte,
    the oracle's stream, the golden stream's length, packet lengths, md5 and -- where the bytes are kept -- the bytes."""
    data = np.ascontiguousarray(case_input(c))
    want, npk, ov = emu_slots(emu.emu_current_encode_slots, data)
    got, _, ov2 = emu_slots(emu.emu_table_encode_slots, data)
    assert ov == ov2 == 0 and np.array_equal(got, want)
    for lane in (0, 37):
        phased, _, ov3 = emu_slots(emu.emu_table_encode_slots_phased, data, lane)
        assert ov3 == 0 and np.array_equal(phased, want), lane
    for lane in (0, 63):
        ragged, _, ov4 = emu_slots(emu.emu_table_encode_slots_ragged, data, lane)
        assert ov4 == 0 and np.array_equal(ragged, want), lane
    stream = slots_to_stream(got, npk)
    assert np.array_equal(stream, port_oracle.encode_stream(data))
    assert stream.size == c["stream_len"] and md5(stream.tobytes()) == c["stream_md5"]
    assert [int(got[p * SLOT]) | (int(got[p * SLOT + 1]) << 8) for p in range(npk)] == c["clens"]
    keep = os.path.join(GOLD, c["name"] + ".stream.bin")
    if os.path.exists(keep):
        assert stream.tobytes() == open(keep, "rb").read()


def special_packets():
    """Packets that visit every table row and the carries around it: 0..255 in order and in reverse (every row, the rows with
    x & 15 == 15, x = 127 and 255), and runs of one symbol 8192 long (counts near 2^13 on one path) for 0x0F, 0xF0 and 0xFF."""
    up = np.tile(np.arange(256, dtype=np.uint8), PACKET // 256)
    return np.concatenate([up, up[::-1], np.full(PACKET, 0x0F, np.uint8), np.full(PACKET, 0xF0, np.uint8), np.full(PACKET, 0xFF, np.uint8)])


def test_table_walk_on_the_host_on_walks_and_runs(emu, port_oracle):
    data = special_packets()
    want, npk, ov = emu_slots(emu.emu_current_encode_slots, data)
    got, _, ov2 = emu_slots(emu.emu_table_encode_slots_phased, data, 5)
    assert ov == ov2 == 0 and np.array_equal(got, want)
    assert np.array_equal(slots_to_stream(got, npk), port_oracle.encode_stream(data))


def mixed_bytes(n, seed):
    """Bytes of changing statistics: uniform, a small alphabet, long runs -- a packet is 8192 of them."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    third = n // 3
    data[third:2 * third] = rng.choice(np.array([0x0F, 0x10, 0x7F, 0x80, 0xEF, 0xF0, 0xFF, 0x00], dtype=np.uint8), third)
    data[2 * third:] = np.repeat(rng.integers(0, 256, (n - 2 * third) // 40 + 1, dtype=np.uint8), 40)[:n - 2 * third]
    return data


def test_whole_phase_and_ragged_forms_at_every_packet_length(emu, port_oracle):
    """The kernel's two forms on all 8192 packets of tests/length_sweep.py (one per length 1 ... 8192, six source models in
    turn), each packet a call of its own with the lane's column rotating through all 64: the whole-phase form (whose last
    phase is a partial one for seven lengths in eight) and the ragged form give the slot of today's host modelers, which is the
    oracle's packet."""
    pkts = LS.packets()
    slot = np.zeros(SLOT, dtype=np.uint8)
    for i, pkt in enumerate(pkts):
        want, _, ov = emu_slots(emu.emu_current_encode_slots, pkt)
        ref = port_oracle.encode_stream(pkt)
        assert ov == 0 and np.array_equal(want[:ref.size], ref) and not want[ref.size:].any(), pkt.size
        for fn, lane in ((emu.emu_table_encode_slots_phased, i % 64), (emu.emu_table_encode_slots_ragged, (37 * i + 11) % 64)):
            slot[:] = 0
            assert fn(pkt.ctypes.data_as(u8p), pkt.size, slot.ctypes.data_as(u8p), lane) == 0
            assert np.array_equal(slot, want), (pkt.size, lane, fn.__name__)


@pytest.mark.parametrize("kind", ["mixed", "carry"])
def test_hand_off_from_the_whole_phase_form_at_every_shortest_length(emu, port_oracle, kind):
    """One 8192-byte packet as a lane of a full group whose shortest lane holds len_min bytes, for every len_min in 0 ... 8192:
    the top modeler goes over to its symbol form after (len_min / 64) * 8 phases on the nodes its last tag-form step fetched,
    the low modeler to prime_tag + step_last_tag after len_min / 8 phases -- for most len_min the top is in symbol form while
    the low one is still in tag form.  Wherever the hand-offs fall, the slot is that of today's host modelers and the oracle's.
    `carry`: packet 0 of the parity suite's keep-carrying family (0x7F / 0x80 either side of the interval's midpoint)."""
    pkt = np.ascontiguousarray(mixed_bytes(PACKET, 77) if kind == "mixed" else PF.keep_carrying(2)[:PACKET])
    assert pkt.size == PACKET
    want, _, ov = emu_slots(emu.emu_current_encode_slots, pkt)
    ref = port_oracle.encode_stream(pkt)
    assert ov == 0 and np.array_equal(want[:ref.size], ref) and not want[ref.size:].any()
    slot = np.zeros(SLOT, dtype=np.uint8)
    for len_min in range(PACKET + 1):
        slot[:] = 0
        assert emu.emu_table_encode_slots_handoff(pkt.ctypes.data_as(u8p), pkt.size, slot.ctypes.data_as(u8p), len_min % 64, len_min) == 0
        assert np.array_equal(slot, want), len_min


FAMILIES = {
    "keep_carrying": lambda: PF.keep_carrying(64),
    "drain_the_window": lambda: PF.drain_the_window(64),
    "ten_source_models_7": lambda: PF.ten_source_models(7, 64),
    "ten_source_models_8": lambda: PF.ten_source_models(8, 64),
}
HANDOFF_LEN_MINS = (1, 8, 63, 64, 71, 4097, 8128, 8191, 8192)     # around a phase, a chunk, the middle, the last chunk, the end


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_all_three_forms_on_the_adversarial_packet_families(emu, port_oracle, family):
    """The first 64 packets of each adversarial family of tests/test_gpu_parity.py (the coder's carry path; models fed bytes
    they have never seen; ten source models with intervals of width 1-3; the two cut families end in a short packet) through
    the whole-phase form, the ragged form and the hand-off at shortest lengths around every boundary the kernel has: the slots
    of today's host modelers, the oracle's stream."""
    data = np.ascontiguousarray(FAMILIES[family]())
    want, npk, ov = emu_slots(emu.emu_current_encode_slots, data)
    assert ov == 0 and npk == 64
    assert np.array_equal(slots_to_stream(want, npk), port_oracle.encode_stream(data))
    for lane, fn in ((21, emu.emu_table_encode_slots_phased), (42, emu.emu_table_encode_slots_ragged)):
        got, _, ov2 = emu_slots(fn, data, lane)
        assert ov2 == 0 and np.array_equal(got, want), fn.__name__
    for k, len_min in enumerate(HANDOFF_LEN_MINS):
        got, _, ov3 = emu_slots(emu.emu_table_encode_slots_handoff, data, (7 * k + 3) % 64, len_min)
        assert ov3 == 0 and np.array_equal(got, want), len_min


# -------------------------------------------------------------------------------------------------------- code object

# per phase of eight symbols, DESIGN.md 4.2 (the table walk): top modeler 19.1 vector + 4.6 LDS instructions per symbol,
# low modeler 20.6 + 12.5, coder as encode_kernel's
TOP_VALU, TOP_LDS = 153, 37
LOW_VALU, LOW_LDS = 165, 100
CODER_VALU, CODER_LDS = 8 * (31 + 13), 12


def test_table_kernel_keeps_four_workgroups_per_cu(code_object):
    meta, _ = code_object
    rec = meta["encode_kernel_t16"]
    assert rec["group_segment_fixed_size"] == 39936 + 256 <= 40960
    assert rec["vgpr_count"] + rec.get("agpr_count", 0) <= 128
    assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0
    assert rec["max_flat_workgroup_size"] == 256 and rec["wavefront_size"] == 64
    assert rec.get("uses_dynamic_stack") in ("false", False, 0)


def test_table_kernel_roles_keep_their_instruction_budgets(code_object):
    """Between two barriers: the low modeler's whole phase reads the pick table eight times, 16 bytes each (one per symbol),
    and no other phase reads it; every role stays within the counts DESIGN.md 4.2 quotes.  The top modeler (depths 1-2, depth 0
    and the x == 255 term: the eight v_bfe_i32) walks two levels fewer than encode_kernel's, the low one (depths 3-7) forms a
    path word for depth 3 alone."""
    _, dis = code_object
    tops, lows, coders = [], [], []
    for seg in phase_segments(dis["encode_kernel_t16"]):
        ops = [t.split()[0] for t in seg]
        valu = sum(1 for o in ops if VEC.match(o))
        lds = sum(1 for o in ops if o.startswith("ds_"))
        branches = sum(1 for o in ops if o.startswith(("s_cbranch", "s_branch")))
        tags = ops.count("v_lshlrev_b32_sdwa")
        rows = sum(1 for t in seg if t.startswith("ds_read_b128") and "offset:39936" in t)
        if tags == 8 and rows == 8 and branches <= 1:
            lows.append((valu, lds, rows))
        elif tags == 8 and ops.count("v_bfe_i32") >= 7 and branches == 0 and not any(o.startswith("global_") for o in ops):
            tops.append((valu, lds, rows))
        elif ops.count("v_mul_hi_u32") == 16 and ops.count("global_store_dword") == 16:
            coders.append((valu, lds, rows))
    assert len(tops) >= 6 and len(lows) == 1 and len(coders) == 1, (tops, lows, coders)
    assert lows[0][2] == 8 and all(t[2] == 0 for t in tops) and coders[0][2] == 0, (tops, lows, coders)
    for valu, lds, _ in tops:
        assert valu <= TOP_VALU and lds <= TOP_LDS, (valu, lds)
    assert lows[0][0] <= LOW_VALU and lows[0][1] <= LOW_LDS, lows
    assert coders[0][0] <= CODER_VALU and coders[0][1] <= CODER_LDS, coders
    # the whole point: fewer vector instructions per symbol step than encode_kernel's 22.1 + 24.0 + 31 (its contract test)
    step = (max(t[0] for t in tops) + lows[0][0]) / 8.0
    assert step <= 22.1 + 24.0 - 6.0, step


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def H():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpuar_amd import hip
    hip.load()          # raises if the HIP library is missing: no fallback
    return hip


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    codec = O.require_best()
    assert codec.kind == O.expected_kind()
    return codec


def gpu_slots(H, data, mode):
    """Slots of `data` through gpuar_hip_encode_mode(mode), into a zeroed array so that two kernels can be compared whole."""
    import torch
    npk = H.packet_count(data.size)
    d_in = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    d_slots = torch.zeros(npk * SLOT, dtype=torch.uint8, device="cuda")
    H.encode(d_in, d_slots, mode=mode)
    torch.cuda.synchronize()
    assert H.status() == 0
    return d_slots.cpu().numpy()


def check_against_throughput_and_oracle(H, oracle, data):
    npk = H.packet_count(data.size)
    table = gpu_slots(H, data, "table")
    assert np.array_equal(table, gpu_slots(H, data, "throughput"))
    assert np.array_equal(slots_to_stream(table, npk), oracle.encode_stream(data))


LAST_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 8191, 8192)


@pytest.mark.gpu
@pytest.mark.parametrize("npk", [1, 63, 64, 65, 129])
def test_table_kernel_slots_at_every_packet_count_and_tail(H, oracle, npk):
    """One wavefront not full, full, one lane over, two workgroups and a lane; the last packet 1 .. 8192 bytes long: shorter
    than a phase, a phase, a phase and a byte, two phases and their neighbours, a byte short of whole, whole."""
    whole = mixed_bytes(npk * PACKET, 100 + npk)
    for last in LAST_LENGTHS:
        check_against_throughput_and_oracle(H, oracle, whole[:(npk - 1) * PACKET + last])


@pytest.mark.gpu
def test_table_kernel_slots_on_walks_and_runs(H, oracle):
    """Every table row in order and in reverse, the rows whose x + 1 carries out of the low four bits, x = 127 and 255;
    8192-long runs of 0x0F, 0xF0 and 0xFF."""
    check_against_throughput_and_oracle(H, oracle, special_packets())


@pytest.fixture(scope="module")
def small_slot_lib():
    """libgpuar_hip.so with 1024-byte slots (tests/_build/, the build of tests/test_gpu_parity.py's fixture of that name)."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libgpuar_hip_slot1024.so")
    srcs = [os.path.join(ROOT, "gpuar_amd", "csrc", f) for f in ("gpuar_kernels.hip", "lane_codec.h")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in srcs):
        host_o = os.path.join(ROOT, "build", "host_codec.o")
        if not os.path.exists(host_o):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "gpuar_amd", "csrc"), host_o])
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT}/include",
                               "-Wno-unused-function", "-mllvm", "-phi-node-folding-threshold=64", "-mllvm",
                               "-two-entry-phi-node-folding-threshold=64", "-DGPUAR_SLOT_BYTES=1024u", "-shared", "-o", so,
                               host_o, srcs[0]], cwd=os.path.dirname(srcs[0]))
    lib = C.CDLL(so)
    lib.gpuar_hip_encode_mode.restype = C.c_int
    lib.gpuar_hip_encode_mode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


@pytest.mark.gpu
def test_table_kernel_contains_a_slot_overflow(small_slot_lib, oracle):
    """tests/test_gpu_parity.py's overflow case through GPUAR_MODE_TABLE: with 1024-byte slots packets of random bytes outgrow
    their slots, packets of zeros fit; the overflow is flagged, nothing lands beyond the slot array or in a neighbour's slot,
    an overflowed slot holds the packet's true prefix and the packets that fit are exact."""
    import torch
    slot, groups = 1024, 3
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, groups * 64 * PACKET, dtype=np.uint8)
    fits = [1, 64, 130]
    for p in fits:
        data[p * PACKET:(p + 1) * PACKET] = 0
    npk = groups * 64
    d_in = torch.from_numpy(data).cuda()
    guard = 4096
    d_slots = torch.full((npk * slot + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = small_slot_lib.gpuar_hip_encode_mode(d_in.data_ptr(), data.size, d_slots.data_ptr(), word.data_ptr(), None, MODE_TABLE)
    torch.cuda.synchronize()
    assert rc == 0 and int(word.item()) & 1, (rc, int(word.item()))
    got = d_slots.cpu().numpy()
    assert (got[npk * slot:] == 0xA5).all()
    zero_pkt = np.frombuffer(oracle.encode_packet(bytes(PACKET)), dtype=np.uint8)
    for p in fits:
        assert np.array_equal(got[p * slot:p * slot + zero_pkt.size], zero_pkt), p
        assert (got[p * slot + zero_pkt.size + 3:(p + 1) * slot] == 0xA5).all(), p
    for p in (0, 2, 63, 65, 191):
        want = np.frombuffer(oracle.encode_packet(data[p * PACKET:(p + 1) * PACKET].tobytes()), dtype=np.uint8)
        s0 = got[p * slot:(p + 1) * slot]
        assert int(s0[0]) | (int(s0[1]) << 8) == slot and int(s0[2]) | (int(s0[3]) << 8) == PACKET, p
        assert np.array_equal(s0[4:slot - 8], want[4:slot - 8]), p


@pytest.mark.gpu
def test_auto_above_the_small_switch_is_the_table_kernel_and_round_trips(H, oracle):
    """513 groups of 64 packets, one more than gpuar_hip_encode sends to the latency kernel: AUTO writes what GPUAR_MODE_TABLE
    writes (and THROUGHPUT: every kernel writes the same bytes -- which one ran shows in a kernel trace, not here), the slots
    decode to the input, and sampled packets are the oracle's."""
    import torch
    npk = 513 * 64
    n = (npk - 1) * PACKET + 4097
    d_in = H.generate("uniform", 42, n)
    auto = torch.zeros(npk * SLOT, dtype=torch.uint8, device="cuda")
    H.encode(d_in, auto, mode="auto")
    assert torch.equal(H.decode(auto, npk)[:n], d_in) and H.status() == 0
    for mode in ("table", "throughput"):
        other = torch.zeros(npk * SLOT, dtype=torch.uint8, device="cuda")
        H.encode(d_in, other, mode=mode)
        assert torch.equal(auto, other), mode
        del other
    assert H.status() == 0
    for p in (0, 63, 64, 512 * 64 - 1, 512 * 64, npk - 1):
        want = np.frombuffer(oracle.encode_packet(d_in[p * PACKET:(p + 1) * PACKET].cpu().numpy().tobytes()), dtype=np.uint8)
        assert np.array_equal(auto[p * SLOT:p * SLOT + want.size].cpu().numpy(), want), p
