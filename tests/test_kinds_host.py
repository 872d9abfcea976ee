"""Raw and sparse packets in a packet stream on the CPU (no GPU needed): the host definitions of gpuar_amd/csrc/kinds.h -- the
stream form, the header checks, store and expand -- against their restatement (tests/kinds_ref.py) on the packet families, with
each of the four on/off combinations of the two options; the pinned maximum estimate and the slot fit; every damaged form
refused; trailer version 6 through Trailer::save / load for every legal flag combination and every unusable variant; and the same
packets and trailers through a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import kinds_ref as K
import sparse_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKET = 8192
GUARD = 64
OPTIONS = [(False, False), (True, False), (False, True), (True, True)]        # (stored, sparse)


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as g
    from gpuar_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        g.build()
    hip.load()
    return hip


@pytest.fixture(scope="module")
def packets():
    return K.packets()


def _ptr(a, at=0):
    return C.c_void_p(a.ctypes.data + at)


def test_the_packet_list_holds_what_it_promises(packets):
    names = [name for name, _x in packets]
    assert len(names) == len(set(names))
    sizes = {x.size for _n, x in packets}
    assert sizes >= set(K.LENGTHS)
    kinds = {o: [K.kind_of(x, *o) for _n, x in packets] for o in OPTIONS}
    assert set(kinds[(False, False)]) == {K.CODED}
    assert set(kinds[(True, False)]) == {K.CODED, K.RAW} and set(kinds[(False, True)]) == {K.CODED, K.SPARSE}
    assert set(kinds[(True, True)]) == {K.CODED, K.RAW, K.SPARSE}
    by_name = dict(packets)
    for fill in S.FILLS:
        for k in (0, 1, 63, 64, 65, 127, 128):
            x = by_name[f"fill{fill:02x}_k{k}_n8192"]
            assert S.scan(x) == (k << 8) | fill
    x = by_name["ends_n8192"]
    assert x[0] != 0x80 and x[127] != 0x80 and x[128] != 0x80 and x[8191] != 0x80 and S.scan(x) >> 8 == 4
    assert (by_name["one_lane_n8192"][640:768] != 0xFF).all() and S.scan(by_name["one_lane_n8192"]) >> 8 == 128


def test_the_restated_estimate_is_the_hosts(H, packets):
    for name, x in packets:
        assert H.estimate_host(x.tobytes()) == [K.estimate(x)], name


@pytest.mark.parametrize("stored,sparse", OPTIONS)
def test_store_and_expand_against_the_restatement(H, packets, stored, sparse):
    lib = H.load()
    for name, x in packets:
        n = x.size
        want_kind, want = K.store(x, stored, sparse)
        pkt = np.full(K.SLOT + GUARD, 0x5A, dtype=np.uint8)
        kind, clen = C.c_uint32(77), C.c_size_t(12345)
        room = len(want)                                     # exactly the room it needs (none for a coded packet)
        assert lib.gpuar_hip_kinds_store_host(_ptr(x), n, int(stored), int(sparse), _ptr(pkt), room, C.byref(kind), C.byref(clen)) == 0, name
        assert (kind.value, clen.value) == (want_kind, len(want)), name
        assert pkt[:clen.value].tobytes() == want and (pkt[clen.value:] == 0x5A).all(), (name, "the packet, and nothing behind it")
        assert H.kinds_store_host(x.tobytes(), stored, sparse) == (want_kind, want), name
        if want_kind == K.CODED:
            continue
        assert clen.value <= K.SLOT and struct.unpack("<HH", want[:4]) == (len(want), n)
        kind.value, clen.value = 77, 12345                   # one byte short: refused, nothing written
        pkt[:] = 0x5A
        assert lib.gpuar_hip_kinds_store_host(_ptr(x), n, int(stored), int(sparse), _ptr(pkt), room - 1, C.byref(kind), C.byref(clen)) == -2, name
        assert (pkt == 0x5A).all() and (kind.value, clen.value) == (77, 12345), name
        out = np.full(n + GUARD, 0x5A, dtype=np.uint8)
        held = np.frombuffer(want, dtype=np.uint8).copy()
        assert lib.gpuar_hip_kinds_expand_host(_ptr(held), held.size, want_kind, _ptr(out), n) == 0, name
        assert (out[:n] == x).all() and (out[n:] == 0x5A).all(), name
        assert (K.expand(want, want_kind, n) == x).all(), name
        assert H.kinds_expand_host(want, want_kind, n) == x.tobytes(), name


def test_the_largest_estimate_and_the_slot_fit(H):
    """est is largest for 8192 bytes that hold each value 32 times (the histogram term is smallest there): 8281, whatever the
    order.  A packet is sparse only if sparse_len(k) + 1 < est, so every form the rule can pick fits the 8704-byte slot."""
    flat = np.repeat(np.arange(256, dtype=np.uint8), 32)
    rng = np.random.default_rng(3)
    assert H.estimate_host(flat.tobytes()) == [K.MAX_EST] == [K.estimate(flat)] == H.estimate_host(rng.permutation(flat).tobytes())
    tilted = flat.copy()
    tilted[0] = 1                                            # one count up, one down: never above
    assert H.estimate_host(tilted.tobytes())[0] <= K.MAX_EST
    for _ in range(20):
        assert H.estimate_host(rng.integers(0, 256, PACKET, dtype=np.uint8).tobytes())[0] <= K.MAX_EST
    assert all(H.estimate_host(flat[:n].tobytes())[0] <= K.MAX_EST for n in (1, 4096, 8191))
    assert 4 + PACKET <= K.SLOT                              # raw
    picked = [S.sparse_len(k) for k in range(PACKET // 2) if S.sparse_len(k) + 1 < K.MAX_EST]
    assert max(picked) == 8276 and all(4 + s <= K.SLOT for s in picked)
    for k in range(PACKET // 2):                             # the host rule picks no other
        if H.sparse_rule((k << 8) | 7, K.MAX_EST, PACKET, False) == S.SPARSE:
            assert 4 + H.sparse_len(k) <= K.SLOT


@pytest.mark.parametrize("name,pkt,kind,n", K.damaged(), ids=[d[0] for d in K.damaged()])
def test_damaged_packets_are_refused(H, name, pkt, kind, n):
    lib = H.load()
    assert K.expand(pkt, kind, n) is None                    # the restatement refuses it too
    held = np.frombuffer(pkt, dtype=np.uint8).copy() if pkt else np.zeros(1, dtype=np.uint8)
    out = np.full(n + GUARD, 0x5A, dtype=np.uint8)
    assert lib.gpuar_hip_kinds_expand_host(_ptr(held), len(pkt), kind, _ptr(out), n) == -2
    assert (out[n:] == 0x5A).all(), "wrote outside the packet"
    if kind != K.SPARSE:
        assert (out == 0x5A).all(), "a raw packet that is refused leaves its destination alone"
    with pytest.raises(H.GpuarError):
        H.kinds_expand_host(pkt, kind, n)


def test_argument_checks(H):
    lib = H.load()
    x, pkt = np.zeros(100, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    kind, clen = C.c_uint32(0), C.c_size_t(0)
    ok = (_ptr(x), 100, 1, 1, _ptr(pkt), 256, C.byref(kind), C.byref(clen))
    assert lib.gpuar_hip_kinds_store_host(*ok) == 0 and (kind.value, clen.value) == (K.SPARSE, 8)
    for at, bad in ((0, None), (1, 0), (1, PACKET + 1), (6, None), (7, None)):
        args = list(ok)
        args[at] = bad
        assert lib.gpuar_hip_kinds_store_host(*args) == -2, at
    assert lib.gpuar_hip_kinds_store_host(_ptr(x), 100, 1, 1, None, 8, C.byref(kind), C.byref(clen)) == -2
    assert lib.gpuar_hip_kinds_expand_host(None, 8, 2, _ptr(x), 100) == -2 and lib.gpuar_hip_kinds_expand_host(_ptr(pkt), 8, 2, None, 100) == -2
    assert lib.gpuar_hip_kinds_expand_host(_ptr(pkt), 8, 2, _ptr(x), 0) == -2 and lib.gpuar_hip_kinds_expand_host(_ptr(pkt), 8, 2, _ptr(x), PACKET + 1) == -2
    a = 1 << 20                                              # the device calls: host-side checks first, in the estimate call's order
    store, expand = lib.gpuar_hip_kinds_store, lib.gpuar_hip_kinds_expand
    assert store(None, 0, None, None, 1, None, None, None, None) == 0
    assert store(None, 100, a, a, 1, a, a, None, None) == -2 and store(a, 100, None, a, 1, a, a, None, None) == -2
    assert store(a + 8, 100, a, a, 1, a, a, None, None) == -1 and store(a, 100, a + 2, a, 1, a, a, None, None) == -1
    assert store(a, 100, a, a, 1, a, a, a + 2, None) == -1
    # (with a status word of the caller's: without one the call asks the device for its fallback word first)
    assert store(a, 100, a, a, 1, None, a, a, None) == -2 and store(a, 100, a, a, 1, a, None, a, None) == -2
    assert store(a, 100, a, a, 1, a + 8, a, a, None) == -1 and store(a, 100, a, a + 2, 1, a, a, a, None) == -1
    assert expand(None, None, None, 0, None, 0, None, None) == 0
    for missing in (0, 1, 2, 4):
        args = [a, a, a, 1, a, 100, None, None]
        args[missing] = None
        assert expand(*args) == -2, missing
    assert expand(a, a, a, 2, a, 100, None, None) == -2 and expand(a, a, a, 1, a, PACKET + 1, None, None) == -2      # n_bytes says another count
    assert expand(a, a + 4, a, 1, a, 100, None, None) == -1 and expand(a, a, a, 1, a + 8, 100, None, None) == -1
    assert expand(a, a, a, 1, a, 100, a + 2, None) == -1
    assert expand(a + 1, a, a + 1, 1, a, 100, a + 2, None) == -1      # (the stream and the kinds may sit anywhere: only the status word is wrong)
    assert lib.gpuar_hip_abi_version() == 2


# ---- trailer version 6 and the sanitized program -----------------------------------------------------------------------

LEGAL = [(crc, delta, base) for crc, delta, base in itertools.product((False, True), repeat=3) if not (base and (delta or not crc))]
WIDTHS = (1, 2, 4, 8)
COUNTS = (0, 1, 5, 6)
UNUSABLE = 6                                                 # Trailer::Status::unusable_kinds


def _trailer_fields(n):
    clens = [4 + 3 * i for i in range(n)]
    return clens, [(i * 2654435761 + 17) & 0xFFFFFFFF for i in range(n)], [i % 3 for i in range(n)]


def _file_with(trailer, clens):
    return bytes(K.HEADER) + bytes(sum(clens)) + trailer


def unusable_trailers():
    """[(name, file bytes)]: version-6 trailers a reader must refuse, one class at a time"""
    clens, crcs, kinds = _trailer_fields(5)
    good = K.trailer_v6(clens, kinds, 2, crcs)

    def patched(at, data, t=good):
        t = bytearray(t)
        t[at:at + len(data)] = data
        return bytes(t)

    kinds_at = 24 + 2 * 5 + 2 + 4 * 5
    assert good[kinds_at:kinds_at + 5] == bytes(kinds)
    out = [("kind_3", patched(kinds_at + 1, b"\x03")), ("kind_255", patched(kinds_at + 4, b"\xff"))]
    out += [(f"width_{w}", patched(16, struct.pack("<I", w))) for w in (0, 3, 16)]
    out += [("flag_bit_4", patched(20, struct.pack("<I", 9 | 16))), ("flag_bit_31", patched(20, struct.pack("<I", 9 | 1 << 31))),
            ("kinds_flag_missing", patched(20, struct.pack("<I", 1))),
            ("base_with_delta", patched(20, struct.pack("<I", 15))),
            ("base_without_crcs", K.trailer_v6(clens, kinds, 2, None)[:20] + struct.pack("<I", 12) + K.trailer_v6(clens, kinds, 2, None)[24:])]
    out += [("n_one_more", patched(8, struct.pack("<Q", 6))), ("n_huge", patched(8, struct.pack("<Q", 1 << 60))),
            ("tail_magic", patched(len(good) - 4, b"XPIX")), ("trailer_bytes", patched(len(good) - 12, struct.pack("<Q", len(good) + 8))),
            ("cut_by_one", good[:-1]), ("cut_to_the_fixed_fields", good[:24]), ("cut_to_8", good[:8]), ("one_byte_more", good + b"\0"),
            ("clen_sum", patched(24, struct.pack("<H", clens[0] + 1)))]
    return [(name, _file_with(t, clens)) for name, t in out]


PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "kinds.h"
#include "host/packet_index.hpp"
static uint32_t word(FILE *f) { uint32_t v = 0; if (fread(&v, 4, 1, f) != 1) std::abort(); return v; }
static std::vector<uint8_t> block(FILE *f, size_t n) { std::vector<uint8_t> v(n); if (n && fread(v.data(), 1, n, f) != n) std::abort(); return v; }
static long size_of(FILE *f) { fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET); return n; }
// packets FILE: every packet with every option pair, each in a heap block of exactly its size; then the damaged packets
static int packets(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    int bad = 0, kept = 0, refused = 0;
    for (uint32_t c = word(f); c > 0; --c) {
        const uint32_t n = word(f);
        const std::vector<uint8_t> x = block(f, n);
        for (int o = 0; o < 4; ++o) {
            uint32_t clen = 777, none = 777;
            std::vector<uint8_t> probe(gpuar::kKindsSlot);
            const uint32_t kind = gpuar::kinds_store_packet(x.data(), n, o & 1, o & 2, probe.data(), probe.size(), &clen);
            bad += kind > 2;
            if (kind == 0) { bad += clen != 0; continue; }
            ++kept;
            std::vector<uint8_t> pkt(clen), back(n), small(clen - 1);
            bad += gpuar::kinds_store_packet(x.data(), n, o & 1, o & 2, pkt.data(), pkt.size(), &none) != kind || none != clen;
            bad += gpuar::kinds_store_packet(x.data(), n, o & 1, o & 2, small.data(), small.size(), &none) != ~0u;
            bad += !gpuar::kinds_expand_packet(pkt.data(), pkt.size(), kind, back.data(), n) || back != x;
            bad += !gpuar::kinds_header_ok(gpuar::kinds_header(clen, n), clen, n);
        }
    }
    for (uint32_t c = word(f); c > 0; --c) {
        const uint32_t n = word(f), kind = word(f), held = word(f);
        const std::vector<uint8_t> pkt = block(f, held);
        std::vector<uint8_t> out(n);
        refused += !gpuar::kinds_expand_packet(pkt.data(), held, kind, out.data(), n);
    }
    fclose(f);
    std::printf("%d %d %d\n", bad, kept, refused);
    return 0;
}
// save DIR: every legal flag combination, width and count through Trailer::save into DIR/<name>, and back through Trailer::load
static int save(const std::string &dir) {
    int bad = 0, files = 0;
    const uint32_t widths[4] = {1, 2, 4, 8};
    const uint64_t counts[4] = {0, 1, 5, 6};
    for (int flags = 0; flags < 8; ++flags) {
        const bool crc = flags & 1, delta = flags & 2, base = flags & 4;
        if (base && (delta || !crc)) continue;
        for (uint32_t w : widths)
            for (uint64_t n : counts) {
                std::vector<uint16_t> clens(n);
                std::vector<uint32_t> crcs(n);
                std::vector<uint8_t> kinds(n);
                uint64_t sum = 0;
                for (uint64_t i = 0; i < n; ++i) clens[i] = 4 + 3 * i, crcs[i] = static_cast<uint32_t>(i * 2654435761u + 17), kinds[i] = i % 3, sum += clens[i];
                const std::string path = dir + "/t_" + std::to_string(flags) + "_" + std::to_string(w) + "_" + std::to_string(n);
                FILE *f = fopen(path.c_str(), "w+b");
                if (!f) return 2;
                std::vector<uint8_t> front(20 + sum, 0);
                fwrite(front.data(), 1, front.size(), f);
                gip::Trailer::save(f, clens, w, crc ? &crcs : nullptr, delta, base, &kinds);
                fflush(f);
                gip::Trailer t;
                const gip::Trailer::Status s = gip::Trailer::load(f, 20, 20 + sum, size_of(f), t);
                bad += s != gip::Trailer::Status::ok || t.version != 6 || t.clens != clens || t.kinds != kinds || t.elem_bytes != w || t.has_crcs != crc ||
                       (crc && t.crcs != crcs) || !t.mixed() || !t.indexed() || t.verify() != crc || t.filtering() != delta || t.based() != base ||
                       t.merging() != (w > 1 || delta || base);
                fclose(f);
                ++files;
            }
    }
    std::printf("%d %d\n", bad, files);
    return 0;
}
// load FILE...: the status a reader gives each file (stream from byte 20 to the header-less file's claimed end: argv pairs FILE END)
static int load(int n, char **args) {
    for (int i = 0; i + 1 < n; i += 2) {
        FILE *f = fopen(args[i], "rb");
        if (!f) return 2;
        gip::Trailer t;
        const gip::Trailer::Status s = gip::Trailer::load(f, 20, std::strtoull(args[i + 1], nullptr, 10), size_of(f), t);
        std::printf("%d %u %zu\n", static_cast<int>(s), t.version, t.clens.size() + t.kinds.size() + t.crcs.size());
        fclose(f);
    }
    return 0;
}
int main(int argc, char **argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "packets")) return packets(argv[2]);
    if (argc >= 3 && !std::strcmp(argv[1], "save")) return save(argv[2]);
    if (argc >= 3 && !std::strcmp(argv[1], "load")) return load(argc - 2, argv + 2);
    return 2;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The stand-alone program (own main) over kinds.h and host/packet_index.hpp, built with AddressSanitizer and UBSan"""
    d = tmp_path_factory.mktemp("kinds_program")
    src, exe = d / "kinds_check.cpp", d / "kinds_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fconstexpr-ops-limit=100000000", "-fconstexpr-loop-limit=1000000",
                           "-I", os.path.join(ROOT, "gpuar_amd", "csrc"), "-o", str(exe), str(src)])
    return str(exe)


def test_sanitized_program_over_the_packets(program, packets, tmp_path):
    data = tmp_path / "packets.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<I", len(packets)))
        for _name, x in packets:
            f.write(struct.pack("<I", x.size) + x.tobytes())
        bad = K.damaged()
        f.write(struct.pack("<I", len(bad)))
        for _name, pkt, kind, n in bad:
            f.write(struct.pack("<III", n, kind, len(pkt)) + pkt)
    r = subprocess.run([program, "packets", str(data)], capture_output=True, text=True, timeout=300)
    kept = sum(K.kind_of(x, *o) != K.CODED for _n, x in packets for o in OPTIONS)
    assert kept > 100
    assert r.returncode == 0 and r.stdout.split() == ["0", str(kept), str(len(K.damaged()))], (r.returncode, r.stdout, r.stderr[-2000:])


def test_trailer_version_6_save_and_load(program, tmp_path):
    r = subprocess.run([program, "save", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["0", str(len(LEGAL) * len(WIDTHS) * len(COUNTS))], (r.returncode, r.stdout, r.stderr[-2000:])
    for crc, delta, base in LEGAL:
        for w in WIDTHS:
            for n in COUNTS:
                clens, crcs, kinds = _trailer_fields(n)
                want = _file_with(K.trailer_v6(clens, kinds, w, crcs if crc else None, delta, base), clens)
                got = (tmp_path / f"t_{crc + 2 * delta + 4 * base}_{w}_{n}").read_bytes()
                assert got == want, (crc, delta, base, w, n)
                t = want[K.HEADER + sum(clens):]
                assert len(t) % 8 == 4 and struct.unpack("<Q", t[-12:-4])[0] == len(t)


def test_the_batch_trailer_is_the_same_bytes(H):
    from gpuar_amd import batch
    for crc, delta, base in LEGAL:
        for n in COUNTS:
            clens, crcs, kinds = _trailer_fields(n)
            assert batch.trailer(clens, 4, crcs if crc else None, delta=delta, base=base, kinds=kinds) == K.trailer_v6(clens, kinds, 4, crcs if crc else None, delta, base)
    with pytest.raises(H.GpuarError):
        batch.trailer([4, 4], kinds=[0, 3])
    with pytest.raises(H.GpuarError):
        batch.trailer([4, 4], kinds=[0])
    assert batch.trailer([4, 7], 2, None) == __import__("planes_ref").trailer_v3([4, 7], 2, None)      # without kinds: as ever


def test_unusable_version_6_trailers_are_refused(program, tmp_path):
    cases = unusable_trailers()
    clens, crcs, kinds = _trailer_fields(5)
    args = []
    for name, blob in [("good", _file_with(K.trailer_v6(clens, kinds, 2, crcs), clens))] + cases:
        (tmp_path / name).write_bytes(blob)
        args += [str(tmp_path / name), str(K.HEADER + sum(clens))]
    r = subprocess.run([program, "load", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = [line.split() for line in r.stdout.splitlines()]
    assert lines[0] == ["1", "6", "15"], lines[0]                              # Status::ok, with everything it carries
    for (name, _blob), line in zip(cases, lines[1:]):
        assert line == [str(UNUSABLE), "0", "0"], (name, line)
    assert len(lines) == len(cases) + 1
