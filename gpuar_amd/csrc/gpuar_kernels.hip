// gpuar_kernels.hip -- gfx950 (MI355X, CDNA4) kernels for the GPUAR packet codec.
//
// One lane = one packet, 64 packets per wavefront.  What the reference does
// with one CUDA thread per packet in 32-thread blocks, a 516-byte Fenwick tree
// per thread in shared memory and bit-at-a-time loops
// (/root/reference/src/gpuar_kernel.cu:894-934, 205-238, 321-367, 787-836) is
// re-derived here for 64-wide wavefronts (per-lane code: lane_codec.h):
//
//  * encode_kernel (throughput): four wavefronts per 64 packets, one role per SIMD -- a TOP MODELER (reads the input,
//    walks depths 1-4 of the 64 adaptive models: per lane a binary left-count tree in LDS, node-major / lane-minor so
//    that lane l always hits bank l & 31; software-pipelined walks that yield cumLo, cumHi and the count update), a
//    LOW MODELER (depth 0 in a register, depths 5-7, the x == 255 term, added onto the top modeler's part in place), a
//    CODER (interval narrowing by a wave-uniform reciprocal, one-clz renormalisation count, the lower bound as a 64-bit
//    window with carries, predicated dword stores) and a COURIER that carries the coder's reciprocals from memory into
//    LDS a phase ahead, so that no working role issues a scalar load.  The roles work one phase (8 symbols) apart and
//    hand a phase on in place through a three-slot LDS ring, one s_barrier per phase;
//  * encode_kernel_t16 (throughput, what gpuar_hip_encode launches for large inputs): the same roles with the tree dealt 2 + 5
//    and the path operands of depths 4-7 read from a 256-byte table in LDS, one 16-byte read per symbol (lane_codec.h, PickTable);
//  * encode_small_kernel (latency): the same integers cut finer for inputs that cannot fill the chip -- four tree
//    roles, an interval role, a sink role and a courier, seven wavefronts per 64 packets, phases of 16 symbols;
//  * decode_*_kernel: one wavefront per 64 packets; the symbol search reads two 16-byte subtree records per symbol
//    instead of walking eight levels, applies the increments of the 8-byte half of each that the path went through by
//    one 64-bit LDS add, and works on a scaled remainder (no division, borrow = path bit); the symbol step is a
//    hand-scheduled instruction stream; the packet stream reaches it through a per-lane ring in LDS, the per-symbol
//    reciprocal multipliers as VECTOR operands, eight at a time by loads with a wave-uniform address (no scalar load,
//    no v_readlane in the loop);
//  * crc32_kernel: the per-packet CRC-32 of the .gip trailer, computed or verified;
//  * split_planes_kernel / merge_planes_kernel, planes_tail_kernel: byte-plane splitting of typed data (planes.h);
//  * split_xor_kernel / merge_xor_kernel, xor_tail_kernel: the same with an XOR against a base buffer fused in (xorbase.h);
//  * split_delta_kernel / merge_delta_kernel, delta_tail_kernel: the same with an element-wise delta filter fused in (delta.h,
//    DESIGN.md 4.9);
//  * split_mixed_kernel / merge_mixed_kernel, mixed_tail_kernel, choose_modes_kernel: the three filters chosen per 64 KiB
//    supergroup of a buffer (mixed.h);
//  * compaction (scan + gather), synthetic-stream generators, a plain copy (the measured HBM roof).
//
// Bit-exact with the reference: same counts, same integer arithmetic, same
// bitstream.  No MFMA: this is integer, bit-serial
// work bounded by VALU issue and LDS operations, not by HBM.
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <mutex>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpuar_hip.h"
#include "gpuar_hip_gip.h"
#include "gpuar_hip_xsurvey.h"
#include "gpuar_hip_mixed.h"

#include "lane_codec.h"
#include "crc32.h"
#include "planes.h"
#include "delta.h"
#include "xorbase.h"
#include "estimate.h"
#include "survey.h"
#include "delta_survey.h"
#include "xor_survey.h"
#include "mixed.h"
#include "sparse.h"
#include "kinds.h"

namespace gpuar {

__constant__ RecipTable g_recip = RecipTable();
// The reciprocal multipliers alone, for the decoder (which fetches them eight at a time, two runs ahead, by vector loads
// with a wave-uniform address); padded so that the look-ahead behind a packet's last symbols stays inside the table.
struct MulTable {
    uint32_t m[kPacket + 64];
    constexpr MulTable() : m{} {
        const RecipTable r = RecipTable();
        for (uint32_t i = 0; i < kPacket + 64; ++i) m[i] = r.r[i < kPacket ? i : kPacket - 1u].mul;
    }
};
__device__ const MulTable g_mul = MulTable();
__constant__ DecodeConstTable g_decode = DecodeConstTable();
__device__ uint32_t g_status = 0;
__device__ uint32_t g_status_taken;         // what take_status_kernel took out of g_status, for gpuar_hip_status to copy back
__device__ uint32_t g_cu_ticket[2048];      // one arrival counter per CU (XCC, SE, SH, CU), see encode_kernel
// What the shader clock really was while the two throughput kernels ran (measurement support, gpuar_hip_clock_samples): every
// 64th workgroup notes how many shader-clock ticks (s_memtime) and how many ticks of the constant 100 MHz clock
// (s_memrealtime) passed between its start and its end, into a slot of its own -- no atomics, two scalar reads at either
// end of one wavefront in 64, nothing inside a symbol loop.  Sum of the first / sum of the second x 100 MHz is the clock the
// vector pipes ran at, which under this load is NOT the 2.4 GHz of the data sheet (bench.py: roofline_valu).
constexpr uint32_t kClockSlots = 256, kClockEvery = 64;
__device__ unsigned long long g_clock_samples[2][kClockSlots][4];      // [encode | decode][slot][shader, 100 MHz at the start; the same at the end]
// (both readings go straight to memory: nothing of this is alive across a symbol loop, so the loops' registers are what they
// were without it -- tests/test_codeobj_contract.py holds the decoder's step to its instruction budget)
__device__ __forceinline__ void clock_sample(uint32_t which, size_t group, uint32_t lane, uint32_t end) {      // group: wave-uniform
    // only the first kClockSlots x kClockEvery groups of a launch (8 GiB) sample: beyond them slots would be shared, and a slot
    // holding the start of one workgroup and the end of another -- possibly on XCDs whose counters differ -- is no measurement
    if ((group & (kClockEvery - 1u)) == 0u && group < size_t(kClockSlots) * kClockEvery && lane == 0u) {
        unsigned long long *slot = g_clock_samples[which][group / kClockEvery] + 2u * end;
        slot[0] = clock64();
        slot[1] = wall_clock64();
    }
}

// Lane's column in a tree row: lanes l and l+32 share a dword (low/high half),
// so the 32 lanes of each LDS lane-group hit 32 distinct banks whatever node
// each of them addresses.
__device__ __forceinline__ uint32_t lane_column(uint32_t lane) {
    return ((lane & 31u) << 1) | (lane >> 5);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t other = __shfl_xor(v, off);
        v = other > v ? other : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// ---------------------------------------------------------------------------
// Encode: replaces garCompress + arCompress (src/gpuar_kernel.cu:894-914, 487-531)
//
// Workgroup = 4 wavefronts, three of them working on the same 64 packets (lane l
// <-> packet 64*group + l in all three); which wavefront plays which role is
// decided per SIMD at run time (see encode_kernel):
//   TOP MODELER: reads the input bytes from memory (whole 128-byte lines), walks
//           depths 1..4 of the 64 adaptive models (LDS), emits its part of
//           cumLo | cumHi << 16 per symbol and hands the bytes on;
//   LOW MODELER: one phase behind: depth 0 (a register), depths 5..7 (LDS) and the
//           x == 255 term, added onto the top modeler's part in place (why 4 + 3:
//           lane_codec.h at TopModeler);
//   CODER: two phases behind: owns the interval state and the bit sink, turns the
//           sums into the packet bitstream;
//   the fourth wavefront carries the coder's reciprocals from the table in memory into LDS, a phase ahead, and meets
//           the barriers.
// They meet in a three-slot LDS ring of kPhase symbols per slot (EncodeLds), one
// s_barrier per phase.
//
// Why three: a packet's model pins 510 B of LDS, so a CU holds only 4 x 64
// packets however the work is arranged, and a lone wavefront issues at most
// one instruction per ~4.6 cycles (VALU) or ~10-12 cycles (LDS) -- measured,
// tools/valu_probe.hip, tools/lds_probe.hip.  One wavefront doing everything
// ran at 108 GB/s; modeler + coder at 290 GB/s with the modeler's serial
// stream (45 VALU + 13 LDS per symbol) as the bottleneck; cutting that stream
// in two puts three wavefronts on every SIMD for the same LDS.  32 KiB tree +
// 7 KiB of rings = 39 KiB per workgroup -> exactly 4 workgroups = 12 working wavefronts/CU
// (plus the 4 that only carry reciprocals and meet the barriers, see encode_kernel).
// ---------------------------------------------------------------------------
constexpr uint32_t kPhase = 8;
// Issue priority of the three roles (s_setprio; a SIMD hosts one wavefront of each role, from different
// groups, and a group moves at the pace of its slowest role between two barriers).  Measured on uniform 2 GiB
// (tools/kind_timing.py): all equal 6.14 ms; coder first 6.25; top modeler first 5.90; top > coder > low 5.70;
// top > low > coder 5.87; with the 4-level share of the tree moved to the low modeler the same numbers with the
// roles swapped -- whoever walks four LDS levels has to go first, the three-level modeler last.
// Round 4 (the coder in carry form, ten vector instructions shorter): top > low > coder.  With the old order the lighter coder
// bought nothing (5.14 ms for 6 + 1 and 5 + 2 depths alike); with the coder last 4.96-4.99 ms for 5 + 2, 4 + 3 and 3 + 4.
constexpr int kPrioTop = 3, kPrioCoder = 0, kPrioLow = 2;

// The three roles work one phase apart -- the top modeler on the symbols of phase p, the low modeler on those of
// p - 1, the coder on those of p - 2 -- and hand a phase on IN PLACE: the top modeler writes its part of
// cumLo | cumHi << 16 per symbol, the low modeler adds its own, the coder reads the sum.  Three phases are alive at
// a time, so the ring has three slots.  The low modeler takes the symbols from the top one as well (the two input dwords
// of a phase, one LDS instruction on either side; it forms its row tags itself, one SDWA shift per symbol -- a u16 tag per
// symbol was eight LDS writes per phase in the top modeler's stream, the longest of the three, and eight reads in the low
// one's), so only one wavefront of a group reads the input from memory.
constexpr uint32_t kRingSlots = 3;
struct alignas(16) EncodeLds {
    uint8_t tree[kTreeRows * kLanes * 2];      // 32 KiB: 255 rows x (64 lanes x u16), in-order layout
    uint32_t sums[kRingSlots][kPhase][kLanes]; // 6 KiB: [slot][symbol][lane]
    uint32_t bytes[2][kPhase / 4][kLanes];     // 1 KiB: [phase parity][dword][lane], the input bytes of a phase's symbols as the
                                               // top modeler read them, for the low one: ONE LDS write per phase and lane
};
__device__ __forceinline__ uint32_t next_slot(uint32_t slot) { return slot == kRingSlots - 1u ? 0u : slot + 1u; }

// Which group of 64 packets a workgroup serves.  Workgroups are dealt to the eight XCDs round-robin
// (blockIdx & 7), each XCD with its own L2.  Serving groups in blockIdx order would give one XCD every
// eighth group, i.e. packets 512 apart -- and 512 slots (8704 B) or 512 packets (8192 B) apart is a
// multiple of the L2's set period, so everything an XCD has in flight would fall into a small fraction
// of its sets.  Instead each XCD walks its own contiguous eighth of the groups.  The grid is rounded up
// to a multiple of 8; a workgroup whose group does not exist returns at once.  (Measured on uniform
// 8 GiB: encoder L2 fetches 14.3 -> 9.6 GB, L2 write-backs 21.6 -> 12.4 GB, same run time.  The
// decoders, whose per-lane stores are whole 64-byte sectors, got slightly worse and keep blockIdx order.)
__device__ __forceinline__ size_t xcd_contiguous_group(uint32_t block, uint32_t grid) {
    const uint32_t per_xcd = grid >> 3;                       // grid is a multiple of 8
    return static_cast<size_t>(block & 7u) * per_xcd + (block >> 3);
}

// LDS only: the global loads/stores of every wave stay in flight across the barrier
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ uint4 load16_guarded(const uint8_t *p, size_t avail) {
    if (avail >= 16) return *reinterpret_cast<const uint4 *>(p);
    uint32_t w[4] = {0, 0, 0, 0};
    for (size_t b = 0; b < avail; ++b) w[b >> 2] |= static_cast<uint32_t>(p[b]) << (8u * (b & 3u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// byte kByte of `word`, seven bits up: the row tag of that symbol (lane_codec.h, InorderModel::tag) in one instruction
__device__ __forceinline__ uint32_t byte_tag(uint32_t word, uint32_t kByte) {     // kByte: a constant once the caller's loop is unrolled
    uint32_t t;
    const uint32_t seven = 7u;
    if (kByte == 0) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(t) : "v"(seven), "v"(word));
    if (kByte == 1) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(t) : "v"(seven), "v"(word));
    if (kByte == 2) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(t) : "v"(seven), "v"(word));
    if (kByte == 3) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(t) : "v"(seven), "v"(word));
    return t;
}

// The top modeler's wavefront.
//
// Input fetch: 64 bytes per lane and CHUNK of eight phases, issued at least a chunk ahead of use, as
// back-to-back 16-byte loads.  Lanes sit 8192 bytes apart, so the lines all the packets of an XCD are
// reading at one moment fall into the same few L2 sets and do not survive until the lane comes back:
// every touch of a line is a fetch from memory (rocprofv3 FETCH_SIZE: 3.3x the input with 16-byte
// pieces and two modelers reading, 1.2-1.8x with 64-byte pieces, 1.01x now that one wavefront reads
// and takes the whole 128-byte line at a time).
// (Model: which depths it walks -- TopModeler<7>, or encode_kernel_t16's TableTopModeler<7>)
template <bool kBatch = false, typename Model = TopModeler<7>>
__device__ __forceinline__ void run_top(EncodeLds &lds, const uint8_t *in, uint32_t lane, uint32_t len,
                                        uint32_t len_min, uint32_t n_phases, uint32_t whole_max = 0) {
    constexpr uint32_t kChunkPhases = 8;                       // phases per fetch
    constexpr uint32_t kChunk = kChunkPhases * kPhase;         // 64 symbols = 64 bytes = 4 x 16-byte loads
    constexpr uint32_t kPieces = kChunk / 16u;
    Model model;
    uint32_t k = 0, slot = 0;
    {
        const uint32_t first = len ? load16_guarded(in, len).x & 0xFFu : 0u;
        model.open(lds.tree, 2u * lane_column(lane), first);
    }
    // ---- whole chunks that every lane of the wavefront owns completely ----
    const uint32_t full_chunks = len_min / kChunk;
    if (full_chunks) {
        const uint4 *src = reinterpret_cast<const uint4 *>(in);
        // A 128-byte line of the input holds two chunks.  Both halves are asked for together (at the start of every
        // odd chunk, for the two chunks behind it) so that a line is fetched from memory once: with one half per
        // chunk the line was gone from L2 by the time the lane came back for the other (8192 packets 8 KiB apart).
        auto fetch = [&](uint32_t chunk, uint4 (&into)[kPieces]) {
#pragma unroll
            for (uint32_t t = 0; t < kPieces; ++t) {
                const uint32_t at = chunk * kChunk + 16u * t;
                if (at + 16u <= len) into[t] = src[kPieces * chunk + t];
                else if (at < len) into[t] = load16_guarded(in + at, len - at);
                else into[t] = make_uint4(0, 0, 0, 0);
            }
        };
        uint4 c[kPieces], n[kPieces], nn[kPieces];            // this chunk, the next one, the one after (odd chunks only)
        fetch(0, c);
        fetch(1, n);
#pragma unroll
        for (uint32_t t = 0; t < kPieces; ++t) nn[t] = make_uint4(0, 0, 0, 0);
        for (uint32_t q = 0; q < full_chunks; ++q) {
            if (q & 1u) {                                     // wave-uniform
                fetch(q + 1u, n);
                fetch(q + 2u, nn);
            }
            uint32_t w[kChunk / 4u + 1u];
#pragma unroll
            for (uint32_t t = 0; t < kPieces; ++t) w[4 * t] = c[t].x, w[4 * t + 1] = c[t].y, w[4 * t + 2] = c[t].z, w[4 * t + 3] = c[t].w;
            w[kChunk / 4u] = n[0].x;
#pragma unroll
            for (uint32_t ph = 0; ph < kChunkPhases; ++ph) {
                uint32_t *out = &lds.sums[slot][0][lane];
                lds.bytes[ph & 1u][0][lane] = w[2 * ph];                 // k = kChunkPhases * q + ph, first term even
                lds.bytes[ph & 1u][1][lane] = w[2 * ph + 1];
#pragma unroll
                for (uint32_t j = 0; j < kPhase; ++j) {
                    const uint32_t i = ph * kPhase + j;                  // symbol index inside the chunk
                    // the successor's row tag straight out of its byte of the input word (one SDWA shift); this symbol's
                    // own tag is the one the step before formed
                    const uint32_t xn_tag = byte_tag(w[(i + 1) >> 2], (i + 1) & 3u);
                    out[j * kLanes] = model.step_tag(model.next_tag, 256u + q * kChunk + i, xn_tag);
                }
                slot = next_slot(slot);
                lds_barrier();
            }
#pragma unroll
            for (uint32_t t = 0; t < kPieces; ++t) c[t] = n[t], n[t] = nn[t];
        }
        k = kChunkPhases * full_chunks;
    }
    // ---- the rest: the phases that hold the file's ragged tail (or a partly dead wavefront), then two phases
    //      in which the other roles finish ----
    uint4 cur = make_uint4(0, 0, 0, 0), nxt = cur;
    if (k * kPhase < len) cur = load16_guarded(in + k * kPhase, len - k * kPhase);
    if (k * kPhase + 16u < len) nxt = load16_guarded(in + k * kPhase + 16u, len - (k * kPhase + 16u));
    if constexpr (kBatch) {
        // A batch (encode_batch_kernel): the lanes' lengths differ anywhere in the wavefront.  Every whole phase a lane
        // owns runs on the whole-phase body, masked by the lane's own count of whole phases (a lane past it sits out with
        // its state untouched); the lane's partial phase, if any, is deferred to ONE last phase in which every lane codes
        // its own at its own symbol index.  The other roles defer it identically (ring slots and barrier counts agree).
        const uint32_t whole = len / kPhase;
        for (; k < whole_max; ++k) {
            const uint32_t base = k * kPhase;
            const bool odd = (k & 1u) != 0u;                   // wave-uniform: second half of `cur`
            const uint32_t words[3] = {odd ? cur.z : cur.x, odd ? cur.w : cur.y, odd ? nxt.x : cur.z};
            if (odd) {
                cur = nxt;
                const uint32_t ahead = base + kPhase + 16u;
                if (ahead < len) nxt = load16_guarded(in + ahead, len - ahead);
                else nxt = make_uint4(0, 0, 0, 0);
            }
            if (k < whole) {
                uint32_t *out = &lds.sums[slot][0][lane];
                lds.bytes[k & 1u][0][lane] = words[0];
                lds.bytes[k & 1u][1][lane] = words[1];
#pragma unroll
                for (uint32_t j = 0; j < kPhase; ++j) {
                    const uint32_t xn_tag = byte_tag(words[(j + 1) >> 2], (j + 1) & 3u);
                    out[j * kLanes] = model.step_tag(model.next_tag, 256u + base + j, xn_tag);
                }
            }
            slot = next_slot(slot);
            lds_barrier();
        }
        if (k < n_phases) {                                    // the deferred partial phases, each lane at its own index
            const uint32_t own = whole * kPhase, part = len - own;
            const uint4 v = part ? load16_guarded(in + own, part) : make_uint4(0, 0, 0, 0);
            lds.bytes[k & 1u][0][lane] = v.x;
            lds.bytes[k & 1u][1][lane] = v.y;
            uint32_t *out = &lds.sums[slot][0][lane];
            uint64_t w = (static_cast<uint64_t>(v.y) << 32) | v.x;
#pragma unroll 1
            for (uint32_t j = 0; j < part; ++j) {
                const uint32_t x = static_cast<uint32_t>(w) & 0xFFu;
                w >>= 8;
                out[j * kLanes] = model.step(x, 256u + own + j, static_cast<uint32_t>(w) & 0xFFu);
            }
            slot = next_slot(slot);
            lds_barrier();
            ++k;
        }
        for (; k < n_phases + 2u; ++k) lds_barrier();
        return;
    }
    for (; k < n_phases + 2u; ++k) {
        if (k < n_phases) {
            const uint32_t base = k * kPhase;
            const bool odd = (k & 1u) != 0u;                   // wave-uniform: second half of `cur`
            const uint32_t words[3] = {odd ? cur.z : cur.x, odd ? cur.w : cur.y, odd ? nxt.x : cur.z};
            if (odd) {                                         // `cur` is used up after this phase
                cur = nxt;
                const uint32_t ahead = base + kPhase + 16u;
                if (ahead < len) nxt = load16_guarded(in + ahead, len - ahead);
                else nxt = make_uint4(0, 0, 0, 0);
            }
            uint32_t *out = &lds.sums[slot][0][lane];
            lds.bytes[k & 1u][0][lane] = words[0];
            lds.bytes[k & 1u][1][lane] = words[1];
#pragma unroll
            for (uint32_t q = 0; q < 2; ++q) {
                uint32_t w = words[q], w_next = words[q + 1];
#pragma unroll 1
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint32_t i = base + 4u * q + b;
                    const uint32_t x = w & 0xFFu;
                    w = (w >> 8) | (w_next << 24);            // next symbol now in the low byte
                    w_next >>= 8;
                    if (i < len) *out = model.step(x, 256u + i, w & 0xFFu);
                    out += kLanes;
                }
            }
            slot = next_slot(slot);
        }
        lds_barrier();
    }
}

// The low modeler: one phase behind the top one; input bytes and the top modeler's parts come through LDS, the
// sums go back to the same slot.  The last symbol of a phase does not know its successor yet (the top modeler is
// writing it in this very phase), so the node of a phase's first symbol is fetched when the phase begins.
// (Model: LowModeler<7>, or encode_kernel_t16's TableLowModeler<7> with `rows`, its pick table in LDS)
template <typename Model = LowModeler<7>>
__device__ __forceinline__ void run_low(EncodeLds &lds, uint32_t lane, uint32_t len, uint32_t len_min, uint32_t n_phases,
                                        const uint8_t *rows = nullptr) {
    Model model;
    model.open(lds.tree, 2u * lane_column(lane), 0u, rows);    // (the prefetch for symbol 0 is repeated below: harmless)
    lds_barrier();                                             // phase 0: the top modeler's first
    uint32_t slot = 0, k = 0;
    const uint32_t whole_phases = len_min / kPhase < n_phases ? len_min / kPhase : n_phases;    // (two loops: see the coder's)
    for (; k < whole_phases; ++k) {                            // the symbols of phase k, during phase k + 1
        const uint32_t base = k * kPhase;
        uint32_t *io = &lds.sums[slot][0][lane];
        {
            uint32_t part[kPhase], tag[kPhase];
            const uint32_t bytes[2] = {lds.bytes[k & 1u][0][lane], lds.bytes[k & 1u][1][lane]};
#pragma unroll
            for (uint32_t j = 0; j < kPhase; ++j) part[j] = io[j * kLanes], tag[j] = byte_tag(bytes[j >> 2], j & 3u);
            model.prime_tag(tag[0]);
#pragma unroll
            for (uint32_t j = 0; j < kPhase; ++j) {
                if (j + 1u < kPhase) io[j * kLanes] = model.step_tag(tag[j], 256u + base + j, tag[j + 1u], part[j]);
                else io[j * kLanes] = model.step_last_tag(tag[j], 256u + base + j, part[j]);
            }
        }
        slot = next_slot(slot);
        lds_barrier();
    }
    for (; k < n_phases; ++k) {                                // the phases that hold a ragged tail
        const uint32_t base = k * kPhase;
        uint32_t *io = &lds.sums[slot][0][lane];
        const uint32_t bytes[2] = {lds.bytes[k & 1u][0][lane], lds.bytes[k & 1u][1][lane]};
        {
#pragma unroll 1
            for (uint32_t j = 0; j < kPhase; ++j) {
                const uint32_t i = base + j;
                if (i < len) {
                    const uint32_t t = model.tree.tag((bytes[j >> 2] >> (8u * (j & 3u))) & 0xFFu);
                    model.prime_tag(t);
                    io[j * kLanes] = model.step_last_tag(t, 256u + i, io[j * kLanes]);
                }
            }
        }
        slot = next_slot(slot);
        lds_barrier();
    }
    lds_barrier();                                             // phase n_phases + 1: the coder's last
}

// The coder (CoderLane, CarryCoderLane), two phases behind the top modeler: slot address = (wave-uniform base of this group's
// first slot) + lane * 8704; phases 0 and 1 are the modelers' first
template <typename Coder>
__device__ __forceinline__ void coder_open(Coder &coder, uint8_t *dst, size_t group, uint32_t lane) {
    __builtin_amdgcn_s_setprio(kPrioCoder);
    coder.open(dst + group * (kLanes * kSlot), lane * kSlot);
    lds_barrier();
    lds_barrier();
}

// The end of a coding lane (CoderLane, CarryCoderLane, CarrySinkLane): the packet's header, SLOT_OVERFLOW if it did not fit
template <typename Lane>
__device__ __forceinline__ void finish_lane(Lane &coder, bool live, uint32_t len, uint32_t *status) {
    if (live) {
        bool overflowed;
        coder.finish(len, overflowed);
        if (overflowed) atomicOr(status, GPUAR_STATUS_SLOT_OVERFLOW);
    }
}

__global__ void __launch_bounds__(4 * kLanes)
encode_kernel(const uint8_t *__restrict__ src, size_t size, uint8_t *__restrict__ dst, uint32_t n_packets, uint32_t *__restrict__ status) {
    __shared__ EncodeLds lds;

    const size_t group = xcd_contiguous_group(blockIdx.x, gridDim.x);
    if (group * kLanes >= n_packets) return;                 // grid padding: the whole workgroup, before any barrier
    const uint32_t lane = threadIdx.x & 63u;
    // Role by SIMD, not by wavefront index.  The dispatcher puts the four wavefronts of a workgroup on
    // four different SIMDs (tools/placement_probe.hip); each workgroup draws a ticket from its CU's
    // arrival counter and leaves SIMD `ticket & 3` idle, the next three SIMDs take top modeler, low
    // modeler, coder.  Workgroups retire in arrival order (same work each), so the four resident ones
    // hold four consecutive tickets and every SIMD hosts exactly one wavefront of each role plus one
    // idle one -- three-wavefront workgroups land 4/3/3/2 on a third of the CUs instead.  Measured on
    // uniform 8 GiB: 28.0 ms (3 wavefronts) -> 27.2 (idle 4th) -> 26.7 (roles by SIMD).
    // If the four SIMD ids are ever not distinct, roles fall back to the wavefront index.
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));        // HW_ID
    const uint32_t simd = (hw >> 4) & 3u;
    uint32_t *hello = &lds.sums[0][0][0];                      // (the ring is not in use yet)
    if (lane == 0) hello[wave] = simd;
    if (threadIdx.x == 0) {
        const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));   // XCC_ID
        hello[4] = atomicAdd(&g_cu_ticket[((xcc & 7u) << 8) | ((hw >> 8) & 0xFFu)], 1u);
    }
    __syncthreads();
    const uint32_t seen = (1u << hello[0]) | (1u << hello[1]) | (1u << hello[2]) | (1u << hello[3]);
    const uint32_t by_simd = (simd - hello[4] - 1u) & 3u;
    const uint32_t role = __builtin_amdgcn_readfirstlane(seen == 0xFu ? by_simd : wave);   // 3 = idle
    __syncthreads();
    const size_t packet = group * kLanes + lane;
    const bool live = packet < n_packets;
    const size_t start = packet * kPacket;
    const uint32_t len = live ? static_cast<uint32_t>(size - start < kPacket ? size - start : kPacket) : 0u;
    const uint32_t len_max = wave_max(len);
    const uint32_t len_min = wave_max(~len) ^ 0xFFFFFFFFu;
    const uint32_t n_phases = (len_max + kPhase - 1) / kPhase;
    const uint8_t *in = src + (live ? start : 0);

    // every role meets n_phases + 2 barriers: the top modeler works in phases 0 .. n_phases - 1, the low one in
    // 1 .. n_phases, the coder in 2 .. n_phases + 1
    if (role == 0) {
        __builtin_amdgcn_s_setprio(kPrioTop);
        run_top(lds, in, lane, len, len_min, n_phases);
    } else if (role == 1) {
        __builtin_amdgcn_s_setprio(kPrioLow);
        run_low(lds, lane, len, len_min, n_phases);
    } else if (role == 3) {
        // The fourth wavefront carries the coder's reciprocals: the eight (multiplier, shift) pairs of a phase, 64 bytes of
        // the table, go into one of two slots in the tree's unused 256th row one barrier before the coder reads them --
        // lanes 0..15 load a dword each (asked for a whole interval ahead), write it, meet the barrier.
        uint32_t *courier = reinterpret_cast<uint32_t *>(lds.tree + 255u * 128u);
        const uint32_t *table = reinterpret_cast<const uint32_t *>(g_recip.r);
        const uint32_t lane16 = lane & 15u;
        clock_sample(0u, group, lane, 0u);                     // (this wavefront has the time, and lives as long as the workgroup)
        uint32_t carried = table[lane16];                      // the pairs of phase 0
        for (uint32_t k = 0; k < n_phases + 2u; ++k) {
            // interval k: the coder will work on the symbols of phase k - 1 during interval k + 1 and reads slot (k + 1) & 1
            if (lane < 16u) courier[((k + 1u) & 1u) * 16u + lane16] = carried;
            const uint32_t next_phase = k < n_phases ? k : 0u;                     // (phase k's pairs, for interval k + 1's write)
            carried = table[next_phase * 16u + lane16];
            lds_barrier();
        }
        clock_sample(0u, group, lane, 1u);
    } else {
        CarryCoderLane coder;                // the lower bound as a 64-bit window, carries instead of owed bits (lane_codec.h)
        coder_open(coder, dst, group, lane);
        uint32_t slot = 0, k = 0;
        // Two loops, not one loop with two bodies: with both bodies in one loop the coder's eight state registers were copied
        // to the whole-phase body's own set at the top of every phase and back at its end (16 of ~280 vector instructions).
        const uint32_t whole_phases = len_min / kPhase < n_phases ? len_min / kPhase : n_phases;    // phases every lane owns completely
        for (; k < whole_phases; ++k) {                      // the symbols of phase k, during phase k + 2
            const uint32_t *in_ring = &lds.sums[slot][0][lane];
            {
                uint32_t cums[kPhase];
#pragma unroll
                for (uint32_t j = 0; j < kPhase; ++j) cums[j] = in_ring[j * kLanes];
                Recip rc[kPhase];
                {
                    // every lane reads the same 64 bytes: four broadcast reads, the pairs arrive as vector operands
                    const uint4 *slot = reinterpret_cast<const uint4 *>(lds.tree + 255u * 128u + (k & 1u) * 64u);
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) {
                        const uint4 v = slot[q];
                        rc[2 * q] = {v.x, v.y}, rc[2 * q + 1] = {v.z, v.w};
                    }
                }
                // the step in its three pieces (lane_codec.h): the NEXT symbol's two divisions sit between this symbol's
                // "who stores?" compare and the store region that reads the answer.
                // (Measured and not kept: a wave-uniform choice per phase between this and a store region that does not
                // clamp its address -- one vector instruction fewer per symbol while every lane has room for the phase's
                // eight dwords: +1 % with the reciprocals coming through LDS, +20 % while they came by scalar loads.)
                CarryCoderLane::Ahead next = coder.ahead(cums[0], rc[0]);
#pragma unroll
                for (uint32_t j = 0; j < kPhase; ++j) {
                    const CarryCoderLane::Narrowed now = coder.narrow(next);
                    if (j + 1u < kPhase) next = coder.ahead(cums[j + 1u], rc[j + 1u]);
                    coder.settle(now);
                }
            }
            slot = next_slot(slot);
            lds_barrier();
        }
        for (; k < n_phases; ++k) {                          // the phases that hold a ragged tail
            const uint32_t base = k * kPhase;
            const uint32_t *in_ring = &lds.sums[slot][0][lane];
            {
#pragma unroll 1
                for (uint32_t j = 0; j < kPhase; ++j) {
                    const uint32_t i = base + j;
                    if (i >= len_max) break;
                    const Recip r = g_recip.r[i];
                    if (i < len) coder.step(in_ring[j * kLanes], r);
                }
            }
            slot = next_slot(slot);
            lds_barrier();
        }
        if (live) {
            bool overflowed;
            coder.finish(len, overflowed);
            if (overflowed) atomicOr(status, GPUAR_STATUS_SLOT_OVERFLOW);
        }
    }
}

// ---------------------------------------------------------------------------
// encode_kernel_t16: encode_kernel with the TABLE WALK (lane_codec.h, PickTable).  The same four roles by SIMD,
// ring, barriers, ticket and coder.  The low modeler takes the path operands of depths 4-7 from a 256-byte table in LDS -- one
// 16-byte read per symbol, its address one bit-field extract of the row tag the low modeler forms anyway -- where encode_kernel
// shifts and masks once per level; with the levels that cheap the tree is dealt 2 + 5 (top: depths 1-2, depth 0 and the
// x == 255 term; low: depths 3-7) and the low modeler issues first.  39 936 + 256 bytes of LDS: still four workgroups per CU.
// Same slots, byte for byte.  What gpuar_hip_encode launches above kSmallGroups groups; encode_kernel stays the batch kernels'
// twin (GPUAR_MODE_THROUGHPUT).
// ---------------------------------------------------------------------------
struct alignas(16) EncodeTableLds {
    EncodeLds ring;
    uint32_t picks[16][4];                     // PickTable::row, written once per workgroup before the roles start
};
static_assert(sizeof(EncodeTableLds) <= 40960, "four workgroups per CU");
// Issue priorities (see kPrioTop): the role with the most LDS levels goes first -- here the LOW modeler, five levels to the top
// one's two (measured both ways, DESIGN.md 4.2: low first 17.31 ms, top first 18.39 on uniform 8 GiB); the coder stays last.
constexpr int kPrioTableLow = 3, kPrioTableTop = 2;

__global__ void __launch_bounds__(4 * kLanes)
encode_kernel_t16(const uint8_t *__restrict__ src, size_t size, uint8_t *__restrict__ dst, uint32_t n_packets, uint32_t *__restrict__ status) {
    __shared__ EncodeTableLds lds_t;
    EncodeLds &lds = lds_t.ring;

    const size_t group = xcd_contiguous_group(blockIdx.x, gridDim.x);
    if (group * kLanes >= n_packets) return;                 // grid padding: the whole workgroup, before any barrier
    const uint32_t lane = threadIdx.x & 63u;
    // roles by SIMD through the CU's ticket: see encode_kernel
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));        // HW_ID
    const uint32_t simd = (hw >> 4) & 3u;
    uint32_t *hello = &lds.sums[0][0][0];                      // (the ring is not in use yet)
    if (lane == 0) hello[wave] = simd;
    if (threadIdx.x == 0) {
        const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));   // XCC_ID
        hello[4] = atomicAdd(&g_cu_ticket[((xcc & 7u) << 8) | ((hw >> 8) & 0xFFu)], 1u);
    }
    if (wave == 3u) {
        // the pick table, a dword per lane, by a wavefront that has nothing else to do here: row = x & 15, column = depth - 4,
        // entry = bit 7 - depth of x | the same bit of x + 1 << 16 (PickTable, lane_codec.h)
        const uint32_t r = lane >> 2, bit = 3u - (lane & 3u);
        lds_t.picks[r][lane & 3u] = ((r >> bit) & 1u) | ((((r + 1u) >> bit) & 1u) << 16);
    }
    __syncthreads();
    const uint32_t seen = (1u << hello[0]) | (1u << hello[1]) | (1u << hello[2]) | (1u << hello[3]);
    const uint32_t by_simd = (simd - hello[4] - 1u) & 3u;
    const uint32_t role = __builtin_amdgcn_readfirstlane(seen == 0xFu ? by_simd : wave);   // 3 = idle
    __syncthreads();
    const size_t packet = group * kLanes + lane;
    const bool live = packet < n_packets;
    const size_t start = packet * kPacket;
    const uint32_t len = live ? static_cast<uint32_t>(size - start < kPacket ? size - start : kPacket) : 0u;
    const uint32_t len_max = wave_max(len);
    const uint32_t len_min = wave_max(~len) ^ 0xFFFFFFFFu;
    const uint32_t n_phases = (len_max + kPhase - 1) / kPhase;
    const uint8_t *in = src + (live ? start : 0);

    // every role meets n_phases + 2 barriers, as in encode_kernel
    if (role == 0) {
        __builtin_amdgcn_s_setprio(kPrioTableTop);
        run_top<false, TableTopModeler<7>>(lds, in, lane, len, len_min, n_phases);
    } else if (role == 1) {
        __builtin_amdgcn_s_setprio(kPrioTableLow);
        run_low<TableLowModeler<7>>(lds, lane, len, len_min, n_phases, reinterpret_cast<const uint8_t *>(lds_t.picks));
    } else if (role == 3) {
        // the courier of the coder's reciprocals (encode_kernel)
        uint32_t *courier = reinterpret_cast<uint32_t *>(lds.tree + 255u * 128u);
        const uint32_t *table = reinterpret_cast<const uint32_t *>(g_recip.r);
        const uint32_t lane16 = lane & 15u;
        clock_sample(0u, group, lane, 0u);
        uint32_t carried = table[lane16];                      // the pairs of phase 0
        for (uint32_t k = 0; k < n_phases + 2u; ++k) {
            if (lane < 16u) courier[((k + 1u) & 1u) * 16u + lane16] = carried;
            const uint32_t next_phase = k < n_phases ? k : 0u;
            carried = table[next_phase * 16u + lane16];
            lds_barrier();
        }
        clock_sample(0u, group, lane, 1u);
    } else {
        // the coder, statement for statement encode_kernel's
        CarryCoderLane coder;
        coder_open(coder, dst, group, lane);
        uint32_t slot = 0, k = 0;
        const uint32_t whole_phases = len_min / kPhase < n_phases ? len_min / kPhase : n_phases;    // phases every lane owns completely
        for (; k < whole_phases; ++k) {                      // the symbols of phase k, during phase k + 2
            const uint32_t *in_ring = &lds.sums[slot][0][lane];
            {
                uint32_t cums[kPhase];
#pragma unroll
                for (uint32_t j = 0; j < kPhase; ++j) cums[j] = in_ring[j * kLanes];
                Recip rc[kPhase];
                {
                    const uint4 *slot = reinterpret_cast<const uint4 *>(lds.tree + 255u * 128u + (k & 1u) * 64u);
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) {
                        const uint4 v = slot[q];
                        rc[2 * q] = {v.x, v.y}, rc[2 * q + 1] = {v.z, v.w};
                    }
                }
                CarryCoderLane::Ahead next = coder.ahead(cums[0], rc[0]);
#pragma unroll
                for (uint32_t j = 0; j < kPhase; ++j) {
                    const CarryCoderLane::Narrowed now = coder.narrow(next);
                    if (j + 1u < kPhase) next = coder.ahead(cums[j + 1u], rc[j + 1u]);
                    coder.settle(now);
                }
            }
            slot = next_slot(slot);
            lds_barrier();
        }
        for (; k < n_phases; ++k) {                          // the phases that hold a ragged tail
            const uint32_t base = k * kPhase;
            const uint32_t *in_ring = &lds.sums[slot][0][lane];
            {
#pragma unroll 1
                for (uint32_t j = 0; j < kPhase; ++j) {
                    const uint32_t i = base + j;
                    if (i >= len_max) break;
                    const Recip r = g_recip.r[i];
                    if (i < len) coder.step(in_ring[j * kLanes], r);
                }
            }
            slot = next_slot(slot);
            lds_barrier();
        }
        finish_lane(coder, live, len, status);
    }
}

// The low modeler of a batch: run_low's whole-phase body on the schedule of run_top<true>
__device__ __forceinline__ void batch_low(EncodeLds &lds, uint32_t lane, uint32_t len, uint32_t len_min, uint32_t n_phases, uint32_t whole_max) {
    LowModeler<7> model;
    model.open(lds.tree, 2u * lane_column(lane), 0u);
    lds_barrier();                                             // phase 0: the top modeler's first
    uint32_t slot = 0, k = 0;
    auto whole_phase = [&](uint32_t k) __attribute__((always_inline)) {     // the symbols of phase k, during phase k + 1
        const uint32_t base = k * kPhase;
        uint32_t *io = &lds.sums[slot][0][lane];
        uint32_t part[kPhase], tag[kPhase];
        const uint32_t bytes[2] = {lds.bytes[k & 1u][0][lane], lds.bytes[k & 1u][1][lane]};
#pragma unroll
        for (uint32_t j = 0; j < kPhase; ++j) part[j] = io[j * kLanes], tag[j] = byte_tag(bytes[j >> 2], j & 3u);
        model.prime_tag(tag[0]);
#pragma unroll
        for (uint32_t j = 0; j < kPhase; ++j) {
            if (j + 1u < kPhase) io[j * kLanes] = model.step_tag(tag[j], 256u + base + j, tag[j + 1u], part[j]);
            else io[j * kLanes] = model.step_last_tag(tag[j], 256u + base + j, part[j]);
        }
    };
    const uint32_t whole_min = len_min / kPhase;
    for (; k < whole_min; ++k) {                               // every lane owns the phase
        whole_phase(k);
        slot = next_slot(slot);
        lds_barrier();
    }
    const uint32_t whole = len / kPhase;
    for (; k < whole_max; ++k) {                               // the lanes that own it; the others sit it out
        if (k < whole) whole_phase(k);
        slot = next_slot(slot);
        lds_barrier();
    }
    if (k < n_phases) {                                        // the deferred partial phases, each lane at its own index
        const uint32_t own = whole * kPhase, part = len - own;
        uint32_t *io = &lds.sums[slot][0][lane];
        uint64_t w = (static_cast<uint64_t>(lds.bytes[k & 1u][1][lane]) << 32) | lds.bytes[k & 1u][0][lane];
#pragma unroll 1
        for (uint32_t j = 0; j < part; ++j) {
            const uint32_t t = model.tree.tag(static_cast<uint32_t>(w) & 0xFFu);
            w >>= 8;
            model.prime_tag(t);
            io[j * kLanes] = model.step_last_tag(t, 256u + own + j, io[j * kLanes]);
        }
        lds_barrier();
    }
    lds_barrier();                                             // phase n_phases + 1: the coder's last
}

// encode_kernel's choice of roles by SIMD (see there), for encode_batch_kernel: 0 top modeler, 1 low modeler, 2 coder, 3 courier
__device__ __forceinline__ uint32_t encode_role(EncodeLds &lds, uint32_t lane) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));        // HW_ID
    const uint32_t simd = (hw >> 4) & 3u;
    uint32_t *hello = &lds.sums[0][0][0];                      // (the ring is not in use yet)
    if (lane == 0) hello[wave] = simd;
    if (threadIdx.x == 0) {
        const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));   // XCC_ID
        hello[4] = atomicAdd(&g_cu_ticket[((xcc & 7u) << 8) | ((hw >> 8) & 0xFFu)], 1u);
    }
    __syncthreads();
    const uint32_t seen = (1u << hello[0]) | (1u << hello[1]) | (1u << hello[2]) | (1u << hello[3]);
    const uint32_t by_simd = (simd - hello[4] - 1u) & 3u;
    const uint32_t role = __builtin_amdgcn_readfirstlane(seen == 0xFu ? by_simd : wave);   // 3 = idle
    __syncthreads();
    return role;
}

// The four roles of encode_kernel for a workgroup of 64 batch packets: lane l codes `len` bytes at `in` into slot
// group * 64 + l.  The lanes' lengths may differ anywhere in the wavefront, so every role keeps each lane on the
// whole-phase body for every whole phase the lane owns and defers its partial phase to one last phase (run_top<true>):
// n_phases = (the most whole phases of any lane) + (1 if some lane has a partial phase), n_phases + 2 barriers per role.
__device__ __forceinline__ void batch_roles(EncodeLds &lds, uint32_t role, size_t group, uint32_t lane, const uint8_t *in,
                                            uint32_t len, bool live, uint8_t *__restrict__ dst, uint32_t *__restrict__ status) {
    const uint32_t len_min = wave_max(~len) ^ 0xFFFFFFFFu;
    const uint32_t whole_max = wave_max(len / kPhase);
    const uint32_t n_phases = whole_max + (wave_max(len % kPhase) ? 1u : 0u);
    if (role == 0) {
        __builtin_amdgcn_s_setprio(kPrioTop);
        run_top<true>(lds, in, lane, len, len_min, n_phases, whole_max);
    } else if (role == 1) {
        __builtin_amdgcn_s_setprio(kPrioLow);
        batch_low(lds, lane, len, len_min, n_phases, whole_max);
    } else if (role == 3) {
        // the courier of encode_kernel; it carries the pairs of the whole phases only (the deferred phase's are per lane)
        uint32_t *courier = reinterpret_cast<uint32_t *>(lds.tree + 255u * 128u);
        const uint32_t *table = reinterpret_cast<const uint32_t *>(g_recip.r);
        const uint32_t lane16 = lane & 15u;
        uint32_t carried = table[lane16];
        for (uint32_t k = 0; k < n_phases + 2u; ++k) {
            if (lane < 16u) courier[((k + 1u) & 1u) * 16u + lane16] = carried;
            const uint32_t next_phase = k < whole_max ? k : 0u;
            carried = table[next_phase * 16u + lane16];
            lds_barrier();
        }
    } else {
        CarryCoderLane coder;
        coder_open(coder, dst, group, lane);
        uint32_t slot = 0, k = 0;
        auto whole_phase = [&](uint32_t k) __attribute__((always_inline)) {   // the symbols of phase k, during phase k + 2
            const uint32_t *in_ring = &lds.sums[slot][0][lane];
            uint32_t cums[kPhase];
#pragma unroll
            for (uint32_t j = 0; j < kPhase; ++j) cums[j] = in_ring[j * kLanes];
            Recip rc[kPhase];
            const uint4 *pairs = reinterpret_cast<const uint4 *>(lds.tree + 255u * 128u + (k & 1u) * 64u);
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint4 v = pairs[q];
                rc[2 * q] = {v.x, v.y}, rc[2 * q + 1] = {v.z, v.w};
            }
            CarryCoderLane::Ahead next = coder.ahead(cums[0], rc[0]);
#pragma unroll
            for (uint32_t j = 0; j < kPhase; ++j) {
                const CarryCoderLane::Narrowed now = coder.narrow(next);
                if (j + 1u < kPhase) next = coder.ahead(cums[j + 1u], rc[j + 1u]);
                coder.settle(now);
            }
        };
        // three loops (whole phases of every lane, whole phases of some lanes, the deferred partial phase), not one loop
        // with several bodies: see encode_kernel's coder
        const uint32_t whole_min = len_min / kPhase;
        for (; k < whole_min; ++k) {
            whole_phase(k);
            slot = next_slot(slot);
            lds_barrier();
        }
        const uint32_t whole = len / kPhase;
        for (; k < whole_max; ++k) {
            if (k < whole) whole_phase(k);
            slot = next_slot(slot);
            lds_barrier();
        }
        if (k < n_phases) {                                  // the lane's own symbols, with its own reciprocals
            const uint32_t own = whole * kPhase, part = len - own;
            const uint32_t *in_ring = &lds.sums[slot][0][lane];
#pragma unroll 1
            for (uint32_t j = 0; j < part; ++j) coder.step(in_ring[j * kLanes], g_recip.r[own + j]);
            lds_barrier();
        }
        finish_lane(coder, live, len, status);
    }
}

// One packet of a batch (gpuar_hip_encode_batch / decode_batch / decode_stream_batch): buffer b owns the batch packets
// first_packet[b] .. first_packet[b + 1] - 1 in order, so the packet's buffer is the LAST b < n_buffers with
// first_packet[b] <= packet (an upper-bound search: a zero-length buffer shares its first_packet with the buffer behind it,
// which is the one that owns the packet).  log2(n_buffers) dependent loads per lane, once per packet.
struct BatchLane {
    const uint8_t *ptr;        // the packet's bytes in its buffer: ptrs[b] + j * 8192
    uint32_t count;            // bytes of the buffer from there on, at most 8192 (0: the packet lies past the buffer's end)
    bool owned;                // some buffer owns the packet and that buffer's pointer is 16-byte aligned
    uint32_t buffer;           // ... which buffer (when one owns the packet)
};
__device__ __forceinline__ BatchLane batch_lane(const uint8_t *const *ptrs, const uint64_t *bytes, const uint64_t *first_packet,
                                                uint32_t n_buffers, uint64_t packet) {
    uint32_t lo = 0, n = n_buffers;                          // first u in [0, n_buffers) with first_packet[u] > packet
    while (n > 0u) {
        const uint32_t half = n >> 1;
        if (first_packet[lo + half] <= packet) lo += half + 1u, n -= half + 1u;
        else n = half;
    }
    BatchLane r = {nullptr, 0u, false, 0u};
    if (lo == 0u || packet >= first_packet[lo]) return r;   // in front of the first buffer, or behind the last one's packets
    const uint32_t b = lo - 1u;
    r.buffer = b;
    const uint64_t at = (packet - first_packet[b]) * kPacket;
    const uint8_t *p = ptrs[b];
    const uint64_t n_bytes = bytes[b];
    r.owned = (reinterpret_cast<uintptr_t>(p) & 15u) == 0u;
    r.ptr = p + at;
    r.count = n_bytes > at ? static_cast<uint32_t>(n_bytes - at < kPacket ? n_bytes - at : kPacket) : 0u;
    return r;
}

// Batch encode, throughput mode: the roles of encode_kernel over the packets of many buffers.  A packet whose descriptor is
// unusable (no buffer owns it, it lies past its buffer's end, the buffer is misaligned) is a dead lane: BAD_BATCH, slot untouched.
__global__ void __launch_bounds__(4 * kLanes)
encode_batch_kernel(const uint8_t *const *__restrict__ ptrs, const uint64_t *__restrict__ bytes, const uint64_t *__restrict__ first_packet,
                    uint32_t n_buffers, uint32_t n_packets, uint8_t *__restrict__ dst, uint32_t *__restrict__ status) {
    __shared__ EncodeLds lds;

    const size_t group = xcd_contiguous_group(blockIdx.x, gridDim.x);
    if (group * kLanes >= n_packets) return;                 // grid padding: the whole workgroup, before any barrier
    const uint32_t lane = threadIdx.x & 63u;
    const size_t packet = group * kLanes + lane;
    bool live = packet < n_packets;
    BatchLane bl = {nullptr, 0u, false, 0u};
    if (live) {
        bl = batch_lane(ptrs, bytes, first_packet, n_buffers, packet);
        if (!bl.owned || bl.count == 0u) {
            live = false;
            if ((threadIdx.x >> 6) == 0u) atomicOr(status, GPUAR_STATUS_BAD_BATCH);
        }
    }
    const uint32_t role = encode_role(lds, lane);
    batch_roles(lds, role, group, lane, live ? bl.ptr : nullptr, live ? bl.count : 0u, live, dst, status);
}

// ---------------------------------------------------------------------------
// Encode, LATENCY mode: inputs too small to fill the chip (at most kSmallGroups groups of 64 packets).
//
// Such a launch takes as long as ONE packet: 8192 serial symbol steps of the slowest role, whatever the chip could do
// next to it -- the three-role kernel above needs ~355 cycles per step there (its coder's own chain), the same for 64
// packets as for 65536.  With the chip mostly idle and LDS plentiful, the step is cut finer instead: SIX working wavefronts
// per 64 packets, each one phase (16 symbols) behind the one before it.  A wavefront with few neighbours pays ~4.5
// cycles per vector instruction AND 12-20 per LDS operation, so the tree -- two LDS operations per
// level -- is what has to be spread thinnest:
//     UPPER    depths 1-2 of the tree; reads the input, hands the bytes on            13 vector + 5.5 LDS per symbol
//     MID1     depths 3-4, added onto the sums in place                               13 + 6
//     MID2     depths 5-6, added in place                                             13 + 6
//     LOW      depth 0 (register), depth 7, the x == 255 term, added in place         15 + 4
//     INTERVAL interval narrowing + renormalisation count -> one word per symbol      ~18 + 2   (lane_codec.h CarryIntervalLane)
//     SINK     the window of held bits, carries, stores                               ~19 + 1   (CarrySinkLane)
//     COURIER  (seventh wavefront) INTERVAL's reciprocals from the table into LDS, a phase ahead: no scalar load in a working role
// Same integers as the throughput kernel (lane_codec.h is shared; tests/test_lane_emulation.py pins the cut coder
// and a three-way tree against the oracle on the CPU), a different cut.  Rings: five slots of sums, four of input
// bytes, two of interval words: 64 KiB of LDS per workgroup with the tree.  Every role meets n_phases + 5 barriers.
// ---------------------------------------------------------------------------
constexpr uint32_t kSmallGroups = 512;       // up to 32768 packets = 256 MiB of input: at most two workgroups per CU
// (Measured and not kept, round 4: ONE tree level per role -- seven tree roles, ten wavefronts, phases of 8 symbols: 0.81 ms for
// 64 MiB against 0.71; every role reads and writes the sums and meets the barrier whatever it carries.)
constexpr uint32_t kSmallTreeRoles = 4;      // UPPER (depths 1-2), MID1 (3-4), MID2 (5-6), LOW (7, 0, the x == 255 term)
constexpr uint32_t kSmallLag = kSmallTreeRoles + 1u;   // the last role (SINK) works this many phases behind the first
constexpr uint32_t kSumSlots = kSmallLag;    // a slot of sums is alive from UPPER's phase to INTERVAL's, kSmallLag - 1 phases later
constexpr uint32_t kByteBufs = kSmallTreeRoles;   // the bytes of a phase are read by the other tree roles, up to kSmallTreeRoles - 1 phases later
constexpr uint32_t kSmallWaves = kSmallTreeRoles + 3u;   // + INTERVAL, SINK, COURIER
// symbols per phase: the roles meet at a barrier once per phase (8: 0.71 ms for 64 MiB; 16: 0.68 -- half as many barriers; 64 KiB
// of LDS per workgroup then)
constexpr uint32_t kSmallPhase = 16;
static_assert(kSmallPhase == 8 || kSmallPhase == 16, "a phase is 2 or 4 input dwords; the courier's lanes carry one dword of reciprocals each");
struct alignas(16) EncodeSmallLds {
    uint8_t tree[kTreeRows * kLanes * 2];     // 32 KiB
    uint32_t sums[kSumSlots][kSmallPhase][kLanes];    // [slot][symbol][lane], cumLo | cumHi << 16 in the making
    uint32_t bytes[kByteBufs][kSmallPhase / 4][kLanes];    // the input bytes of a phase
    uint32_t words[2][kSmallPhase][kLanes];   // CarryIntervalLane -> CarrySinkLane: dn | n << 16 per symbol
    // (the courier's two slots -- INTERVAL's (multiplier, shift) pairs of a phase, up to 128 bytes -- are the tree's two unused
    // rows: row 127, where depth 0 would live if it were not a register, and row 255)
    __device__ uint32_t *recips(uint32_t parity) { return reinterpret_cast<uint32_t *>(tree + (parity ? 255u : 127u) * 128u); }
};

// the input bytes of one phase at in + at (a multiple of the phase length), zero beyond `len`
struct PhaseBytes {
    uint32_t w[kSmallPhase / 4];
};
__device__ __forceinline__ PhaseBytes load_phase(const uint8_t *in, uint32_t at, uint32_t len) {
    PhaseBytes r;
    if (at + kSmallPhase <= len) {
#pragma unroll
        for (uint32_t q = 0; q < kSmallPhase / 8; ++q) {
            const uint2 v = *reinterpret_cast<const uint2 *>(in + at + 8u * q);
            r.w[2 * q] = v.x, r.w[2 * q + 1] = v.y;
        }
        return r;
    }
#pragma unroll
    for (uint32_t q = 0; q < kSmallPhase / 4; ++q) {            // (static positions: the words stay in registers)
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b)
            if (at + 4u * q + b < len) v |= static_cast<uint32_t>(in[at + 4u * q + b]) << (8u * b);
        r.w[q] = v;
    }
    return r;
}
__device__ __forceinline__ uint32_t byte_of(const PhaseBytes &p, uint32_t j) {      // j static
    return (p.w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
}

template <int kUpperDepths>
__device__ __forceinline__ void small_upper(EncodeSmallLds &lds, const uint8_t *in, uint32_t lane, uint32_t len, uint32_t len_min,
                                            uint32_t n_phases) {
    PartialModeler<7, 1, kUpperDepths, 0, false> model;
    PhaseBytes cur, nxt = load_phase(in, 0, len);
    model.open(lds.tree, 2u * lane_column(lane), nxt.w[0] & 0xFFu);
    for (uint32_t k = 0; k < n_phases + kSmallLag; ++k) {
        if (k < n_phases) {
            const uint32_t base = k * kSmallPhase;
            cur = nxt;
            nxt = load_phase(in, base + kSmallPhase, len);
#pragma unroll
            for (uint32_t q = 0; q < kSmallPhase / 4; ++q) lds.bytes[k % kByteBufs][q][lane] = cur.w[q];
            uint32_t *out = &lds.sums[k % kSumSlots][0][lane];
            if (base + kSmallPhase <= len_min) {
#pragma unroll
                for (uint32_t j = 0; j < kSmallPhase; ++j)
                    out[j * kLanes] = model.step(byte_of(cur, j), 256u + base + j, j + 1u < kSmallPhase ? byte_of(cur, j + 1u) : nxt.w[0] & 0xFFu);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < kSmallPhase; ++j)
                    if (base + j < len)
                        out[j * kLanes] = model.step(byte_of(cur, j), 256u + base + j, j + 1u < kSmallPhase ? byte_of(cur, j + 1u) : nxt.w[0] & 0xFFu);
            }
        }
        lds_barrier();
    }
}

// MIDDLE and LOW: `lag` phases behind UPPER; bytes and the sums so far come through LDS, the sums go back in place
template <typename Model>
__device__ __forceinline__ void small_follow(EncodeSmallLds &lds, uint32_t lane, uint32_t len, uint32_t len_min, uint32_t n_phases, uint32_t lag) {
    Model model;
    model.open(lds.tree, 2u * lane_column(lane), 0u);
    for (uint32_t b = 0; b < lag; ++b) lds_barrier();
    for (uint32_t k = 0; k < n_phases; ++k) {
        const uint32_t base = k * kSmallPhase;
        uint32_t *io = &lds.sums[k % kSumSlots][0][lane];
        PhaseBytes w;
#pragma unroll
        for (uint32_t q = 0; q < kSmallPhase / 4; ++q) w.w[q] = lds.bytes[k % kByteBufs][q][lane];
        if (base + kSmallPhase <= len_min) {
            uint32_t part[kSmallPhase];
#pragma unroll
            for (uint32_t j = 0; j < kSmallPhase; ++j) part[j] = io[j * kLanes];
            model.prime(w.w[0] & 0xFFu);
#pragma unroll
            for (uint32_t j = 0; j < kSmallPhase; ++j)
                io[j * kLanes] = j + 1u < kSmallPhase ? model.step(byte_of(w, j), 256u + base + j, byte_of(w, j + 1u), part[j])
                                                      : model.step_last(byte_of(w, j), 256u + base + j, part[j]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kSmallPhase; ++j) {          // (unrolled: the byte's position must be static)
                const uint32_t x = byte_of(w, j);
                if (base + j < len) {
                    model.prime(x);
                    io[j * kLanes] = model.step_last(x, 256u + base + j, io[j * kLanes]);
                }
            }
        }
        lds_barrier();
    }
    for (uint32_t b = lag; b < kSmallLag; ++b) lds_barrier();
}

// SINK's body for a phase the lane owns completely
__device__ __forceinline__ void sink_whole_phase(CarrySinkLane &sink, const uint32_t *in_words) {
    uint32_t w[kSmallPhase];
#pragma unroll
    for (uint32_t j = 0; j < kSmallPhase; ++j) w[j] = in_words[j * kLanes];
#pragma unroll
    for (uint32_t j = 0; j < kSmallPhase; ++j) sink.take(w[j]);
}

__global__ void __launch_bounds__(kSmallWaves * kLanes)
encode_small_kernel(const uint8_t *__restrict__ src, size_t size, uint8_t *__restrict__ dst, uint32_t n_packets, uint32_t *__restrict__ status) {
    __shared__ EncodeSmallLds lds;
    const size_t group = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t packet = group * kLanes + lane;
    const bool live = packet < n_packets;
    const size_t start = packet * kPacket;
    const uint32_t len = live ? static_cast<uint32_t>(size - start < kPacket ? size - start : kPacket) : 0u;
    const uint32_t len_max = wave_max(len);
    const uint32_t len_min = wave_max(~len) ^ 0xFFFFFFFFu;
    const uint32_t n_phases = (len_max + kSmallPhase - 1) / kSmallPhase;
    const uint8_t *in = src + (live ? start : 0);
    // The dispatcher deals a workgroup's wavefronts round the four SIMDs: wavefronts 0 and 4 share one, 1 and 5 another;
    // the four tree roles pair up there (one's LDS operations issue under the other's vector instructions), the two
    // coder roles have a SIMD each.
    constexpr uint32_t kWaveInterval = 2u, kWaveSink = 3u, kWaveCourier = 6u;
    if (wave == 1u) {
        small_upper<2>(lds, in, lane, len, len_min, n_phases);
    } else if (wave == 4u) {
        small_follow<PartialModeler<7, 3, 2, 0, false>>(lds, lane, len, len_min, n_phases, 1u);
    } else if (wave == 5u) {
        small_follow<PartialModeler<7, 5, 2, 0, false>>(lds, lane, len, len_min, n_phases, 2u);
    } else if (wave == 0u) {
        small_follow<DeepestModeler<7>>(lds, lane, len, len_min, n_phases, 3u);
    } else if (wave == kWaveCourier) {
        // The last wavefront carries INTERVAL's reciprocals (as encode_kernel's fourth carries the coder's): the eight pairs
        // of a phase go into one of two slots in the tree's unused 256th row one barrier before INTERVAL reads them, so that
        // the wavefront that owns the interval chain never waits for a scalar load.
        constexpr uint32_t kPhaseDwords = 2u * kSmallPhase;
        const uint32_t *table = reinterpret_cast<const uint32_t *>(g_recip.r);
        const uint32_t mine = lane & (kPhaseDwords - 1u);
        uint32_t carried = table[mine];
        for (uint32_t t = 0; t < n_phases + kSmallLag; ++t) {
            // INTERVAL works on phase p during interval p + kSmallLag - 1 and reads slot p & 1: the pairs of phase
            // t + 2 - kSmallLag are written during interval t (one barrier ahead), those of the phase behind it asked for
            constexpr uint32_t kAhead = kSmallLag - 2u;
            if (lane < kPhaseDwords) lds.recips((t + kAhead) & 1u)[mine] = carried;
            const uint32_t next_phase = t + 1u >= kAhead && t + 1u - kAhead < n_phases ? t + 1u - kAhead : 0u;
            carried = table[next_phase * kPhaseDwords + mine];
            lds_barrier();
        }
    } else if (wave == kWaveInterval) {
        CarryIntervalLane interval;
        interval.open();
        for (uint32_t b = 0; b < kSmallLag - 1u; ++b) lds_barrier();
        for (uint32_t k = 0; k < n_phases; ++k) {
            const uint32_t base = k * kSmallPhase;
            const uint32_t *sums = &lds.sums[k % kSumSlots][0][lane];
            uint32_t *out = &lds.words[k & 1u][0][lane];
            if (base + kSmallPhase <= len_min) {
                uint32_t cums[kSmallPhase];
#pragma unroll
                for (uint32_t j = 0; j < kSmallPhase; ++j) cums[j] = sums[j * kLanes];
                Recip rc[kSmallPhase];
                {
                    const uint4 *slot = reinterpret_cast<const uint4 *>(lds.recips(k & 1u));
#pragma unroll
                    for (uint32_t q = 0; q < kSmallPhase / 2; ++q) {
                        const uint4 v = slot[q];
                        rc[2 * q] = {v.x, v.y}, rc[2 * q + 1] = {v.z, v.w};
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < kSmallPhase; ++j) out[j * kLanes] = interval.step(cums[j], rc[j]);
            } else {
#pragma unroll 1
                for (uint32_t j = 0; j < kSmallPhase; ++j) {
                    if (base + j >= len_max) break;
                    const Recip r = g_recip.r[base + j];
                    if (base + j < len) out[j * kLanes] = interval.step(sums[j * kLanes], r);
                }
            }
            lds_barrier();
        }
        lds_barrier();
    } else if (wave == kWaveSink) {
        CarrySinkLane sink;
        sink.open(dst + group * (kLanes * kSlot), lane * kSlot);
        for (uint32_t b = 0; b < kSmallLag; ++b) lds_barrier();
        for (uint32_t k = 0; k < n_phases; ++k) {
            const uint32_t base = k * kSmallPhase;
            const uint32_t *in_words = &lds.words[k & 1u][0][lane];
            if (base + kSmallPhase <= len_min) {
                sink_whole_phase(sink, in_words);
            } else {
#pragma unroll 1
                for (uint32_t j = 0; j < kSmallPhase; ++j)
                    if (base + j < len) sink.take(in_words[j * kLanes]);
            }
            lds_barrier();
        }
        finish_lane(sink, live, len, status);
    }
}

// ---- batch, latency mode: the roles of encode_small_kernel on the schedule of run_top<true> (phases of kSmallPhase symbols):
//      whole phases masked by each lane's own count of them, then one phase in which every lane codes its own partial phase
template <int kUpperDepths>
__device__ __forceinline__ void batch_small_upper(EncodeSmallLds &lds, const uint8_t *in, uint32_t lane, uint32_t len, uint32_t n_phases,
                                                  uint32_t whole_max) {
    PartialModeler<7, 1, kUpperDepths, 0, false> model;
    PhaseBytes cur, nxt = load_phase(in, 0, len);
    model.open(lds.tree, 2u * lane_column(lane), nxt.w[0] & 0xFFu);
    const uint32_t whole = len / kSmallPhase;
    uint32_t k = 0;
    for (; k < whole_max; ++k) {
        const uint32_t base = k * kSmallPhase;
        cur = nxt;
        nxt = load_phase(in, base + kSmallPhase, len);
#pragma unroll
        for (uint32_t q = 0; q < kSmallPhase / 4; ++q) lds.bytes[k % kByteBufs][q][lane] = cur.w[q];
        if (k < whole) {
            uint32_t *out = &lds.sums[k % kSumSlots][0][lane];
#pragma unroll
            for (uint32_t j = 0; j < kSmallPhase; ++j)
                out[j * kLanes] = model.step(byte_of(cur, j), 256u + base + j, j + 1u < kSmallPhase ? byte_of(cur, j + 1u) : nxt.w[0] & 0xFFu);
        }
        lds_barrier();
    }
    if (k < n_phases) {
        const uint32_t own = whole * kSmallPhase;
        cur = load_phase(in, own, len);
#pragma unroll
        for (uint32_t q = 0; q < kSmallPhase / 4; ++q) lds.bytes[k % kByteBufs][q][lane] = cur.w[q];
        uint32_t *out = &lds.sums[k % kSumSlots][0][lane];
#pragma unroll
        for (uint32_t j = 0; j < kSmallPhase; ++j)
            if (own + j < len) out[j * kLanes] = model.step(byte_of(cur, j), 256u + own + j, j + 1u < kSmallPhase ? byte_of(cur, j + 1u) : 0u);
        lds_barrier();
        ++k;
    }
    for (; k < n_phases + kSmallLag; ++k) lds_barrier();
}

template <typename Model>
__device__ __forceinline__ void batch_small_follow(EncodeSmallLds &lds, uint32_t lane, uint32_t len, uint32_t n_phases, uint32_t lag,
                                                   uint32_t whole_max) {
    Model model;
    model.open(lds.tree, 2u * lane_column(lane), 0u);
    for (uint32_t b = 0; b < lag; ++b) lds_barrier();
    const uint32_t whole = len / kSmallPhase;
    uint32_t k = 0;
    for (; k < whole_max; ++k) {                               // whole phases, each lane up to its own count
        if (k < whole) {
            const uint32_t base = k * kSmallPhase;
            uint32_t *io = &lds.sums[k % kSumSlots][0][lane];
            PhaseBytes w;
#pragma unroll
            for (uint32_t q = 0; q < kSmallPhase / 4; ++q) w.w[q] = lds.bytes[k % kByteBufs][q][lane];
            uint32_t part[kSmallPhase];
#pragma unroll
            for (uint32_t j = 0; j < kSmallPhase; ++j) part[j] = io[j * kLanes];
            model.prime(w.w[0] & 0xFFu);
#pragma unroll
            for (uint32_t j = 0; j < kSmallPhase; ++j)
                io[j * kLanes] = j + 1u < kSmallPhase ? model.step(byte_of(w, j), 256u + base + j, byte_of(w, j + 1u), part[j])
                                                      : model.step_last(byte_of(w, j), 256u + base + j, part[j]);
        }
        lds_barrier();
    }
    if (k < n_phases) {                                        // the deferred phase: the lane's own partial phase
        const uint32_t own = whole * kSmallPhase;
        uint32_t *io = &lds.sums[k % kSumSlots][0][lane];
        PhaseBytes w;
#pragma unroll
        for (uint32_t q = 0; q < kSmallPhase / 4; ++q) w.w[q] = lds.bytes[k % kByteBufs][q][lane];
#pragma unroll
        for (uint32_t j = 0; j < kSmallPhase; ++j) {            // (unrolled: the byte's position must be static)
            const uint32_t x = byte_of(w, j);
            if (own + j < len) {
                model.prime(x);
                io[j * kLanes] = model.step_last(x, 256u + own + j, io[j * kLanes]);
            }
        }
        lds_barrier();
    }
    for (uint32_t b = lag; b < kSmallLag; ++b) lds_barrier();
}

__device__ __forceinline__ void batch_small_roles(EncodeSmallLds &lds, size_t group, uint32_t lane, uint32_t wave, const uint8_t *in,
                                                  uint32_t len, bool live, uint8_t *__restrict__ dst, uint32_t *__restrict__ status) {
    const uint32_t whole_max = wave_max(len / kSmallPhase);
    const uint32_t n_phases = whole_max + (wave_max(len % kSmallPhase) ? 1u : 0u);
    const uint32_t whole = len / kSmallPhase;
    constexpr uint32_t kWaveInterval = 2u, kWaveSink = 3u, kWaveCourier = 6u;      // (encode_small_kernel's placement)
    if (wave == 1u) {
        batch_small_upper<2>(lds, in, lane, len, n_phases, whole_max);
    } else if (wave == 4u) {
        batch_small_follow<PartialModeler<7, 3, 2, 0, false>>(lds, lane, len, n_phases, 1u, whole_max);
    } else if (wave == 5u) {
        batch_small_follow<PartialModeler<7, 5, 2, 0, false>>(lds, lane, len, n_phases, 2u, whole_max);
    } else if (wave == 0u) {
        batch_small_follow<DeepestModeler<7>>(lds, lane, len, n_phases, 3u, whole_max);
    } else if (wave == kWaveCourier) {
        // encode_small_kernel's courier; it carries the pairs of the whole phases only (the deferred phase's are per lane)
        constexpr uint32_t kPhaseDwords = 2u * kSmallPhase;
        const uint32_t *table = reinterpret_cast<const uint32_t *>(g_recip.r);
        const uint32_t mine = lane & (kPhaseDwords - 1u);
        uint32_t carried = table[mine];
        for (uint32_t t = 0; t < n_phases + kSmallLag; ++t) {
            constexpr uint32_t kAhead = kSmallLag - 2u;
            if (lane < kPhaseDwords) lds.recips((t + kAhead) & 1u)[mine] = carried;
            const uint32_t next_phase = t + 1u >= kAhead && t + 1u - kAhead < whole_max ? t + 1u - kAhead : 0u;
            carried = table[next_phase * kPhaseDwords + mine];
            lds_barrier();
        }
    } else if (wave == kWaveInterval) {
        CarryIntervalLane interval;
        interval.open();
        for (uint32_t b = 0; b < kSmallLag - 1u; ++b) lds_barrier();
        uint32_t k = 0;
        for (; k < whole_max; ++k) {
            if (k < whole) {
                const uint32_t *sums = &lds.sums[k % kSumSlots][0][lane];
                uint32_t *out = &lds.words[k & 1u][0][lane];
                uint32_t cums[kSmallPhase];
#pragma unroll
                for (uint32_t j = 0; j < kSmallPhase; ++j) cums[j] = sums[j * kLanes];
                Recip rc[kSmallPhase];
                const uint4 *pairs = reinterpret_cast<const uint4 *>(lds.recips(k & 1u));
#pragma unroll
                for (uint32_t q = 0; q < kSmallPhase / 2; ++q) {
                    const uint4 v = pairs[q];
                    rc[2 * q] = {v.x, v.y}, rc[2 * q + 1] = {v.z, v.w};
                }
#pragma unroll
                for (uint32_t j = 0; j < kSmallPhase; ++j) out[j * kLanes] = interval.step(cums[j], rc[j]);
            }
            lds_barrier();
        }
        if (k < n_phases) {                                    // the lane's own partial phase, its own reciprocals
            const uint32_t own = whole * kSmallPhase;
            const uint32_t *sums = &lds.sums[k % kSumSlots][0][lane];
            uint32_t *out = &lds.words[k & 1u][0][lane];
#pragma unroll 1
            for (uint32_t j = 0; own + j < len; ++j) out[j * kLanes] = interval.step(sums[j * kLanes], g_recip.r[own + j]);
            lds_barrier();
        }
        lds_barrier();
    } else if (wave == kWaveSink) {
        CarrySinkLane sink;
        sink.open(dst + group * (kLanes * kSlot), lane * kSlot);
        for (uint32_t b = 0; b < kSmallLag; ++b) lds_barrier();
        uint32_t k = 0;
        for (; k < whole_max; ++k) {
            if (k < whole) sink_whole_phase(sink, &lds.words[k & 1u][0][lane]);
            lds_barrier();
        }
        if (k < n_phases) {
            const uint32_t *in_words = &lds.words[k & 1u][0][lane];
#pragma unroll 1
            for (uint32_t j = 0; whole * kSmallPhase + j < len; ++j) sink.take(in_words[j * kLanes]);
            lds_barrier();
        }
        finish_lane(sink, live, len, status);
    }
}

// Batch encode, latency mode (see encode_batch_kernel)
__global__ void __launch_bounds__(kSmallWaves * kLanes)
encode_small_batch_kernel(const uint8_t *const *__restrict__ ptrs, const uint64_t *__restrict__ bytes, const uint64_t *__restrict__ first_packet,
                          uint32_t n_buffers, uint32_t n_packets, uint8_t *__restrict__ dst, uint32_t *__restrict__ status) {
    __shared__ EncodeSmallLds lds;
    const size_t group = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t packet = group * kLanes + lane;
    bool live = packet < n_packets;
    BatchLane bl = {nullptr, 0u, false, 0u};
    if (live) {
        bl = batch_lane(ptrs, bytes, first_packet, n_buffers, packet);
        if (!bl.owned || bl.count == 0u) {
            live = false;
            if (wave == 0u) atomicOr(status, GPUAR_STATUS_BAD_BATCH);
        }
    }
    batch_small_roles(lds, group, lane, wave, live ? bl.ptr : nullptr, live ? bl.count : 0u, live, dst, status);
}

// ---------------------------------------------------------------------------
// Decode: replaces garDecompress + arDecompress (:916-934, 848-892)
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// The symbol step of the decoder, scheduled by hand for a wavefront that is ALONE on its SIMD
// (the per-packet model pins 36 KiB of LDS per wavefront, four wavefronts per CU).
//
// What tools/lat_probe.hip measures for such a wavefront (profiles/archive/r02_lat_probe.txt): every vector
// instruction costs one issue slot of 4.2-4.7 cycles whether or not it depends on its predecessor;
// `s_nop 0` costs a whole slot (4 cycles), `s_nop 1` two; a scalar instruction costs a slot as well;
// ds_read_b128 comes back after ~65 cycles and holds the issue port ~12, ds_write_b128 ~20.  So the
// step is priced in SLOTS, the two LDS round trips are free exactly when ~15 independent
// instructions sit behind each read, and anything the wavefront has to WAIT for is pure loss: a
// scalar load (thousands of cycles under load, and it can only be waited for with lgkmcnt(0)) or a
// vector load the whole wavefront waits for (~720 cycles under load, longer than the step) -- the
// loop below contains neither.  The compiler's own schedule of lane_codec.h's
// step_symbol spends ~135 slots per symbol (selects for the path bits, s_nop pads behind every lane
// mask it writes); the statements below spend 80 vector + 4.5 LDS (an even step and the odd one behind it: 82 + 4, 78 + 5).
//
//   R0 = off*total + total - 1; depths 0 and 1 (registers); READ #1 (mid record) issued
//       in its shadow: the half of the previous symbol's low record that its path took takes its increments
//       (one ds_add_u64: count +1, child +1 if left, grandchild +1 if left -- fields stay below 2^14, nothing
//       carries into a neighbour); even step: register nodes bumped, the stream reader's subtraction;
//       odd step: the stream reader moves on and reads its next dword
//   wait; mid record: 3 decisions; READ #2 (low record) issued
//       in its shadow: the mid record's half takes its increments the same way; even step: the stream window's selects and
//       refill; odd step: register nodes bumped
//   wait; low record: 3 decisions, the symbol's count for the upper bound; interval narrowed and renormalised;
//       off = ((off - dn) : window) << n   (which also steps the window over the n bits)
// What sits in which shadow was settled by timing (profiles/r06_decode_step_budget.txt): since round 6 both waits are worth
// 3-6 cycles, i.e. the step takes the time its instructions take to issue.
//
// Lane masks: v_sub_co writes "went left" as its borrow; v_min keeps the remainder; the mask is
// read two or more instructions later (path add-with-carry, selects of the next node and of the
// record update).  The LDS operands need aligned register quads / pairs and the 64-bit shift a
// pair: they are pinned (v200-v217); everything else is allocated by the compiler.  Both waits have
// the form "an LDS read, one LDS operation behind it, s_waitcnt lgkmcnt(1)" -- two and lgkmcnt(2) behind the odd step's
// first read, which has the stream read behind it as well -- (LDS operations of a wavefront complete in order).  Results are those of DecoderLane::step_symbol (same integers), which
// the CPU tests pin against the oracle; the GPU parity tests then compare this path with the oracle
// directly.
// ---------------------------------------------------------------------------
#define GPUAR_SDWA_W0 " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t"
#define GPUAR_SDWA_W1 " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD\n\t"
#define GPUAR_SDWA_HALVES " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1\n\t"

// One symbol of the hand-scheduled decoder (see above), in text pieces.  The step forms the whole 64-bit increment of
// its low half itself, in v204:v205, and the NEXT step applies it with one ds_add_u64 in the shadow of its first LDS read
// (profiles/archive/r03_decode_cost_attribution.txt: an LDS add costs this wavefront ~20 cycles to issue, a ds_write_b64 ~28, and
// the four vector instructions that used to rebuild the half's two dwords are gone; WAITED for, an LDS atomic is 60-440
// cycles dearer than a write, tools/lat_probe.hip).  One more instruction of a step waits for that shadow: clearing the
// top bit of lo (an instruction behind an LDS operation's issue costs this wavefront less than one in the chain; a variant
// that kept a select of the increment there needed a lane mask carried between statements in a scalar register).
// The same text serves the one wavefront of a file that holds its short last packet (lanes drop out under `if`).
// It uses decode_wave's locals by name.
// This section holds the shipped step only.  The placements that lost their A/B and the builds that priced the step by taking
// pieces out of it (profiles/r06_decode_step_budget.txt) were deleted once their numbers were written down in the comments
// below; their code is in git at 220c1c2.
// The model's total (256 + position, the same in every lane) reaches the step as a VECTOR register that the step itself counts up in
// an LDS shadow (round 6b).  Rounds 2-6a passed it as a scalar operand, which the compiler formed by one s_or per statement right in
// front of the step's first instruction -- on the chain, and a scalar instruction costs a lone wavefront a slot like any other.
#define GPUAR_TOTAL_STEP "v_add_u32 %[totv], 1, %[totv]\n\t" /* counted up in the first LDS shadow (in the second: the same) */
// A record read goes out as soon as its address is there: the remainder's minimum behind the decision in front of it (which the
// address does not need) is taken in the read's shadow (round 6b; in front of the read, as in rounds 2-6a: 24.06 against
// 23.87 ms).  The step's time is the vector instructions OUTSIDE the two LDS round trips + the round trips: both shadows are
// full (moving the instruction that files the symbol into the next step's first shadow changed nothing: 23.82 / 23.83 against
// 23.82 / 23.85), so only what shortens the stretch in front of a read still pays.
#define GPUAR_STEP_HEAD \
            "v_mul_u32_u24_sdwa %[R0], %[off], %[totv]" GPUAR_SDWA_W0 /* off = the low half of lo : off */ \
            "v_mul_u32_u24 %[t0], %[root], %[rng]\n\t" \
            "v_add3_u32 %[R0], %[R0], %[totv], -1\n\t" /* off*total + total - 1 */ \
            "v_sub_co_u32 %[t1], %[m0], %[R0], %[t0]\n\t" /* borrow = went left at depth 0 */ \
            "v_min_u32 %[R], %[R0], %[t1]\n\t" \
            "v_cndmask_b32 %[t2], %[h1], %[h0], %[m0]\n\t" /* the depth-1 node on the path */ \
            "v_mul_u32_u24 %[t0], %[t2], %[rng]\n\t" \
            "v_sub_co_u32 %[t1], %[m1], %[R], %[t0]\n\t" \
            "v_cndmask_b32 %[np], 0, 2, %[m0]\n\t" \
            "v_addc_co_u32 %[np], vcc, %[np], 0, %[m1]\n\t" /* complemented top two symbol bits */ \
            "v_lshl_add_u32 %[am], %[np], 10, %[col]\n\t" \
            "ds_read2_b64 v[200:203], %[am] offset1:64\n\t" /* READ #1: mid record, right half -> v200:201, left half -> v202:203 */ \
            "v_min_u32 %[R], %[R], %[t1]\n\t" /* (the remainder behind the second decision: the record's address does not need it) */

#define GPUAR_SHADOW_PLAIN \
         /* in its shadow: the half of the PREVIOUS symbol's low record its path went through takes its increments by ONE \
            64-bit LDS add (v204: +1 on the count, +0x10000 on the child if left; v205: the grandchild's, if left there); no field \
            can carry into its neighbour (counts stay below 2^14) */ \
            "ds_add_u64 %[oaddr], v[204:205]\n\t"
// The same with the previous symbol's low half ADDRESSED here -- one shift-add off the end of the chain into a shadow in which
// the wavefront waits anyway (round 4: 26.64 -> 26.42 ms).  Measured and not kept: the filing of the previous symbol here
// as well (its last decision's lane mask saved by s_mov_b64 and put back into vcc in front of the SDWA add-with-carry:
// 26.83 ms) and, on top of that, the three selects that form the half's increments, from saved lane masks (27.89 ms): a
// lane mask that travels vector -> scalar -> vector costs more than the instructions it moves off the chain; the filing
// alone with the mask re-made here from the grandchild's increment (v_cmp_ne 0, v205 -- two instructions here for one on the
// chain): +3 cycles, this shadow has no room left.
#define GPUAR_SHADOW_DEFERRED \
            "v_lshl_add_u32 %[oaddr], %[c6], 9, %[collow]\n\t" \
            "ds_add_u64 %[oaddr], v[204:205]\n\t"
// Where a step bumps its register nodes: in its first LDS shadow (rounds 2-5) or in its second (vcc and mj are free there too).
// The even step keeps them in the first shadow; the odd step -- whose first shadow holds the stream reader's move and read and
// whose second would otherwise wait -- bumps them in the second (round 6 A/B on uniform 8 GiB: 25.13 -> 24.76 ms; both steps in
// the second shadow 25.20, only the even step 25.59).  After this both waits of a step are worth 3-6 cycles: the step's time is
// its instructions' issue time (profiles/r06_decode_step_budget.txt).
#define GPUAR_REG_NODES \
         /* register nodes += went left: the root by the first decision's mask, of the two depth-1 nodes the one on the path by \
            the second one's -- which of them it is, is settled between the two lane masks by the scalar unit (both were written \
            a dozen instructions ago: no wait), so each node takes ONE add-with-carry (rounds 2-4: the chosen node's copy bumped, \
            then two selects to put it back) */ \
            "s_and_b64 %[sx], %[m0], %[m1]\n\t" \
            "s_andn2_b64 %[mj], %[m1], %[m0]\n\t" \
            "v_addc_co_u32 %[root], vcc, %[root], 0, %[m0]\n\t" \
            "v_addc_co_u32 %[h0], vcc, %[h0], 0, %[sx]\n\t" \
            "v_addc_co_u32 %[h1], vcc, %[h1], 0, %[mj]\n\t"

// (the path after the record's first decision stays in `np` -- the two later ones go on in t3 -- so that the address of the
// half that takes the increments is formed behind read #2, next to the LDS add that uses it, and not on the chain)
#define GPUAR_MID_WALK \
         /* ---- mid record: v200 = aR | bR << 16, v201 = cRR | cRL << 16 (right half), v202 = a | bL << 16, v203 = cLR | cLL << 16 (left half) */ \
            "v_mul_u32_u24_sdwa %[t0], v202, %[rng]" GPUAR_SDWA_W0 \
            "v_sub_co_u32 %[t1], %[ma], %[R], %[t0]\n\t" \
            "v_min_u32 %[R], %[R], %[t1]\n\t" \
            "v_cndmask_b32 %[bw], v200, v202, %[ma]\n\t" /* the half the path takes: count and chosen child ... */ \
            "v_cndmask_b32 %[cc], v201, v203, %[ma]\n\t" /* ... and its two children */ \
            "v_mul_u32_u24_sdwa %[t0], %[bw], %[rng]" GPUAR_SDWA_W1 \
            "v_sub_co_u32 %[t1], vcc, %[R], %[t0]\n\t" \
            "v_min_u32 %[R], %[R], %[t1]\n\t" \
            "v_addc_co_u32 %[np], %[mj], %[np], %[np], %[ma]\n\t" \
            "v_cndmask_b32_sdwa %[t2], %[cc], %[cc], vcc" GPUAR_SDWA_HALVES \
            "v_mul_u32_u24 %[t0], %[t2], %[rng]\n\t" \
            "v_sub_co_u32 %[t1], %[mc], %[R], %[t0]\n\t" \
            "v_addc_co_u32 %[t3], %[mj], %[np], %[np], vcc\n\t" \
            "v_addc_co_u32 %[t3], %[mj], %[t3], %[t3], %[mc]\n\t" \
            "v_lshl_add_u32 %[oaddr], %[t3], 10, %[collow]\n\t" \
            "ds_read2_b64 v[212:215], %[oaddr] offset1:64\n\t" /* READ #2: low record */ \
            "v_min_u32 %[R], %[R], %[t1]\n\t" \
         /* ---- the mid half takes its increments by one 64-bit LDS add in the shadow of read #2 */ \
            "v_lshl_add_u32 %[am], %[np], 9, %[col]\n\t" /* where that half lives: its index is the path up to the record's first decision */ \
            "v_cndmask_b32 v208, 1, %[k64k1], vcc\n\t" /* +1 on the half's count, +1 for bL/bR if left at the middle decision */ \
            "v_cndmask_b32 %[t2], 1, %[k64k], vcc\n\t" \
            "v_cndmask_b32 v209, 0, %[t2], %[mc]\n\t" \
            "ds_add_u64 %[am], v[208:209]\n\t"

// OWN_ADDRESS: the address of the step's own low half, formed at once (GPUAR_LOW_ADDRESS_NOW: the last symbol of a loop body)
// or left to the next step's first shadow (empty; GPUAR_SHADOW_DEFERRED)
#define GPUAR_LOW_ADDRESS_NOW \
            "v_lshl_add_u32 %[oaddr], %[c6], 9, %[collow]\n\t" /* the low half that takes the increments (in the next step's shadow) */
#define GPUAR_LOW_WALK(OWN_ADDRESS) \
         /* ---- low record: v212 = aR | bR << 16, v213 = cRR | cRL << 16 (right half), v214 = a | bL << 16, v215 = cLR | cLL << 16 (left half). \
                 Next to the walk (three decisions on the scaled remainder) the symbol's own COUNT is picked out of the half: \
                 under the chosen side there are `count` symbols (a or aR), `child` of them left of the child node, the \
                 grandchild node holds the left one of the two leaves: count -> (lb ? child : count - child) -> (lc ? gc : that - gc). \
                 Two subtractions and two selects off the chain, then cnt * range is added to cumLo * range: one instruction fewer \
                 than carrying the scaled upper bound through the walk (round 2: Z = R - V, a sum, a product, a difference and three maxima). */ \
            "v_mul_u32_u24_sdwa %[pa], v214, %[rng]" GPUAR_SDWA_W0 \
            "v_sub_co_u32 %[t1], %[lma], %[R], %[pa]\n\t" \
            "v_min_u32 %[R], %[R], %[t1]\n\t" \
            "v_cndmask_b32 %[lbw], v212, v214, %[lma]\n\t" \
            "v_cndmask_b32 %[lcc], v213, v215, %[lma]\n\t" \
            "v_mul_u32_u24_sdwa %[pb], %[lbw], %[rng]" GPUAR_SDWA_W1 \
            "v_sub_co_u32 %[t1], vcc, %[R], %[pb]\n\t" \
            "v_sub_u32_sdwa %[ps], %[lbw], %[lbw] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1\n\t" /* count - child: right of the child node */ \
            "v_min_u32 %[R], %[R], %[t1]\n\t" \
            "v_addc_co_u32 %[c6], %[mj], %[t3], %[t3], %[lma]\n\t" /* the path after six decisions (c6, c7: kept for the next step's shadow) */ \
            OWN_ADDRESS \
         /* everything that hangs on the MIDDLE decision (vcc) comes first: the last decision's lane mask goes to vcc as well, \
            because the instruction that files the symbol takes its carry from there */ \
            "v_cndmask_b32_sdwa %[t2], %[lcc], %[lcc], vcc" GPUAR_SDWA_HALVES \
            "v_cndmask_b32_sdwa %[ps], %[ps], %[lbw], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1\n\t" /* symbols under the chosen grandchild node */ \
            "v_mul_u32_u24 %[pc], %[t2], %[rng]\n\t" \
            "v_addc_co_u32 %[c7], %[mj], %[c6], %[c6], vcc\n\t" \
            "v_cndmask_b32 v204, 1, %[k64k1], vcc\n\t" /* the increments of the low half -> v204:v205 (added in the next step's shadow) */ \
            "v_cndmask_b32 %[ti], 1, %[k64k], vcc\n\t" \
            "v_sub_co_u32 %[t1], vcc, %[R], %[pc]\n\t" \
            "v_sub_u32 %[t3], %[ps], %[t2]\n\t" /* the right leaf */ \
            "v_min_u32 %[R], %[R], %[t1]\n\t" \
            "v_cndmask_b32 %[t3], %[t3], %[t2], vcc\n\t" /* cnt(symbol) */
#define GPUAR_LOW_INTERVAL(MUL) /* MUL: the name of the operand that holds this symbol's reciprocal multiplier */ \
         /* ---- applySymbolRange (:256-299) and the renormalisation (:787-836) */ \
            "v_sub_u32 %[t0], %[R0], %[R]\n\t" /* cumLo * range */ \
            "v_mad_u32_u24 %[t1], %[t3], %[rng], %[t0]\n\t" /* cumHi * range = cumLo * range + cnt * range */ \
            "v_mul_hi_u32 %[dn], %[t0], %[" MUL "]\n\t" \
            "v_mul_hi_u32 %[t1], %[t1], %[" MUL "]\n\t" \
            "v_lshrrev_b32 %[dn], %[shift], %[dn]\n\t" \
            "v_lshrrev_b32 %[t1], %[shift], %[t1]\n\t" \
            "v_mad_u32_u24 v217, %[dn], %[kffff], v217\n\t" /* lo : off -> (lo + dn) : (off - dn) in one: + dn * 0xFFFF (dn <= off, lo + dn < 2^16) */ \
            "v_sub_u32 %[wd], %[t1], %[dn]\n\t" /* new hi - new lo + 1 */ \
            "v_lshl_add_u32 %[t2], %[wd], 16, %[km32k]\n\t" /* (2 * width - 1) << 15: hi - lo with both one bit longer, at the top; its high half is width - 1 */ \
         /* (gfx950: a result written into HALF a register -- SDWA dst_sel -- may be read by the second instruction behind \
            its producer at the earliest; the assembler does not pad hand-written text, so the order below keeps that distance) */ \
            "v_add_u32_sdwa %[h], v217, %[t2] dst_sel:WORD_1 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1\n\t" /* new hi (high half) */ \
            "v_ffbh_u32 %[e], %[t2]\n\t" /* lane_codec.h renorm_count: n = that count - 1 + [the bounds differ at that bit] */ \
            "v_xor_b32_sdwa %[kff], v217, %[h] dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_1\n\t"

// The end of the step: the grandchild's increment sits between the SDWA write of kff and its reader; the last instruction
// but one files the symbol: all eight complemented path bits = 2 * (the first seven) + the last decision's borrow, written
// straight into byte J of the output word (SDWA dst_sel, the other bytes preserved) -- no shift-or per symbol.
#define GPUAR_STEP_END(N) /* N: the name of the operand this step leaves its bit count in ("ne" in an even step, "no" in an odd one) */ \
            "v_cndmask_b32 v205, 0, %[ti], vcc\n\t" \
            "v_lshlrev_b32 %[t2], %[e], %[kff]\n\t" \
            "v_lshrrev_b32 %[t2], 31, %[t2]\n\t" \
            "v_add3_u32 %[" N "], %[e], %[t2], -1\n\t" \
            "v_lshlrev_b32 %[rng], %[" N "], %[wd]\n\t"
// (not the statement's very last instruction: what reads the word behind the statement is the compiler's, and it does
// not know that the word was written by halves)
#define GPUAR_FILE_SYMBOL(J, WORD) \
            "v_addc_co_u32_sdwa %[" WORD "], vcc, %[c7], %[c7], vcc dst_sel:BYTE_" #J " dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"

// The stream reader.  What a step needs of the stream is the window v216: the next stream bits, left-aligned, of which the
// 64-bit shift at the end of the step (GPUAR_OFF_TEXT) moves the top n <= 16 into lo : off -- and leaves v216 = window << n,
// i.e. ALREADY stepped over the bits it took.  So v216 filled with 32 fresh bits lasts TWO symbols whatever they consume, and
// the reader runs at a fixed cadence, in all lanes alike, with no lane mask on exec.  (Rounds 1-5 refilled under a saved exec
// mask on every symbol -- 7 vector + 1 LDS + 2 scalar instructions per symbol, some lane needing it almost every time; now
// 10 + 1 + 0 per TWO symbols.)
//   EVEN step (symbols 0, 2, 4, ... of a block): the bits of the two symbols before it come off `rem` (unread bits of w0) in
//     one subtraction; its borrow says that w0 ran out: w1 moves up and takes the dword `ahead` (swapped to big-endian order
//     here); v216 = the 32 bits at `rem`.
//   ODD step: the lanes whose w0 ran out move their reader on by a dword, and every lane -- moved or not -- reads `ahead` again
//     from where its reader now stands (the lane's 64-byte ring in LDS, dword-major / lane-minor: dword d of lane l at ring
//     region + 256 * d + 4 * l, so the 64 lanes of a read hit 64 different banks whatever dwords they are at; `next` is the
//     byte offset of that dword times 64, i.e. already 256 * dword index; decode_wave keeps the ring filled).
// The even step's selects read the borrow as a lane mask (a scalar pair that only vector instructions read: nothing goes
// through the scalar unit); the odd step takes the same fact from the sign of the unwrapped difference, a vector register.  The read of `ahead` is never waited for by itself: it
// is older than the record reads of the next step, whose s_waitcnt lgkmcnt(1) (LDS operations complete in order) comes before
// the next even step looks at `ahead`.
// Where the pieces sit was settled by timing (profiles/r06_decode_step_budget.txt, uniform 8 GiB, one box, rounds 4-5's per-symbol
// reader 26.4-26.5 ms): the whole reader in the even step's second LDS shadow 25.8; split between the two steps' second shadows
// 25.8; the even step's subtraction moved to its first shadow 25.6; the odd step's part in ITS first shadow as well 25.2-25.3
// (kept); everything in first shadows 25.7.  A shadow hides three or four instructions, not ten.
#define GPUAR_STREAM_EVEN_TAKE /* the even step's first shadow */ \
            "v_add_u32 %[pc], %[no], %[ne]\n\t" /* the bits of the two symbols since the last refill: <= 32 */ \
            "v_sub_co_u32 %[raw], %[sb], %[rem], %[pc]\n\t" /* borrow: w0 ran out */ \
            "v_and_b32 %[rem], 31, %[raw]\n\t"
#define GPUAR_STREAM_EVEN_WINDOW /* the even step's second shadow */ \
            "v_perm_b32 %[pa], 0, %[ahead], %[bsw]\n\t" /* big-endian order restored */ \
            "v_cndmask_b32 %[w0], %[w0], %[w1], %[sb]\n\t" \
            "v_cndmask_b32 %[w1], %[w1], %[pa], %[sb]\n\t" \
            "v_alignbit_b32 v216, %[w0], %[w1], %[rem]\n\t" /* the next 32 stream bits */
#define GPUAR_STREAM_ODD_MOVE /* the odd step's first shadow: two LDS operations behind read #1 then, not one */ \
            "v_lshrrev_b32 %[pb], 31, %[raw]\n\t" /* the difference before it was wrapped: negative where w0 ran out */ \
            "v_lshl_add_u32 %[next], %[pb], 8, %[next]\n\t" \
            "v_and_or_b32 %[pc], %[next], %[kf00], %[ring]\n\t" /* ring + 256 * (dword index mod 16) */ \
            "ds_read_b32 %[ahead], %[pc]\n\t"

// lo' : off' = (((lo + dn) : (off - dn)) : window) << n, upper half, with lo's top bit cleared: ONE 64-bit shift moves both
// (v217 = lo << 16 | off, the window in v216).  What leaves lo at the top falls off the register; (off - dn + 1) << n
// <= width << n = range' <= 2^16 keeps the lower half inside its 16 bits; bit 31 is the last underflow position
// (lo' = (a << n) & 0x7FFF) and is cleared in the NEXT step's LDS shadow (GPUAR_SHADOW_*; decode_wave clears it once
// more behind the last step).
#define GPUAR_OFF_TEXT(N) \
            "v_lshlrev_b64 v[216:217], %[" N "], v[216:217]\n\t"

#define GPUAR_STEP_OPERANDS_COMMON \
              [R0] "=&v"(R0), [R] "=&v"(R), [np] "=&v"(np), [am] "=&v"(am), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), \
              [m0] "=&s"(m0), [m1] "=&s"(m1), [ma] "=&s"(ma), [mc] "=&s"(mc), [mj] "=&s"(mj), [sx] "=&s"(sx), [sb] "=&s"(sb), [raw] "+v"(rem_raw), \
              [root] "+v"(dec.model.root), [h0] "+v"(dec.model.half0), [h1] "+v"(dec.model.half1), \
              [rng] "+v"(dec.range), [off] "+v"(offr), [kff] "+v"(kff), [oaddr] "+v"(oaddr), \
              [rem] "+v"(dec.rem), [w0] "+v"(dec.w0), [w1] "+v"(dec.w1), [ahead] "+v"(dec.ahead), [next] "+v"(next64), "+v"(window), \
              [dn] "=&v"(dn), [bw] "=&v"(bw), [cc] "=&v"(cc), [pa] "=&v"(pa), [pb] "=&v"(pb), [pc] "=&v"(pc), [ps] "=&v"(ps), \
              [wd] "=&v"(wd), [h] "=&v"(h), [e] "=&v"(e)

#define GPUAR_STEP_LOCALS \
        uint32_t R0, R, np, am, t0, t1, t2, t3, dn, bw, cc, pa, pb, pc, ps, wd, h, e; \
        unsigned long long m0, m1, ma, mc, mj, sx, sb;

// The kinds of step in a loop body of 32 symbols.  By position: all but the last leave the address of their low half to the next
// step's first LDS shadow (the path after six decisions stays in a register of its own, `path6`), all but the first form it
// there for their predecessor.  By parity: even steps refill the stream window, odd steps live on what the even one left.
// J: the byte of its output word the step files its symbol in; MUL, WORD: the NAMES of the operands that hold the symbol's
// reciprocal multiplier and its output word (a run of eight steps is ONE asm statement, below); the step leaves the number of stream
// bits it took in "ne" (even steps) or "no" (odd steps): the even step's refill needs both.
// The two steps, their pieces in the order they execute.  SHADOW: GPUAR_SHADOW_PLAIN or _DEFERRED; OWN_ADDRESS: GPUAR_LOW_ADDRESS_NOW
// or empty.  LDS operations complete in order, so "read #N is back" is a wait for all but the operations issued behind it.
#define GPUAR_STEP_EVEN_TEXT(SHADOW, OWN_ADDRESS, J, MUL, WORD) \
    GPUAR_STEP_HEAD                                /* depths 0 and 1, READ #1 */ \
    SHADOW GPUAR_TOTAL_STEP GPUAR_REG_NODES GPUAR_STREAM_EVEN_TAKE \
    "s_waitcnt lgkmcnt(1)\n\t"                     /* read #1 is back; behind it: the low half's LDS add */ \
    GPUAR_MID_WALK                                 /* mid walk, READ #2, the mid half's LDS add */ \
    GPUAR_STREAM_EVEN_WINDOW \
    "s_waitcnt lgkmcnt(1)\n\t"                     /* read #2 is back; behind it: the mid half's LDS add */ \
    GPUAR_LOW_WALK(OWN_ADDRESS) GPUAR_LOW_INTERVAL(MUL) GPUAR_STEP_END("ne") GPUAR_FILE_SYMBOL(J, WORD) GPUAR_OFF_TEXT("ne")
#define GPUAR_STEP_ODD_TEXT(SHADOW, OWN_ADDRESS, J, MUL, WORD) \
    GPUAR_STEP_HEAD \
    SHADOW GPUAR_TOTAL_STEP GPUAR_STREAM_ODD_MOVE \
    "s_waitcnt lgkmcnt(2)\n\t"                     /* read #1 is back; behind it: the low half's LDS add AND the stream reader's dword */ \
    GPUAR_MID_WALK \
    GPUAR_REG_NODES \
    "s_waitcnt lgkmcnt(1)\n\t"                     /* read #2 is back; behind it: the mid half's LDS add */ \
    GPUAR_LOW_WALK(OWN_ADDRESS) GPUAR_LOW_INTERVAL(MUL) GPUAR_STEP_END("no") GPUAR_FILE_SYMBOL(J, WORD) GPUAR_OFF_TEXT("no")
// (every step forming its own address, as in rounds 2-4a: 26.64 against 26.42 ms, see GPUAR_SHADOW_DEFERRED)
#define GPUAR_STEP_FIRST(J, MUL, WORD) GPUAR_STEP_EVEN_TEXT(GPUAR_SHADOW_PLAIN, , J, MUL, WORD)
#define GPUAR_STEP_EVEN(J, MUL, WORD) GPUAR_STEP_EVEN_TEXT(GPUAR_SHADOW_DEFERRED, , J, MUL, WORD)
#define GPUAR_STEP_ODD(J, MUL, WORD) GPUAR_STEP_ODD_TEXT(GPUAR_SHADOW_DEFERRED, , J, MUL, WORD)
#define GPUAR_STEP_LAST(J, MUL, WORD) GPUAR_STEP_ODD_TEXT(GPUAR_SHADOW_DEFERRED, GPUAR_LOW_ADDRESS_NOW, J, MUL, WORD)

// LDS of a decoder workgroup (one wavefront): the 64 models and the 64 stream rings, 40 KiB -> four per CU.
constexpr uint32_t kRingPieces = 4;                        // 16-byte pieces per lane: 64 bytes of stream
constexpr uint32_t kDecodeLdsQuads = (kDecodeRecords + kRingPieces) * kLanes;

// `base` is the same in every lane (4-byte aligned); lane offsets are 32-bit.  `col` = this lane's 8-byte
// column of the workgroup's LDS (72 half-records, 512 bytes apart); `ring` = this lane's dword 0 in the 4 KiB
// stream-ring region behind the records (16 dwords per lane, 256 bytes apart; the region is 4 KiB-aligned).
// kBatch, `room`: the bytes the lane's output may take (a batch buffer's rest); a packet whose ulen exceeds it is BAD_PACKET
// and writes nothing.
template <bool kBatch = false>
__device__ __forceinline__ void decode_wave(uint8_t *col, uint8_t *ring, const uint8_t *base, uint32_t pkt_off, uint32_t limit_off,
                                            uint8_t *out, bool live, uint32_t *status, uint32_t room = kPacket) {
    DecoderLane<9> dec;
    dec.template open<kBatch>(col, base, pkt_off, limit_off, live, room);
    const uint32_t len_max = wave_max(dec.ulen);
    // Whole blocks of 64 symbols: the 64 output bytes gather in 16 registers and leave as four
    // back-to-back 16-byte stores, i.e. one whole 64-byte sector of this lane's output line
    // at a time (dword-at-a-time stores from 64 lanes at an 8 KiB stride were
    // measured to cost ~10x the output bytes in HBM writes: every partial
    // sector left L2 before its neighbours arrived).  A lane that does not own the whole block -- a
    // dead lane of the last wavefront, the file's short last packet -- sits the block out with its
    // state untouched (plain SIMT divergence), so one such lane no longer slows the other 63 down.
    uint32_t i = 0;

    // ---- state of the hand-scheduled step ----
    const uint32_t col_lds = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(col));   // LDS byte address of this lane's column
    const uint32_t ring_lds = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(ring));  // ... and of dword 0 of its stream ring
    // the refill's address arithmetic ORs a dword index into bits 8-11: the ring region must start on a 4 KiB
    // boundary of LDS (the kernels' only __shared__ array is declared that way); anything else is a build error
    // that would decode garbage, so the wavefront flags every packet bad and decodes nothing instead
    if ((ring_lds & 0xF00u) != 0u) {
        atomicOr(status, GPUAR_STATUS_BAD_PACKET);
        return;
    }
    register uint32_t o0 asm("v204");          // the increments the previous symbol's low half still has to take (v204:v205)
    register uint32_t o1 asm("v205");
    register uint32_t offr asm("v217");        // lo << 16 | (code - lo): v216:v217 is the pair the 64-bit shift works on, and
    offr = dec.off | (dec.lo << 16);           // lower bound and code offset move through the step as ONE register
    // the stream bits the last two symbols took and the reader has not stepped over yet: the even step's and the odd step's, a
    // register each (GPUAR_STREAM_EVEN_TAKE takes both off `rem` at once)
    uint32_t n_even = 0, n_odd = dec.owed_bits;
    uint32_t total_v = 256u;                   // the model's total as a vector register (the same in every lane): GPUAR_TOTAL_STEP
    uint32_t rem_raw = 0;                      // the even step's `rem` before it was wrapped into 0..31: negative where w0 ran out -- the odd step
                                               // behind it moves those lanes' reader on (a vector register: nothing crosses statements as a lane mask)
    register uint32_t window asm("v216");      // the stream bits in front of the reader, left-aligned: filled by every even step, shifted
    asm volatile("v_mov_b32 %0, 0" : "=v"(window));       // on by every step (the low half of the pair the 64-bit shift works on)
    const uint32_t col_low_lds = col_lds + SubtreeModel<9>::kLowBase;               // ... and of its first low half
    uint32_t oaddr = col_lds + dec.model.owed.at;                                   // where the half owed goes
    // (No check for "a code value no symbol owns" -- off >= range, where the reference stops decoding, :873-877 -- in
    // this loop: it cannot happen, whatever the bits are.  off < range holds at the start (off < 2^16 = range); the walk
    // finds s with cumLo*range <= R0 < cumHi*range for R0 = (off + 1)*total - 1 < range*total; then
    // dn = floor(cumLo*range/total) <= off and (off + 1)*total <= cumHi*range gives off + 1 <= up, so
    // 0 <= off - dn < up - dn = width, and appending n stream bits to both keeps ((off - dn) : bits) << n below
    // width << n.  Round 2 carried a per-symbol minimum for it; 65 million symbols of garbage never raised it.  The
    // reference decodes every packet of tests/damage_sweep.py to its full ulen, as this argument says it must.)
    uint32_t kff = 0xFFFFu;                    // low half stays 0xFFFF, high half is scratch of the renormalisation
    const uint32_t k64k = 0x10000u, k64k1 = 0x10001u;
    const uint32_t minus_half = 0xFFFF8000u;               // (2 * width - 1) << 15 = (width << 16) + this: see renorm_count
    uint32_t bswap_sel, ring_wrap, low_half;
    asm volatile("s_mov_b32 %0, 0xffff" : "=s"(low_half));
    asm volatile("s_mov_b32 %0, 0x00010203" : "=s"(bswap_sel));     // (through asm: a known constant would be spliced in as a literal)
    asm volatile("s_movk_i32 %0, 0xf00" : "=s"(ring_wrap));        // 256 * 15: the ring's dword index, scaled

    // ---- the stream ring ----
    // The step takes its stream dwords from a per-lane ring of 64 bytes in LDS, NOT from memory: a load from
    // memory that every symbol waits for (whichever lane asked for it) makes the symbol as long as a
    // round trip to L2, which at full load is LONGER than the step itself (~740 against ~600 cycles).
    // The ring is refilled here, every eight symbols, in pieces of 16 bytes that are asked for one phase
    // (eight symbols) before they are written to LDS: the vector-memory wait is for something issued
    // ~4000 cycles ago.  Offsets are counted from base16 = base rounded down to 16 bytes, so pieces are
    // aligned (an aligned piece that holds one readable byte never crosses a page); past the end of what
    // may be read the last such piece is repeated (a well-formed packet decodes the same whatever follows).
    // Unlike DecoderLane::fetch it is not masked: a damaged packet read past the end sees that piece, its
    // bytes behind the end included, again and again instead of zeros (include/gpuar_hip.h,
    // garDecompressExecutor; tests/test_gpu_damaged.py part 4).  Masking it costs: a build whose phase masked the
    // landed piece in place (a v_cmp, s_and_saveexec, s_cbranch_execz and s_or per phase; the masks themselves on the
    // rare path only) decoded the bench workload in 24.30 / 24.29 ms against 23.95 / 23.91 ms unmasked, interleaved
    // runs on one MI355X: +1.5 %, against run-to-run noise of about 0.04 ms.
    // A lane consumes at most 16 bits per symbol (n = e + u <= 16: range' = width << n <= 2^16, whatever the
    // bits are) = 16 bytes per phase of EIGHT symbols (rounds 1-3 reckoned with 31 bits and ran the phase every
    // four), a phase brings 16.  The reader's position A is the offset of the dword `ahead` holds, as of the last even step
    // (which has taken off the bits of all symbols before it): that dword is read AGAIN at every even step until the reader
    // moves on, so everything from A on must stay in the ring.  Asking for piece P = `fill` once fill - A <= 48: (1) the piece
    // P overwrites, P - 64, ends at or below A when P is written a phase later (A only grows); (2) the gap fill - A at a phase
    // never falls below 33 (49 or more and nothing is asked for: the next phase sees 16 less at most; below that a piece is asked
    // for and the gap keeps its size), while the even steps up to the next phase read dwords below A + 16 + 4 <= fill, all
    // written by then.  The ring starts full from the piece that holds `ahead` (gap >= 49).
    const uint32_t skew16 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(base) & 15u);
    const uint8_t *base16 = base - skew16;
    const uint32_t next16 = dec.next + skew16;                   // offset from base16 of the dword after `ahead` ...
    // ... and, times 64 (bits 8-11 = 256 * (dword index mod 16)), of the dword `ahead` holds itself: the even step reads
    // `ahead` again from where the reader stands whether or not it has moved
    uint32_t next64 = (next16 - 4u) << 6;
    const uint32_t last_piece = (dec.last + skew16) & ~15u;
    const uint32_t first_piece = (next16 - 4u) & ~15u;           // the piece that holds `ahead`'s dword: the ring starts there
    uint32_t fill = first_piece + 16u * kRingPieces;             // offset of the next piece to ask for
    // piece `at` (a multiple of 16) = dwords 4p .. 4p+3 of the ring, p = (at / 16) mod 4: two ds_write2st64_b32
    register uint32_t q0 asm("v220");          // the piece asked for last (in flight, or already in the ring:
    register uint32_t q1 asm("v221");          // writing it a second time is harmless) ...
    register uint32_t q2 asm("v222");
    register uint32_t q3 asm("v223");
    uint32_t slot_lds = ring_lds;              // ... and the LDS address of its dword 0
#pragma unroll
    for (uint32_t k = 0; k < kRingPieces; ++k) {
        const uint32_t at = first_piece + 16u * k;
        const Quad q = load128(base16 + (at < last_piece ? at : last_piece));
        uint32_t *slot = reinterpret_cast<uint32_t *>(ring + ((at & 0x30u) << 6));
        slot[0] = q.w[0], slot[64] = q.w[1], slot[128] = q.w[2], slot[192] = q.w[3];
        if (k == kRingPieces - 1u) {
            q0 = q.w[0], q1 = q.w[1], q2 = q.w[2], q3 = q.w[3];
            slot_lds = ring_lds + ((at & 0x30u) << 6);
        }
    }
    // One phase, by hand (the compiler's version of it, two divergent branches and their bookkeeping, was 24 issue
    // slots per four symbols): the piece asked for last is (re)written to its place, then the lanes whose reader
    // is within 48 bytes of `fill` ask for the next piece -- a predicated region without a branch around it.
    // s_waitcnt vmcnt(0): the piece was asked for a phase ago; the block's output stores drain here as well.
// ... and, since round 4, the reciprocal multipliers of the run AFTER NEXT: eight dwords by two loads with a wave-uniform
// address (`mulbase` = the half block's first multiplier, a scalar pair; OFF = byte offset of that run) that put the same
// value into every lane of the eight registers of set SET (v224 + 8 * SET ..., named in the text as two tuples; the compiler
// knows them as the pinned variables m<SET>0..7) -- where the step's two v_mul_hi_u32 take it from directly.  The
// loads land before the next phase's s_waitcnt vmcnt(0), one whole run before they are used.  (Rounds 2-3 kept symbol j's
// multiplier in lane j of ONE register per block of 64 and fetched it with a v_readlane per symbol.)
// (the phase is the tail of its run's asm statement -- GPUAR_DECODE_RUN8 --: it shares the run's operands `next`, `ring`, `t2`, `sx`)
#define GPUAR_RING_PHASE_TEXT(TUPLE_LO, TUPLE_HI)                                                                    \
            "v_lshrrev_b32 %[rt], 6, %[next]\n\t"                                                                    \
            "v_sub_u32 %[rt], %[fill], %[rt]\n\t"                                                                    \
            "v_cmp_gt_u32 vcc, 49, %[rt]\n\t" /* (first: the scalar unit reads this mask five instructions later) */ \
            "s_waitcnt vmcnt(0)\n\t"                                                                                 \
            "ds_write2st64_b32 %[slot], v220, v221 offset1:1\n\t"                                                    \
            "ds_write2st64_b32 %[slot], v222, v223 offset0:2 offset1:3\n\t"                                          \
            "global_load_dwordx4 " TUPLE_LO ", %[zero], %[mulbase] offset:%[roff]\n\t"                               \
            "global_load_dwordx4 " TUPLE_HI ", %[zero], %[mulbase] offset:%[roff]+16\n\t"                            \
            "s_and_saveexec_b64 %[sx], vcc\n\t"                                                                      \
            "v_min_u32 %[rt], %[fill], %[lastp]\n\t"                                                                 \
            "global_load_dwordx4 v[220:223], %[rt], %[base]\n\t"                                                     \
            "v_and_b32 %[t2], 48, %[fill]\n\t"                                                                       \
            "v_lshl_add_u32 %[slot], %[t2], 6, %[ring]\n\t"                                                          \
            "v_add_u32 %[fill], 16, %[fill]\n\t"                                                                     \
            "s_or_b64 exec, exec, %[sx]"

    // The per-symbol reciprocal multipliers (wave-uniform) reach the symbol step WITHOUT scalar loads and -- since round 4 --
    // without a v_readlane: the ring phase above fetches the eight of the run after next into registers by vector loads
    // with a wave-uniform address (every lane gets the same dword), four sets of eight registers taking turns; the shift
    // that goes with a multiplier is the same for all 64 symbols of a block (RecipTable) and follows from the block's first
    // total; the model total is simply counted up.  Scalar loads were the costliest thing in this loop: a scalar load that
    // misses its cache goes to L2 like everything else, and while 1024 wavefronts stream their packets in and their
    // output out that round trip is thousands of cycles; it counts in lgkmcnt with the LDS operations, can
    // only be waited for with lgkmcnt(0), and even issued eight symbols ahead of its use it cost ~80 of
    // ~720 cycles per symbol (one group ahead: ~175 of 830; measured by taking the table walk out,
    // tools/kind_timing.py).  The waits of the symbol step have the form "an LDS read, one LDS operation
    // behind it, s_waitcnt lgkmcnt(1)", which holds whatever else is in flight.
    // four sets of eight pinned registers, v224 + 8 * set + j: set s holds the multipliers of run s of a half block
    register uint32_t m00 asm("v224"); register uint32_t m01 asm("v225"); register uint32_t m02 asm("v226"); register uint32_t m03 asm("v227"); register uint32_t m04 asm("v228"); register uint32_t m05 asm("v229"); register uint32_t m06 asm("v230"); register uint32_t m07 asm("v231");
    register uint32_t m10 asm("v232"); register uint32_t m11 asm("v233"); register uint32_t m12 asm("v234"); register uint32_t m13 asm("v235"); register uint32_t m14 asm("v236"); register uint32_t m15 asm("v237"); register uint32_t m16 asm("v238"); register uint32_t m17 asm("v239");
    register uint32_t m20 asm("v240"); register uint32_t m21 asm("v241"); register uint32_t m22 asm("v242"); register uint32_t m23 asm("v243"); register uint32_t m24 asm("v244"); register uint32_t m25 asm("v245"); register uint32_t m26 asm("v246"); register uint32_t m27 asm("v247");
    register uint32_t m30 asm("v248"); register uint32_t m31 asm("v249"); register uint32_t m32 asm("v250"); register uint32_t m33 asm("v251"); register uint32_t m34 asm("v252"); register uint32_t m35 asm("v253"); register uint32_t m36 asm("v254"); register uint32_t m37 asm("v255");
    uint32_t vzero;                                             // (a zero the compiler does not know: the loads' vector offset)
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
// Eight symbols (two output words) and the ring phase behind them, as ONE asm statement; RUN (0..3) is the run's static position
// in the half block.  (Rounds 2-6a: a statement per symbol.  Between two statements the compiler puts what it likes -- the s_or
// that formed the symbol's total, the halves of an s_add_u32 / s_addc_u32 pair, a wait state for a store hazard the statement
// next door cannot have -- and every scalar instruction or s_nop there is a slot on the chain: 24.9 -> 24.4 ms for the total as a
// self-counting vector register, and the rest with the statements joined.)
// scc is clobbered: s_and_b64 / s_andn2_b64 / s_and_saveexec_b64 / s_or_b64 write it, and the compiler DOES keep a carry alive
// across a statement when it has such a pair to spread (a build without the per-statement s_or faulted on exactly that).
#define GPUAR_DECODE_RUN8(RUN, FIRST_KIND, LAST_KIND, WORD_A, WORD_B, SET_AHEAD, TUPLE_LO, TUPLE_HI)                         \
        {                                                                                                            \
            GPUAR_STEP_LOCALS                                                                                        \
            uint32_t lbw_, lcc_, ti_, path7_, rt_;                                                                   \
            unsigned long long lma_;                                                                                 \
            asm volatile(                                                                                            \
                FIRST_KIND(0, "mul0", "wa") GPUAR_STEP_ODD(1, "mul1", "wa") GPUAR_STEP_EVEN(2, "mul2", "wa") GPUAR_STEP_ODD(3, "mul3", "wa") \
                GPUAR_STEP_EVEN(0, "mul4", "wb") GPUAR_STEP_ODD(1, "mul5", "wb") GPUAR_STEP_EVEN(2, "mul6", "wb") LAST_KIND(3, "mul7", "wb") \
                /* ... and the phase fetches the multipliers of the run after next: 8 * (RUN + 2) dwords behind the half block's first */ \
                GPUAR_RING_PHASE_TEXT(TUPLE_LO, TUPLE_HI)                                                            \
                : GPUAR_STEP_OPERANDS_COMMON,                                                                        \
                  [lbw] "=&v"(lbw_), [lcc] "=&v"(lcc_), [ti] "=&v"(ti_), [lma] "=&s"(lma_), [wa] "+v"(WORD_A), [wb] "+v"(WORD_B),     \
                  "+v"(o0), "+v"(o1), [c6] "+v"(path6), [c7] "=&v"(path7_), [ne] "+v"(n_even), [no] "+v"(n_odd), [totv] "+v"(total_v), \
                  [slot] "+v"(slot_lds), [fill] "+v"(fill), [rt] "=&v"(rt_), "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3),               \
                  "=v"(m##SET_AHEAD##0), "=v"(m##SET_AHEAD##1), "=v"(m##SET_AHEAD##2), "=v"(m##SET_AHEAD##3),                     \
                  "=v"(m##SET_AHEAD##4), "=v"(m##SET_AHEAD##5), "=v"(m##SET_AHEAD##6), "=v"(m##SET_AHEAD##7)                      \
                : [mul0] "v"(m##RUN##0), [mul1] "v"(m##RUN##1), [mul2] "v"(m##RUN##2), [mul3] "v"(m##RUN##3),                     \
                  [mul4] "v"(m##RUN##4), [mul5] "v"(m##RUN##5), [mul6] "v"(m##RUN##6), [mul7] "v"(m##RUN##7),                     \
                  [shift] "s"(block_shift), [col] "v"(col_lds), [collow] "v"(col_low_lds), [ring] "v"(ring_lds),                  \
                  [k64k] "v"(k64k), [k64k1] "v"(k64k1), [bsw] "s"(bswap_sel), [kf00] "s"(ring_wrap), [km32k] "s"(minus_half), [kffff] "s"(low_half), \
                  [lastp] "v"(last_piece), [base] "s"(base16), [zero] "v"(vzero), [mulbase] "s"(mul_base), [roff] "n"(32 * ((RUN) + 2))   \
                : "vcc", "scc", "memory", "v200", "v201", "v202", "v203", "v208", "v209", "v212", "v213", "v214", "v215");         \
        }
// A block of 64 symbols as two half blocks of 32: the loop body is 32 symbols long, so every output word has a register
// of its own by name -- rounds 1-3 looped over runs of eight and filed each word into a register array by index (a
// v_not, an s_set_gpr_idx_on / v_mov / s_set_gpr_idx_off and a scalar add per word, 1.5 issue slots per symbol, plus
// the loop's own six per eight symbols).
#define GPUAR_DECODE_BLOCK                                                                                           \
    {                                                                                                                \
        /* the shift that goes with the multipliers: floor(log2(total)) - 1, the same for all 64 totals of a block */ \
        const uint32_t block_shift = 30u - static_cast<uint32_t>(__builtin_clz(256u + i));                           \
        total_v = 256u + i; /* the model's total at the block's first symbol; every step counts it up */              \
        asm volatile("" : "+v"(total_v));                                                                            \
        _Pragma("unroll 1") for (uint32_t half = 0; half < 2u; ++half) {                                             \
            const uint32_t *mul_base = g_mul.m + i + 32u * half; /* wave-uniform: a scalar pair */                  \
            /* what a step leaves to the next one's first shadow: the path after six decisions (written by every step of   */ \
            /* the body, read by all but the first; defined here, for the compiler, without an instruction)                */ \
            uint32_t path6;                                                                                          \
            asm volatile("" : "=v"(path6));                                                                          \
            GPUAR_DECODE_RUN8(0, GPUAR_STEP_FIRST, GPUAR_STEP_ODD, w0, w1, 2, "v[240:243]", "v[244:247]")            \
            GPUAR_DECODE_RUN8(1, GPUAR_STEP_EVEN, GPUAR_STEP_ODD, w2, w3, 3, "v[248:251]", "v[252:255]")             \
            GPUAR_DECODE_RUN8(2, GPUAR_STEP_EVEN, GPUAR_STEP_ODD, w4, w5, 0, "v[224:227]", "v[228:231]")             \
            GPUAR_DECODE_RUN8(3, GPUAR_STEP_EVEN, GPUAR_STEP_LAST, w6, w7, 1, "v[232:235]", "v[236:239]")            \
            /* the block's 64 bytes leave TOGETHER, as four back-to-back 16-byte stores (a whole 64-byte sector: with two */ \
            /* stores per half block the L2 wrote 5 % and fetched 9 % more than the bytes): the first half's words wait,    */ \
            /* complemented, in k0..k7 (the path bits are the COMPLEMENTED symbol bits)                                     */ \
            if (half == 0u) {                                                                                        \
                k0 = ~w0, k1 = ~w1, k2 = ~w2, k3 = ~w3, k4 = ~w4, k5 = ~w5, k6 = ~w6, k7 = ~w7;                      \
            } else {                                                                                                 \
                uint4 *dst = reinterpret_cast<uint4 *>(out + i);                                                     \
                dst[0] = make_uint4(k0, k1, k2, k3);                                                                 \
                dst[1] = make_uint4(k4, k5, k6, k7);                                                                 \
                dst[2] = make_uint4(~w0, ~w1, ~w2, ~w3);                                                             \
                dst[3] = make_uint4(~w4, ~w5, ~w6, ~w7);                                                             \
            }                                                                                                        \
        }                                                                                                            \
    }

    // ---- blocks that every lane of the wavefront owns: uniform control flow ----
    const uint32_t len_min = wave_max(~dec.ulen) ^ 0xFFFFFFFFu;
    // v204:v205 = the 64-bit increment the previous symbol's low half still has to take (added in the shadow of the
    // next step's first read); nothing is owed yet: an add of zero to the half reset() named.
    // (Initial values go through asm: a known constant would be spliced into the statements as an immediate.)
    asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0" : "=v"(o0), "=v"(o1));
    // the eight output words of a half block (every byte of each is written before it is read; defined once for the compiler)
    uint32_t w0, w1, w2, w3, w4, w5, w6, w7;
    uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0, k4 = 0, k5 = 0, k6 = 0, k7 = 0;     // the first half block's words, until the second half's are there
    asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 0\n\tv_mov_b32 %3, 0\n\tv_mov_b32 %4, 0\n\tv_mov_b32 %5, 0\n\tv_mov_b32 %6, 0\n\tv_mov_b32 %7, 0"
                 : "=v"(w0), "=v"(w1), "=v"(w2), "=v"(w3), "=v"(w4), "=v"(w5), "=v"(w6), "=v"(w7));
    // the multipliers of the packet's first two runs (symbols 0..15); from then on every run fetches those of the run after next
    asm volatile("global_load_dwordx4 v[224:227], %[zero], %[mulbase]\n\t"
                 "global_load_dwordx4 v[228:231], %[zero], %[mulbase] offset:16\n\t"
                 "global_load_dwordx4 v[232:235], %[zero], %[mulbase] offset:32\n\t"
                 "global_load_dwordx4 v[236:239], %[zero], %[mulbase] offset:48\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=v"(m00), "=v"(m01), "=v"(m02), "=v"(m03), "=v"(m04), "=v"(m05), "=v"(m06), "=v"(m07),
                   "=v"(m10), "=v"(m11), "=v"(m12), "=v"(m13), "=v"(m14), "=v"(m15), "=v"(m16), "=v"(m17)
                 : [zero] "v"(vzero), [mulbase] "s"(static_cast<const uint32_t *>(g_mul.m))
                 : "memory");
    for (; i + 64u <= len_min; i += 64u) {
        GPUAR_DECODE_BLOCK
    }
    // ---- the remaining whole blocks of a wavefront whose lanes differ in length (the file's short last packet,
    //      dead lanes of the last wavefront): lanes that do not own the block sit it out ----
    for (; i + 64u <= len_max; i += 64u) {
        if (i + 64u <= dec.ulen) GPUAR_DECODE_BLOCK
    }
#undef GPUAR_DECODE_BLOCK
#undef GPUAR_DECODE_RUN8

#undef GPUAR_RING_PHASE_TEXT
    // hand the state back to the plain step (the tail below, finish()); `ahead` may still be on its way from the ring
    // (and a piece the last ring phase asked for may still be on its way into v220-v223)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(dec.ahead), "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3) : : "memory");
    dec.next = (next64 >> 6) + 4u - skew16;    // (next64 is the offset of `ahead`'s own dword, dec.next of the one behind it)
    dec.off = offr & 0xFFFFu;
    dec.lo = (offr >> 16) & 0x7FFFu;           // (the step leaves lo's top bit to the next step's shadow)
    dec.owed_bits = n_even + n_odd;            // what the last two symbols took is still to be stepped over (skip() takes up to 32 bits at once)
    // the increment still owed goes in now; what the plain step is then handed as "owed" is a rewrite of that half with
    // the values it holds (its write_back stores, it does not add)
    asm volatile("ds_add_u64 %[oaddr], v[204:205]\n\ts_waitcnt lgkmcnt(0)" : "+v"(o0), "+v"(o1) : [oaddr] "v"(oaddr) : "memory");
    dec.model.owed.at = oaddr - col_lds;
    {
        const Pair now = load64(col + dec.model.owed.at);
        dec.model.owed.w0 = now.w[0], dec.model.owed.w1 = now.w[1];
    }
    // the last, partial block of a packet whose length is not a multiple of 64 (at most one per file,
    // unless the packets are malformed): symbol by symbol, only the lanes that are inside such a block
    const uint32_t part_from = dec.ulen & ~63u;
    const uint32_t part_end = wave_max((dec.ulen & 63u) ? dec.ulen : 0u);
    const uint32_t part_begin = wave_max((dec.ulen & 63u) ? ~part_from : 0u) ^ 0xFFFFFFFFu;   // min over those lanes
    for (i = part_begin; i < part_end; ++i) {
        const DecodeConst k = g_decode.c[i];
        if (i >= part_from && i < dec.ulen) dec.step(i, k, out);
    }
    if (live) {
        dec.finish(out);
        if (dec.bad) atomicOr(status, GPUAR_STATUS_BAD_PACKET);
    }
}

// A group's slots (wave-uniform base) and what the lane may read: its slot, cut short where the `n_bytes` of slots end
// (the last slot of garDecompressExecutor's `size` bytes may be a partial one, src/gpuar_kernel.cu:916-934)
__device__ __forceinline__ const uint8_t *group_slots(const uint8_t *slots, size_t n_bytes, uint32_t lane, uint32_t &limit_off) {
    const size_t group_at = static_cast<size_t>(blockIdx.x) * (kLanes * kSlot);
    const uint8_t *base = slots + group_at;                                                       // wave-uniform
    const size_t group_left = n_bytes - group_at;
    const uint32_t slot_end = (lane + 1u) * kSlot;
    limit_off = group_left < slot_end ? static_cast<uint32_t>(group_left) : slot_end;
    return base;
}

__global__ void __launch_bounds__(kLanes)
decode_slots_kernel(const uint8_t *__restrict__ slots, uint32_t n_packets, size_t n_bytes, uint8_t *__restrict__ out, uint32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(4096))) uint4 lds[kDecodeLdsQuads];    // 40 KiB: 72 half-records x 64 lanes x 8 B, then 4 KiB of stream rings
    const uint32_t lane = threadIdx.x;
    const size_t packet = static_cast<size_t>(blockIdx.x) * kLanes + lane;
    const bool live = packet < n_packets;
    uint32_t limit_off;
    const uint8_t *base = group_slots(slots, n_bytes, lane, limit_off);
    clock_sample(1u, blockIdx.x, lane, 0u);
    decode_wave(reinterpret_cast<uint8_t *>(lds) + 8u * lane, reinterpret_cast<uint8_t *>(lds + kDecodeRecords * kLanes) + 4u * lane, base, lane * kSlot, limit_off,
                out + (live ? packet : 0) * static_cast<size_t>(kPacket), live, status);
    clock_sample(1u, blockIdx.x, lane, 1u);
}

// Decode from a back-to-back packet stream (the bytes after the 20-byte .gip
// header): lane p starts at stream + offsets[p].
__global__ void __launch_bounds__(kLanes)
decode_stream_kernel(const uint8_t *__restrict__ stream, const uint64_t *__restrict__ offsets,
                     uint32_t n_packets, uint8_t *__restrict__ out, uint32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(4096))) uint4 lds[kDecodeLdsQuads];
    const uint32_t lane = threadIdx.x;
    const size_t packet = static_cast<size_t>(blockIdx.x) * kLanes + lane;
    const bool live = packet < n_packets;
    // wave-uniform base: the (4-byte aligned) start of this group's first packet
    const uint64_t first = offsets[static_cast<size_t>(blockIdx.x) * kLanes] & ~3ull;
    const uint32_t first_hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(first >> 32))));
    const uint32_t first_lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(first))));
    const uint8_t *group_stream = stream + ((static_cast<uint64_t>(first_hi) << 32) | first_lo);
    const uint64_t left = offsets[n_packets] - first;                       // bytes from the base to the end of the stream
    const uint32_t limit_off = left < 0x7FFFFFFFull ? static_cast<uint32_t>(left) : 0x7FFFFFFFu;
    const uint32_t pkt_off = live ? static_cast<uint32_t>(offsets[packet] - first) : 0u;
    clock_sample(1u, blockIdx.x, lane, 0u);
    decode_wave(reinterpret_cast<uint8_t *>(lds) + 8u * lane, reinterpret_cast<uint8_t *>(lds + kDecodeRecords * kLanes) + 4u * lane, group_stream, pkt_off, limit_off,
                out + (live ? packet : 0) * static_cast<size_t>(kPacket), live, status);
    clock_sample(1u, blockIdx.x, lane, 1u);
}

// The output of a batch packet (gpuar_hip_decode_batch, decode_stream_batch): packet j of buffer b writes at outs[b] + j * 8192
// and has the buffer's rest from there, at most 8192 bytes, as its room.  A packet no buffer owns, that lies past its
// buffer's end, or whose buffer is misaligned is a dead lane (BAD_BATCH, nothing written), as in the batch encoders.
__device__ __forceinline__ bool batch_output(uint8_t *const *outs, const uint64_t *out_bytes, const uint64_t *first_packet, uint32_t n_buffers,
                                             size_t packet, bool live, uint8_t *&out, uint32_t &room, uint32_t *status) {
    out = nullptr;
    room = 0u;
    if (!live) return false;
    const BatchLane bl = batch_lane(reinterpret_cast<const uint8_t *const *>(outs), out_bytes, first_packet, n_buffers, packet);
    if (!bl.owned || bl.count == 0u) {
        atomicOr(status, GPUAR_STATUS_BAD_BATCH);
        return false;
    }
    out = const_cast<uint8_t *>(bl.ptr);
    room = bl.count;
    return true;
}

// decode_slots_kernel over the slots of a batch: slot p = batch packet p, lane p % 64 of group p / 64 (the slot addressing
// and the hand-scheduled step are decode_slots_kernel's; only the output pointer and the room check are per lane)
__global__ void __launch_bounds__(kLanes)
decode_slots_batch_kernel(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ first_packet, uint32_t n_buffers, uint32_t n_packets,
                          uint8_t *const *__restrict__ outs, const uint64_t *__restrict__ out_bytes, uint32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(4096))) uint4 lds[kDecodeLdsQuads];
    const uint32_t lane = threadIdx.x;
    const size_t packet = static_cast<size_t>(blockIdx.x) * kLanes + lane;
    uint32_t limit_off;
    const uint8_t *base = group_slots(slots, static_cast<size_t>(n_packets) * kSlot, lane, limit_off);
    uint8_t *out;
    uint32_t room;
    const bool live = batch_output(outs, out_bytes, first_packet, n_buffers, packet, packet < n_packets, out, room, status);
    decode_wave<true>(reinterpret_cast<uint8_t *>(lds) + 8u * lane, reinterpret_cast<uint8_t *>(lds + kDecodeRecords * kLanes) + 4u * lane, base, lane * kSlot, limit_off,
                      out, live, status, room);
}

// decode_stream_kernel over the compacted stream of a batch: offsets in batch order, as gpuar_hip_compact of the batch's
// slots produced them, so consecutive packets of a group are still adjacent (wave-uniform base, 32-bit lane offsets)
__global__ void __launch_bounds__(kLanes)
decode_stream_batch_kernel(const uint8_t *__restrict__ stream, const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ first_packet,
                           uint32_t n_buffers, uint32_t n_packets, uint8_t *const *__restrict__ outs, const uint64_t *__restrict__ out_bytes,
                           uint32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(4096))) uint4 lds[kDecodeLdsQuads];
    const uint32_t lane = threadIdx.x;
    const size_t packet = static_cast<size_t>(blockIdx.x) * kLanes + lane;
    const bool in_range = packet < n_packets;
    const uint64_t first = offsets[static_cast<size_t>(blockIdx.x) * kLanes] & ~3ull;
    const uint32_t first_hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(first >> 32))));
    const uint32_t first_lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(first))));
    const uint8_t *group_stream = stream + ((static_cast<uint64_t>(first_hi) << 32) | first_lo);
    const uint64_t left = offsets[n_packets] - first;                       // bytes from the base to the end of the stream
    const uint32_t limit_off = left < 0x7FFFFFFFull ? static_cast<uint32_t>(left) : 0x7FFFFFFFu;
    const uint32_t pkt_off = in_range ? static_cast<uint32_t>(offsets[packet] - first) : 0u;
    uint8_t *out;
    uint32_t room;
    const bool live = batch_output(outs, out_bytes, first_packet, n_buffers, packet, in_range, out, room, status);
    decode_wave<true>(reinterpret_cast<uint8_t *>(lds) + 8u * lane, reinterpret_cast<uint8_t *>(lds + kDecodeRecords * kLanes) + 4u * lane, group_stream, pkt_off, limit_off,
                      out, live, status, room);
}

// ---------------------------------------------------------------------------
// Compaction: exclusive scan of the packet lengths, then a gather of the
// defined bytes of every slot into one back-to-back stream.
// ---------------------------------------------------------------------------
constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kScanItems = 16;                        // packets per thread
constexpr uint32_t kScanTile = kScanThreads * kScanItems;  // 4096 packets per block
// Per-tile sums/prefixes live at the start of the OUTPUT stream buffer until the gather overwrites
// it (one u64 per 4096 packets, and the stream holds >= 4 bytes per packet): no global scratch,
// so compactions on different streams or devices never share state.  A single tile needs no prefix
// and gets no scratch (tile_prefix == nullptr): one packet of clen < 8 would otherwise have its
// scratch word run past the end of the stream (tests/test_gpu_lengths.py::
// test_compact_equals_a_plain_concatenation[1]).

__device__ __forceinline__ uint32_t slot_clen(const uint8_t *slots, size_t p) {
    return *reinterpret_cast<const uint16_t *>(slots + p * kSlot);
}

template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T &block_total) {
    __shared__ T wave_sums[kScanThreads / kLanes];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T other = __shfl_up(incl, off);
        if (lane >= static_cast<uint32_t>(off)) incl += other;
    }
    if (lane == 63u) wave_sums[wave] = incl;
    __syncthreads();
    T before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScanThreads / kLanes; ++w) {
        const T s = wave_sums[w];
        before += (w < wave) ? s : T(0);
        total += s;
    }
    __syncthreads();
    block_total = total;
    return before + incl - v;
}

__global__ void __launch_bounds__(kScanThreads)
scan_tile_sums_kernel(const uint8_t *__restrict__ slots, uint32_t n_packets, uint64_t *__restrict__ tile_prefix) {
    const size_t first = static_cast<size_t>(blockIdx.x) * kScanTile + threadIdx.x * kScanItems;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < kScanItems; ++k)
        if (first + k < n_packets) sum += slot_clen(slots, first + k);
    uint32_t total;
    block_exclusive_scan(sum, total);
    if (threadIdx.x == 0) tile_prefix[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kScanThreads)
scan_tile_prefix_kernel(uint32_t n_tiles, uint64_t *__restrict__ tile_prefix) {   // one block
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_tiles; base += kScanThreads) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t v = t < n_tiles ? tile_prefix[t] : 0;
        // a tile sum fits 32 bits (4096 * 8704); sums over tiles need 64
        uint64_t total;
        const uint64_t excl = block_exclusive_scan<uint64_t>(v, total);
        const uint64_t start = carry;
        if (t < n_tiles) tile_prefix[t] = start + excl;
        __syncthreads();
        if (threadIdx.x == 0) carry = start + total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kScanThreads)
scan_offsets_kernel(const uint8_t *__restrict__ slots, uint32_t n_packets, uint64_t *__restrict__ offsets,
                    const uint64_t *__restrict__ tile_prefix) {
    const size_t first = static_cast<size_t>(blockIdx.x) * kScanTile + threadIdx.x * kScanItems;
    uint32_t lens[kScanItems];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        lens[k] = (first + k < n_packets) ? slot_clen(slots, first + k) : 0u;
        sum += lens[k];
    }
    uint32_t total;
    uint64_t run = (tile_prefix ? tile_prefix[blockIdx.x] : 0ull) + block_exclusive_scan(sum, total);
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) {
        if (first + k < n_packets) offsets[first + k] = run;
        run += lens[k];
        if (first + k + 1 == n_packets) offsets[n_packets] = run;
    }
}

// One workgroup of 256 threads moves one packet, 16 bytes per lane and round (three rounds for a packet of uniform data,
// two for text): destination-aligned stores, the source read through byte-exact unaligned loads.  Rounds 1-3 gave
// every packet ONE wavefront that looped over it (four packets per workgroup): 3.43 ms for the 8.66 GB stream of the
// bench workload, 5.0 TB/s read + write; with a workgroup per packet (measured, uniform / text 8 GiB: 192 threads 3.37 /
// 2.14 ms, 256: 3.00 / 2.03, 320: 2.90 / 2.15, 384: 2.93 / 2.17, 448: 3.03 / 2.25, 576 = one quad per thread: 3.26 /
// 2.70) it is 5.76 TB/s = 72 % of the datasheet's 8 TB/s, 93 % of what a plain copy reaches on this part (6.18 TB/s).
constexpr uint32_t kGatherThreads = 256;
__global__ void __launch_bounds__(kGatherThreads)
gather_kernel(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ offsets, uint32_t n_packets,
              uint8_t *__restrict__ stream) {
    const size_t packet = blockIdx.x;
    const uint8_t *src = slots + packet * kSlot;
    const uint64_t off = offsets[packet];
    const uint32_t len = static_cast<uint32_t>(offsets[packet + 1] - off);
    uint8_t *dst = stream + off;
    // head: bytes up to the first 16-byte boundary of dst
    uint32_t head = static_cast<uint32_t>((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    if (head > len) head = len;
    const uint32_t body = (len - head) & ~15u;
    const uint32_t tail = len - head - body;
    for (uint32_t at = threadIdx.x * 16u; at < body; at += kGatherThreads * 16u) {
        uint4 v;
        __builtin_memcpy(&v, src + head + at, 16);
        *reinterpret_cast<uint4 *>(dst + head + at) = v;
    }
    // the ragged ends: 32 lanes of the last wavefront
    const uint32_t spare = threadIdx.x - (kGatherThreads - 32u);
    if (spare < head) dst[spare] = src[spare];
    else if (spare >= 16u && spare - 16u < tail) dst[head + body + spare - 16u] = src[head + body + spare - 16u];
}

// ---------------------------------------------------------------------------
// Synthetic input streams; bench/test support.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix_word(uint64_t seed, uint64_t k) {
    uint64_t z = seed + k * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256)
generate_uniform_kernel(uint64_t seed, uint64_t first_word, size_t n, uint8_t *__restrict__ out) {
    const size_t w = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    const size_t at = w * 8u;
    if (at >= n) return;
    const uint64_t v = splitmix_word(seed, first_word + w + 1u);
    if (at + 8u <= n) {
        *reinterpret_cast<uint64_t *>(out + at) = v;
    } else {
        for (size_t b = 0; at + b < n; ++b) out[at + b] = static_cast<uint8_t>(v >> (8u * b));
    }
}

struct ZipfTable {
    uint32_t cum[256];
    uint8_t sym[256];
};

// K ranks, weight floor(2^24 / r); each thread makes 8 bytes from 4 words
__global__ void __launch_bounds__(256)
generate_zipf_kernel(uint64_t seed, uint64_t first_word, size_t n, uint8_t *__restrict__ out,
                     ZipfTable table, uint32_t K) {
    __shared__ uint32_t cum[256];
    __shared__ uint8_t sym[256];
    cum[threadIdx.x] = threadIdx.x < K ? table.cum[threadIdx.x] : 0xFFFFFFFFu;
    sym[threadIdx.x] = table.sym[threadIdx.x];
    __syncthreads();
    const uint64_t W = table.cum[K - 1];
    const size_t g = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;  // group of 4 words = 8 bytes
    const size_t at = g * 8u;
    if (at >= n) return;
    uint64_t packed = 0;
    for (uint32_t j = 0; j < 4; ++j) {
        const uint64_t word = splitmix_word(seed, first_word + g * 4u + j + 1u);
        for (uint32_t h = 0; h < 2; ++h) {
            const uint64_t u = h ? (word >> 32) : (word & 0xFFFFFFFFull);
            const uint32_t t = static_cast<uint32_t>((u * W) >> 32);
            uint32_t lo = 0, hi = K;   // first index with cum[idx] > t
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (cum[mid] > t) hi = mid; else lo = mid + 1;
            }
            packed |= static_cast<uint64_t>(sym[lo]) << (8u * (2u * j + h));
        }
    }
    if (at + 8u <= n) {
        *reinterpret_cast<uint64_t *>(out + at) = packed;
    } else {
        for (size_t b = 0; at + b < n; ++b) out[at + b] = static_cast<uint8_t>(packed >> (8u * b));
    }
}

// ---------------------------------------------------------------------------
// The roof bench.py quotes next to the datasheet's: a plain device-to-device copy, 16 bytes per lane, ONE quad per thread
// and one 4 KiB tile per workgroup ("confirm a practical peak on the box with a device-to-device
// copy and report both").  Of the shapes tried (tools/copy_probe.hip, profiles/r04_copy_probe.txt: hipMemcpyAsync 4.8 TB/s,
// grid-stride loops with 4-8 loads in flight 4.7-5.2, tiles of 4 or 8 quads per thread 3.7-5.6) this, the simplest one,
// is the fastest: 6.18 TB/s read + write on 8 GiB.  Measurement support, not part of the codec path.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
copy_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n_quads) {
    const size_t q = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (q < n_quads) dst[q] = src[q];
}

// ---------------------------------------------------------------------------
// Per-packet CRC-32 (crc32.h): compute (crc[p] = CRC of packet p's uncompressed bytes) and verify (recompute,
// compare with crc[p]: GPUAR_STATUS_CHECKSUM and an atomic min of p on a mismatch), for one buffer or a batch.
//
// One wavefront per packet, lane l on bytes [128 l, 128 l + 128), slicing-by-4 (four table reads per word).  The four tables
// sit in LDS 32 times over, bank-private: entry x of copy b is at dword (x * 32 + b), and lane l reads copy l % 32, so every
// ds_read_b32 of a 32-lane half hits 32 distinct banks whatever the data (one table for all lanes conflicts 3-4 ways).  That
// is 128 KiB: one workgroup of 16 wavefronts per CU, persistent over the packets (16 x 8 KiB of loads in flight per CU hide
// the memory latency without a second buffer per wavefront).  A full packet's lanes shift their raw CRCs by the GF(2) matrices of CrcLaneColumns
// (kept in registers); a packet of 1-8191 bytes takes the general path: partial words byte by byte, the shift by
// crc_mulmod with the constant of its own distance.  Nothing is read beyond the 16-byte piece that holds a packet's last
// byte.  Separate kernels, not fused into the codec kernels (their schedules are pinned: DESIGN.md 4.3b).
// ---------------------------------------------------------------------------
__device__ const CrcTables g_crc_tables = CrcTables();
__device__ const CrcShiftTable g_crc_shift = CrcShiftTable();
__device__ const CrcLaneColumns g_crc_columns = CrcLaneColumns();
constexpr uint32_t kCrcWaves = 16;
constexpr uint32_t kCrcGroups = 256;       // one workgroup per CU of an MI355X (the LDS allows no second one)

struct CrcArgs {
    const uint8_t *in;                      // one buffer: `in`, `n_bytes` ...
    size_t n_bytes;
    const uint8_t *const *ptrs;             // ... or a batch (ptrs != nullptr)
    const uint64_t *bytes;
    const uint64_t *first_packet;
    uint32_t n_buffers;
    uint32_t n_packets;
    uint32_t *crc;                          // compute: written; verify: read
    unsigned long long *first_bad;          // verify: lowest mismatching packet (may be null)
    uint32_t *status;
};

struct CrcPacket {
    const uint8_t *ptr;
    uint32_t count;                         // 0: no packet (or an unusable batch descriptor)
};

__device__ __forceinline__ CrcPacket crc_locate(const CrcArgs &a, uint32_t packet) {
    CrcPacket r = {nullptr, 0u};
    if (!a.ptrs) {
        const size_t at = static_cast<size_t>(packet) * kPacket;
        r.ptr = a.in + at;
        r.count = a.n_bytes - at < kPacket ? static_cast<uint32_t>(a.n_bytes - at) : kPacket;
        return r;
    }
    const BatchLane bl = batch_lane(a.ptrs, a.bytes, a.first_packet, a.n_buffers, packet);
    if (bl.owned && bl.count) r.ptr = bl.ptr, r.count = bl.count;
    return r;
}

// lane's quads of a packet: quad k (bytes 128 lane + 16 k ..) where it starts before the packet's end, else zeros.  (A pointer
// read from the batch descriptors is generic to the compiler: it is named global here, so that the loads are global_ ones.)
typedef uint32_t CrcQuad __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void crc_load(CrcQuad (&q)[8], const CrcPacket &p, uint32_t lane) {
    using GlobalQuad = const __attribute__((address_space(1))) CrcQuad;
    GlobalQuad *src = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(p.ptr + kCrcChunk * lane));
    if (p.count == kPacket) {
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) q[k] = src[k];
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) q[k] = kCrcChunk * lane + 16u * k < p.count ? src[k] : CrcQuad(0u);
    }
}

// how many of the lane's 128 bytes lie inside a packet of `count` bytes
__device__ __forceinline__ uint32_t lane_have(uint32_t count, uint32_t lane) {
    const uint32_t start = kCrcChunk * lane;
    return count > start ? (count - start < kCrcChunk ? count - start : kCrcChunk) : 0u;
}

// one slicing-by-4 step; tab: the lane's copy (dword x * 32 of table t at t * 8192)
__device__ __forceinline__ uint32_t crc_word(const uint32_t *tab, uint32_t c, uint32_t w) {
    c ^= w;
    return tab[(3u * 256u + (c & 255u)) * 32u] ^ tab[(2u * 256u + ((c >> 8) & 255u)) * 32u] ^
           tab[(256u + ((c >> 16) & 255u)) * 32u] ^ tab[(c >> 24) * 32u];
}

__device__ __forceinline__ uint32_t crc_byte(const uint32_t *tab, uint32_t c, uint32_t b) {
    return tab[((c ^ b) & 255u) * 32u] ^ (c >> 8);
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
    return v;
}

// the packet's CRC-32 (in every lane)
__device__ __forceinline__ uint32_t crc_packet(const uint32_t *tab, const CrcQuad (&q)[8], uint32_t count, uint32_t lane, const uint32_t (&col)[32]) {
    uint32_t c = lane == 0u ? 0xFFFFFFFFu : 0u;          // lane 0 carries the initial value through the whole packet
    if (count == kPacket) {                              // wave-uniform
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            c = crc_word(tab, c, q[k].x);
            c = crc_word(tab, c, q[k].y);
            c = crc_word(tab, c, q[k].z);
            c = crc_word(tab, c, q[k].w);
        }
        uint32_t s = 0;
#pragma unroll
        for (uint32_t i = 0; i < 32; ++i) s ^= col[i] & (0u - ((c >> i) & 1u));
        c = s;
    } else {
        const uint32_t start = kCrcChunk * lane;      // (lane_have, written out: through the function crc32_kernel gains an instruction)
        const uint32_t have = count > start ? (count - start < kCrcChunk ? count - start : kCrcChunk) : 0u;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t at = 16u * k + 4u * j;
                if (at + 4u <= have) {
                    c = crc_word(tab, c, w[j]);
                } else {
                    for (uint32_t b = 0; at + b < have; ++b) c = crc_byte(tab, c, (w[j] >> (8u * b)) & 255u);
                }
            }
        }
        const uint32_t behind = have ? count - start - have : 0u;     // (a lane past the end has c = 0 and reads k[0])
        c = crc_mulmod(c, g_crc_shift.k[behind]);
    }
    return wave_xor(c) ^ 0xFFFFFFFFu;
}

template <bool Verify>
__global__ void __launch_bounds__(kCrcWaves * kLanes)
crc32_kernel(CrcArgs a) {
    __shared__ uint32_t lds[4 * 256 * 32];
    for (uint32_t e = threadIdx.x; e < 4u * 256u * 32u; e += kCrcWaves * kLanes) lds[e] = g_crc_tables.t[e >> 13][(e >> 5) & 255u];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t col[32];
#pragma unroll
    for (uint32_t i = 0; i < 32; ++i) col[i] = g_crc_columns.c[i][lane];
    __syncthreads();
    const uint32_t *tab = lds + (lane & 31u);
    const uint32_t stride = gridDim.x * kCrcWaves;
    // (n_packets <= 2^32 - 1 and stride <= 4096: the index wraps only past the last packet, which `packet < next` catches)
    for (uint32_t packet = blockIdx.x * kCrcWaves + (threadIdx.x >> 6), next; packet < a.n_packets; packet = next) {
        next = packet + stride;
        const CrcPacket p = crc_locate(a, packet);
        if (p.count == 0u) {
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
        } else {
            CrcQuad q[8];
            crc_load(q, p, lane);
            const uint32_t crc = crc_packet(tab, q, p.count, lane, col);
            if (lane == 0u) {
                if (!Verify) {
                    a.crc[packet] = crc;
                } else if (crc != a.crc[packet]) {
                    atomicOr(a.status, GPUAR_STATUS_CHECKSUM);
                    if (a.first_bad) atomicMin(a.first_bad, static_cast<unsigned long long>(packet));
                }
            }
        }
        if (next < packet) break;
    }
}

// ---------------------------------------------------------------------------
// Byte-plane splitting (planes.h): pure data movement in front of the encoder (split) and behind the decoder
// (merge), for one buffer or a batch with one element width per buffer.
//
// Full groups: one workgroup of 512 threads per packet; the workgroup of a group's FIRST packet moves the whole group
// (w packets), the others return.  A thread owns one block of 16 elements: 16 w mixed bytes = w quads back to back on the
// mixed side, one quad of every plane on the other, regrouped in registers by byte permutes (planes_block: v_perm_b32; no
// LDS).  So the plane side is read or written perfectly coalesced and the mixed side w quads per lane, 16-byte accesses
// on both.  Every thread holds its loads in registers before the workgroup's barrier and stores behind it: the group is
// read completely before any of it is written, which is what lets `out` be `in`.
// The tail of a buffer (n mod G bytes: fewer than w packets) is planes_tail_kernel's, one workgroup per buffer through
// LDS: by quads in (never beyond the 16-byte piece that holds the buffer's last byte), by dwords and bytes out (never
// beyond byte n), again all loads before any store.
// Separate launches, not fused into the codec kernels (their schedules are pinned: DESIGN.md 4.3b).
// ---------------------------------------------------------------------------
constexpr uint32_t kPlaneThreads = kPlanePacket / kPlaneBlock;        // 512: a block of 16 elements per thread
constexpr uint32_t kPlaneGridCap = GPUAR_PLANE_GRID_CAP;              // workgroups per launch (they stride over the packets): planes.h; the launch code alone reads it

struct PlanesArgs {
    const uint8_t *in;                      // one buffer: `in`, `out`, `n_bytes`, `elem` ...
    uint8_t *out;
    size_t n_bytes;
    uint32_t elem;
    const uint8_t *const *in_ptrs;          // ... or a batch (in_ptrs != nullptr)
    uint8_t *const *out_ptrs;
    const uint64_t *bytes;
    const uint64_t *first_packet;
    const uint64_t *elem_bytes;
    uint32_t n_buffers;
    uint32_t n_packets;
    uint32_t *status;
};

// A batch buffer the transform can take: both pointers 16-byte aligned, a width of 1, 2, 4 or 8, and exactly the packets its
// bytes make (a group is moved as a whole, so a buffer that owns only some of its packets is refused as a whole).
struct PlanesBuffer {
    const uint8_t *in;
    uint8_t *out;
    uint64_t n_bytes;
    uint32_t w;                             // 0: unusable
};
__device__ __forceinline__ PlanesBuffer planes_buffer(const PlanesArgs &a, uint32_t b) {
    PlanesBuffer r = {a.in_ptrs[b], a.out_ptrs[b], a.bytes[b], 0u};
    const uint64_t w = a.elem_bytes[b];
    const uint64_t owns = a.first_packet[b + 1u] - a.first_packet[b];
    const bool aligned = ((reinterpret_cast<uintptr_t>(r.in) | reinterpret_cast<uintptr_t>(r.out)) & 15u) == 0u;
    if (aligned && (w == 1u || w == 2u || w == 4u || w == 8u) && owns == (r.n_bytes + kPacket - 1u) / kPacket) r.w = static_cast<uint32_t>(w);
    return r;
}

typedef uint32_t PlanesQuad __attribute__((ext_vector_type(4)));
using PlanesGlobalQuad = __attribute__((address_space(1))) PlanesQuad;
using PlanesGlobalWord = __attribute__((address_space(1))) uint32_t;
using PlanesGlobalHalf = __attribute__((address_space(1))) uint16_t;
using PlanesGlobalByte = __attribute__((address_space(1))) uint8_t;
// ... and what is read at less than its own alignment: out of a slot (4-byte aligned) or a compacted stream (any byte)
typedef uint32_t KindsQuad4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at a 4-byte-aligned address
typedef uint32_t KindsQuad1 __attribute__((ext_vector_type(4), aligned(1)));      // ... and at any address
typedef uint32_t KindsWord1 __attribute__((aligned(1)));
typedef uint16_t KindsHalf1 __attribute__((aligned(1)));
using GlobalQuad4 = __attribute__((address_space(1))) KindsQuad4;
using LooseQuad = const __attribute__((address_space(1))) KindsQuad1;
using LooseWord = const __attribute__((address_space(1))) KindsWord1;
using LooseHalf = const __attribute__((address_space(1))) KindsHalf1;

struct PlanesPerm {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b, uint32_t sel) const { return __builtin_amdgcn_perm(a, b, sel); }
};

// one full group at `in` -> `out` (both 16-byte aligned; out == in is fine), the whole workgroup
template <int W, bool Merge>
__device__ __forceinline__ void planes_group(const uint8_t *in, uint8_t *out) {
    using GlobalQuad = __attribute__((address_space(1))) PlanesQuad;
    const uint32_t t = threadIdx.x;
    // mixed side: the thread's 16 elements back to back; plane side: its quad of plane k at k * 8192
    const uint32_t from_at = Merge ? 16u * t : 16u * W * t, from_step = Merge ? kPlanePacket : 16u;
    const uint32_t to_at = Merge ? 16u * W * t : 16u * t, to_step = Merge ? 16u : kPlanePacket;
    const GlobalQuad *src = reinterpret_cast<const GlobalQuad *>(reinterpret_cast<uintptr_t>(in + from_at));
    PlanesQuad q[W];
#pragma unroll
    for (int k = 0; k < W; ++k) q[k] = src[k * (from_step / 16u)];
    // the loads have arrived in every thread before any thread stores (in place: another thread's store goes where this one reads)
#pragma unroll
    for (int k = 0; k < W; ++k) asm volatile("" : "+v"(q[k]));
    __syncthreads();
    uint32_t from[4 * W], to[4 * W];
#pragma unroll
    for (int k = 0; k < W; ++k) from[4 * k] = q[k].x, from[4 * k + 1] = q[k].y, from[4 * k + 2] = q[k].z, from[4 * k + 3] = q[k].w;
    planes_block<W, Merge>(from, to, PlanesPerm());
    GlobalQuad *dst = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(out + to_at));
#pragma unroll
    for (int k = 0; k < W; ++k) {
        PlanesQuad v;
        v.x = to[4 * k], v.y = to[4 * k + 1], v.z = to[4 * k + 2], v.w = to[4 * k + 3];
        dst[k * (to_step / 16u)] = v;
    }
}

template <bool Merge>
__device__ __forceinline__ void planes_full(const PlanesArgs &a) {
    for (uint64_t packet = blockIdx.x; packet < a.n_packets; packet += gridDim.x) {
        const uint8_t *in = a.in;
        uint8_t *out = a.out;
        uint64_t n_bytes = a.n_bytes, j = packet;
        uint32_t w = a.elem;
        if (a.in_ptrs) {
            const BatchLane bl = batch_lane(a.in_ptrs, a.bytes, a.first_packet, a.n_buffers, packet);
            PlanesBuffer pb = {nullptr, nullptr, 0u, 0u};
            if (bl.owned && bl.count) pb = planes_buffer(a, bl.buffer);
            if (pb.w == 0u) {
                if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
                continue;
            }
            in = pb.in, out = pb.out, n_bytes = pb.n_bytes, w = pb.w;
            j = packet - a.first_packet[bl.buffer];
        }
        w = __builtin_amdgcn_readfirstlane(w);
        const uint32_t lead = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(j & (w - 1u)));
        const uint64_t at = j * kPacket;
        if (lead != 0u || n_bytes - at < static_cast<uint64_t>(w) * kPacket) continue;      // not a group's first packet, or the tail
        if (w == 1u && in == out) continue;
        if (w == 8u) planes_group<8, Merge>(in + at, out + at);
        else if (w == 4u) planes_group<4, Merge>(in + at, out + at);
        else if (w == 2u) planes_group<2, Merge>(in + at, out + at);
        else planes_group<1, Merge>(in + at, out + at);
    }
}

__global__ void __launch_bounds__(kPlaneThreads)
split_planes_kernel(PlanesArgs a) {
    planes_full<false>(a);
}

__global__ void __launch_bounds__(kPlaneThreads)
merge_planes_kernel(PlanesArgs a) {
    planes_full<true>(a);
}

// What a tail kernel does with one buffer: refuse it, move it as planes alone, or filter it -- and `side`, the pointer the XOR
// reads beside the buffer.  The kernel says it once for a single buffer and per buffer of a batch (a functor of the buffer's
// index); the tails' loop (filter_tails) acts on it and does not know which filter it serves.
struct BufferFilter {
    bool bad;                               // a batch only: the buffer is left alone (the full-group kernel flags BAD_BATCH)
    uint32_t filtered;                      // 0: planes alone
    const uint8_t *side;
};
constexpr BufferFilter kPlanesAlone = {false, 0u, nullptr};
struct PlanesAlone {                        // planes_tail_kernel's answers: no buffer is filtered, so no filtered tail is ever asked for
    __device__ __forceinline__ BufferFilter operator()(uint32_t) const { return kPlanesAlone; }
    __device__ __forceinline__ void operator()(const PlanesBuffer &, const uint8_t *) const {}
};

// The tail's frame, shared by the three filters.  tail_load: r bytes at `from` into LDS by quads (never beyond the 16-byte piece
// that holds the buffer's last byte), XORed with those at `with` on the way where Xor.  tail_store: r bytes to `to` by dwords
// and the last r mod 4 bytes (never beyond byte n), word(i) giving dword i and byte(o) byte o.
template <bool Xor>
__device__ __forceinline__ void tail_load(const uint8_t *from, const uint8_t *with, uint32_t r, PlanesQuad *lds) {
    const PlanesGlobalQuad *src = reinterpret_cast<const PlanesGlobalQuad *>(reinterpret_cast<uintptr_t>(from));
    for (uint32_t i = threadIdx.x; i * 16u < r; i += kPlaneThreads) {
        PlanesQuad v = src[i];
        if constexpr (Xor) v ^= reinterpret_cast<const PlanesGlobalQuad *>(reinterpret_cast<uintptr_t>(with))[i];
        lds[i] = v;
    }
    __syncthreads();
}

template <typename Word, typename Byte>
__device__ __forceinline__ void tail_store(uint8_t *to, uint32_t r, Word word, Byte byte) {
    PlanesGlobalWord *words = reinterpret_cast<PlanesGlobalWord *>(reinterpret_cast<uintptr_t>(to));
    for (uint32_t i = threadIdx.x; i * 4u + 4u <= r; i += kPlaneThreads) words[i] = word(i);
    PlanesGlobalByte *last = reinterpret_cast<PlanesGlobalByte *>(reinterpret_cast<uintptr_t>(to));
    if (threadIdx.x < (r & 3u)) last[(r & ~3u) + threadIdx.x] = byte((r & ~3u) + threadIdx.x);
}

// the tail of a buffer, its last n mod G bytes (the general path of planes.h's definition); Xor: against `base` (xorbase.h), on
// the way into LDS for the split -- the base read by quads like the buffer -- and on the way out of it for the merge, which
// reads the base by the dwords and last bytes it writes
template <bool Merge, bool Xor>
__device__ __forceinline__ void planes_tail(const PlanesBuffer &pb, const uint8_t *base, PlanesQuad *lds) {
    const uint32_t w = pb.w;
    if constexpr (!Xor) {
        if (w == 0u || (w == 1u && pb.in == pb.out)) return;
    }
    const uint32_t r = static_cast<uint32_t>(pb.n_bytes % (static_cast<uint64_t>(w) * kPlanePacket)), e = r / w;
    if (r == 0u) return;
    const uint8_t *with = Xor ? base + (pb.n_bytes - r) : nullptr;
    tail_load<Xor && !Merge>(pb.in + (pb.n_bytes - r), with, r, lds);
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(lds);
    const uint32_t log_w = 31u - __builtin_clz(w);
    // output byte o of the tail comes from input byte ...
    auto source = [&](uint32_t o) -> uint32_t {
        if (o >= e * w) return o;                                           // the last r mod w bytes (and everything when e = 0)
        if (!Merge) return (o % e << log_w) + o / e;                        // o = k e + i  <-  i w + k
        return (o & (w - 1u)) * e + (o >> log_w);                           // o = i w + k  <-  k e + i
    };
    tail_store(
        pb.out + (pb.n_bytes - r), r,
        [&](uint32_t i) -> uint32_t {
            const uint32_t o = 4u * i;
            uint32_t v = bytes[source(o)] | static_cast<uint32_t>(bytes[source(o + 1u)]) << 8 | static_cast<uint32_t>(bytes[source(o + 2u)]) << 16 |
                         static_cast<uint32_t>(bytes[source(o + 3u)]) << 24;
            if constexpr (Xor && Merge) v ^= reinterpret_cast<const PlanesGlobalWord *>(reinterpret_cast<uintptr_t>(with))[i];
            return v;
        },
        [&](uint32_t o) -> uint8_t {
            uint8_t v = bytes[source(o)];
            if constexpr (Xor && Merge) v ^= reinterpret_cast<const PlanesGlobalByte *>(reinterpret_cast<uintptr_t>(with))[o];
            return v;
        });
}

// The tail kernels' loop: one buffer, or workgroup b on buffer b of a batch with a barrier between buffers.  A buffer that is
// not filtered takes planes_tail, a filtered one tail(buffer, side); a refused one is left alone (a refused buffer with
// packets was flagged by the full-group kernel).
// `buffer(b)` is buffer b of a batch as the tail takes it: planes_buffer for the filters with one width per buffer (filter_tails).
template <bool Merge, typename Buffer, typename PerBuffer, typename Tail>
__device__ __forceinline__ void filter_tails_of(const PlanesArgs &a, Buffer buffer, const BufferFilter &single, PerBuffer per_buffer, PlanesQuad *lds,
                                                Tail tail) {
    auto one = [&](const PlanesBuffer &pb, const BufferFilter &f) {
        if (f.bad) return;
        if (f.filtered == 0u) planes_tail<Merge, false>(pb, nullptr, lds);
        else if (pb.w != 0u) tail(pb, f.side);
    };
    if (!a.in_ptrs) {
        one({a.in, a.out, a.n_bytes, a.elem}, single);
        return;
    }
    const uint64_t n_buffers = a.n_buffers;
    for (uint64_t b = blockIdx.x; b < n_buffers; b += gridDim.x) {
        one(buffer(static_cast<uint32_t>(b)), per_buffer(static_cast<uint32_t>(b)));
        __syncthreads();                                                          // the next buffer's tail goes into the same LDS
    }
}

template <bool Merge, typename PerBuffer, typename Tail>
__device__ __forceinline__ void filter_tails(const PlanesArgs &a, const BufferFilter &single, PerBuffer per_buffer, PlanesQuad *lds, Tail tail) {
    filter_tails_of<Merge>(a, [&](uint32_t b) { return planes_buffer(a, b); }, single, per_buffer, lds, tail);
}

template <bool Merge>
__global__ void __launch_bounds__(kPlaneThreads)
planes_tail_kernel(PlanesArgs a) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    filter_tails<Merge>(a, kPlanesAlone, PlanesAlone(), lds, PlanesAlone());
}

// ---------------------------------------------------------------------------
// Delta filter (delta.h): split_delta = split_planes of the element-wise differences inside every group,
// merge_delta its inverse, fused into the byte-plane kernels' shape so that the filter costs no pass over memory of its own.
//
// Full groups are planes_group's: 512 threads, 16 elements each, 16-byte accesses on both sides, every load before the
// barrier and every store behind it.  SPLIT: a thread's predictor is the last element of the thread in front -- a lane shift
// inside the wavefront, a few bytes of LDS (written before the barrier) across wavefronts, 0 for the group's first element;
// then delta_block and planes_block.  MERGE: planes_block, the block's local scan (delta_scan_block), an exclusive scan of the
// 512 block totals (delta_workgroup_scan: lane shifts, then the 8 wave totals through LDS behind one more barrier) and the
// thread's offset added to its 16 elements.  Modular addition is associative, so the scan order does not matter.
// A batch carries one more word per buffer, `filter`: 0 takes planes_group (the output is split_planes_batch's), 1 the path
// above, anything else flags BAD_BATCH and leaves the buffer alone; the choice is uniform over a workgroup.
// The tail is delta_tail_kernel's, one workgroup per buffer through LDS like planes_tail: a thread takes 16 elements from
// LDS into registers, filters them, and puts them back in the other layout; then LDS goes out by dwords and bytes.
// Shared with the other filters: the tail's way into LDS and out of it (tail_load, tail_store), the tail kernels' loop over the
// buffers (filter_tails, which sends a buffer with `filter` 0 to planes_tail) and, on the host, the launcher and the argument
// checks.  The delta's own: delta_tail's register pass between the two, and the full-group kernels, whose code is their own
// so that it stays instruction for instruction what DESIGN.md 4.9 measured.
// ---------------------------------------------------------------------------
struct DeltaArgs {
    PlanesArgs p;
    const uint64_t *filter;                 // a batch: per buffer 0 = planes alone, 1 = delta; one buffer: unused (delta)
};

template <int W> struct DeltaLane { typedef uint32_t type; };       // what crosses lanes: an element, or a sum of them
template <> struct DeltaLane<8> { typedef uint64_t type; };

// the exclusive prefix sum of `total` over the workgroup's 512 threads, in thread order, mod 2^32 or 2^64; `waves`: 8 entries
// of LDS that no thread still reads
template <typename T>
__device__ __forceinline__ T delta_workgroup_scan(T total, T *waves) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T incl = total;
#pragma unroll
    for (uint32_t s = 1u; s < 64u; s <<= 1) {
        const T up = __shfl_up(incl, s);
        if (lane >= s) incl += up;
    }
    if (lane == 63u) waves[wave] = incl;
    __syncthreads();
    T front = 0;
#pragma unroll
    for (uint32_t k = 0; k + 1u < kPlaneThreads / 64u; ++k) front += k < wave ? waves[k] : static_cast<T>(0);
    return front + incl - total;
}

// one full group at `in` -> `out` (both 16-byte aligned; out == in is fine), the whole workgroup; `lds`: 8 entries (split: not
// those of the group before)
template <int W, bool Merge>
__device__ __forceinline__ void delta_group(const uint8_t *in, uint8_t *out, typename DeltaLane<W>::type *lds) {
    using T = typename DeltaLane<W>::type;
    using GlobalQuad = __attribute__((address_space(1))) PlanesQuad;
    const uint32_t t = threadIdx.x;
    const uint32_t from_at = Merge ? 16u * t : 16u * W * t, from_step = Merge ? kPlanePacket : 16u;
    const uint32_t to_at = Merge ? 16u * W * t : 16u * t, to_step = Merge ? 16u : kPlanePacket;
    const GlobalQuad *src = reinterpret_cast<const GlobalQuad *>(reinterpret_cast<uintptr_t>(in + from_at));
    PlanesQuad q[W];
#pragma unroll
    for (int k = 0; k < W; ++k) q[k] = src[k * (from_step / 16u)];
#pragma unroll
    for (int k = 0; k < W; ++k) asm volatile("" : "+v"(q[k]));
    uint32_t from[4 * W], to[4 * W];
#pragma unroll
    for (int k = 0; k < W; ++k) from[4 * k] = q[k].x, from[4 * k + 1] = q[k].y, from[4 * k + 2] = q[k].z, from[4 * k + 3] = q[k].w;
    if constexpr (!Merge) {
        T last;                                                         // the thread's last element: the next thread's predictor
        if constexpr (W == 8) last = static_cast<uint64_t>(from[31]) << 32 | from[30];
        else last = from[4 * W - 1] >> (32 - 8 * W);
        if ((t & 63u) == 63u) lds[t >> 6] = last;
        __syncthreads();
        T pred = __shfl_up(last, 1u);
        if ((t & 63u) == 0u) pred = t ? lds[(t >> 6) - 1u] : static_cast<T>(0);
        delta_block<W>(from, pred);
        planes_block<W, false>(from, to, PlanesPerm());
    } else {
        __syncthreads();
        planes_block<W, true>(from, to, PlanesPerm());
        const T total = static_cast<T>(delta_scan_block<W>(to));
        delta_offset_block<W>(to, delta_workgroup_scan<T>(total, lds));
    }
    GlobalQuad *dst = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(out + to_at));
#pragma unroll
    for (int k = 0; k < W; ++k) {
        PlanesQuad v;
        v.x = to[4 * k], v.y = to[4 * k + 1], v.z = to[4 * k + 2], v.w = to[4 * k + 3];
        dst[k * (to_step / 16u)] = v;
    }
}

template <bool Merge>
__device__ __forceinline__ void delta_full(const DeltaArgs &d, uint64_t *lds) {
    const PlanesArgs &a = d.p;
    uint32_t turn = 0u;
    for (uint64_t packet = blockIdx.x; packet < a.n_packets; packet += gridDim.x) {
        const uint8_t *in = a.in;
        uint8_t *out = a.out;
        uint64_t n_bytes = a.n_bytes, j = packet;
        uint32_t w = a.elem, filter = 1u;
        if (a.in_ptrs) {
            const BatchLane bl = batch_lane(a.in_ptrs, a.bytes, a.first_packet, a.n_buffers, packet);
            PlanesBuffer pb = {nullptr, nullptr, 0u, 0u};
            uint64_t f = 0u;
            if (bl.owned && bl.count) pb = planes_buffer(a, bl.buffer), f = d.filter[bl.buffer];
            if (pb.w == 0u || f > 1u) {
                if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
                continue;
            }
            in = pb.in, out = pb.out, n_bytes = pb.n_bytes, w = pb.w, filter = static_cast<uint32_t>(f);
            j = packet - a.first_packet[bl.buffer];
        }
        w = __builtin_amdgcn_readfirstlane(w);
        filter = __builtin_amdgcn_readfirstlane(filter);
        const uint32_t lead = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(j & (w - 1u)));
        const uint64_t at = j * kPacket;
        if (lead != 0u || n_bytes - at < static_cast<uint64_t>(w) * kPacket) continue;      // not a group's first packet, or the tail
        if (filter == 0u) {                                                                 // planes alone: planes_full's path
            if (w == 1u && in == out) continue;
            if (w == 8u) planes_group<8, Merge>(in + at, out + at);
            else if (w == 4u) planes_group<4, Merge>(in + at, out + at);
            else if (w == 2u) planes_group<2, Merge>(in + at, out + at);
            else planes_group<1, Merge>(in + at, out + at);
            continue;
        }
        // split has one barrier per group: a wavefront may write the next group's predictors while another still reads this one's
        uint64_t *mine = lds + 8u * (turn++ & 1u);
        if (w == 8u) delta_group<8, Merge>(in + at, out + at, mine);
        else if (w == 4u) delta_group<4, Merge>(in + at, out + at, reinterpret_cast<uint32_t *>(mine));
        else if (w == 2u) delta_group<2, Merge>(in + at, out + at, reinterpret_cast<uint32_t *>(mine));
        else delta_group<1, Merge>(in + at, out + at, reinterpret_cast<uint32_t *>(mine));
    }
}

__global__ void __launch_bounds__(kPlaneThreads)
split_delta_kernel(DeltaArgs d) {
    __shared__ uint64_t lds[16];
    delta_full<false>(d, lds);
}

__global__ void __launch_bounds__(kPlaneThreads)
merge_delta_kernel(DeltaArgs d) {
    __shared__ uint64_t lds[16];
    delta_full<true>(d, lds);
}

struct DeltaPerBuffer {
    const uint64_t *filter;
    __device__ __forceinline__ BufferFilter operator()(uint32_t b) const {
        const uint64_t f = filter[b];
        return {f > 1u, static_cast<uint32_t>(f), nullptr};
    }
};
constexpr BufferFilter kDeltaSingle = {false, 1u, nullptr};

// the tail of a buffer the filter is on for: e = r div w <= 8191 elements, thread t takes elements 16 t .. 16 t + 15
template <bool Merge>
__device__ __forceinline__ void delta_tail(const PlanesBuffer &pb, PlanesQuad *lds, uint64_t *waves) {
    const uint32_t w = pb.w;
    const uint32_t r = static_cast<uint32_t>(pb.n_bytes % (static_cast<uint64_t>(w) * kPlanePacket)), e = r / w;
    if (r == 0u) return;
    tail_load<false>(pb.in + (pb.n_bytes - r), nullptr, r, lds);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(lds);
    // element i (< e): its byte k lies at i w + k on the mixed side and at k e + i on the plane side
    auto element = [&](uint32_t i, bool planes) -> uint64_t {
        uint64_t v = 0u;
        if (i < e)
            for (uint32_t k = 0; k < w; ++k) v |= static_cast<uint64_t>(bytes[planes ? k * e + i : i * w + k]) << (8u * k);
        return v;
    };
    const uint32_t first = 16u * threadIdx.x;
    uint64_t v[16];
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) v[j] = element(first + j, Merge);
    if constexpr (!Merge) {
        const uint64_t pred = first ? element(first - 1u, false) : 0u;
        __syncthreads();                                                    // every element is in registers before LDS is rewritten
#pragma unroll
        for (uint32_t j = 15u; j > 0u; --j) v[j] -= v[j - 1u];
        v[0] -= pred;
    } else {
#pragma unroll
        for (uint32_t j = 1u; j < 16u; ++j) v[j] += v[j - 1u];              // (elements beyond e count as 0)
        const uint64_t offset = delta_workgroup_scan<uint64_t>(v[15], waves);      // its barrier: as above
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) v[j] += offset;
    }
    uint32_t again = first;                 // (opaque: the 16 lane masks of the loads above are not kept in scalar registers until here)
    asm volatile("" : "+v"(again));
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t i = again + j;
        if (i < e)
            for (uint32_t k = 0; k < w; ++k) bytes[Merge ? i * w + k : k * e + i] = static_cast<uint8_t>(v[j] >> (8u * k));
    }
    __syncthreads();
    const uint32_t *done = reinterpret_cast<const uint32_t *>(lds);
    tail_store(
        pb.out + (pb.n_bytes - r), r, [&](uint32_t i) -> uint32_t { return done[i]; }, [&](uint32_t o) -> uint8_t { return bytes[o]; });
}

template <bool Merge>
__global__ void __launch_bounds__(kPlaneThreads)
delta_tail_kernel(DeltaArgs d) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    __shared__ uint64_t waves[kPlaneThreads / 64u];
    filter_tails<Merge>(d.p, kDeltaSingle, DeltaPerBuffer{d.filter}, lds,
                        [&](const PlanesBuffer &pb, const uint8_t *) { delta_tail<Merge>(pb, lds, waves); });
}

// ---------------------------------------------------------------------------
// XOR against a base (xorbase.h): split_xor = split_planes of buffer ^ base, merge_xor its inverse, fused into
// the byte-plane kernels' shape: no second pass over memory and no temporary buffer.
//
// Full groups are planes_group's: 512 threads, 16 elements each, 16-byte accesses on both sides, every load -- of the buffer
// and of the base -- before the barrier and every store behind it.  The base is needed on the MIXED side in both directions (w
// quads back to back per thread), the side that is slow to read for w >= 4 (neighbouring lanes 16 w bytes apart), so it is read
// like a plane, perfectly coalesced, and handed to its lanes through one group of LDS around the barrier the shape already has
// (w = 1: no LDS); one more barrier behind the stores frees the LDS for a workgroup that strides on.  SPLIT XORs the registers
// in front of planes_block, MERGE behind it.
// A batch carries one more pointer per buffer, `base_ptrs`: 0 takes planes_group (the output is split_planes_batch's), a
// 16-byte aligned pointer the path above, a misaligned one flags BAD_BATCH and leaves the buffer alone; the choice is uniform
// over a workgroup.  A base never overlaps an output: the single-buffer calls check it, a batch's caller sees to it.
// The tail is xor_tail_kernel's, one workgroup per buffer through LDS like planes_tail: by quads in -- buffer and, for the
// split, base, XORed on the way into LDS; the merge reads the base by the dwords and last bytes it writes -- so nothing
// is read beyond the 16-byte piece that holds the last byte and nothing written beyond byte n.
// Shared with the other filters: the tail itself -- planes_tail with the XOR as its optional part -- the tail kernels' loop over
// the buffers (filter_tails), and on the host the launcher and the argument checks.  The XOR's own: the full-group kernels, whose
// code is their own so that it stays instruction for instruction what DESIGN.md 4.10 measured.
// ---------------------------------------------------------------------------
struct XorArgs {
    PlanesArgs p;
    const uint8_t *base;                    // one buffer: its base ...
    const uint8_t *const *base_ptrs;        // ... a batch: per buffer 0 = planes alone, else the base
};

// one full group at `in` -> `out` against `base` (all 16-byte aligned; out == in is fine), the whole workgroup; `lds`: room for
// one group (W > 1)
template <int W, bool Merge>
__device__ __forceinline__ void xor_group(const uint8_t *in, const uint8_t *base, uint8_t *out, PlanesQuad *lds) {
    using GlobalQuad = __attribute__((address_space(1))) PlanesQuad;
    const uint32_t t = threadIdx.x;
    const uint32_t from_at = Merge ? 16u * t : 16u * W * t, from_step = Merge ? kPlanePacket : 16u;
    const uint32_t to_at = Merge ? 16u * W * t : 16u * t, to_step = Merge ? 16u : kPlanePacket;
    const GlobalQuad *src = reinterpret_cast<const GlobalQuad *>(reinterpret_cast<uintptr_t>(in + from_at));
    // the base is needed on the mixed side, W quads back to back per thread, but read like a plane: quad k * 512 + t, perfectly
    // coalesced, and handed to its thread through LDS (W = 1: the two shapes are one)
    const GlobalQuad *with = reinterpret_cast<const GlobalQuad *>(reinterpret_cast<uintptr_t>(base + 16u * t));
    PlanesQuad q[W], b[W];
#pragma unroll
    for (int k = 0; k < W; ++k) q[k] = src[k * (from_step / 16u)];
#pragma unroll
    for (int k = 0; k < W; ++k) b[k] = with[k * kPlaneThreads];
    // the loads have arrived in every thread before any thread stores (in place: another thread's store goes where this one reads)
#pragma unroll
    for (int k = 0; k < W; ++k) asm volatile("" : "+v"(q[k]), "+v"(b[k]));
    if constexpr (W > 1) {
#pragma unroll
        for (int k = 0; k < W; ++k) lds[k * kPlaneThreads + t] = b[k];
    }
    __syncthreads();
    if constexpr (W > 1) {
#pragma unroll
        for (int k = 0; k < W; ++k) b[k] = lds[W * t + k];
    }
    uint32_t from[4 * W], to[4 * W], mask[4 * W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        from[4 * k] = q[k].x, from[4 * k + 1] = q[k].y, from[4 * k + 2] = q[k].z, from[4 * k + 3] = q[k].w;
        mask[4 * k] = b[k].x, mask[4 * k + 1] = b[k].y, mask[4 * k + 2] = b[k].z, mask[4 * k + 3] = b[k].w;
    }
    if constexpr (!Merge) xor_block<W>(from, mask);
    planes_block<W, Merge>(from, to, PlanesPerm());
    if constexpr (Merge) xor_block<W>(to, mask);
    GlobalQuad *dst = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(out + to_at));
#pragma unroll
    for (int k = 0; k < W; ++k) {
        PlanesQuad v;
        v.x = to[4 * k], v.y = to[4 * k + 1], v.z = to[4 * k + 2], v.w = to[4 * k + 3];
        dst[k * (to_step / 16u)] = v;
    }
    if constexpr (W > 1) __syncthreads();      // a workgroup that strides on puts the next group's base into the same LDS
}

template <bool Merge>
__device__ __forceinline__ void xor_full(const XorArgs &x, PlanesQuad *lds) {
    const PlanesArgs &a = x.p;
    for (uint64_t packet = blockIdx.x; packet < a.n_packets; packet += gridDim.x) {
        const uint8_t *in = a.in, *base = x.base;
        uint8_t *out = a.out;
        uint64_t n_bytes = a.n_bytes, j = packet;
        uint32_t w = a.elem;
        if (a.in_ptrs) {
            const BatchLane bl = batch_lane(a.in_ptrs, a.bytes, a.first_packet, a.n_buffers, packet);
            PlanesBuffer pb = {nullptr, nullptr, 0u, 0u};
            base = nullptr;
            if (bl.owned && bl.count) pb = planes_buffer(a, bl.buffer), base = x.base_ptrs[bl.buffer];
            if (pb.w == 0u || (reinterpret_cast<uintptr_t>(base) & 15u) != 0u) {
                if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
                continue;
            }
            in = pb.in, out = pb.out, n_bytes = pb.n_bytes, w = pb.w;
            j = packet - a.first_packet[bl.buffer];
        }
        w = __builtin_amdgcn_readfirstlane(w);
        const uint32_t based = __builtin_amdgcn_readfirstlane(base != nullptr ? 1u : 0u);
        const uint32_t lead = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(j & (w - 1u)));
        const uint64_t at = j * kPacket;
        if (lead != 0u || n_bytes - at < static_cast<uint64_t>(w) * kPacket) continue;      // not a group's first packet, or the tail
        if (based == 0u) {                                                                  // planes alone: planes_full's path
            if (w == 1u && in == out) continue;
            if (w == 8u) planes_group<8, Merge>(in + at, out + at);
            else if (w == 4u) planes_group<4, Merge>(in + at, out + at);
            else if (w == 2u) planes_group<2, Merge>(in + at, out + at);
            else planes_group<1, Merge>(in + at, out + at);
            continue;
        }
        if (w == 8u) xor_group<8, Merge>(in + at, base + at, out + at, lds);
        else if (w == 4u) xor_group<4, Merge>(in + at, base + at, out + at, lds);
        else if (w == 2u) xor_group<2, Merge>(in + at, base + at, out + at, lds);
        else xor_group<1, Merge>(in + at, base + at, out + at, lds);
    }
}

__global__ void __launch_bounds__(kPlaneThreads)
split_xor_kernel(XorArgs x) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    xor_full<false>(x, lds);
}

__global__ void __launch_bounds__(kPlaneThreads)
merge_xor_kernel(XorArgs x) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    xor_full<true>(x, lds);
}

struct XorPerBuffer {
    const uint8_t *const *base_ptrs;
    __device__ __forceinline__ BufferFilter operator()(uint32_t b) const {
        const uint8_t *base = base_ptrs[b];
        return {(reinterpret_cast<uintptr_t>(base) & 15u) != 0u, base != nullptr ? 1u : 0u, base};
    }
};

template <bool Merge>
__global__ void __launch_bounds__(kPlaneThreads)
xor_tail_kernel(XorArgs x) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    filter_tails<Merge>(x.p, {false, 1u, x.base}, XorPerBuffer{x.base_ptrs}, lds,
                        [&](const PlanesBuffer &pb, const uint8_t *base) { planes_tail<Merge, true>(pb, base, lds); });
}

// ---------------------------------------------------------------------------
// Mixed filter (mixed.h): every supergroup (8 packets = 65536 bytes) of a buffer is split as planes alone, with
// the delta filter or against the base, at a width of its own, as its mode byte says; merge_mixed is the inverse.  No filter is
// defined anew: the kernels below read a supergroup's mode and hand the group to planes_group, delta_group or xor_group, and the
// tail to planes_tail or delta_tail, the device functions of the three sections above.
//
// Full groups have the other filters' shape: 512 threads, the workgroups stride over the packets, packet j of its buffer belongs
// to supergroup j / 8, the mode is made uniform (readfirstlane) and the workgroup of a group's first packet moves the whole group.
// A supergroup is a multiple of every group, so a group never straddles two modes.  LDS: one group for the base (xor_group) and,
// apart from it, the delta's two times eight predictor slots.
// A workgroup that strides on may go from a group of one kind to a group of another.  Two things are carried from group to group:
//  * delta_group's LDS slots.  The split has ONE barrier per group, so a wavefront may write the next delta group's predictors
//    while another still reads this one's: the slots alternate (`turn`, advanced by delta groups alone).  A slot is written again
//    two delta groups later; the writer has then passed the barrier of the delta group in between, which no wavefront reaches
//    before it has read the earlier slot.  Groups of other kinds between two delta groups only add barriers; they never touch the
//    slots, which lie apart from the base's LDS.  (The merge has two barriers per group and needs no alternation; it takes it.)
//  * xor_group's LDS.  Its trailing barrier (w > 1) stands behind the last read of the base from LDS, so whatever group comes next
//    -- an XOR group that writes the same LDS, or a planes or delta group that does not touch it -- starts with the LDS free; a
//    planes or delta group in front of an XOR group never uses that LDS at all.
// Groups touch disjoint bytes of their buffers, so no load of one group depends on a store of another, in place or not.
// Refused, each flagged BAD_BATCH: a supergroup whose mode is not 0 .. 11, or asks for a base where the buffer has none, is left
// alone (the others of its buffer are moved); a buffer whose pointers or base are misaligned, or that does not own exactly its
// packets (planes_buffer's rule), is left alone as a whole.
// The tail -- only a buffer's last supergroup has one: n mod (w_last * 8192) bytes -- is mixed_tail_kernel's, one workgroup per
// buffer through filter_tails' frame: planes_tail, delta_tail or planes_tail with the XOR, with the width of the last mode.
// choose_modes_kernel is the choice itself: one lane per supergroup of the batch sums the survey rows of its 1 .. 8 packets and
// writes the mode and the predicted total with mixed.h's choose_supergroup_mode, the host's own function.
// ---------------------------------------------------------------------------
struct MixedArgs {
    PlanesArgs p;                           // elem and elem_bytes are not used: the widths are in the modes
    const uint8_t *modes;                   // one buffer: its mode_count(n_bytes) modes; a batch: every buffer's, at first_mode[b]
    const uint64_t *first_mode;             // a batch: n_buffers entries
    const uint8_t *base;                    // one buffer: its base, or null ...
    const uint8_t *const *base_ptrs;        // ... a batch: per buffer 0 = no base, else the base
};

// planes_buffer's rule without a width: both pointers 16-byte aligned and exactly the packets the bytes make; w = 1 says usable
__device__ __forceinline__ PlanesBuffer mixed_buffer(const PlanesArgs &a, uint32_t b) {
    PlanesBuffer r = {a.in_ptrs[b], a.out_ptrs[b], a.bytes[b], 0u};
    const uint64_t owns = a.first_packet[b + 1u] - a.first_packet[b];
    const bool aligned = ((reinterpret_cast<uintptr_t>(r.in) | reinterpret_cast<uintptr_t>(r.out)) & 15u) == 0u;
    if (aligned && owns == (r.n_bytes + kPacket - 1u) / kPacket) r.w = 1u;
    return r;
}

// a mode the kernels act on: valid, and with a base where it asks for one
__device__ __forceinline__ bool mixed_usable(uint32_t mode, const uint8_t *base) {
    return mixed_mode_ok(mode) && (mixed_kind(mode) != kMixedBase || base != nullptr);
}

template <bool Merge>
__device__ __forceinline__ void mixed_full(const MixedArgs &m, PlanesQuad *lds, uint64_t *slots) {
    const PlanesArgs &a = m.p;
    uint32_t turn = 0u;
    for (uint64_t packet = blockIdx.x; packet < a.n_packets; packet += gridDim.x) {
        const uint8_t *in = a.in, *base = m.base, *modes = m.modes;
        uint8_t *out = a.out;
        uint64_t n_bytes = a.n_bytes, j = packet;
        if (a.in_ptrs) {
            const BatchLane bl = batch_lane(a.in_ptrs, a.bytes, a.first_packet, a.n_buffers, packet);
            PlanesBuffer pb = {nullptr, nullptr, 0u, 0u};
            base = nullptr;
            if (bl.owned && bl.count) pb = mixed_buffer(a, bl.buffer), base = m.base_ptrs[bl.buffer], modes = m.modes + m.first_mode[bl.buffer];
            if (pb.w == 0u || (reinterpret_cast<uintptr_t>(base) & 15u) != 0u) {
                if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
                continue;
            }
            in = pb.in, out = pb.out, n_bytes = pb.n_bytes;
            j = packet - a.first_packet[bl.buffer];
        }
        const uint32_t mode = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(modes[j / kSurveyPackets]));
        const uint32_t usable = __builtin_amdgcn_readfirstlane(mixed_usable(mode, base) ? 1u : 0u);
        if (usable == 0u) {
            if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
            continue;
        }
        const uint32_t w = mixed_width(mode), kind = mixed_kind(mode);
        const uint32_t lead = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(j & (w - 1u)));
        const uint64_t at = j * kPacket;
        if (lead != 0u || n_bytes - at < static_cast<uint64_t>(w) * kPacket) continue;      // not a group's first packet, or the tail
        if (kind == kMixedPlanes) {
            if (w == 1u && in == out) continue;
            if (w == 8u) planes_group<8, Merge>(in + at, out + at);
            else if (w == 4u) planes_group<4, Merge>(in + at, out + at);
            else if (w == 2u) planes_group<2, Merge>(in + at, out + at);
            else planes_group<1, Merge>(in + at, out + at);
        } else if (kind == kMixedDelta) {
            uint64_t *mine = slots + 8u * (turn++ & 1u);                                    // (the comment above: why they alternate)
            if (w == 8u) delta_group<8, Merge>(in + at, out + at, mine);
            else if (w == 4u) delta_group<4, Merge>(in + at, out + at, reinterpret_cast<uint32_t *>(mine));
            else if (w == 2u) delta_group<2, Merge>(in + at, out + at, reinterpret_cast<uint32_t *>(mine));
            else delta_group<1, Merge>(in + at, out + at, reinterpret_cast<uint32_t *>(mine));
        } else {
            if (w == 8u) xor_group<8, Merge>(in + at, base + at, out + at, lds);
            else if (w == 4u) xor_group<4, Merge>(in + at, base + at, out + at, lds);
            else if (w == 2u) xor_group<2, Merge>(in + at, base + at, out + at, lds);
            else xor_group<1, Merge>(in + at, base + at, out + at, lds);
        }
    }
}

__global__ void __launch_bounds__(kPlaneThreads)
split_mixed_kernel(MixedArgs m) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    __shared__ uint64_t slots[16];
    mixed_full<false>(m, lds, slots);
}

__global__ void __launch_bounds__(kPlaneThreads)
merge_mixed_kernel(MixedArgs m) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    __shared__ uint64_t slots[16];
    mixed_full<true>(m, lds, slots);
}

// What the tail of a buffer of n_bytes bytes is: the mode of its last supergroup decides (the buffer has bytes).
struct MixedTail {
    uint32_t w;                             // 0: refused
    BufferFilter filter;                    // filtered: the mode's kind; side: the base of an XOR tail
};
__device__ __forceinline__ MixedTail mixed_tail_of(const uint8_t *modes, uint64_t n_bytes, const uint8_t *base) {
    const uint32_t mode = modes[(n_bytes - 1u) / kSurveyBytes];
    const bool bad = !mixed_usable(mode, base) || (reinterpret_cast<uintptr_t>(base) & 15u) != 0u;
    const uint32_t kind = mixed_kind(mode);
    return {bad ? 0u : mixed_width(mode), {bad, kind, kind == kMixedBase ? base : nullptr}};
}

template <bool Merge>
__global__ void __launch_bounds__(kPlaneThreads)
mixed_tail_kernel(MixedArgs m) {
    __shared__ PlanesQuad lds[8u * kPlanePacket / 16u];
    __shared__ uint64_t waves[kPlaneThreads / 64u];
    PlanesArgs a = m.p;
    BufferFilter single = kPlanesAlone;
    if (!a.in_ptrs) {
        const MixedTail t = mixed_tail_of(m.modes, a.n_bytes, m.base);      // (launched for a buffer with bytes alone)
        a.elem = t.w, single = t.filter;
    }
    auto of = [&](uint32_t b) { return mixed_tail_of(m.modes + m.first_mode[b], a.bytes[b], m.base_ptrs[b]); };
    filter_tails_of<Merge>(
        a,
        [&](uint32_t b) {
            PlanesBuffer pb = mixed_buffer(a, b);
            if (pb.w != 0u) pb.w = pb.n_bytes ? of(b).w : 0u;
            return pb;
        },
        single, [&](uint32_t b) { return a.bytes[b] ? of(b).filter : kPlanesAlone; }, lds,
        [&](const PlanesBuffer &pb, const uint8_t *side) {
            if (side) planes_tail<Merge, true>(pb, side, lds);
            else delta_tail<Merge>(pb, lds, waves);
        });
}

struct ChooseModesArgs {
    const uint32_t *plain;                  // the survey rows: row j at + j * stride, entry p the batch's packet p ...
    const uint32_t *delta;                  // ... null: not offered
    const uint32_t *xored;
    uint64_t stride;
    uint64_t n_bytes;                       // one buffer ...
    const uint64_t *bytes;                  // ... or a batch (bytes != nullptr)
    const uint64_t *first_packet;
    const uint64_t *first_mode;
    uint32_t n_buffers;
    uint32_t n_packets;
    uint32_t n_modes;
    uint8_t *modes;
    uint32_t *totals;                       // may be null
    uint32_t *status;
};

constexpr uint32_t kChooseThreads = 256;

__global__ void __launch_bounds__(kChooseThreads)
choose_modes_kernel(ChooseModesArgs a) {
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kChooseThreads + threadIdx.x;
    if (g >= a.n_modes) return;
    uint64_t s = g, first = 0u, packets = (a.n_bytes + kPacket - 1u) / kPacket;
    if (a.bytes) {
        uint32_t lo = 0, n = a.n_buffers;                        // batch_lane's search: the last buffer with first_mode[b] <= g
        while (n > 0u) {
            const uint32_t half = n >> 1;
            if (a.first_mode[lo + half] <= g) lo += half + 1u, n -= half + 1u;
            else n = half;
        }
        const uint32_t b = lo - 1u;
        bool owned = lo != 0u;
        if (owned) {
            s = g - a.first_mode[b], first = a.first_packet[b], packets = a.first_packet[b + 1u] - first;
            owned = packets == (a.bytes[b] + kPacket - 1u) / kPacket && s * kSurveyPackets < packets && first + packets <= a.n_packets;
        }
        if (!owned) {                                            // a supergroup nobody owns, or a buffer that does not own its packets
            atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
            return;
        }
    }
    const ModeChoice c = choose_supergroup_mode(a.plain + first, a.delta ? a.delta + first : nullptr, a.xored ? a.xored + first : nullptr, a.stride, s,
                                                packets);
    a.modes[g] = static_cast<uint8_t>(c.mode);
    if (a.totals) a.totals[g] = static_cast<uint32_t>(c.total);
}

// ---------------------------------------------------------------------------
// Packet size estimate (estimate.h): est[p] = the clen the codec would give packet p, from the packet's byte
// histogram alone, for one buffer or a batch -- and the copy that moves the packets the estimate says cannot shrink.
//
// estimate_kernel has crc32_kernel's shape and reuses its descriptor code (CrcArgs with `crc` as `est`, crc_locate, crc_load):
// one wavefront per packet, lane l on bytes [128 l, 128 l + 128) as eight 16-byte loads, one workgroup of 16 wavefronts per
// CU, persistent over the packets.  Each wavefront owns a histogram in LDS: 256 bins of u32, 8 times over -- a lane adds
// into copy (lane & 7), bin s of copy c at dword 8 s + c, so the eight lanes that read neighbouring bytes never share a
// counter and a packet of 8192 equal bytes spreads over 8 addresses in 8 banks (4 lanes of a 32-lane half on each) instead
// of 64 lanes on one.  That is 8 KiB per wavefront, 128 KiB per workgroup.  Nobody but the wavefront touches its histogram,
// so there is no barrier: LDS operations of one wavefront complete in order.  The wavefront then reads the histogram back as
// 512 quads (lane l: quads l + 64 k, conflict-free; a quad is four copies of one bin, the neighbouring lane holds the other
// four), clears it for its next packet, and each lane looks up LF[h] for 4 of the 256 bins in the table built from
// estimate.h (66 KiB, L2-resident); a wave reduction in u64 follows and lane 0 writes est[p].
// ---------------------------------------------------------------------------
__device__ const EstimateTable g_est_table = EstimateTable();
constexpr uint32_t kEstWaves = 16;
constexpr uint32_t kEstCopies = 8;
constexpr uint32_t kEstWaveDwords = 256u * kEstCopies;      // 8 KiB per wavefront
constexpr uint32_t kEstGroups = 256;                        // one workgroup per CU of an MI355X (128 KiB of LDS each)

__device__ __forceinline__ void est_count(uint32_t *hist, uint32_t w, uint32_t kByte) {      // hist: the lane's copy; kByte static
    __hip_atomic_fetch_add(hist + (((w >> (8u * kByte)) & 255u) * kEstCopies), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), off), hi = __shfl_xor(static_cast<uint32_t>(v >> 32), off);
        v += static_cast<uint64_t>(hi) << 32 | lo;
    }
    return v;
}

__global__ void __launch_bounds__(kEstWaves * kLanes)
estimate_kernel(CrcArgs a) {
    __shared__ CrcQuad lds[kEstWaves * kEstWaveDwords / 4u];
    const uint32_t lane = threadIdx.x & 63u;
    CrcQuad *quads = lds + (threadIdx.x >> 6) * (kEstWaveDwords / 4u);
    uint32_t *hist = reinterpret_cast<uint32_t *>(quads) + (lane & (kEstCopies - 1u));
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) quads[lane + 64u * k] = CrcQuad(0u);
    const uint32_t stride = gridDim.x * kEstWaves;
    for (uint32_t packet = blockIdx.x * kEstWaves + (threadIdx.x >> 6), next; packet < a.n_packets; packet = next) {
        next = packet + stride;
        const CrcPacket p = crc_locate(a, packet);
        if (p.count == 0u) {
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
        } else {
            CrcQuad q[8];
            crc_load(q, p, lane);
            asm volatile("" ::: "memory");                   // the histogram was cleared (by other lanes) in front of these adds
            if (p.count == kPacket) {                        // wave-uniform
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
#pragma unroll
                        for (uint32_t b = 0; b < 4; ++b) est_count(hist, w[j], b);
                    }
                }
            } else {
                const uint32_t have = lane_have(p.count, lane);
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
#pragma unroll
                        for (uint32_t b = 0; b < 4; ++b)
                            if (16u * k + 4u * j + b < have) est_count(hist, w[j], b);
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // every lane's adds in front of the reads of other lanes' counters
            // quad l + 64 k: copies 4 (l & 1) .. + 3 of bin (l >> 1) + 32 k; with the neighbouring lane's four that is the bin
            // both lanes of a pair then hold the pair's 8 bins: the even lane looks up the even k, the odd lane the odd ones
            using GlobalLf = const __attribute__((address_space(1))) uint64_t;
            GlobalLf *lf = reinterpret_cast<GlobalLf *>(reinterpret_cast<uintptr_t>(g_est_table.lf));
            const bool odd = (lane & 1u) != 0u;
            uint64_t sum = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8; k += 2) {
                const CrcQuad v0 = quads[lane + 64u * k], v1 = quads[lane + 64u * k + 64u];
                quads[lane + 64u * k] = CrcQuad(0u);
                quads[lane + 64u * k + 64u] = CrcQuad(0u);
                const uint32_t part0 = v0.x + v0.y + v0.z + v0.w, part1 = v1.x + v1.y + v1.z + v1.w;
                const uint32_t count0 = part0 + __shfl_xor(part0, 1), count1 = part1 + __shfl_xor(part1, 1);
                sum += lf[odd ? count1 : count0];
            }
            sum = wave_sum64(sum);
            if (lane == 0u) a.crc[packet] = est_clen_from_sum(lf[p.count + 255u], lf[255], sum);
        }
        if (next < packet) break;
    }
}

// move_packets_kernel: region r is bytes[r] (1 .. 8192) bytes from src[r] to dst[r], both 16-byte aligned -- the packets
// batch.compress(stored=...) keeps raw.  One workgroup of 512 threads per region, one quad per thread; the region's last,
// partial quad is loaded whole (nothing beyond the 16-byte piece that holds the last byte) and stored by dwords and bytes
// (nothing beyond the last byte).  A misaligned pointer or bytes > 8192: BAD_BATCH, the region is skipped.
constexpr uint32_t kMoveThreads = kPacket / 16u;

struct MoveArgs {
    const uint8_t *const *src;
    uint8_t *const *dst;
    const uint64_t *bytes;
    uint32_t n_regions;
    uint32_t *status;
};

// A packet's last, partial quad: bytes [0, left) of q, left = 1 .. 15, to `to` (4-byte aligned) by dwords and bytes -- nothing
// behind byte `left` is written.  The one copy for every kernel that stores a packet from registers.
__device__ __forceinline__ void store_partial_quad(uintptr_t to, const PlanesQuad &q, uint32_t left) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    PlanesGlobalWord *words = reinterpret_cast<PlanesGlobalWord *>(to);
    PlanesGlobalByte *bytes = reinterpret_cast<PlanesGlobalByte *>(to);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (4u * j + 4u <= left) {
            words[j] = w[j];
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 3; ++b)
                if (4u * j + b < left) bytes[4u * j + b] = static_cast<uint8_t>(w[j] >> (8u * b));
        }
    }
}

__global__ void __launch_bounds__(kMoveThreads)
move_packets_kernel(MoveArgs a) {
    const uint32_t at = 16u * threadIdx.x;
    for (uint64_t r = blockIdx.x; r < a.n_regions; r += gridDim.x) {
        const uintptr_t src = reinterpret_cast<uintptr_t>(a.src[r]), dst = reinterpret_cast<uintptr_t>(a.dst[r]);
        const uint64_t n = a.bytes[r];
        if (((src | dst) & 15u) != 0u || n > kPacket) {
            if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
            continue;
        }
        if (at >= n) continue;
        const uint32_t left = static_cast<uint32_t>(n) - at;
        const PlanesQuad q = reinterpret_cast<const PlanesGlobalQuad *>(src)[threadIdx.x];
        if (left >= 16u) reinterpret_cast<PlanesGlobalQuad *>(dst)[threadIdx.x] = q;
        else store_partial_quad(dst + at, q, left);
    }
}

// ---------------------------------------------------------------------------
// Sparse packets (sparse.h): a packet that is one byte value almost everywhere is kept as that byte and a list
// of (position, value) exceptions instead of being coded.  Three bandwidth-bound passes, one wavefront per packet, lane l on
// bytes [128 l, 128 l + 128) as eight 16-byte loads that stay in registers (crc_load; nothing is read beyond the 16-byte piece
// that holds the packet's last byte, and bytes past the packet's end are masked out of every count).
//
// sparse_scan_kernel (one buffer or a batch: CrcArgs with `crc` as `scan`, crc_locate): bit b of the only possible majority
// byte is 1 iff more than half of the packet's bytes have bit b set -- eight masked popcounts per dword, the eight counts
// reduced over the wave two to a register --, and a second pass over the registers counts the bytes equal to that candidate.
// No LDS, no histogram.  Lane 0 writes scan[p].
//
// sparse_pack_kernel (regions, as move_packets_kernel) is sparse_count, the check, the head, sparse_emit: the count gives the
// wave's total and the lane's first slot, and the total is checked against scan[r] BEFORE anything is written: the slots are
// then all inside the record's sparse_len(k) bytes.
//
// sparse_unpack_kernel (regions) validates the record's head and hands it to sparse_build, which builds the packet in the
// wavefront's own 8 KiB of LDS and stores it like move_packets_kernel's.
//
// sparse_build and store_partial_quad are also what kinds_expand_kernel (below) does with a sparse packet, so each check on a
// damaged record exists once; kinds_store_kernel shares sparse_differ and store_partial_quad and keeps the writer's text.
// ---------------------------------------------------------------------------
constexpr uint32_t kSparseWaves = 4;                        // wavefronts per workgroup, a packet each
constexpr uint32_t kSparseGroups = 2048;                    // scan: 8 workgroups per CU of an MI355X, persistent over the packets
constexpr uint32_t kSparseLow = 0x01010101u, kSparseHigh = 0x80808080u;

// the bytes of the dword at byte `at` of the lane's 128 that lie inside the packet (have: how many of the 128 do)
template <bool Full>
__device__ __forceinline__ uint32_t sparse_mask(uint32_t at, uint32_t have) {
    if (Full) return 0xFFFFFFFFu;
    return at + 4u <= have ? 0xFFFFFFFFu : at < have ? (1u << (8u * (have - at))) - 1u : 0u;
}

// 0x80 in every byte of x that is zero
__device__ __forceinline__ uint32_t sparse_zero_bytes(uint32_t x) {
    return ~(((x & ~kSparseHigh) + ~kSparseHigh) | x) & kSparseHigh;
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the packet's scan word (in every lane)
template <bool Full>
__device__ __forceinline__ uint32_t sparse_scan_packet_wave(const CrcQuad (&q)[8], uint32_t count, uint32_t lane) {
    const uint32_t have = lane_have(count, lane);
    uint32_t bits[4] = {0u, 0u, 0u, 0u};                    // bits[i]: the counts of bit 2 i (low half) and bit 2 i + 1 (high half)
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t v = w[j] & sparse_mask<Full>(16u * k + 4u * j, have);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                bits[i] += __popc(v & (kSparseLow << (2u * i))) + (__popc(v & (kSparseLow << (2u * i + 1u))) << 16);
        }
    }
    uint32_t candidate = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t both = wave_sum32(bits[i]);          // (a count is at most 8192: the halves do not meet)
        candidate |= (2u * (both & 0xFFFFu) > count ? 1u << (2u * i) : 0u) | (2u * (both >> 16) > count ? 2u << (2u * i) : 0u);
    }
    uint32_t equal = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            equal += __popc(sparse_zero_bytes(w[j] ^ (candidate * kSparseLow)) & sparse_mask<Full>(16u * k + 4u * j, have));
    }
    return sparse_scan_word(candidate, wave_sum32(equal), count);
}

__global__ void __launch_bounds__(kSparseWaves * kLanes)
sparse_scan_kernel(CrcArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * kSparseWaves;
    for (uint32_t packet = blockIdx.x * kSparseWaves + (threadIdx.x >> 6), next; packet < a.n_packets; packet = next) {
        next = packet + stride;
        const CrcPacket p = crc_locate(a, packet);
        if (p.count == 0u) {
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
        } else {
            CrcQuad q[8];
            crc_load(q, p, lane);
            const uint32_t scan = p.count == kPacket ? sparse_scan_packet_wave<true>(q, p.count, lane)       // wave-uniform
                                                     : sparse_scan_packet_wave<false>(q, p.count, lane);
            if (lane == 0u) a.crc[packet] = scan;
        }
        if (next < packet) break;
    }
}

struct SparsePackArgs {
    const uint8_t *const *src;
    const uint64_t *bytes;
    const uint32_t *scan;
    uint8_t *const *dst;
    uint32_t n_regions;
    uint32_t *status;
};

// one wavefront per item (a region, a packet), persistent: `for (uint64_t r = wave_item(); r < n; r += wave_items())`
__device__ __forceinline__ uint64_t wave_item() { return static_cast<uint64_t>(blockIdx.x) * kSparseWaves + (threadIdx.x >> 6); }
__device__ __forceinline__ uint64_t wave_items() { return static_cast<uint64_t>(gridDim.x) * kSparseWaves; }

// 0x80 in every byte of dword w, at byte `at` of the lane's 128, that lies inside the packet and is not the fill: an exception.
// The one predicate behind the count and the stores of a record.
__device__ __forceinline__ uint32_t sparse_differ(uint32_t w, uint32_t fill, uint32_t at, uint32_t have) {
    return ~sparse_zero_bytes(w ^ (fill * kSparseLow)) & kSparseHigh & sparse_mask<false>(at, have);
}

// The record writer, first half: the packet's exceptions counted over the wave (the total, in every lane) and `slot`, the
// lane's first slot in the record -- an inclusive prefix sum less the lane's own count, so that lane order times in-lane order
// is ascending position.  Nothing is written: the caller checks the total against the scan word, and what else it has to,
// before it calls sparse_emit.
__device__ __forceinline__ uint32_t sparse_count(const CrcQuad (&q)[8], uint32_t fill, uint32_t have, uint32_t lane, uint32_t &slot) {
    uint32_t mine = 0;                                       // the lane's exceptions
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) mine += __popc(sparse_differ(w[j], fill, 16u * i + 4u * j, have));
    }
    uint32_t upto = mine;                                    // inclusive prefix sum over the wave
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t below = __shfl_up(upto, off);
        if (lane >= off) upto += below;
    }
    slot = upto - mine;
    return __shfl(upto, 63);
}

// ... second half: behind the record's head at `rec` (4-byte aligned; the head itself is the caller's), pos[k], val[k] and the
// pad up to sparse_len(k).  k is sparse_count's total and slot its slot: every store below is then to a slot below k, the same
// predicate having been counted.
__device__ __forceinline__ void sparse_emit(uintptr_t rec, const CrcQuad (&q)[8], uint32_t fill, uint32_t k, uint32_t have, uint32_t lane, uint32_t slot) {
    PlanesGlobalHalf *pos = reinterpret_cast<PlanesGlobalHalf *>(rec + 4u);
    PlanesGlobalByte *val = reinterpret_cast<PlanesGlobalByte *>(rec + 4u + 2u * k);
    if (lane < sparse_len(k) - (4u + 3u * k)) val[k + lane] = 0;               // the pad
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t at = 16u * i + 4u * j;
            const uint32_t differ = sparse_differ(w[j], fill, at, have);
            if (differ != 0u) {
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b) {
                    if (differ & (0x80u << (8u * b))) {
                        pos[slot] = static_cast<uint16_t>(kCrcChunk * lane + at + b);
                        val[slot] = static_cast<uint8_t>(w[j] >> (8u * b));
                        ++slot;
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kSparseWaves * kLanes)
sparse_pack_kernel(SparsePackArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r = wave_item(); r < a.n_regions; r += wave_items()) {
        const uintptr_t src = reinterpret_cast<uintptr_t>(a.src[r]), dst = reinterpret_cast<uintptr_t>(a.dst[r]);
        const uint64_t n64 = a.bytes[r];
        const uint32_t scan = a.scan[r];
        if ((src & 15u) != 0u || (dst & 3u) != 0u || n64 == 0u || n64 > kPacket || scan == kSparseNone) {
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
            continue;
        }
        const uint32_t n = static_cast<uint32_t>(n64), fill = scan & 255u, k = scan >> 8;
        const CrcPacket p = {reinterpret_cast<const uint8_t *>(src), n};
        CrcQuad q[8];
        crc_load(q, p, lane);
        const uint32_t have = lane_have(n, lane);
        uint32_t slot;
        const uint32_t total = sparse_count(q, fill, have, lane, slot);
        if (total != k || 2u * k >= n) {                     // wave-uniform; nothing has been written
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
            continue;
        }
        if (lane == 0u) *reinterpret_cast<PlanesGlobalWord *>(dst) = sparse_head(fill, k);
        sparse_emit(dst, q, fill, k, have, lane, slot);
    }
}

struct SparseUnpackArgs {
    const uint8_t *const *rec;
    const uint64_t *rec_bytes;
    uint8_t *const *dst;
    const uint64_t *bytes;
    uint32_t n_regions;
    uint32_t *status;
};

// The packet builder: the n bytes (1 .. 8192) of the record at `rec` to dst (16-byte aligned), through `quads`, the wavefront's
// own 8 KiB of LDS.  The caller has checked the record's head (sparse_head_ok: 4 + 3 k <= rec_bytes, 2 k < n); Loose says how
// the positions are read: aligned u16 (false: sparse_unpack_kernel) or at any byte (true: kinds_expand_kernel).  The packet is filled by
// quads, the exceptions are scattered into it -- every position checked against n, the value against the fill and the position
// against the one in front BEFORE the LDS byte is written: no address is formed from an unchecked position --, and it is read
// back as quads and stored like move_packets_kernel's.  A record that fails a check is BAD_PACKET, its destination left as it
// was.  LDS operations of one wavefront complete in order: no barrier.
template <bool Loose>
__device__ __forceinline__ void sparse_build(PlanesQuad *quads, uintptr_t rec, uint32_t head, uint32_t n, uintptr_t dst, uint32_t lane, uint32_t *status) {
    const uint32_t fill = head & 255u, k = head >> 16;
    uint8_t *packet = reinterpret_cast<uint8_t *>(quads);
    // pos[i] under either type (a bool, not the pointer's type: a typedef's alignment does not travel through a template argument)
    const PlanesGlobalHalf *tight = reinterpret_cast<const PlanesGlobalHalf *>(rec + 4u);
    LooseHalf *loose = reinterpret_cast<LooseHalf *>(rec + 4u);
    const PlanesGlobalByte *val = reinterpret_cast<const PlanesGlobalByte *>(rec + 4u + 2u * k);
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j)
        if (16u * (lane + 64u * j) < n) quads[lane + 64u * j] = PlanesQuad(fill * kSparseLow);
    asm volatile("" ::: "memory");                           // the fill in front of the exceptions, which other lanes write
    bool bad = false;
    for (uint32_t i = lane; i < k; i += 64u) {
        const uint32_t at = Loose ? loose[i] : tight[i], v = val[i];
        const bool ascending = i == 0u || (Loose ? loose[i - 1u] : tight[i - 1u]) < at;
        if (at < n && v != fill && ascending) packet[at] = static_cast<uint8_t>(v);          // at < n <= 8192: inside the wavefront's LDS
        else bad = true;
    }
    if (__any(bad)) {                                        // wave-uniform
        if (lane == 0u) atomicOr(status, GPUAR_STATUS_BAD_PACKET);
    } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane's exceptions in front of the reads of whole quads
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t at = 16u * (lane + 64u * j);
            if (at >= n) continue;
            const PlanesQuad v = quads[lane + 64u * j];
            if (n - at >= 16u) reinterpret_cast<PlanesGlobalQuad *>(dst)[lane + 64u * j] = v;
            else store_partial_quad(dst + at, v, n - at);
        }
    }
    // On both paths: what this packet did to the LDS in front of the next packet's fill.  A refused record leaves bytes that
    // other lanes scattered; the compiler keeps those stores ahead of the fill anyway (a byte store may alias it), so on that path
    // the barrier costs nothing and only says what is relied on -- one exit, one barrier, rather than one kernel with and one without.
    asm volatile("" ::: "memory");
}

__global__ void __launch_bounds__(kSparseWaves * kLanes)
sparse_unpack_kernel(SparseUnpackArgs a) {
    __shared__ PlanesQuad lds[kSparseWaves * (kPacket / 16u)];
    const uint32_t lane = threadIdx.x & 63u;
    PlanesQuad *quads = lds + (threadIdx.x >> 6) * (kPacket / 16u);          // the wavefront's own packet
    for (uint64_t r = wave_item(); r < a.n_regions; r += wave_items()) {
        const uintptr_t rec = reinterpret_cast<uintptr_t>(a.rec[r]), dst = reinterpret_cast<uintptr_t>(a.dst[r]);
        const uint64_t rec_bytes = a.rec_bytes[r], n64 = a.bytes[r];
        if ((rec & 3u) != 0u || (dst & 15u) != 0u || n64 == 0u || n64 > kPacket) {
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
            continue;
        }
        const uint32_t n = static_cast<uint32_t>(n64);
        const uint32_t head = rec_bytes >= 4u ? __builtin_amdgcn_readfirstlane(*reinterpret_cast<const PlanesGlobalWord *>(rec)) : 0xFFFFFFFFu;
        if (rec_bytes < 4u || !sparse_head_ok(head, rec_bytes, n)) {         // wave-uniform; nothing behind the head is read
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_PACKET);
            continue;
        }
        sparse_build<false>(quads, rec, head, n, dst, lane, a.status);
    }
}

// ---------------------------------------------------------------------------
// Raw and sparse packets in a packet stream (kinds.h): every packet keeps its 4-byte header, so a file's
// stream is still walked by `off += clen` and compacted by gpuar_hip_compact.  Two bandwidth-bound passes over ALL packets of
// one buffer (a pipeline chunk), one wavefront per packet, persistent; a coded packet's wavefront returns at once.
//
// kinds_store_kernel runs behind the encoder, which has filled every slot: it applies sparse_kind to est[p] and scan[p]
// (scan null: sparse off), writes kind[p], and overwrites the slot of a raw packet with header + bytes (the lane's 128 bytes in
// registers as crc_load leaves them, stored to slot + 4 by 4-byte-aligned quads; the last partial quad by store_partial_quad)
// and the slot of a sparse packet with header + record: count, prefix sum and stores as sparse_count and sparse_emit have them
// (the same sparse_differ over the same registers), the total compared with scan >> 8 and the record's length with the slot
// BEFORE anything is written.  The kernel keeps that text as a copy of its own, for a measured reason: see in front of it.  A
// scan word that is not that of the bytes: BAD_BATCH, the slot stays the encoder's, kind[p] = 0 -- the stream is still valid.
//
// kinds_expand_kernel takes packet p of kind 1 or 2 out of a compacted stream, at any byte alignment, to out + 8192 p (16-byte
// aligned): the header is checked against offsets[p + 1] - offsets[p] and the packet's bytes in n_bytes first (kinds.h); raw
// bytes go by destination-aligned 16-byte stores fed from unaligned loads (as gather_kernel), the last partial quad by dwords
// and bytes loaded one by one; a sparse packet is sparse_unpack_kernel's own sparse_build, with the positions read at any byte.
// Nothing before offsets[p] or from offsets[p + 1] on is read, nothing outside the packet's bytes is written.
// ---------------------------------------------------------------------------
struct KindsStoreArgs {
    const uint8_t *in;
    size_t n_bytes;
    const uint32_t *est;
    const uint32_t *scan;                   // null: sparse is off
    uint32_t stored_on;
    uint8_t *slots;
    uint8_t *kind;
    uint32_t n_packets;
    uint32_t *status;
};

__global__ void __launch_bounds__(kSparseWaves * kLanes)
kinds_store_kernel(KindsStoreArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    PlanesGlobalByte *kinds = reinterpret_cast<PlanesGlobalByte *>(reinterpret_cast<uintptr_t>(a.kind));
    for (uint64_t r = wave_item(); r < a.n_packets; r += wave_items()) {
        const size_t first = static_cast<size_t>(r) * kPacket;
        const uint32_t n = a.n_bytes - first < kPacket ? static_cast<uint32_t>(a.n_bytes - first) : kPacket;
        const uint32_t est = __builtin_amdgcn_readfirstlane(a.est[r]);
        const uint32_t scan = a.scan ? __builtin_amdgcn_readfirstlane(a.scan[r]) : kSparseNone;
        const uint32_t kind = sparse_kind(scan, est, n, a.stored_on != 0u);         // wave-uniform
        if (kind == kSparseCoded) {                          // the slot is the encoder's
            if (lane == 0u) kinds[r] = static_cast<uint8_t>(kSparseCoded);
            continue;
        }
        const uintptr_t slot = reinterpret_cast<uintptr_t>(a.slots) + static_cast<size_t>(r) * kSlot;
        const CrcPacket p = {a.in + first, n};
        CrcQuad q[8];
        crc_load(q, p, lane);
        const uint32_t have = lane_have(n, lane);
        if (kind == kSparseRaw) {                            // 4 + n <= 8196 bytes of the slot
            if (lane == 0u) {
                *reinterpret_cast<PlanesGlobalWord *>(slot) = kinds_header(kinds_raw_clen(n), n);
                kinds[r] = static_cast<uint8_t>(kSparseRaw);
            }
            const uintptr_t dst = slot + kKindsHeader + kCrcChunk * lane;
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) {
                const uint32_t at = 16u * i;
                if (at >= have) continue;
                if (have - at >= 16u) *reinterpret_cast<GlobalQuad4 *>(dst + at) = q[i];
                else store_partial_quad(dst + at, q[i], have - at);
            }
            continue;
        }
        const uint32_t fill = scan & 255u, k = scan >> 8;   // (sparse_kind took the word: it is not kSparseNone)
        // sparse_count and, behind the check, sparse_emit, written out.  Through the two functions the kernel
        // needs 168 vector registers instead of 248, a third wavefront fits a SIMD, and the RAW path above then takes 7.5 ms
        // instead of 4.8 on 8 GiB of raw packets: its stores, 16 bytes per lane at a stride of 128, get slower with more of them
        // in flight.  Capping the occupancy by attribute costs 250 registers.  When the raw path has another layout, call them.
        uint32_t mine = 0;                                   // the lane's exceptions
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) mine += __popc(sparse_differ(w[j], fill, 16u * i + 4u * j, have));
        }
        uint32_t upto = mine;                                // inclusive prefix sum over the wave
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t below = __shfl_up(upto, off);
            if (lane >= off) upto += below;
        }
        const uint32_t total = __shfl(upto, 63);
        if (total != k || 2u * k >= n || kinds_sparse_clen(k) > kSlot) {      // wave-uniform; nothing has been written to the slot
            if (lane == 0u) {
                atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
                kinds[r] = static_cast<uint8_t>(kSparseCoded);
            }
            continue;
        }
        if (lane == 0u) {
            *reinterpret_cast<PlanesGlobalWord *>(slot) = kinds_header(kinds_sparse_clen(k), n);
            *reinterpret_cast<PlanesGlobalWord *>(slot + kKindsHeader) = sparse_head(fill, k);
            kinds[r] = static_cast<uint8_t>(kSparseSparse);
        }
        PlanesGlobalHalf *pos = reinterpret_cast<PlanesGlobalHalf *>(slot + kKindsHeader + 4u);
        PlanesGlobalByte *val = reinterpret_cast<PlanesGlobalByte *>(slot + kKindsHeader + 4u + 2u * k);
        if (lane < sparse_len(k) - (4u + 3u * k)) val[k + lane] = 0;           // the pad
        uint32_t at_slot = upto - mine;                      // < k wherever a store below is reached: the same predicate was counted
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t at = 16u * i + 4u * j;
                const uint32_t differ = sparse_differ(w[j], fill, at, have);
                if (differ != 0u) {
#pragma unroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        if (differ & (0x80u << (8u * b))) {
                            pos[at_slot] = static_cast<uint16_t>(kCrcChunk * lane + at + b);
                            val[at_slot] = static_cast<uint8_t>(w[j] >> (8u * b));
                            ++at_slot;
                        }
                    }
                }
            }
        }
    }
}

struct KindsExpandArgs {
    const uint8_t *stream;
    const uint64_t *offsets;
    const uint8_t *kind;
    uint32_t n_packets;
    uint8_t *out;
    size_t n_bytes;
    uint32_t *status;
};

__global__ void __launch_bounds__(kSparseWaves * kLanes)
kinds_expand_kernel(KindsExpandArgs a) {
    __shared__ PlanesQuad lds[kSparseWaves * (kPacket / 16u)];
    const uint32_t lane = threadIdx.x & 63u;
    PlanesQuad *quads = lds + (threadIdx.x >> 6) * (kPacket / 16u);          // the wavefront's own packet
    const PlanesGlobalByte *kinds = reinterpret_cast<const PlanesGlobalByte *>(reinterpret_cast<uintptr_t>(a.kind));
    for (uint64_t r = wave_item(); r < a.n_packets; r += wave_items()) {
        const uint32_t kind = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(kinds[r]));
        if (kind == kSparseCoded) continue;                  // the decoder's
        const size_t first = static_cast<size_t>(r) * kPacket;
        const uint32_t n = a.n_bytes - first < kPacket ? static_cast<uint32_t>(a.n_bytes - first) : kPacket;
        const uint64_t off = a.offsets[r], end = a.offsets[r + 1u];
        const uint64_t pkt_bytes = end - off;
        if (kind > kSparseSparse || end < off || pkt_bytes < kKindsHeader || pkt_bytes > kSlot) {        // wave-uniform; nothing of the stream is read
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_PACKET);
            continue;
        }
        const uintptr_t src = reinterpret_cast<uintptr_t>(a.stream) + off, dst = reinterpret_cast<uintptr_t>(a.out) + first;
        const uint32_t header = __builtin_amdgcn_readfirstlane(*reinterpret_cast<LooseWord *>(src));
        if (kind == kSparseRaw) {
            if (!kinds_raw_ok(header, pkt_bytes, n)) {       // the destination is left as it was
                if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_PACKET);
                continue;
            }
            const uintptr_t body = src + kKindsHeader;       // n bytes: up to offsets[r + 1]
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t at = 16u * (lane + 64u * j);
                if (at >= n) continue;
                const uint32_t left = n - at;
                if (left >= 16u) {
                    const PlanesQuad whole = *reinterpret_cast<LooseQuad *>(body + at);
                    reinterpret_cast<PlanesGlobalQuad *>(dst)[lane + 64u * j] = whole;
                } else {
                    // store_partial_quad's shape, kept apart from it: that one takes the whole quad in registers, and a 16-byte load
                    // here would read from offsets[r + 1] on.  Each dword and byte is loaded only where it is stored.
                    PlanesGlobalWord *words = reinterpret_cast<PlanesGlobalWord *>(dst + at);
                    PlanesGlobalByte *bytes = reinterpret_cast<PlanesGlobalByte *>(dst + at);
#pragma unroll
                    for (uint32_t d = 0; d < 4; ++d) {
                        if (4u * d + 4u <= left) {
                            words[d] = *reinterpret_cast<LooseWord *>(body + at + 4u * d);
                        } else {
#pragma unroll
                            for (uint32_t b = 0; b < 3; ++b)
                                if (4u * d + b < left) bytes[4u * d + b] = *reinterpret_cast<const PlanesGlobalByte *>(body + at + 4u * d + b);
                        }
                    }
                }
            }
            continue;
        }
        const uintptr_t rec = src + kKindsHeader;
        const uint64_t rec_bytes = pkt_bytes - kKindsHeader;
        const uint32_t head = kinds_header_ok(header, pkt_bytes, n) && rec_bytes >= 4u
                                  ? __builtin_amdgcn_readfirstlane(*reinterpret_cast<LooseWord *>(rec)) : 0xFFFFFFFFu;
        if (!kinds_header_ok(header, pkt_bytes, n) || rec_bytes < 4u || !sparse_head_ok(head, rec_bytes, n)) {      // wave-uniform; nothing behind the head is read
            if (lane == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_PACKET);
            continue;
        }
        sparse_build<true>(quads, rec, head, n, dst, lane, a.status);
    }
}

// move_bytes_kernel: region r is bytes[r] (1 .. 8704; 0 moves nothing) bytes from src[r] to dst[r], both at ANY
// byte alignment -- the packets of a version-6 .gip stream taken apart into the three regions of a batch.Compressed.  The shape is
// gather_kernel's, with its workgroup of 256 threads (the size gather_kernel's own sweep chose for regions of this length): the
// bytes up to dst's first 16-byte boundary (head, 0 .. 15) and those behind its last (tail, 0 .. 15) go by single bytes from 32
// lanes of the last wavefront, the quads between by destination-aligned 16-byte stores fed from byte-exact unaligned loads: three
// rounds at most.  Every load lies in [src, src + bytes) and every store in [dst, dst + bytes): destinations may stand back to
// back at byte grain.  A null pointer or bytes > 8704: BAD_BATCH, the region is skipped.
constexpr uint32_t kMoveBytesThreads = 256;

__global__ void __launch_bounds__(kMoveBytesThreads)
move_bytes_kernel(MoveArgs a) {
    using GlobalQuad = __attribute__((address_space(1))) PlanesQuad;
    using GlobalByte = __attribute__((address_space(1))) uint8_t;
    using LooseQuad = const __attribute__((address_space(1))) KindsQuad1;
    for (uint64_t r = blockIdx.x; r < a.n_regions; r += gridDim.x) {
        const uintptr_t src = reinterpret_cast<uintptr_t>(a.src[r]), dst = reinterpret_cast<uintptr_t>(a.dst[r]);
        const uint64_t n = a.bytes[r];
        if (src == 0u || dst == 0u || n > kSlot) {           // uniform over the workgroup; nothing is read or written
            if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
            continue;
        }
        const uint32_t len = static_cast<uint32_t>(n);
        uint32_t head = static_cast<uint32_t>((16u - (dst & 15u)) & 15u);
        if (head > len) head = len;
        const uint32_t body = (len - head) & ~15u;           // head + body <= len: whole quads of dst, all inside the region
        const uint32_t tail = len - head - body;
        for (uint32_t at = threadIdx.x * 16u; at < body; at += kMoveBytesThreads * 16u) {
            const PlanesQuad whole = *reinterpret_cast<LooseQuad *>(src + head + at);
            *reinterpret_cast<GlobalQuad *>(dst + head + at) = whole;
        }
        // the ragged ends: of the last wavefront's upper half, lanes 0 .. 15 take the head and lanes 16 .. 31 the tail
        const uint32_t spare = threadIdx.x - (kMoveBytesThreads - 32u);
        if (spare < head) *reinterpret_cast<GlobalByte *>(dst + spare) = *reinterpret_cast<const GlobalByte *>(src + spare);
        else if (spare >= 16u && spare - 16u < tail)
            *reinterpret_cast<GlobalByte *>(dst + head + body + spare - 16u) = *reinterpret_cast<const GlobalByte *>(src + head + body + spare - 16u);
    }
}

// ---------------------------------------------------------------------------
// Plane-width survey (survey.h): est[j][p] = estimate(split_planes(buffer, 1 << j))[p] for the four widths at
// once, from one read of the original bytes and without making any split, for one buffer or a batch.
//
// One workgroup of 8 wavefronts per SUPERGROUP (8 packets = 65536 bytes of one buffer), persistent over the supergroups, two
// workgroups resident per CU.  Wavefront e reads eighth e as estimate_kernel reads a packet (lane l: bytes [128 l, 128 l + 128)
// as eight 16-byte loads) and counts it into the eighth's 8 residue histograms h[e][r], r = byte offset mod 8: bin s of residue
// r at dword 2048 e + 8 s + r, 8 KiB per wavefront, 64 KiB in all -- u32 counters, because packed u16 increments cost three
// more vector instructions per byte (4.7) and 64 KiB already fits twice in a CU.  A byte's residue is its position in its
// 8-byte pair, so one lane's eight adds go to eight histograms; so that the 64 lanes of ONE add do not, every lane rotates its
// pair by (lane & 7) bytes first (two v_alignbyte_b32 and two selects per 8 bytes): in step t a lane counts its byte
// (t + lane) & 7, and a packet of equal bytes spreads every add over 8 counters in 8 banks, as estimate_kernel's copies do.
// Behind a barrier, thread (half, s) sums, for bin s, the 32 counters of its half's four eighths into the bin of 4 packets of
// each width (for w = 8: its half's four residues, with the other half's eighths), looks the 16 counts up in LF, and 16 wave
// sums, a 1 KiB exchange and 32 threads give the 32 estimates: one writer each.
// A buffer's last, short supergroup (1 .. 65535 bytes) takes the general path: each byte is added to the packet histogram it
// lands in at each width (survey_packet: the tail rule of planes.h), 32 histograms of 256 u32 in the same LDS.  It reads by
// 16-byte pieces, never beyond the piece that holds the last byte, and is bounded by one supergroup per buffer.
// In a batch, window u = batch packets [8 u, 8 u + 8) belongs to one workgroup, which takes every supergroup that STARTS there
// (one for a large buffer, up to eight for short ones).  A buffer the survey cannot take -- misaligned, or not owning exactly
// the packets its bytes make -- is BAD_BATCH and none of its entries is written; so is a packet nobody owns.
// ---------------------------------------------------------------------------
constexpr uint32_t kSurveyWaves = 8;                                    // one wavefront per eighth
constexpr uint32_t kSurveyThreads = kSurveyWaves * kLanes;
constexpr uint32_t kSurveyEighthDwords = 8u * 256u;                     // 8 residues x 256 bins
constexpr uint32_t kSurveyGroups = 512;                                 // two workgroups per CU of an MI355X (65 KiB of LDS each)

struct SurveyArgs {
    const uint8_t *in;                      // one buffer: `in`, `n_bytes` ...
    size_t n_bytes;
    const uint8_t *const *ptrs;             // ... or a batch (ptrs != nullptr)
    const uint64_t *bytes;
    const uint64_t *first_packet;
    uint32_t n_buffers;
    uint32_t n_packets;
    uint32_t *est;                          // row j at est + j * stride
    size_t stride;
    uint32_t *status;
};

// the 8 bytes {lo, hi} of a lane, rotated by c = lane & 7 bytes: step t counts byte (t + c) & 7 into residue (t + c) & 7, whose
// histogram (and the wavefront's base) is in slot[t]
__device__ __forceinline__ void survey_count8(uint32_t *hist, uint32_t lo, uint32_t hi, uint32_t c, const uint32_t (&slot)[8]) {
    const uint32_t a = __builtin_amdgcn_alignbyte(hi, lo, c & 3u), b = __builtin_amdgcn_alignbyte(lo, hi, c & 3u);
    const uint32_t first = (c & 4u) ? b : a, second = (c & 4u) ? a : b;
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) {
        __hip_atomic_fetch_add(hist + (((first >> (8u * t)) & 255u) * 8u + slot[t]), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(hist + (((second >> (8u * t)) & 255u) * 8u + slot[4u + t]), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// The pieces the three surveys (this one, the delta survey and the XOR-base survey below) are made of.

// The walk over windows and descriptors with the supergroup's work as a parameter: every supergroup that starts in one of this
// workgroup's windows goes to body(sg, bs, len, first) -- `len` bytes (1 .. 65536) at `sg`, whose first packet is batch packet
// `first` -- and every unusable descriptor to BAD_BATCH.  kBased: the XOR survey's walk, with a base beside the buffer (`base`,
// or one pointer per buffer in `bases`); bs is the base's bytes of the supergroup, null where a batch's base pointer is 0 ("no
// base"), and a base pointer that is not 16-byte aligned makes its buffer BAD_BATCH.  Otherwise bs is null at compile time.
template <bool kBased, typename Body>
__device__ __forceinline__ void survey_walk(const SurveyArgs &a, const uint8_t *base, const uint8_t *const *bases, Body body) {
    const uint32_t n_windows = (a.n_packets >> 3) + ((a.n_packets & 7u) ? 1u : 0u);
    for (uint32_t u = blockIdx.x; u < n_windows; u += gridDim.x) {
        uint64_t p = 8ull * u;
        const uint64_t end = p + 8u < a.n_packets ? p + 8u : a.n_packets;
        while (p < end) {                   // (every value here is the same in all threads)
            const uint8_t *sg = nullptr, *bs = nullptr;
            uint64_t left = 0, next = end;  // left: the buffer's bytes from this supergroup on; 0: nothing to survey at p
            if (!a.ptrs) {                  // one buffer: the window is the supergroup
                sg = a.in + p * kPacket;
                if constexpr (kBased) bs = base + p * kPacket;
                left = a.n_bytes - p * kPacket;
            } else {
                const BatchLane bl = batch_lane(a.ptrs, a.bytes, a.first_packet, a.n_buffers, p);
                if (!bl.owned && bl.ptr == nullptr) {                  // no buffer owns the packet
                    if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
                    next = p + 1u;
                } else {
                    const uint64_t lead = a.first_packet[bl.buffer], behind = a.first_packet[bl.buffer + 1u], n_bytes = a.bytes[bl.buffer];
                    const uint8_t *own = nullptr;                      // the buffer's base
                    if constexpr (kBased) own = bases[bl.buffer];
                    const uint64_t j = p - lead;
                    next = p + 8u - (j & 7u) < behind ? p + 8u - (j & 7u) : behind;      // the buffer's next supergroup, or the next buffer
                    if (!bl.owned || (reinterpret_cast<uintptr_t>(own) & 15u) != 0u || behind - lead != (n_bytes + kPacket - 1u) / kPacket) {
                        if (threadIdx.x == 0u) atomicOr(a.status, GPUAR_STATUS_BAD_BATCH);
                    } else if ((j & 7u) == 0u) {                       // (else: the supergroup started in another window)
                        sg = bl.ptr;
                        bs = own ? own + j * kPacket : nullptr;
                        left = n_bytes - j * kPacket;
                    }
                }
            }
            const uint32_t len = __builtin_amdgcn_readfirstlane(left < kSurveyBytes ? static_cast<uint32_t>(left) : kSurveyBytes);
            if (len != 0u) body(sg, bs, len, p);
            p = next;
        }
    }
}

// every kernel's first step: the histograms clear, and a barrier
__device__ __forceinline__ void survey_prologue(CrcQuad *lds) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) lds[threadIdx.x + kSurveyThreads * k] = CrcQuad(0u);
    __syncthreads();
}

// slot[t]: the wavefront's base and the residue (t + c) & 7, c = lane & 7, that survey_count8's step t counts into
__device__ __forceinline__ void survey_slots(uint32_t wave, uint32_t lane, uint32_t (&slot)[8]) {
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) slot[t] = wave * kSurveyEighthDwords + ((t + (lane & 7u)) & 7u);
}

// a full supergroup's bytes of this lane: [128 lane, 128 lane + 128) of eighth `wave` as eight 16-byte loads -- XORed, where
// there is a base (bs != nullptr), with the same bytes of the base
template <bool kXor>
__device__ __forceinline__ void survey_load8(const uint8_t *sg, const uint8_t *bs, uint32_t wave, uint32_t lane, CrcQuad (&q)[8]) {
    using GlobalQuad = const __attribute__((address_space(1))) CrcQuad;
    const uint32_t at = wave * kPacket + kCrcChunk * lane;
    GlobalQuad *src = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(sg + at));
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) q[k] = src[k];
    if constexpr (kXor) {
        if (bs != nullptr) {                                                 // workgroup-uniform
            GlobalQuad *bsrc = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(bs + at));
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const CrcQuad b = bsrc[k];
                q[k].x ^= b.x, q[k].y ^= b.y, q[k].z ^= b.z, q[k].w ^= b.w;
            }
        }
    }
}

// the general path's fill: every byte of the short supergroup (XORed with the base's, where there is one) into packet histogram
// (j, p) at dword (8 j + p) * 256, for every width j
template <bool kXor>
__device__ __forceinline__ void survey_short(uint32_t *hist, const uint8_t *sg, const uint8_t *bs, uint32_t len) {
    using GlobalQuad = const __attribute__((address_space(1))) CrcQuad;
    GlobalQuad *src = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(sg));
    GlobalQuad *bsrc = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(bs));
    for (uint32_t i = threadIdx.x; i * 16u < len; i += kSurveyThreads) {
        const CrcQuad q = src[i];
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
        if constexpr (kXor) {
            if (bs != nullptr) {
                const CrcQuad b = bsrc[i];
                w[0] ^= b.x, w[1] ^= b.y, w[2] ^= b.z, w[3] ^= b.w;
            }
        }
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
#pragma unroll 1
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t o = 16u * i + 4u * d + b, byte = (w[d] >> (8u * b)) & 255u;
                if (o >= len) break;
#pragma unroll
                for (uint32_t j = 0; j < kSurveyWidths; ++j)
                    __hip_atomic_fetch_add(hist + ((j * kSurveyPackets + survey_packet(o, len, j)) * 256u + byte), 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
}

// cnt[4 j + m]: bin s of packet 4 half + m at width 1 << j -- of a full supergroup from the residue histograms, of a short one
// from the packet histograms
__device__ __forceinline__ void survey_counts16(const CrcQuad *lds, bool full, uint32_t half, uint32_t s, uint32_t (&cnt)[16]) {
    if (full) {
        CrcQuad lo[4], hi[4], other[4];      // residues 0-3 and 4-7 of the half's own eighths; residues 4 half .. + 3 of the other half's
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            lo[e] = lds[((4u * half + e) * kSurveyEighthDwords + 8u * s) / 4u];
            hi[e] = lds[((4u * half + e) * kSurveyEighthDwords + 8u * s) / 4u + 1u];
            other[e] = lds[((4u * (1u - half) + e) * kSurveyEighthDwords + 8u * s) / 4u + half];
        }
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) cnt[e] = lo[e].x + lo[e].y + lo[e].z + lo[e].w + hi[e].x + hi[e].y + hi[e].z + hi[e].w;
#pragma unroll
        for (uint32_t g = 0; g < 2; ++g) {
            const CrcQuad t = lo[2 * g] + hi[2 * g] + lo[2 * g + 1] + hi[2 * g + 1];
            cnt[4 + 2 * g] = t.x + t.z;
            cnt[4 + 2 * g + 1] = t.y + t.w;
        }
        const CrcQuad l4 = lo[0] + lo[1] + lo[2] + lo[3], h4 = hi[0] + hi[1] + hi[2] + hi[3];
        const CrcQuad w4 = l4 + h4, w8 = (half ? h4 : l4) + other[0] + other[1] + other[2] + other[3];
        cnt[8] = w4.x, cnt[9] = w4.y, cnt[10] = w4.z, cnt[11] = w4.w;
        cnt[12] = w8.x, cnt[13] = w8.y, cnt[14] = w8.z, cnt[15] = w8.w;
    } else {
        const uint32_t *hist = reinterpret_cast<const uint32_t *>(lds);
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) cnt[i] = hist[((i >> 2) * kSurveyPackets + 4u * half + (i & 3u)) * 256u + s];
    }
}

// a value's trip to lane ^ off: a 64-bit one as the two __shfl_xor of its halves
__device__ __forceinline__ uint32_t lane_swap(uint32_t v, uint32_t off) { return __shfl_xor(v, off); }
__device__ __forceinline__ uint64_t lane_swap(uint64_t v, uint32_t off) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), off), hi = __shfl_xor(static_cast<uint32_t>(v >> 32), off);
    return static_cast<uint64_t>(hi) << 32 | lo;
}

// N wave reductions by `op` in N - 1 + log2(64 / N) exchanges instead of 6 N (N = 16: 17 instead of 96): every step halves the
// values a lane carries (it keeps the half its lane bit names and hands the other half to its partner), then a plain butterfly
// over the offsets left, so lane l ends with the whole wavefront's result for value l / (64 / N) in v[0]
template <uint32_t N, typename T, typename Op>
__device__ __forceinline__ void wave_fold(T (&v)[N], uint32_t lane, Op op) {
    static_assert(N >= 2u && N <= 64u && (N & (N - 1u)) == 0u, "a power of two of values, at most one per lane");
#pragma unroll
    for (uint32_t n = N / 2u, off = 32; n >= 1; n >>= 1, off >>= 1) {
        const bool upper = (lane & off) != 0u;
#pragma unroll
        for (uint32_t m = 0; m < n; ++m) {
            const T low = v[m], high = v[m + n];                  // (values, so that the choice is of registers and never of addresses)
            v[m] = op(upper ? high : low, lane_swap(upper ? low : high, off));
        }
    }
#pragma unroll
    for (uint32_t off = 32u / N; off >= 1; off >>= 1) v[0] = op(v[0], lane_swap(v[0], off));
}

// every counter was read in front of the barrier before: clear them (thread (half, s): both quads of bin s of its four eighths)
__device__ __forceinline__ void survey_clear(CrcQuad *lds, uint32_t half, uint32_t s) {
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
        lds[((4u * half + e) * kSurveyEighthDwords + 8u * s) / 4u] = CrcQuad(0u);
        lds[((4u * half + e) * kSurveyEighthDwords + 8u * s) / 4u + 1u] = CrcQuad(0u);
    }
}

// the bytes of packet p of a supergroup of `len` bytes (p * kPacket < len)
__device__ __forceinline__ uint32_t survey_packet_bytes(uint32_t len, uint32_t p) {
    return len - p * kPacket < kPacket ? len - p * kPacket : kPacket;
}

// one estimate, one writer: packet p of the supergroup at width 1 << j, from column `col` of the exchange of its half's four
// wave sums, into entry first + p of row j
template <uint32_t N>
__device__ __forceinline__ void survey_store_est(uint32_t *est_rows, size_t stride, uint32_t j, uint64_t first, uint32_t p, uint32_t len,
                                                 const uint64_t (*sums)[N], uint32_t col) {
    using GlobalLf = const __attribute__((address_space(1))) uint64_t;
    using GlobalWord = __attribute__((address_space(1))) uint32_t;
    GlobalLf *lf = reinterpret_cast<GlobalLf *>(reinterpret_cast<uintptr_t>(g_est_table.lf));
    const uint32_t w0 = p & ~3u, count = survey_packet_bytes(len, p);
    const uint64_t total = sums[w0][col] + sums[w0 + 1u][col] + sums[w0 + 2u][col] + sums[w0 + 3u][col];
    GlobalWord *est = reinterpret_cast<GlobalWord *>(reinterpret_cast<uintptr_t>(est_rows));
    est[j * stride + first + p] = est_clen_from_sum(lf[count + 255u], lf[255], total);
}

// one supergroup of the plane survey (kXor = false: bs, scan and keys unused, a.est there) and of the XOR-base survey (kXor = true:
// the bytes counted are the buffer's XORed with the base's unless bs is null, and a.est or scan may be null): `len` bytes
// (1 .. 65536) at `sg` and at `bs` (both 16-byte aligned), whose first packet is entry `first` of every row; the whole workgroup,
// with the histograms clear on entry and on return
template <bool kXor>
__device__ __forceinline__ void survey_supergroup(const SurveyArgs &a, uint32_t *scan, const uint8_t *sg, const uint8_t *bs, uint32_t len,
                                                  uint64_t first, CrcQuad *lds, uint64_t (*sums)[16], uint32_t (*keys)[16]) {
    using GlobalLf = const __attribute__((address_space(1))) uint64_t;
    using GlobalWord = __attribute__((address_space(1))) uint32_t;
    GlobalLf *lf = reinterpret_cast<GlobalLf *>(reinterpret_cast<uintptr_t>(g_est_table.lf));
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t s = threadIdx.x & 255u, half = threadIdx.x >> 8;          // of the aggregation: bin s, eighths / packets 4 half .. + 3
    const bool full = len == kSurveyBytes;                                   // workgroup-uniform
    const bool want_est = !kXor || a.est != nullptr, want_scan = kXor && scan != nullptr;
    if (full) {
        CrcQuad q[8];
        survey_load8<kXor>(sg, bs, wave, lane, q);
        uint32_t slot[8];
        survey_slots(wave, lane, slot);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            survey_count8(hist, q[k].x, q[k].y, lane & 7u, slot);
            survey_count8(hist, q[k].z, q[k].w, lane & 7u, slot);
        }
    } else {
        survey_short<kXor>(hist, sg, bs, len);
    }
    __syncthreads();
    uint32_t cnt[16];
    survey_counts16(lds, full, half, s, cnt);
    // the scan words: 16 wave maxima of the keys (xor_scan_key: count << 8 | s), lane l ending with that of value l >> 2
    if (want_scan) {
        uint32_t key[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) key[i] = xor_scan_key(cnt[i], s);
        wave_fold(key, lane, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
        if ((lane & 3u) == 0u) keys[wave][lane >> 2] = key[0];
    }
    // the estimates: 16 wave sums of the counts' LF
    if (want_est) {
        uint64_t sum[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) sum[i] = lf[cnt[i]];
        wave_fold(sum, lane, [](uint64_t x, uint64_t y) { return x + y; });
        if ((lane & 3u) == 0u) sums[wave][lane >> 2] = sum[0];
    }
    __syncthreads();
    survey_clear(lds, half, s);
    if (threadIdx.x < 32u) {
        const uint32_t i = threadIdx.x & 15u, hh = threadIdx.x >> 4, p = 4u * hh + (i & 3u);
        if (p * kPacket < len) {
            if (want_est) survey_store_est(a.est, a.stride, i >> 2, first, p, len, sums, i);
            if (want_scan) {
                const uint32_t k01 = keys[4u * hh][i] > keys[4u * hh + 1u][i] ? keys[4u * hh][i] : keys[4u * hh + 1u][i];
                const uint32_t k23 = keys[4u * hh + 2u][i] > keys[4u * hh + 3u][i] ? keys[4u * hh + 2u][i] : keys[4u * hh + 3u][i];
                GlobalWord *out = reinterpret_cast<GlobalWord *>(reinterpret_cast<uintptr_t>(scan));
                out[(i >> 2) * a.stride + first + p] = xor_scan_word(k01 > k23 ? k01 : k23, survey_packet_bytes(len, p));
            }
        }
    }
    __syncthreads();      // the clears and the reads of the exchanges in front of the next supergroup
}

__global__ void __launch_bounds__(kSurveyThreads) __attribute__((amdgpu_waves_per_eu(4)))      // two workgroups per CU: 128 VGPRs
survey_planes_kernel(SurveyArgs a) {
    __shared__ CrcQuad lds[kSurveyWaves * kSurveyEighthDwords / 4u];
    __shared__ uint64_t sums[kSurveyWaves][16];
    survey_prologue(lds);
    survey_walk<false>(a, nullptr, nullptr, [&](const uint8_t *sg, const uint8_t *, uint32_t len, uint64_t first) {
        survey_supergroup<false>(a, nullptr, sg, nullptr, len, first, lds, sums, nullptr);
    });
}

// ---------------------------------------------------------------------------
// Delta survey (delta_survey.h): est[j][p] = estimate(split_delta(buffer, 1 << j))[p] for the widths asked for
// (widths_mask, uniform over the launch), from one read of the original bytes and without filtering or splitting anything into
// memory, for one buffer or a batch.  Supergroups, windows, descriptors and BAD_BATCH are survey_planes_kernel's (survey_walk),
// and so is the workgroup: wavefront e loads eighth e once, lane l bytes [128 l, 128 l + 128) as eight 16-byte loads, and keeps
// those 32 dwords in registers for all widths.
// The filtered byte at a position differs per width, so the widths take turns with the one set of counters.  For a width the lane
// filters its 128 bytes in registers (delta.h's delta_block over 16 elements at a time, with the element in front: the last
// one of the block before, of the lane before -- two lane shuffles --, for lane 0 the 8 bytes in front of the eighth, loaded
// once, and 0 where a group starts, e mod w = 0) and counts them into its wavefront's eight residue histograms exactly as the
// plane survey counts unfiltered bytes: the filter is for data whose differences are constant, so all lanes on one counter is
// this kernel's typical input and the rotation by (lane & 7) (survey_count8) what keeps it off one bank.  Behind a barrier
// thread (half, s) sums bin s of this width's packets 4 half .. + 3 (the sums survey.h lists), looks the four counts up in LF;
// four wave sums in 7 u64 exchanges, a 256-byte exchange and 8 threads give the width's 8 estimates: one writer each.  The counters
// are cleared behind a second barrier and a third one lets the next width count: three barriers a width.
// A buffer's last, short supergroup (1 .. 65535 bytes) takes the general path, width by width: a thread takes 8-byte pieces
// (whole elements at every width, since groups and tails start on multiples of 8192) with the 8 bytes in front, forms the
// differences (delta_sub; the tail's whole elements only, the predecessor reset where a group or the tail starts) and adds
// every byte to the packet histogram survey_packet names: 8 histograms of 256 u32 in the same LDS.  It reads nothing in front of
// the supergroup and nothing beyond the 16-byte piece that holds its last byte, and is bounded by one supergroup per buffer.
// ---------------------------------------------------------------------------
struct DeltaSurveyArgs {
    SurveyArgs s;
    uint32_t widths_mask;                   // bit j: row j (width 1 << j) is wanted
};

// the last W-byte element of the 8 bytes {lo, hi}
template <int W>
__device__ __forceinline__ uint64_t dsurvey_last(uint32_t lo, uint32_t hi) {
    if constexpr (W == 8) return static_cast<uint64_t>(hi) << 32 | lo;
    else if constexpr (W == 4) return hi;
    else return hi >> (32 - 8 * W);
}

// the lane's 128 bytes `d` filtered at width W and counted; {front_lo, front_hi}: the 8 bytes in front of them
template <int W>
__device__ __forceinline__ void dsurvey_count(uint32_t *hist, const uint32_t (&d)[32], uint32_t front_lo, uint32_t front_hi, bool group_start,
                                              uint32_t c, const uint32_t (&slot)[8]) {
    constexpr int D = 4 * W;                // dwords of a block of 16 elements
    uint64_t pred = group_start ? 0ull : dsurvey_last<W>(front_lo, front_hi);
#pragma unroll
    for (int b = 0; b < 32 / D; ++b) {
        uint32_t m[D];
#pragma unroll
        for (int i = 0; i < D; ++i) m[i] = d[D * b + i];
        delta_block<W>(m, pred);
        pred = dsurvey_last<W>(d[D * b + D - 2], d[D * b + D - 1]);
#pragma unroll
        for (int i = 0; i < D; i += 2) survey_count8(hist, m[i], m[i + 1], c, slot);
    }
}

// the general path at width W: the short supergroup's filtered bytes into packet histogram p at dword 256 p
template <int W, int J>
__device__ __forceinline__ void dsurvey_short(uint32_t *hist, const uint8_t *sg, uint32_t len) {
    using GlobalWord = const __attribute__((address_space(1))) uint32_t;
    GlobalWord *src = reinterpret_cast<GlobalWord *>(reinterpret_cast<uintptr_t>(sg));
    constexpr uint32_t G = W * kPacket;
    for (uint32_t i = threadIdx.x; i * 8u < len; i += kSurveyThreads) {
        const uint32_t o = 8u * i, B = o & ~(G - 1u);
        const uint32_t whole = (len - B < G ? len - B : G) & ~static_cast<uint32_t>(W - 1);      // the group's or the tail's whole elements
        const uint32_t lo = src[2u * i], hi = src[2u * i + 1u];
        uint32_t before = 0, front = 0;      // the dword in front of the piece, and the one in front of that (W = 8): 0 at a reset
        if (o != B) front = src[2u * i - 1u];
        if (W == 8 && o != B) before = src[2u * i - 2u];
        uint32_t f_lo, f_hi;
        if constexpr (W == 8) {
            const uint64_t dif = (static_cast<uint64_t>(hi) << 32 | lo) - (static_cast<uint64_t>(front) << 32 | before);
            f_lo = static_cast<uint32_t>(dif), f_hi = static_cast<uint32_t>(dif >> 32);
        } else if constexpr (W == 4) {
            f_lo = delta_sub<W>(lo, front), f_hi = delta_sub<W>(hi, lo);
        } else {
            f_lo = delta_sub<W>(lo, lo << (8 * W) | front >> (32 - 8 * W)), f_hi = delta_sub<W>(hi, hi << (8 * W) | lo >> (32 - 8 * W));
        }
#pragma unroll 1
        for (uint32_t b = 0; b < 8u; ++b) {
            const uint32_t at = o + b;
            if (at >= len) break;
            const bool filtered = at - B < whole;      // (else: the tail's last bytes, as they are)
            const uint32_t word = b < 4u ? (filtered ? f_lo : lo) : (filtered ? f_hi : hi);
            const uint32_t byte = (word >> (8u * (b & 3u))) & 255u;
            __hip_atomic_fetch_add(hist + (survey_packet(at, len, J) * 256u + byte), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// bin s of the packets 4 half .. + 3 of a full supergroup at width 1 << J, from the residue histograms
template <int J>
__device__ __forceinline__ void dsurvey_bins(const CrcQuad *lds, uint32_t half, uint32_t s, uint32_t (&cnt)[4]) {
    if constexpr (J == 3) {                 // packet k: residue k of all eighths
        CrcQuad t = CrcQuad(0u);
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e) t += lds[(e * kSurveyEighthDwords + 8u * s) / 4u + half];
        cnt[0] = t.x, cnt[1] = t.y, cnt[2] = t.z, cnt[3] = t.w;
    } else {
        CrcQuad t[4];                       // residues r and r + 4 of the half's own eighths
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
            t[e] = lds[((4u * half + e) * kSurveyEighthDwords + 8u * s) / 4u] + lds[((4u * half + e) * kSurveyEighthDwords + 8u * s) / 4u + 1u];
        if constexpr (J == 0) {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) cnt[e] = t[e].x + t[e].y + t[e].z + t[e].w;
        } else if constexpr (J == 1) {
#pragma unroll
            for (uint32_t g = 0; g < 2; ++g) {
                const CrcQuad u = t[2 * g] + t[2 * g + 1];
                cnt[2 * g] = u.x + u.z;
                cnt[2 * g + 1] = u.y + u.w;
            }
        } else {
            const CrcQuad u = t[0] + t[1] + t[2] + t[3];
            cnt[0] = u.x, cnt[1] = u.y, cnt[2] = u.z, cnt[3] = u.w;
        }
    }
}

// one width of one supergroup; the whole workgroup, with the counters clear on entry and on return
template <int J>
__device__ __forceinline__ void dsurvey_width(const DeltaSurveyArgs &a, const uint8_t *sg, uint32_t len, uint64_t first, const uint32_t (&d)[32],
                                              uint32_t front_lo, uint32_t front_hi, CrcQuad *lds, uint64_t (*sums)[4]) {
    using GlobalLf = const __attribute__((address_space(1))) uint64_t;
    constexpr int W = 1 << J;
    GlobalLf *lf = reinterpret_cast<GlobalLf *>(reinterpret_cast<uintptr_t>(g_est_table.lf));
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t s = threadIdx.x & 255u, half = threadIdx.x >> 8;          // of the aggregation: bin s, packets 4 half .. + 3
    const bool full = len == kSurveyBytes;                                   // workgroup-uniform
    if (full) {
        const uint32_t c = lane & 7u;
        uint32_t slot[8];                   // survey_slots, written out (see dsurvey_supergroup)
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) slot[t] = wave * kSurveyEighthDwords + ((t + c) & 7u);
        dsurvey_count<W>(hist, d, front_lo, front_hi, lane == 0u && (wave & (W - 1u)) == 0u, c, slot);
    } else {
        dsurvey_short<W, J>(hist, sg, len);
    }
    __syncthreads();
    uint32_t cnt[4];
    if (full) {
        dsurvey_bins<J>(lds, half, s, cnt);
    } else {
#pragma unroll
        for (uint32_t m = 0; m < 4; ++m) cnt[m] = hist[(4u * half + m) * 256u + s];
    }
    // four wave sums: wave_fold<4>, written out (see dsurvey_supergroup) -- two steps halve the values a lane carries, four more
    // sum value lane >> 4 up
    uint64_t sum[4];
#pragma unroll
    for (uint32_t m = 0; m < 4; ++m) sum[m] = lf[cnt[m]];
#pragma unroll
    for (uint32_t n = 2, off = 32; n >= 1; n >>= 1, off >>= 1) {
        const bool upper = (lane & off) != 0u;
#pragma unroll
        for (uint32_t m = 0; m < n; ++m) {
            const uint64_t keep = upper ? sum[m + n] : sum[m], give = upper ? sum[m] : sum[m + n];
            const uint32_t lo = __shfl_xor(static_cast<uint32_t>(give), off), hi = __shfl_xor(static_cast<uint32_t>(give >> 32), off);
            sum[m] = keep + (static_cast<uint64_t>(hi) << 32 | lo);
        }
    }
#pragma unroll
    for (uint32_t off = 8; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(sum[0]), off), hi = __shfl_xor(static_cast<uint32_t>(sum[0] >> 32), off);
        sum[0] += static_cast<uint64_t>(hi) << 32 | lo;
    }
    if ((lane & 15u) == 0u) sums[wave][lane >> 4] = sum[0];
    __syncthreads();
    survey_clear(lds, half, s);
    if (threadIdx.x < 8u && threadIdx.x * kPacket < len) survey_store_est(a.s.est, a.s.stride, J, first, threadIdx.x, len, sums, threadIdx.x & 3u);
    __syncthreads();      // the clears and the reads of `sums` in front of the next width
}

// one supergroup: `len` bytes (1 .. 65536) at `sg` (16-byte aligned), whose first packet is entry `first` of every row.
// This kernel takes the walk, the prologue, the clear and the estimate writer from the plane survey and keeps three pieces written
// out, survey_load8 here and survey_slots and wave_fold<4> in dsurvey_width, for a measured reason.  With all three shared the
// kernel was 231 instructions shorter (wave_fold chooses between registers where the text below makes the compiler index sum[]
// through compare-and-select chains) and 0.8 % faster with all four widths on 8 GiB, but a single width of incompressible bytes
// was slower in both of two alternating runs against the kernel as it is here: w = 1 on uniform bytes 2.530 / 2.546 ms against
// 2.462 / 2.457 ms, w = 1 on bf16 2.534 / 2.545 against 2.462 / 2.461, w = 2 on uniform 2.587 / 2.590 against 2.555 / 2.548; with
// only the reduction written out it was slower still (w = 1 on uniform 2.568 / 2.550 against 2.460 / 2.454).  Why was not found:
// the kernel and the LF table lie at the same addresses in all three code objects and the loads and their waits are the same;
// what differs is register allocation and address arithmetic throughout.  With these three written out the instruction stream
// is the one that was measured as the faster.
__device__ __forceinline__ void dsurvey_supergroup(const DeltaSurveyArgs &a, const uint8_t *sg, uint32_t len, uint64_t first, CrcQuad *lds,
                                                   uint64_t (*sums)[4]) {
    using GlobalQuad = const __attribute__((address_space(1))) CrcQuad;
    using GlobalWord = const __attribute__((address_space(1))) uint32_t;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t d[32] = {}, front_lo = 0, front_hi = 0;
    if (len == kSurveyBytes) {                                               // workgroup-uniform
        GlobalQuad *src = reinterpret_cast<GlobalQuad *>(reinterpret_cast<uintptr_t>(sg + wave * kPacket + kCrcChunk * lane));
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const CrcQuad q = src[k];
            d[4 * k] = q.x, d[4 * k + 1] = q.y, d[4 * k + 2] = q.z, d[4 * k + 3] = q.w;
        }
        if (wave != 0u) {                                                    // (nothing is read in front of the supergroup)
            GlobalWord *front = reinterpret_cast<GlobalWord *>(reinterpret_cast<uintptr_t>(sg + wave * kPacket - 8u));
            front_lo = front[0], front_hi = front[1];
        }
        const uint32_t up_lo = __shfl_up(d[30], 1), up_hi = __shfl_up(d[31], 1);
        if (lane != 0u) front_lo = up_lo, front_hi = up_hi;
    }
    if (a.widths_mask & 1u) dsurvey_width<0>(a, sg, len, first, d, front_lo, front_hi, lds, sums);
    if (a.widths_mask & 2u) dsurvey_width<1>(a, sg, len, first, d, front_lo, front_hi, lds, sums);
    if (a.widths_mask & 4u) dsurvey_width<2>(a, sg, len, first, d, front_lo, front_hi, lds, sums);
    if (a.widths_mask & 8u) dsurvey_width<3>(a, sg, len, first, d, front_lo, front_hi, lds, sums);
}

__global__ void __launch_bounds__(kSurveyThreads) __attribute__((amdgpu_waves_per_eu(4)))      // two workgroups per CU: 128 VGPRs
survey_delta_kernel(DeltaSurveyArgs a) {
    __shared__ CrcQuad lds[kSurveyWaves * kSurveyEighthDwords / 4u];
    __shared__ uint64_t sums[kSurveyWaves][4];
    survey_prologue(lds);
    survey_walk<false>(a.s, nullptr, nullptr, [&](const uint8_t *sg, const uint8_t *, uint32_t len, uint64_t first) {
        dsurvey_supergroup(a, sg, len, first, lds, sums);
    });
}

// ---------------------------------------------------------------------------
// XOR-base survey (xor_survey.h): est[j][p] = estimate(split_xor(buffer, base, 1 << j))[p] and scan[j][p] =
// sparse_scan(split_xor(buffer, base, 1 << j))[p] for the four widths at once, from one read of the buffer and one of its base and
// without XORing or splitting anything into memory, for one buffer or a batch.  XOR commutes with the regrouping, so this is the
// plane survey of buffer ^ base and runs that survey's own code: survey_walk<true> (the walk with a base beside the buffer) and
// survey_supergroup<true> (the XOR in front of the count, a second reduction behind it).  Wavefront e loads eighth e of the
// buffer and of the base, lane l bytes [128 l, 128 l + 128) of each as eight 16-byte loads, XORs them in registers and counts the
// result with survey_count8: a tensor equal to its base is all zeros, all lanes on one bin, which is what the rotation by
// (lane & 7) is for.
// Behind the barrier thread (half, s) forms the plane survey's 16 counts of bin s.  The estimates leave through the sum exchange;
// the scan words through a second reduction of the same shape over 32-bit keys (xor_scan_key: count << 8 | s) by MAXIMUM --
// a packet's majority byte, if it has one, is its fullest bin -- with an exchange of 8 x 16 words and one writer per entry.
// A short supergroup takes the general path, with the base read by the same 16-byte pieces and the same two reductions.
// Either output may be missing (null): its reduction is skipped and nothing of it is written.
// In a batch a base pointer of 0 means "no base": the buffer's rows are the plane survey's, with scan rows beside them.  A base
// pointer that is not 16-byte aligned makes its buffer BAD_BATCH, as a misaligned buffer is: none of its entries is written.
// ---------------------------------------------------------------------------
struct XorSurveyArgs {
    SurveyArgs s;                           // s.est may be null
    const uint8_t *base;                    // one buffer: its base ...
    const uint8_t *const *bases;            // ... or a batch: one pointer per buffer, 0: no base
    uint32_t *scan;                         // row j at scan + j * s.stride; may be null
};

__global__ void __launch_bounds__(kSurveyThreads) __attribute__((amdgpu_waves_per_eu(4)))      // two workgroups per CU: 128 VGPRs
survey_xor_kernel(XorSurveyArgs a) {
    __shared__ CrcQuad lds[kSurveyWaves * kSurveyEighthDwords / 4u];
    __shared__ uint64_t sums[kSurveyWaves][16];
    __shared__ uint32_t keys[kSurveyWaves][16];
    survey_prologue(lds);
    survey_walk<true>(a.s, a.base, a.bases, [&](const uint8_t *sg, const uint8_t *bs, uint32_t len, uint64_t first) {
        survey_supergroup<true>(a.s, a.scan, sg, bs, len, first, lds, sums, keys);
    });
}

// gpuar_hip_status: reads and clears the fallback word in ONE device atomic.  A bit that another launch ORs in at any
// moment is then either in what this exchange returns or still in the word for the next call; a copy to the host
// followed by a separate clear would drop a bit that arrives between the two.
__global__ void __launch_bounds__(kLanes)
take_status_kernel() {
    if (threadIdx.x == 0) g_status_taken = atomicExch(&g_status, 0u);
}

}  // namespace gpuar

// ===========================================================================
// C ABI (include/gpuar_hip.h)
// ===========================================================================
namespace {

thread_local int t_last_error = GPUAR_OK;

constexpr size_t kMaxCount = 0xFFFFFFFFull;            // packets, buffers or regions of one call: the kernels count in 32 bits

// The alignment test of every pointer argument: data, slots and outputs 16, descriptor arrays and 64-bit words 8, 32-bit words and
// records 4.  A null pointer passes: whether it may be null is another test.
inline bool misaligned(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1u)) != 0; }

// The grid of every kernel that strides over its work: one workgroup for every `per` items, `cap` at most.
constexpr uint32_t capped_blocks(uint64_t n, uint32_t per, uint32_t cap) {
    const uint64_t groups = n / per + (n % per ? 1u : 0u);
    return static_cast<uint32_t>(groups < cap ? groups : cap);
}

// The same rule in the other spellings a launch may carry, in the width each kernel counts in: the compiler holds capped_blocks to
// them at the edges of every (per, cap) in use.
constexpr uint32_t blocks_added(uint64_t n, uint32_t per, uint32_t cap) {                  // CRC, estimate, sparse scan
    const size_t groups = (static_cast<size_t>(n) + per - 1) / per;
    return static_cast<uint32_t>(groups < cap ? groups : cap);
}
constexpr uint32_t blocks_shifted(uint64_t n, uint32_t, uint32_t cap) {                    // the surveys: windows of 8 packets
    const uint32_t windows = (static_cast<uint32_t>(n) >> 3) + ((static_cast<uint32_t>(n) & 7u) ? 1u : 0u);
    return windows < cap ? windows : cap;
}
constexpr uint32_t blocks_divided(uint64_t n, uint32_t per, uint32_t cap) {                // sparse pack / unpack, kinds; per = 1: filters, move
    const uint32_t groups = static_cast<uint32_t>(n) / per + (static_cast<uint32_t>(n) % per ? 1u : 0u);
    return groups < cap ? groups : cap;
}
constexpr bool same_blocks(uint32_t (*old)(uint64_t, uint32_t, uint32_t), uint32_t per, uint32_t cap) {
    const uint64_t edge = static_cast<uint64_t>(cap) * per;
    for (const uint64_t n : {uint64_t{0}, uint64_t{1}, uint64_t{per} - 1, uint64_t{per}, uint64_t{per} + 1, edge, edge + 1})
        if (capped_blocks(n, per, cap) != old(n, per, cap)) return false;
    return true;
}
static_assert(same_blocks(blocks_added, gpuar::kCrcWaves, gpuar::kCrcGroups) && same_blocks(blocks_added, gpuar::kEstWaves, gpuar::kEstGroups) &&
              same_blocks(blocks_shifted, 8u, gpuar::kSurveyGroups) && same_blocks(blocks_added, gpuar::kSparseWaves, gpuar::kSparseGroups) &&
              same_blocks(blocks_divided, gpuar::kSparseWaves, gpuar::kSparseGroups) &&
              same_blocks(blocks_divided, gpuar::kSparseWaves, gpuar::kPlaneGridCap) && same_blocks(blocks_divided, 1u, gpuar::kPlaneGridCap),
              "capped_blocks is not the grid of one of the launches");

int check_launch() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPUAR_OK : static_cast<int>(e);
}

// Where a launch reports SLOT_OVERFLOW / BAD_PACKET: the caller's own device word, or -- for callers that pass
// none (the reference-named executors) -- the current device's fallback word, which gpuar_hip_status() reads.
uint32_t *status_word(uint32_t *d_status) {
    if (d_status) return d_status;
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(gpuar::g_status)) != hipSuccess) return nullptr;
    return static_cast<uint32_t *>(p);
}

// The filters' launches (byte planes, delta, XOR against a base): the full-group kernel over the packets, then the tail kernel
// over the buffers that have a tail.  `args` is what the filter's kernels take, `p` the PlanesArgs inside it.
template <typename Args>
struct FilterKernels {
    void (*split)(Args);
    void (*merge)(Args);
    void (*split_tail)(Args);
    void (*merge_tail)(Args);
};
const FilterKernels<gpuar::PlanesArgs> kPlanesKernels = {gpuar::split_planes_kernel, gpuar::merge_planes_kernel,
                                                                gpuar::planes_tail_kernel<false>, gpuar::planes_tail_kernel<true>};
const FilterKernels<gpuar::DeltaArgs> kDeltaKernels = {gpuar::split_delta_kernel, gpuar::merge_delta_kernel,
                                                              gpuar::delta_tail_kernel<false>, gpuar::delta_tail_kernel<true>};
const FilterKernels<gpuar::XorArgs> kXorKernels = {gpuar::split_xor_kernel, gpuar::merge_xor_kernel,
                                                          gpuar::xor_tail_kernel<false>, gpuar::xor_tail_kernel<true>};

template <typename Args>
int launch_filter(const FilterKernels<Args> &kernels, bool merge, const Args &args, const gpuar::PlanesArgs &p, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    // a batch: any buffer may have a tail; one buffer: it has one or not
    const size_t n_tails = p.in_ptrs ? p.n_buffers : (p.n_bytes % (static_cast<size_t>(p.elem) * GPUAR_PACKET_BYTES) ? 1u : 0u);
    const uint32_t tails = capped_blocks(n_tails, 1u, gpuar::kPlaneGridCap);
    (merge ? kernels.merge : kernels.split)<<<capped_blocks(p.n_packets, 1u, gpuar::kPlaneGridCap), gpuar::kPlaneThreads, 0, s>>>(args);
    const int e = check_launch();
    if (e != GPUAR_OK || tails == 0u) return e;
    (merge ? kernels.merge_tail : kernels.split_tail)<<<tails, gpuar::kPlaneThreads, 0, s>>>(args);
    return check_launch();
}

// the host-side checks every batch call makes before any device work; d_packets (the slots or the stream) must be aligned to
// packets_align bytes; *status_out: where the launch reports
int batch_arguments(const void *d_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet, size_t n_buffers, size_t n_packets,
                    const void *d_packets, uintptr_t packets_align, uint32_t *d_status, uint32_t **status_out) {
    if (!d_ptrs || !d_bytes || !d_first_packet || !d_packets) return GPUAR_ERR_ARGUMENT;
    if (n_packets > kMaxCount || n_buffers > kMaxCount) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_ptrs, 8) || misaligned(d_bytes, 8) || misaligned(d_first_packet, 8) || misaligned(d_status, 4) ||
        misaligned(d_packets, packets_align))
        return GPUAR_ERR_ALIGNMENT;
    *status_out = status_word(d_status);
    return *status_out ? GPUAR_OK : GPUAR_ERR_NO_DEVICE;
}

// The source of a per-packet kernel, in the fields every such kernel's arguments (CrcArgs, SurveyArgs, KindsStoreArgs) name alike:
// one buffer ...
template <typename Args>
Args buffer_source(const uint8_t *d_in, size_t n_bytes, uint32_t *status) {
    Args a = {};
    a.in = d_in;
    a.n_bytes = n_bytes;
    a.n_packets = static_cast<uint32_t>(gpuar_hip_packet_count(n_bytes));
    a.status = status;
    return a;
}

// ... or a batch
template <typename Args>
Args batch_source(const uint8_t *const *d_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet, size_t n_buffers, size_t n_packets,
                  uint32_t *status) {
    Args a = {};
    a.ptrs = d_ptrs;
    a.bytes = d_bytes;
    a.first_packet = d_first_packet;
    a.n_buffers = static_cast<uint32_t>(n_buffers);
    a.n_packets = static_cast<uint32_t>(n_packets);
    a.status = status;
    return a;
}

// The checks of a per-packet call on one buffer that takes one array of 32-bit words (d_words: CRCs, estimates, scan words) and
// maybe a 64-bit word (d_word64), in the order include/gpuar_hip.h gives: nothing to do; `own_ok`, the test of the call's own
// values (the surveys' stride and mask); null pointers and the packet count; alignments; the status word.  *a: the call's source,
// once *launch says there is something to launch.
template <typename Args>
int packet_checks(bool own_ok, const uint8_t *d_data, size_t n_bytes, const uint32_t *d_words, const uint64_t *d_word64, uint32_t *d_status,
                  Args *a, bool *launch) {
    *launch = false;
    if (n_bytes == 0) return GPUAR_OK;
    if (!own_ok || !d_data || !d_words || gpuar_hip_packet_count(n_bytes) > kMaxCount) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_data, 16) || misaligned(d_words, 4) || misaligned(d_word64, 8) || misaligned(d_status, 4)) return GPUAR_ERR_ALIGNMENT;
    uint32_t *status = status_word(d_status);
    if (!status) return GPUAR_ERR_NO_DEVICE;
    *a = buffer_source<Args>(d_data, n_bytes, status);
    *launch = true;
    return GPUAR_OK;
}

// The same on a batch: d_words (4) and d_word64 (8) in front of batch_arguments' checks, where the buffers' pointer array stands in
// for the packets (8-byte aligned).
template <typename Args>
int packet_batch_checks(bool own_ok, const uint8_t *const *d_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet, size_t n_buffers,
                        size_t n_packets, const uint32_t *d_words, const uint64_t *d_word64, uint32_t *d_status, Args *a, bool *launch) {
    *launch = false;
    if (n_packets == 0) return GPUAR_OK;
    if (!own_ok || !d_words || !d_ptrs || !d_bytes || !d_first_packet || n_packets > kMaxCount || n_buffers > kMaxCount) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_words, 4) || misaligned(d_word64, 8)) return GPUAR_ERR_ALIGNMENT;
    uint32_t *status = nullptr;
    const int e = batch_arguments(d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_ptrs, 8u, d_status, &status);
    if (e != GPUAR_OK) return e;
    *a = batch_source<Args>(d_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, status);
    *launch = true;
    return GPUAR_OK;
}

// The frame of a per-region call (move_packets, sparse_pack, sparse_unpack): `a` with the call's pointers in place, which are also
// listed by alignment -- d_arrays8: the descriptor arrays, d_arrays4: arrays of 32-bit words.  Nothing to do; a null array or too
// many regions; a misaligned array or status word; the status word; one workgroup for every `per` regions.
template <typename Args>
int region_call(void (*kernel)(Args), uint32_t per, uint32_t threads, Args a, std::initializer_list<const void *> d_arrays8,
                std::initializer_list<const void *> d_arrays4, size_t n_regions, uint32_t *d_status, void *stream) {
    if (n_regions == 0) return GPUAR_OK;
    bool missing = n_regions > kMaxCount, skewed = misaligned(d_status, 4);
    for (const void *p : d_arrays8) {
        missing |= !p;
        skewed |= misaligned(p, 8);
    }
    for (const void *p : d_arrays4) {
        missing |= !p;
        skewed |= misaligned(p, 4);
    }
    if (missing) return GPUAR_ERR_ARGUMENT;
    if (skewed) return GPUAR_ERR_ALIGNMENT;
    a.n_regions = static_cast<uint32_t>(n_regions);
    a.status = status_word(d_status);
    if (!a.status) return GPUAR_ERR_NO_DEVICE;
    kernel<<<capped_blocks(a.n_regions, per, gpuar::kPlaneGridCap), threads, 0, static_cast<hipStream_t>(stream)>>>(a);
    return check_launch();
}

}  // namespace

extern "C" {

size_t gpuar_hip_packet_count(size_t n_bytes) { return (n_bytes + GPUAR_PACKET_BYTES - 1) / GPUAR_PACKET_BYTES; }

int gpuar_hip_encode_mode(const uint8_t *d_in, size_t n_bytes, uint8_t *d_slots, uint32_t *d_status, void *stream, int mode) {
    if (mode != GPUAR_MODE_AUTO && mode != GPUAR_MODE_THROUGHPUT && mode != GPUAR_MODE_LATENCY && mode != GPUAR_MODE_TABLE) return GPUAR_ERR_ARGUMENT;
    if (n_bytes == 0) return GPUAR_OK;
    if (!d_in || !d_slots) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_in, 16) || misaligned(d_slots, 16) || misaligned(d_status, 4)) return GPUAR_ERR_ALIGNMENT;
    uint32_t *status = status_word(d_status);
    if (!status) return GPUAR_ERR_NO_DEVICE;
    const size_t n_packets = gpuar_hip_packet_count(n_bytes);
    if (n_packets > kMaxCount) return GPUAR_ERR_ARGUMENT;
    const uint32_t groups = static_cast<uint32_t>((n_packets + gpuar::kLanes - 1) / gpuar::kLanes);
    // Small inputs cannot fill the chip and take as long as one packet: left to itself (GPUAR_MODE_AUTO) such a launch
    // goes to the latency-mode kernel (six working roles and a courier, a shorter step).  The slots are the same bytes either way; the
    // caller's `mode` is the only switch (no environment is read here).
    const bool latency = mode == GPUAR_MODE_LATENCY || (mode == GPUAR_MODE_AUTO && groups <= gpuar::kSmallGroups);
    if (latency) {
        gpuar::encode_small_kernel<<<groups, gpuar::kSmallWaves * gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(
            d_in, n_bytes, d_slots, static_cast<uint32_t>(n_packets), status);
        return check_launch();
    }
    const uint32_t blocks = (groups + 7u) & ~7u;              // see xcd_contiguous_group
    // Above that switch AUTO takes the table walk (encode_kernel_t16: the same roles, seven vector instructions fewer per symbol);
    // THROUGHPUT names encode_kernel, the batch kernels' twin, and TABLE the table walk at any size.
    if (mode == GPUAR_MODE_THROUGHPUT)
        gpuar::encode_kernel<<<blocks, 4 * gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(
            d_in, n_bytes, d_slots, static_cast<uint32_t>(n_packets), status);
    else
        gpuar::encode_kernel_t16<<<blocks, 4 * gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(
            d_in, n_bytes, d_slots, static_cast<uint32_t>(n_packets), status);
    return check_launch();
}

int gpuar_hip_encode(const uint8_t *d_in, size_t n_bytes, uint8_t *d_slots, uint32_t *d_status, void *stream) {
    return gpuar_hip_encode_mode(d_in, n_bytes, d_slots, d_status, stream, GPUAR_MODE_AUTO);
}

// n_bytes: how much of d_slots may be read (n_packets * 8704, or less when the last slot is a partial one)
static int launch_decode_slots(const uint8_t *d_slots, size_t n_packets, size_t n_bytes, uint8_t *d_out, uint32_t *d_status, void *stream) {
    if (n_packets == 0) return GPUAR_OK;
    if (!d_slots || !d_out || n_packets > kMaxCount) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_slots, 16) || misaligned(d_out, 16) || misaligned(d_status, 4)) return GPUAR_ERR_ALIGNMENT;
    uint32_t *status = status_word(d_status);
    if (!status) return GPUAR_ERR_NO_DEVICE;
    const uint32_t blocks = static_cast<uint32_t>((n_packets + gpuar::kLanes - 1) / gpuar::kLanes);
    gpuar::decode_slots_kernel<<<blocks, gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(
        d_slots, static_cast<uint32_t>(n_packets), n_bytes, d_out, status);
    return check_launch();
}

int gpuar_hip_decode(const uint8_t *d_slots, size_t n_packets, uint8_t *d_out, uint32_t *d_status, void *stream) {
    return launch_decode_slots(d_slots, n_packets, n_packets * static_cast<size_t>(GPUAR_SLOT_BYTES), d_out, d_status, stream);
}

int gpuar_hip_compact(const uint8_t *d_slots, size_t n_packets, uint8_t *d_stream, uint64_t *d_offsets, void *stream) {
    if (!d_offsets) return GPUAR_ERR_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_packets == 0) {
        const hipError_t e = hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), s);
        return e == hipSuccess ? GPUAR_OK : static_cast<int>(e);
    }
    if (!d_slots || !d_stream) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_slots, 16) || misaligned(d_offsets, 8) || misaligned(d_stream, 8)) return GPUAR_ERR_ALIGNMENT;
    // the gather launches one workgroup per packet, and gridDim.x * blockDim.x must stay below 2^32 threads: 16.7 M packets
    // = 128 GiB of input per call with 256-thread workgroups (a device holds 288 GB; the CLI compacts 512 MiB chunks)
    if (n_packets * static_cast<size_t>(gpuar::kGatherThreads) > 0xFFFFFFFFull) return GPUAR_ERR_ARGUMENT;
    const size_t tiles = (n_packets + gpuar::kScanTile - 1) / gpuar::kScanTile;
    const uint32_t np = static_cast<uint32_t>(n_packets);
    // scratch until the gather overwrites it; with two tiles or more there are >= 4097 packets of >= 4 bytes behind it
    uint64_t *tile_prefix = tiles > 1 ? reinterpret_cast<uint64_t *>(d_stream) : nullptr;
    if (tile_prefix) {
        gpuar::scan_tile_sums_kernel<<<static_cast<uint32_t>(tiles), gpuar::kScanThreads, 0, s>>>(d_slots, np, tile_prefix);
        gpuar::scan_tile_prefix_kernel<<<1, gpuar::kScanThreads, 0, s>>>(static_cast<uint32_t>(tiles), tile_prefix);
    }
    gpuar::scan_offsets_kernel<<<static_cast<uint32_t>(tiles), gpuar::kScanThreads, 0, s>>>(d_slots, np, d_offsets, tile_prefix);
    gpuar::gather_kernel<<<np, gpuar::kGatherThreads, 0, s>>>(d_slots, d_offsets, np, d_stream);
    return check_launch();
}

int gpuar_hip_decode_stream(const uint8_t *d_stream, const uint64_t *d_offsets, size_t n_packets,
                            uint8_t *d_out, uint32_t *d_status, void *stream) {
    if (n_packets == 0) return GPUAR_OK;
    if (!d_stream || !d_offsets || !d_out || n_packets > kMaxCount) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_out, 16) || misaligned(d_stream, 4) || misaligned(d_status, 4)) return GPUAR_ERR_ALIGNMENT;
    uint32_t *status = status_word(d_status);
    if (!status) return GPUAR_ERR_NO_DEVICE;
    const uint32_t blocks = static_cast<uint32_t>((n_packets + gpuar::kLanes - 1) / gpuar::kLanes);
    gpuar::decode_stream_kernel<<<blocks, gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(
        d_stream, d_offsets, static_cast<uint32_t>(n_packets), d_out, status);
    return check_launch();
}

size_t gpuar_hip_batch_packet_count(const uint64_t *bytes, size_t n_buffers, uint64_t *first_packet) {
    if (n_buffers && !bytes) return 0;
    size_t total = 0;
    for (size_t b = 0; b < n_buffers; ++b) {
        if (first_packet) first_packet[b] = total;
        total += gpuar_hip_packet_count(bytes[b]);
    }
    if (first_packet) first_packet[n_buffers] = total;
    return total;
}

int gpuar_hip_encode_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                           size_t n_buffers, size_t n_packets, uint8_t *d_slots, uint32_t *d_status, void *stream, int mode) {
    if (mode != GPUAR_MODE_AUTO && mode != GPUAR_MODE_THROUGHPUT && mode != GPUAR_MODE_LATENCY) return GPUAR_ERR_ARGUMENT;
    if (n_packets == 0) return GPUAR_OK;
    uint32_t *status = nullptr;
    const int e = batch_arguments(d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, d_slots, 16u, d_status, &status);
    if (e != GPUAR_OK) return e;
    const uint32_t groups = static_cast<uint32_t>((n_packets + gpuar::kLanes - 1) / gpuar::kLanes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool latency = mode == GPUAR_MODE_LATENCY || (mode == GPUAR_MODE_AUTO && groups <= gpuar::kSmallGroups);   // as gpuar_hip_encode_mode
    if (latency) {
        gpuar::encode_small_batch_kernel<<<groups, gpuar::kSmallWaves * gpuar::kLanes, 0, s>>>(
            d_in_ptrs, d_in_bytes, d_first_packet, static_cast<uint32_t>(n_buffers), static_cast<uint32_t>(n_packets), d_slots, status);
        return check_launch();
    }
    const uint32_t blocks = (groups + 7u) & ~7u;              // see xcd_contiguous_group
    gpuar::encode_batch_kernel<<<blocks, 4 * gpuar::kLanes, 0, s>>>(
        d_in_ptrs, d_in_bytes, d_first_packet, static_cast<uint32_t>(n_buffers), static_cast<uint32_t>(n_packets), d_slots, status);
    return check_launch();
}

int gpuar_hip_decode_batch(const uint8_t *d_slots, const uint64_t *d_first_packet, size_t n_buffers, size_t n_packets,
                           uint8_t *const *d_out_ptrs, const uint64_t *d_out_bytes, uint32_t *d_status, void *stream) {
    if (n_packets == 0) return GPUAR_OK;
    uint32_t *status = nullptr;
    const int e = batch_arguments(d_out_ptrs, d_out_bytes, d_first_packet, n_buffers, n_packets, d_slots, 16u, d_status, &status);
    if (e != GPUAR_OK) return e;
    const uint32_t blocks = static_cast<uint32_t>((n_packets + gpuar::kLanes - 1) / gpuar::kLanes);
    gpuar::decode_slots_batch_kernel<<<blocks, gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(
        d_slots, d_first_packet, static_cast<uint32_t>(n_buffers), static_cast<uint32_t>(n_packets), d_out_ptrs, d_out_bytes, status);
    return check_launch();
}

int gpuar_hip_decode_stream_batch(const uint8_t *d_stream, const uint64_t *d_offsets, const uint64_t *d_first_packet,
                                  size_t n_buffers, size_t n_packets, uint8_t *const *d_out_ptrs,
                                  const uint64_t *d_out_bytes, uint32_t *d_status, void *stream) {
    if (n_packets == 0) return GPUAR_OK;
    if (!d_offsets) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_offsets, 8)) return GPUAR_ERR_ALIGNMENT;
    uint32_t *status = nullptr;
    const int e = batch_arguments(d_out_ptrs, d_out_bytes, d_first_packet, n_buffers, n_packets, d_stream, 4u, d_status, &status);
    if (e != GPUAR_OK) return e;
    const uint32_t blocks = static_cast<uint32_t>((n_packets + gpuar::kLanes - 1) / gpuar::kLanes);
    gpuar::decode_stream_batch_kernel<<<blocks, gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(
        d_stream, d_offsets, d_first_packet, static_cast<uint32_t>(n_buffers), static_cast<uint32_t>(n_packets), d_out_ptrs, d_out_bytes, status);
    return check_launch();
}

static int launch_crc32(bool verify, const gpuar::CrcArgs &a, void *stream) {
    const uint32_t blocks = capped_blocks(a.n_packets, gpuar::kCrcWaves, gpuar::kCrcGroups);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (verify) gpuar::crc32_kernel<true><<<blocks, gpuar::kCrcWaves * gpuar::kLanes, 0, s>>>(a);
    else gpuar::crc32_kernel<false><<<blocks, gpuar::kCrcWaves * gpuar::kLanes, 0, s>>>(a);
    return check_launch();
}

int gpuar_hip_crc32(const uint8_t *d_in, size_t n_bytes, uint32_t *d_crc, void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_checks(true, d_in, n_bytes, d_crc, nullptr, nullptr, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = d_crc;
    return launch_crc32(false, a, stream);
}

int gpuar_hip_verify_crc32(const uint8_t *d_out, size_t n_bytes, const uint32_t *d_crc, uint64_t *d_first_bad, uint32_t *d_status,
                           void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_checks(true, d_out, n_bytes, d_crc, d_first_bad, d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = const_cast<uint32_t *>(d_crc);
    a.first_bad = reinterpret_cast<unsigned long long *>(d_first_bad);
    return launch_crc32(true, a, stream);
}

int gpuar_hip_crc32_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                          size_t n_buffers, size_t n_packets, uint32_t *d_crc, uint32_t *d_status, void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_batch_checks(true, d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, d_crc, nullptr, d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = d_crc;
    return launch_crc32(false, a, stream);
}

int gpuar_hip_verify_crc32_batch(const uint8_t *const *d_out_ptrs, const uint64_t *d_out_bytes,
                                 const uint64_t *d_first_packet, size_t n_buffers, size_t n_packets,
                                 const uint32_t *d_crc, uint64_t *d_first_bad, uint32_t *d_status, void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_batch_checks(true, d_out_ptrs, d_out_bytes, d_first_packet, n_buffers, n_packets, d_crc, d_first_bad, d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = const_cast<uint32_t *>(d_crc);
    a.first_bad = reinterpret_cast<unsigned long long *>(d_first_bad);
    return launch_crc32(true, a, stream);
}

static bool ranges_meet(uintptr_t a, uintptr_t b, size_t n_bytes) { return a < b + n_bytes && b < a + n_bytes; }

// The checks of a single-buffer filter call, on the device or (on_host: no packet limit, no alignment) on the host, in the order
// the calls have always made them; `based`: the call takes a base, which is only read.  *work: there is something to do.
static int filter_checks(bool on_host, const uint8_t *in, bool based, const uint8_t *base, size_t n_bytes, uint32_t elem_bytes,
                         const uint8_t *out, bool *work) {
    *work = false;
    if (!gpuar::planes_width_ok(elem_bytes)) return GPUAR_ERR_ARGUMENT;
    if (n_bytes == 0) return GPUAR_OK;
    if (!in || !out || (based && !base)) return GPUAR_ERR_ARGUMENT;
    if (!on_host && gpuar_hip_packet_count(n_bytes) > kMaxCount) return GPUAR_ERR_ARGUMENT;
    if (!on_host && (misaligned(in, 16) || misaligned(out, 16) || (based && misaligned(base, 16)))) return GPUAR_ERR_ALIGNMENT;
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    if (a != b && ranges_meet(a, b, n_bytes)) return GPUAR_ERR_ARGUMENT;                        // in place or apart, nothing in between
    if (based && ranges_meet(reinterpret_cast<uintptr_t>(base), b, n_bytes)) return GPUAR_ERR_ARGUMENT;
    *work = true;
    return GPUAR_OK;
}

// one buffer on the device: the checks, then the PlanesArgs of its launch
static int single_arguments(const uint8_t *d_in, bool based, const uint8_t *d_base, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out,
                            gpuar::PlanesArgs *p, bool *launch) {
    const int e = filter_checks(false, d_in, based, d_base, n_bytes, elem_bytes, d_out, launch);
    if (e != GPUAR_OK || !*launch) return e;
    p->in = d_in;
    p->out = d_out;
    p->n_bytes = n_bytes;
    p->elem = elem_bytes;
    p->n_packets = static_cast<uint32_t>(gpuar_hip_packet_count(n_bytes));
    return GPUAR_OK;
}

// a batch: the checks of its descriptors -- `d_extra` is the one that delta (filter) and XOR (base_ptrs) add, `extra` whether the
// call has one -- then the PlanesArgs of its launch
static int batch_filter_arguments(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                  const uint64_t *d_elem_bytes, bool extra, const void *d_extra, size_t n_buffers, size_t n_packets,
                                  uint8_t *const *d_out_ptrs, uint32_t *d_status, gpuar::PlanesArgs *p, bool *launch) {
    *launch = false;
    if (n_packets == 0) return GPUAR_OK;
    if (!d_elem_bytes || (extra && !d_extra) || !d_out_ptrs) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_elem_bytes, 8) || (extra && misaligned(d_extra, 8)) || misaligned(d_out_ptrs, 8)) return GPUAR_ERR_ALIGNMENT;
    uint32_t *status = nullptr;
    const int e = batch_arguments(d_in_ptrs, d_bytes, d_first_packet, n_buffers, n_packets, d_in_ptrs, 8u, d_status, &status);
    if (e != GPUAR_OK) return e;
    p->in_ptrs = d_in_ptrs;
    p->out_ptrs = d_out_ptrs;
    p->bytes = d_bytes;
    p->first_packet = d_first_packet;
    p->elem_bytes = d_elem_bytes;
    p->n_buffers = static_cast<uint32_t>(n_buffers);
    p->n_packets = static_cast<uint32_t>(n_packets);
    p->status = status;
    *launch = true;
    return GPUAR_OK;
}

static int planes_single(bool merge, const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    gpuar::PlanesArgs a = {};
    bool launch = false;
    const int e = single_arguments(d_in, false, nullptr, n_bytes, elem_bytes, d_out, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    if (elem_bytes == 1u && d_in == d_out) return GPUAR_OK;                     // planes alone: a width of 1 in place is nothing
    return launch_filter(kPlanesKernels, merge, a, a, stream);
}

static int planes_batch(bool merge, const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                        const uint64_t *d_elem_bytes, size_t n_buffers, size_t n_packets, uint8_t *const *d_out_ptrs, uint32_t *d_status,
                        void *stream) {
    gpuar::PlanesArgs a = {};
    bool launch = false;
    const int e = batch_filter_arguments(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, false, nullptr, n_buffers, n_packets, d_out_ptrs,
                                         d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    return launch_filter(kPlanesKernels, merge, a, a, stream);
}

int gpuar_hip_split_planes(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    return planes_single(false, d_in, n_bytes, elem_bytes, d_out, stream);
}

int gpuar_hip_merge_planes(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    return planes_single(true, d_in, n_bytes, elem_bytes, d_out, stream);
}

int gpuar_hip_split_planes_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                 const uint64_t *d_elem_bytes, size_t n_buffers, size_t n_packets, uint8_t *const *d_out_ptrs,
                                 uint32_t *d_status, void *stream) {
    return planes_batch(false, d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, d_status, stream);
}

int gpuar_hip_merge_planes_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                 const uint64_t *d_elem_bytes, size_t n_buffers, size_t n_packets, uint8_t *const *d_out_ptrs,
                                 uint32_t *d_status, void *stream) {
    return planes_batch(true, d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, n_buffers, n_packets, d_out_ptrs, d_status, stream);
}

static int planes_on_host(bool merge, const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    bool work = false;
    const int e = filter_checks(true, in, false, nullptr, n_bytes, elem_bytes, out, &work);
    if (e != GPUAR_OK || !work) return e;
    if (merge) gpuar::planes_host<true>(in, n_bytes, elem_bytes, out);
    else gpuar::planes_host<false>(in, n_bytes, elem_bytes, out);
    return GPUAR_OK;
}

int gpuar_hip_split_planes_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    return planes_on_host(false, in, n_bytes, elem_bytes, out);
}

int gpuar_hip_merge_planes_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    return planes_on_host(true, in, n_bytes, elem_bytes, out);
}

static int delta_single(bool merge, const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    gpuar::DeltaArgs d = {};
    bool launch = false;
    const int e = single_arguments(d_in, false, nullptr, n_bytes, elem_bytes, d_out, &d.p, &launch);      // (a width of 1 in place is work too)
    if (e != GPUAR_OK || !launch) return e;
    return launch_filter(kDeltaKernels, merge, d, d.p, stream);
}

static int delta_batch(bool merge, const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                       const uint64_t *d_elem_bytes, const uint64_t *d_filter, size_t n_buffers, size_t n_packets,
                       uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    gpuar::DeltaArgs d = {};
    bool launch = false;
    const int e = batch_filter_arguments(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, true, d_filter, n_buffers, n_packets, d_out_ptrs,
                                         d_status, &d.p, &launch);
    if (e != GPUAR_OK || !launch) return e;
    d.filter = d_filter;
    return launch_filter(kDeltaKernels, merge, d, d.p, stream);
}

int gpuar_hip_split_delta(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    return delta_single(false, d_in, n_bytes, elem_bytes, d_out, stream);
}

int gpuar_hip_merge_delta(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    return delta_single(true, d_in, n_bytes, elem_bytes, d_out, stream);
}

int gpuar_hip_split_delta_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_elem_bytes, const uint64_t *d_filter, size_t n_buffers, size_t n_packets,
                                uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    return delta_batch(false, d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_filter, n_buffers, n_packets, d_out_ptrs, d_status, stream);
}

int gpuar_hip_merge_delta_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_elem_bytes, const uint64_t *d_filter, size_t n_buffers, size_t n_packets,
                                uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    return delta_batch(true, d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_filter, n_buffers, n_packets, d_out_ptrs, d_status, stream);
}

static int delta_on_host(bool merge, const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    bool work = false;
    const int e = filter_checks(true, in, false, nullptr, n_bytes, elem_bytes, out, &work);
    if (e != GPUAR_OK || !work) return e;
    if (merge) gpuar::merge_delta_host(in, n_bytes, elem_bytes, out);
    else gpuar::split_delta_host(in, n_bytes, elem_bytes, out);
    return GPUAR_OK;
}

int gpuar_hip_split_delta_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    return delta_on_host(false, in, n_bytes, elem_bytes, out);
}

int gpuar_hip_merge_delta_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    return delta_on_host(true, in, n_bytes, elem_bytes, out);
}

static int xor_single(bool merge, const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    gpuar::XorArgs x = {};
    bool launch = false;
    const int e = single_arguments(d_in, true, d_base, n_bytes, elem_bytes, d_out, &x.p, &launch);      // (a width of 1 in place is work too)
    if (e != GPUAR_OK || !launch) return e;
    x.base = d_base;
    return launch_filter(kXorKernels, merge, x, x.p, stream);
}

static int xor_batch(bool merge, const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                     const uint64_t *d_elem_bytes, const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets,
                     uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    gpuar::XorArgs x = {};
    bool launch = false;
    const int e = batch_filter_arguments(d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, true, d_base_ptrs, n_buffers, n_packets, d_out_ptrs,
                                         d_status, &x.p, &launch);
    if (e != GPUAR_OK || !launch) return e;
    x.base_ptrs = d_base_ptrs;
    return launch_filter(kXorKernels, merge, x, x.p, stream);
}

int gpuar_hip_split_xor(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    return xor_single(false, d_in, d_base, n_bytes, elem_bytes, d_out, stream);
}

int gpuar_hip_merge_xor(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream) {
    return xor_single(true, d_in, d_base, n_bytes, elem_bytes, d_out, stream);
}

int gpuar_hip_split_xor_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                              const uint64_t *d_elem_bytes, const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets,
                              uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    return xor_batch(false, d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_base_ptrs, n_buffers, n_packets, d_out_ptrs, d_status, stream);
}

int gpuar_hip_merge_xor_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                              const uint64_t *d_elem_bytes, const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets,
                              uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    return xor_batch(true, d_in_ptrs, d_bytes, d_first_packet, d_elem_bytes, d_base_ptrs, n_buffers, n_packets, d_out_ptrs, d_status, stream);
}

static int xor_on_host(bool merge, const uint8_t *in, const uint8_t *base, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    bool work = false;
    const int e = filter_checks(true, in, true, base, n_bytes, elem_bytes, out, &work);
    if (e != GPUAR_OK || !work) return e;
    if (merge) gpuar::merge_xor_host(in, base, n_bytes, elem_bytes, out);
    else gpuar::split_xor_host(in, base, n_bytes, elem_bytes, out);
    return GPUAR_OK;
}

int gpuar_hip_split_xor_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    return xor_on_host(false, in, base, n_bytes, elem_bytes, out);
}

int gpuar_hip_merge_xor_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, uint32_t elem_bytes, uint8_t *out) {
    return xor_on_host(true, in, base, n_bytes, elem_bytes, out);
}

// ---- the mixed filter (include/gpuar_hip_mixed.h) ----

size_t gpuar_hip_mode_count(size_t n_bytes) { return static_cast<size_t>(gpuar::mode_count(n_bytes)); }

size_t gpuar_hip_batch_mode_count(const uint64_t *bytes, size_t n_buffers, uint64_t *first_mode) {
    uint64_t total = 0;
    for (size_t b = 0; b < n_buffers; ++b) {
        if (first_mode) first_mode[b] = total;
        total += bytes ? gpuar::mode_count(bytes[b]) : 0u;
    }
    if (first_mode) first_mode[n_buffers] = total;
    return static_cast<size_t>(total);
}

int gpuar_hip_choose_mode(const uint64_t plain[4], const uint64_t *delta, const uint64_t *xored, uint64_t n_packets, uint64_t *total) {
    if (!plain) return GPUAR_ERR_ARGUMENT;
    const gpuar::ModeChoice c = gpuar::choose_mode(plain, delta, xored, n_packets);
    if (total) *total = c.total;
    return static_cast<int>(c.mode);
}

// the launch of both device calls: a lane per supergroup
static int launch_choose_modes(gpuar::ChooseModesArgs a, const uint32_t *d_plain, const uint32_t *d_delta, const uint32_t *d_xored, size_t stride,
                               uint8_t *d_modes, uint32_t *d_totals, void *stream) {
    a.plain = d_plain, a.delta = d_delta, a.xored = d_xored, a.stride = stride, a.modes = d_modes, a.totals = d_totals;
    const uint32_t blocks = capped_blocks(a.n_modes, gpuar::kChooseThreads, 0xFFFFFFFFu);
    gpuar::choose_modes_kernel<<<blocks, gpuar::kChooseThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    return check_launch();
}

// what both device calls check of their rows and outputs: d_plain and d_modes are there (else ARGUMENT); the rows and the totals
// are 4-byte aligned (else ALIGNMENT)
static int choose_modes_pointers(const uint32_t *d_plain, const uint32_t *d_delta, const uint32_t *d_xored, const uint8_t *d_modes,
                                 const uint32_t *d_totals, const uint32_t *d_status) {
    if (!d_plain || !d_modes) return GPUAR_ERR_ARGUMENT;
    return misaligned(d_plain, 4) || misaligned(d_delta, 4) || misaligned(d_xored, 4) || misaligned(d_totals, 4) || misaligned(d_status, 4)
               ? GPUAR_ERR_ALIGNMENT
               : GPUAR_OK;
}

int gpuar_hip_choose_modes(const uint32_t *d_plain, const uint32_t *d_delta, const uint32_t *d_xored, size_t stride, size_t n_bytes,
                           uint8_t *d_modes, uint32_t *d_totals, uint32_t *d_status, void *stream) {
    if (n_bytes == 0) return GPUAR_OK;
    if (stride < gpuar_hip_packet_count(n_bytes) || gpuar_hip_packet_count(n_bytes) > kMaxCount) return GPUAR_ERR_ARGUMENT;
    const int e = choose_modes_pointers(d_plain, d_delta, d_xored, d_modes, d_totals, d_status);
    if (e != GPUAR_OK) return e;
    gpuar::ChooseModesArgs a = {};
    a.n_bytes = n_bytes;
    a.n_packets = static_cast<uint32_t>(gpuar_hip_packet_count(n_bytes));
    a.n_modes = static_cast<uint32_t>(gpuar::mode_count(n_bytes));
    a.status = status_word(d_status);
    if (!a.status) return GPUAR_ERR_NO_DEVICE;
    return launch_choose_modes(a, d_plain, d_delta, d_xored, stride, d_modes, d_totals, stream);
}

int gpuar_hip_choose_modes_batch(const uint32_t *d_plain, const uint32_t *d_delta, const uint32_t *d_xored, size_t stride, const uint64_t *d_bytes,
                                 const uint64_t *d_first_packet, const uint64_t *d_first_mode, size_t n_buffers, size_t n_packets, size_t n_modes,
                                 uint8_t *d_modes, uint32_t *d_totals, uint32_t *d_status, void *stream) {
    if (n_modes == 0) return GPUAR_OK;
    if (stride < n_packets || !d_bytes || !d_first_packet || !d_first_mode || n_packets > kMaxCount || n_buffers > kMaxCount || n_modes > kMaxCount)
        return GPUAR_ERR_ARGUMENT;
    const int e = choose_modes_pointers(d_plain, d_delta, d_xored, d_modes, d_totals, d_status);
    if (e != GPUAR_OK) return e;
    if (misaligned(d_bytes, 8) || misaligned(d_first_packet, 8) || misaligned(d_first_mode, 8)) return GPUAR_ERR_ALIGNMENT;
    gpuar::ChooseModesArgs a = {};
    a.bytes = d_bytes, a.first_packet = d_first_packet, a.first_mode = d_first_mode;
    a.n_buffers = static_cast<uint32_t>(n_buffers);
    a.n_packets = static_cast<uint32_t>(n_packets);
    a.n_modes = static_cast<uint32_t>(n_modes);
    a.status = status_word(d_status);
    if (!a.status) return GPUAR_ERR_NO_DEVICE;
    return launch_choose_modes(a, d_plain, d_delta, d_xored, stride, d_modes, d_totals, stream);
}

int gpuar_hip_choose_modes_host(const uint32_t *plain, const uint32_t *delta, const uint32_t *xored, size_t stride, size_t n_bytes, uint8_t *modes,
                                uint32_t *totals) {
    if (n_bytes == 0) return GPUAR_OK;
    if (!plain || !modes || stride < gpuar_hip_packet_count(n_bytes)) return GPUAR_ERR_ARGUMENT;
    gpuar::choose_modes_host(plain, delta, xored, stride, n_bytes, modes, totals);
    return GPUAR_OK;
}

const FilterKernels<gpuar::MixedArgs> kMixedKernels = {gpuar::split_mixed_kernel, gpuar::merge_mixed_kernel, gpuar::mixed_tail_kernel<false>,
                                                       gpuar::mixed_tail_kernel<true>};

static int mixed_single(bool merge, const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, const uint8_t *d_modes, uint8_t *d_out,
                        uint32_t *d_status, void *stream) {
    gpuar::MixedArgs m = {};
    bool launch = false;
    const int e = single_arguments(d_in, d_base != nullptr, d_base, n_bytes, 1u, d_out, &m.p, &launch);
    if (e != GPUAR_OK || !launch) return e;
    if (!d_modes) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_status, 4)) return GPUAR_ERR_ALIGNMENT;
    m.p.status = status_word(d_status);
    if (!m.p.status) return GPUAR_ERR_NO_DEVICE;
    m.modes = d_modes;
    m.base = d_base;
    // launch_filter asks p.elem whether one buffer has a tail: at 8 it has one unless it ends on a supergroup's edge, where no width has
    m.p.elem = 8u;
    return launch_filter(kMixedKernels, merge, m, m.p, stream);
}

static int mixed_batch(bool merge, const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                       const uint64_t *d_first_mode, const uint8_t *d_modes, const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets,
                       uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    gpuar::MixedArgs m = {};
    bool launch = false;
    if (n_packets != 0 && !d_modes) return GPUAR_ERR_ARGUMENT;
    if (n_packets != 0 && misaligned(d_base_ptrs, 8)) return GPUAR_ERR_ALIGNMENT;
    // (the widths' place in the checks goes to first_mode, `extra` to the base pointers)
    const int e = batch_filter_arguments(d_in_ptrs, d_bytes, d_first_packet, d_first_mode, true, d_base_ptrs, n_buffers, n_packets, d_out_ptrs,
                                         d_status, &m.p, &launch);
    if (e != GPUAR_OK || !launch) return e;
    m.p.elem_bytes = nullptr;
    m.modes = d_modes;
    m.first_mode = d_first_mode;
    m.base_ptrs = d_base_ptrs;
    return launch_filter(kMixedKernels, merge, m, m.p, stream);
}

int gpuar_hip_split_mixed(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, const uint8_t *d_modes, uint8_t *d_out, uint32_t *d_status,
                          void *stream) {
    return mixed_single(false, d_in, d_base, n_bytes, d_modes, d_out, d_status, stream);
}

int gpuar_hip_merge_mixed(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, const uint8_t *d_modes, uint8_t *d_out, uint32_t *d_status,
                          void *stream) {
    return mixed_single(true, d_in, d_base, n_bytes, d_modes, d_out, d_status, stream);
}

int gpuar_hip_split_mixed_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_first_mode, const uint8_t *d_modes, const uint8_t *const *d_base_ptrs, size_t n_buffers,
                                size_t n_packets, uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    return mixed_batch(false, d_in_ptrs, d_bytes, d_first_packet, d_first_mode, d_modes, d_base_ptrs, n_buffers, n_packets, d_out_ptrs, d_status,
                       stream);
}

int gpuar_hip_merge_mixed_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_first_mode, const uint8_t *d_modes, const uint8_t *const *d_base_ptrs, size_t n_buffers,
                                size_t n_packets, uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream) {
    return mixed_batch(true, d_in_ptrs, d_bytes, d_first_packet, d_first_mode, d_modes, d_base_ptrs, n_buffers, n_packets, d_out_ptrs, d_status,
                       stream);
}

static int mixed_on_host(bool merge, const uint8_t *in, const uint8_t *base, size_t n_bytes, const uint8_t *modes, uint8_t *out) {
    bool work = false;
    const int e = filter_checks(true, in, base != nullptr, base, n_bytes, 1u, out, &work);
    if (e != GPUAR_OK || !work) return e;
    if (!modes || !gpuar::mixed_modes_ok(modes, n_bytes, base != nullptr)) return GPUAR_ERR_ARGUMENT;      // before anything is written
    if (merge) gpuar::merge_mixed_host(in, base, n_bytes, modes, out);
    else gpuar::split_mixed_host(in, base, n_bytes, modes, out);
    return GPUAR_OK;
}

int gpuar_hip_split_mixed_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, const uint8_t *modes, uint8_t *out) {
    return mixed_on_host(false, in, base, n_bytes, modes, out);
}

int gpuar_hip_merge_mixed_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, const uint8_t *modes, uint8_t *out) {
    return mixed_on_host(true, in, base, n_bytes, modes, out);
}

// one 16-element block through delta.h's register transforms, as the kernels apply them, on the host (for the tests):
// mixed: 4 * elem_bytes dwords, in place; undo = 0: delta_block with `carried` as pred; 1: undelta_block with it as offset.
// *total (may be null) receives undelta_block's total.
int gpuar_hip_delta_block_host(uint32_t *mixed, uint32_t elem_bytes, int undo, uint64_t carried, uint64_t *total) {
    if (!mixed || !gpuar::planes_width_ok(elem_bytes)) return GPUAR_ERR_ARGUMENT;
    auto run = [&](auto width) {
        constexpr int W = decltype(width)::value;
        uint32_t block[4 * W];
        memcpy(block, mixed, sizeof block);
        uint64_t sum = 0;
        if (undo) sum = gpuar::undelta_block<W>(block, carried);
        else gpuar::delta_block<W>(block, carried);
        memcpy(mixed, block, sizeof block);
        if (total) *total = sum;
    };
    if (elem_bytes == 8u) run(std::integral_constant<int, 8>());
    else if (elem_bytes == 4u) run(std::integral_constant<int, 4>());
    else if (elem_bytes == 2u) run(std::integral_constant<int, 2>());
    else run(std::integral_constant<int, 1>());
    return GPUAR_OK;
}

static int launch_estimate(const gpuar::CrcArgs &a, void *stream) {
    const uint32_t blocks = capped_blocks(a.n_packets, gpuar::kEstWaves, gpuar::kEstGroups);
    gpuar::estimate_kernel<<<blocks, gpuar::kEstWaves * gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(a);
    return check_launch();
}

int gpuar_hip_estimate(const uint8_t *d_in, size_t n_bytes, uint32_t *d_est, void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_checks(true, d_in, n_bytes, d_est, nullptr, nullptr, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = d_est;
    return launch_estimate(a, stream);
}

int gpuar_hip_estimate_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                             size_t n_buffers, size_t n_packets, uint32_t *d_est, uint32_t *d_status, void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_batch_checks(true, d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, d_est, nullptr, d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = d_est;
    return launch_estimate(a, stream);
}

int gpuar_hip_estimate_host(const uint8_t *in, size_t n_bytes, uint32_t *est) {
    if (n_bytes == 0) return GPUAR_OK;
    if (!in || !est) return GPUAR_ERR_ARGUMENT;
    gpuar::estimate_host(in, n_bytes, est);
    return GPUAR_OK;
}

// the grid of the three surveys: a workgroup takes a window of 8 packets at a time
static uint32_t survey_blocks(uint32_t n_packets) { return capped_blocks(n_packets, 8u, gpuar::kSurveyGroups); }

// both surveys, into the rows at d_est: delta_mask 0 is the plane survey, anything else the delta survey of those widths
static int launch_survey(gpuar::SurveyArgs a, uint32_t *d_est, size_t est_stride, uint32_t delta_mask, void *stream) {
    a.est = d_est;
    a.stride = est_stride;
    const uint32_t blocks = survey_blocks(a.n_packets);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (delta_mask) gpuar::survey_delta_kernel<<<blocks, gpuar::kSurveyThreads, 0, s>>>(gpuar::DeltaSurveyArgs{a, delta_mask});
    else gpuar::survey_planes_kernel<<<blocks, gpuar::kSurveyThreads, 0, s>>>(a);
    return check_launch();
}

int gpuar_hip_survey_planes(const uint8_t *d_in, size_t n_bytes, uint32_t *d_est, size_t est_stride, void *stream) {
    gpuar::SurveyArgs a;
    bool launch = false;
    const int e = packet_checks(est_stride >= gpuar_hip_packet_count(n_bytes), d_in, n_bytes, d_est, nullptr, nullptr, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    return launch_survey(a, d_est, est_stride, 0u, stream);
}

int gpuar_hip_survey_planes_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                                  size_t n_buffers, size_t n_packets, uint32_t *d_est, size_t est_stride, uint32_t *d_status, void *stream) {
    gpuar::SurveyArgs a;
    bool launch = false;
    const int e = packet_batch_checks(est_stride >= n_packets, d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, d_est, nullptr, d_status,
                                      &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    return launch_survey(a, d_est, est_stride, 0u, stream);
}

int gpuar_hip_survey_planes_host(const uint8_t *in, size_t n_bytes, uint32_t *est, size_t est_stride) {
    if (n_bytes == 0) return GPUAR_OK;
    if (!in || !est || est_stride < gpuar_hip_packet_count(n_bytes)) return GPUAR_ERR_ARGUMENT;
    gpuar::survey_host(in, n_bytes, est, est_stride);
    return GPUAR_OK;
}

static bool delta_survey_mask_ok(uint32_t widths_mask) { return widths_mask != 0u && (widths_mask & ~gpuar::kSurveyAllWidths) == 0u; }

int gpuar_hip_survey_delta(const uint8_t *d_in, size_t n_bytes, uint32_t widths_mask, uint32_t *d_est, size_t est_stride, void *stream) {
    gpuar::SurveyArgs a;
    bool launch = false;
    const int e = packet_checks(est_stride >= gpuar_hip_packet_count(n_bytes) && delta_survey_mask_ok(widths_mask), d_in, n_bytes, d_est, nullptr,
                                nullptr, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    return launch_survey(a, d_est, est_stride, widths_mask, stream);
}

int gpuar_hip_survey_delta_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet, size_t n_buffers,
                                 size_t n_packets, uint32_t widths_mask, uint32_t *d_est, size_t est_stride, uint32_t *d_status, void *stream) {
    gpuar::SurveyArgs a;
    bool launch = false;
    const int e = packet_batch_checks(est_stride >= n_packets && delta_survey_mask_ok(widths_mask), d_in_ptrs, d_in_bytes, d_first_packet, n_buffers,
                                      n_packets, d_est, nullptr, d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    return launch_survey(a, d_est, est_stride, widths_mask, stream);
}

int gpuar_hip_survey_delta_host(const uint8_t *in, size_t n_bytes, uint32_t widths_mask, uint32_t *est, size_t est_stride) {
    if (n_bytes == 0) return GPUAR_OK;
    if (!in || !est || est_stride < gpuar_hip_packet_count(n_bytes) || !delta_survey_mask_ok(widths_mask)) return GPUAR_ERR_ARGUMENT;
    gpuar::delta_survey_host(in, n_bytes, widths_mask, est, est_stride);
    return GPUAR_OK;
}

int gpuar_hip_choose_filter(const uint64_t plain[4], const uint64_t filtered[4], uint64_t n_packets, uint32_t *width) {
    gpuar::FilterChoice c = {1u, false};
    if (plain && filtered) c = gpuar::choose_filter(plain, filtered, n_packets);
    if (width) *width = c.width;
    return c.filter ? 1 : 0;
}

uint32_t gpuar_hip_choose_planes(const uint64_t total[4], uint64_t n_packets) { return total ? gpuar::choose_width(total, n_packets) : 1u; }

// the XOR-base survey (include/gpuar_hip_xsurvey.h): `a` with its source, base and status in place
static int launch_survey_xor(gpuar::XorSurveyArgs a, uint32_t *d_est, uint32_t *d_scan, size_t stride, void *stream) {
    a.s.est = d_est;
    a.s.stride = stride;
    a.scan = d_scan;
    const uint32_t blocks = survey_blocks(a.s.n_packets);
    gpuar::survey_xor_kernel<<<blocks, gpuar::kSurveyThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    return check_launch();
}

// What the XOR survey's calls add to the plane survey's checks: the base (or the array of base pointers) is there and one output
// at least (else ARGUMENT); the base and the scan rows are aligned (else ALIGNMENT; the est rows, or the scan rows where there are
// none, go through packet_checks as the plane survey's d_est does).
static int xsurvey_pointers(const void *base, uintptr_t base_align, const uint32_t *d_est, const uint32_t *d_scan) {
    if (!base || (!d_est && !d_scan)) return GPUAR_ERR_ARGUMENT;
    return misaligned(base, base_align) || misaligned(d_scan, 4) ? GPUAR_ERR_ALIGNMENT : GPUAR_OK;
}

// ... in the header's order: nothing to do, every ARGUMENT defect, every ALIGNMENT defect, then the status word.  `own`: what
// xsurvey_pointers said (its ARGUMENT went into own_ok), `e`: what the plane survey's checks said.
static int xsurvey_order(int own, int e, bool launch) {
    if ((e == GPUAR_OK && !launch) || e == GPUAR_ERR_ARGUMENT || e == GPUAR_ERR_ALIGNMENT) return e;
    return own != GPUAR_OK ? own : e;
}

int gpuar_hip_survey_xor(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, uint32_t *d_est, uint32_t *d_scan, size_t stride,
                         void *stream) {
    gpuar::XorSurveyArgs a = {};
    bool launch = false;
    const int own = xsurvey_pointers(d_base, 16u, d_est, d_scan);
    const int e = xsurvey_order(own, packet_checks(stride >= gpuar_hip_packet_count(n_bytes) && own != GPUAR_ERR_ARGUMENT, d_in, n_bytes,
                                                   d_est ? d_est : d_scan, nullptr, nullptr, &a.s, &launch), launch);
    if (e != GPUAR_OK || !launch) return e;
    a.base = d_base;
    return launch_survey_xor(a, d_est, d_scan, stride, stream);
}

int gpuar_hip_survey_xor_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                               const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets, uint32_t *d_est, uint32_t *d_scan,
                               size_t stride, uint32_t *d_status, void *stream) {
    gpuar::XorSurveyArgs a = {};
    bool launch = false;
    const int own = xsurvey_pointers(d_base_ptrs, 8u, d_est, d_scan);
    const int e = xsurvey_order(own, packet_batch_checks(stride >= n_packets && own != GPUAR_ERR_ARGUMENT, d_in_ptrs, d_in_bytes, d_first_packet,
                                                         n_buffers, n_packets, d_est ? d_est : d_scan, nullptr, d_status, &a.s, &launch), launch);
    if (e != GPUAR_OK || !launch) return e;
    a.bases = d_base_ptrs;
    return launch_survey_xor(a, d_est, d_scan, stride, stream);
}

int gpuar_hip_survey_xor_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, uint32_t *est, uint32_t *scan, size_t stride) {
    if (n_bytes == 0) return GPUAR_OK;
    if (!in || !base || (!est && !scan) || stride < gpuar_hip_packet_count(n_bytes)) return GPUAR_ERR_ARGUMENT;
    gpuar::xor_survey_host(in, base, n_bytes, est, scan, stride);
    return GPUAR_OK;
}

int gpuar_hip_move_packets(const uint8_t *const *d_src_ptrs, uint8_t *const *d_dst_ptrs, const uint64_t *d_bytes, size_t n_regions,
                           uint32_t *d_status, void *stream) {
    gpuar::MoveArgs a = {};
    a.src = d_src_ptrs;
    a.dst = d_dst_ptrs;
    a.bytes = d_bytes;
    return region_call(gpuar::move_packets_kernel, 1u, gpuar::kMoveThreads, a, {d_src_ptrs, d_dst_ptrs, d_bytes}, {}, n_regions, d_status, stream);
}

int gpuar_hip_move_bytes(const uint8_t *const *d_src_ptrs, uint8_t *const *d_dst_ptrs, const uint64_t *d_bytes, size_t n_regions,
                         uint32_t *d_status, void *stream) {
    gpuar::MoveArgs a = {};
    a.src = d_src_ptrs;
    a.dst = d_dst_ptrs;
    a.bytes = d_bytes;
    return region_call(gpuar::move_bytes_kernel, 1u, gpuar::kMoveBytesThreads, a, {d_src_ptrs, d_dst_ptrs, d_bytes}, {}, n_regions, d_status, stream);
}

uint32_t gpuar_hip_sparse_len(uint32_t k) { return gpuar::sparse_len(k); }

int gpuar_hip_sparse_rule(uint32_t scan, uint32_t est, uint32_t ulen, int stored_on) {
    return static_cast<int>(gpuar::sparse_kind(scan, est, ulen, stored_on != 0));
}

static int launch_sparse_scan(const gpuar::CrcArgs &a, void *stream) {
    const uint32_t blocks = capped_blocks(a.n_packets, gpuar::kSparseWaves, gpuar::kSparseGroups);
    gpuar::sparse_scan_kernel<<<blocks, gpuar::kSparseWaves * gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(a);
    return check_launch();
}

int gpuar_hip_sparse_scan(const uint8_t *d_in, size_t n_bytes, uint32_t *d_scan, void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_checks(true, d_in, n_bytes, d_scan, nullptr, nullptr, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = d_scan;
    return launch_sparse_scan(a, stream);
}

int gpuar_hip_sparse_scan_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                                size_t n_buffers, size_t n_packets, uint32_t *d_scan, uint32_t *d_status, void *stream) {
    gpuar::CrcArgs a;
    bool launch = false;
    const int e = packet_batch_checks(true, d_in_ptrs, d_in_bytes, d_first_packet, n_buffers, n_packets, d_scan, nullptr, d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    a.crc = d_scan;
    return launch_sparse_scan(a, stream);
}

int gpuar_hip_sparse_scan_host(const uint8_t *in, size_t n_bytes, uint32_t *scan) {
    if (n_bytes == 0) return GPUAR_OK;
    if (!in || !scan) return GPUAR_ERR_ARGUMENT;
    gpuar::sparse_scan_host(in, n_bytes, scan);
    return GPUAR_OK;
}

int gpuar_hip_sparse_pack(const uint8_t *const *d_src_ptrs, const uint64_t *d_bytes, const uint32_t *d_scan, uint8_t *const *d_dst_ptrs,
                          size_t n_regions, uint32_t *d_status, void *stream) {
    gpuar::SparsePackArgs a = {};
    a.src = d_src_ptrs;
    a.bytes = d_bytes;
    a.scan = d_scan;
    a.dst = d_dst_ptrs;
    return region_call(gpuar::sparse_pack_kernel, gpuar::kSparseWaves, gpuar::kSparseWaves * gpuar::kLanes, a, {d_src_ptrs, d_bytes, d_dst_ptrs},
                       {d_scan}, n_regions, d_status, stream);
}

int gpuar_hip_sparse_unpack(const uint8_t *const *d_rec_ptrs, const uint64_t *d_rec_bytes, uint8_t *const *d_dst_ptrs, const uint64_t *d_bytes,
                            size_t n_regions, uint32_t *d_status, void *stream) {
    gpuar::SparseUnpackArgs a = {};
    a.rec = d_rec_ptrs;
    a.rec_bytes = d_rec_bytes;
    a.dst = d_dst_ptrs;
    a.bytes = d_bytes;
    return region_call(gpuar::sparse_unpack_kernel, gpuar::kSparseWaves, gpuar::kSparseWaves * gpuar::kLanes, a,
                       {d_rec_ptrs, d_rec_bytes, d_dst_ptrs, d_bytes}, {}, n_regions, d_status, stream);
}

int gpuar_hip_sparse_pack_host(const uint8_t *in, size_t n_bytes, uint8_t *rec, size_t rec_room, size_t *rec_len) {
    if (!in || !rec || !rec_len || n_bytes == 0 || n_bytes > gpuar::kSparsePacket) return GPUAR_ERR_ARGUMENT;
    return gpuar::sparse_pack_host(in, static_cast<uint32_t>(n_bytes), rec, rec_room, rec_len) ? GPUAR_OK : GPUAR_ERR_ARGUMENT;
}

int gpuar_hip_sparse_unpack_host(const uint8_t *rec, size_t rec_bytes, uint8_t *out, size_t n_bytes) {
    if (!rec || !out || n_bytes == 0 || n_bytes > gpuar::kSparsePacket) return GPUAR_ERR_ARGUMENT;
    return gpuar::sparse_unpack_host(rec, rec_bytes, out, static_cast<uint32_t>(n_bytes)) ? GPUAR_OK : GPUAR_ERR_ARGUMENT;
}

int gpuar_hip_kinds_store(const uint8_t *d_in, size_t n_bytes, const uint32_t *d_est, const uint32_t *d_scan, int stored_on, uint8_t *d_slots,
                          uint8_t *d_kind, uint32_t *d_status, void *stream) {
    gpuar::KindsStoreArgs a;
    bool launch = false;
    const int e = packet_checks(true, d_in, n_bytes, d_est, nullptr, d_status, &a, &launch);
    if (e != GPUAR_OK || !launch) return e;
    if (!d_slots || !d_kind) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_slots, 16) || misaligned(d_scan, 4)) return GPUAR_ERR_ALIGNMENT;
    a.est = d_est;
    a.scan = d_scan;
    a.stored_on = stored_on != 0 ? 1u : 0u;
    a.slots = d_slots;
    a.kind = d_kind;
    const uint32_t blocks = capped_blocks(a.n_packets, gpuar::kSparseWaves, gpuar::kSparseGroups);
    gpuar::kinds_store_kernel<<<blocks, gpuar::kSparseWaves * gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(a);
    return check_launch();
}

int gpuar_hip_kinds_expand(const uint8_t *d_stream, const uint64_t *d_offsets, const uint8_t *d_kind, size_t n_packets, uint8_t *d_out,
                           size_t n_bytes, uint32_t *d_status, void *stream) {
    if (n_packets == 0) return GPUAR_OK;
    if (!d_stream || !d_offsets || !d_kind || !d_out || n_packets > kMaxCount || gpuar_hip_packet_count(n_bytes) != n_packets)
        return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_out, 16) || misaligned(d_offsets, 8) || misaligned(d_status, 4)) return GPUAR_ERR_ALIGNMENT;
    gpuar::KindsExpandArgs a = {};
    a.stream = d_stream;
    a.offsets = d_offsets;
    a.kind = d_kind;
    a.n_packets = static_cast<uint32_t>(n_packets);
    a.out = d_out;
    a.n_bytes = n_bytes;
    a.status = status_word(d_status);
    if (!a.status) return GPUAR_ERR_NO_DEVICE;
    const uint32_t blocks = capped_blocks(a.n_packets, gpuar::kSparseWaves, gpuar::kSparseGroups);
    gpuar::kinds_expand_kernel<<<blocks, gpuar::kSparseWaves * gpuar::kLanes, 0, static_cast<hipStream_t>(stream)>>>(a);
    return check_launch();
}

int gpuar_hip_kinds_store_host(const uint8_t *in, size_t n_bytes, int stored_on, int sparse_on, uint8_t *pkt, size_t room, uint32_t *kind,
                               size_t *clen) {
    if (!in || !kind || !clen || n_bytes == 0 || n_bytes > gpuar::kKindsPacket || (!pkt && room)) return GPUAR_ERR_ARGUMENT;
    uint32_t len = 0;
    const uint32_t k = gpuar::kinds_store_packet(in, static_cast<uint32_t>(n_bytes), stored_on != 0, sparse_on != 0, pkt, room, &len);
    if (k == ~0u) return GPUAR_ERR_ARGUMENT;
    *kind = k;
    *clen = len;
    return GPUAR_OK;
}

int gpuar_hip_kinds_expand_host(const uint8_t *pkt, size_t pkt_bytes, uint32_t kind, uint8_t *out, size_t n_bytes) {
    if (!pkt || !out || n_bytes == 0 || n_bytes > gpuar::kKindsPacket) return GPUAR_ERR_ARGUMENT;
    return gpuar::kinds_expand_packet(pkt, pkt_bytes, kind, out, static_cast<uint32_t>(n_bytes)) ? GPUAR_OK : GPUAR_ERR_ARGUMENT;
}

int gpuar_hip_status(uint32_t *flags) {
    if (!flags) return GPUAR_ERR_ARGUMENT;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return static_cast<int>(e);
    // g_status_taken is one word per device: one caller at a time between the exchange and the copy that reads it
    static std::mutex taking;
    std::lock_guard<std::mutex> hold(taking);
    gpuar::take_status_kernel<<<1, gpuar::kLanes, 0, nullptr>>>();      // the copy below waits for it (same stream)
    const int launched = check_launch();
    if (launched != GPUAR_OK) return launched;
    uint32_t v = 0;
    e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(gpuar::g_status_taken), sizeof v);
    if (e != hipSuccess) return static_cast<int>(e);
    *flags = v;
    return GPUAR_OK;
}

int gpuar_hip_last_error(void) {
    const int e = t_last_error;
    t_last_error = GPUAR_OK;
    return e;
}

const char *gpuar_hip_error_string(int code) {
    switch (code) {
        case GPUAR_OK: return "ok";
        case GPUAR_ERR_ALIGNMENT: return "device pointer is not suitably aligned (16 bytes)";
        case GPUAR_ERR_ARGUMENT: return "invalid argument";
        case GPUAR_ERR_NO_DEVICE: return "no HIP device";
        default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "unknown gpuar error";
    }
}

const char *gpuar_hip_version(void) { return "gpuar-hip 0.2 gfx950"; }

int gpuar_hip_abi_version(void) { return GPUAR_HIP_ABI_VERSION; }

int gpuar_hip_generate(int kind, uint64_t seed, uint64_t offset, size_t n, uint8_t *d_out, void *stream) {
    if (n == 0) return GPUAR_OK;
    if (!d_out || (offset & 7u) || kind < 0 || kind > 2) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_out, 8)) return GPUAR_ERR_ALIGNMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t groups = (n + 7) / 8;
    const uint32_t blocks = static_cast<uint32_t>((groups + 255) / 256);
    if (kind == 0) {
        gpuar::generate_uniform_kernel<<<blocks, 256, 0, s>>>(seed, offset / 8, n, d_out);
    } else {
        static const char rank[] =
            " etaoinshrdlcumwfgypbvkjxqz\n.,ETAOINSHRDLCUMWFGYPBVKJXQZ0123456789-'\"()/:;=_<>[]{}!?#$%&*+@\\^`|~";
        gpuar::ZipfTable t;
        memset(&t, 0, sizeof t);
        const uint32_t K = kind == 1 ? 256u : 96u;
        uint32_t run = 0;
        for (uint32_t r = 1; r <= K; ++r) {
            run += (1u << 24) / r;
            t.cum[r - 1] = run;
            t.sym[r - 1] = kind == 1 ? static_cast<uint8_t>(((r - 1) * 167u + 13u) & 255u) : static_cast<uint8_t>(rank[r - 1]);
        }
        gpuar::generate_zipf_kernel<<<blocks, 256, 0, s>>>(seed, offset / 2, n, d_out, t, K);
    }
    return check_launch();
}

int gpuar_hip_copy(const uint8_t *d_src, uint8_t *d_dst, size_t n_bytes, void *stream) {
    if (n_bytes == 0) return GPUAR_OK;
    if (!d_src || !d_dst || (n_bytes & 15u)) return GPUAR_ERR_ARGUMENT;
    if (misaligned(d_src, 16) || misaligned(d_dst, 16)) return GPUAR_ERR_ALIGNMENT;
    const size_t n_quads = n_bytes / 16u;
    const size_t want = (n_quads + 255u) / 256u;                    // one quad per thread
    // HIP rejects a launch once gridDim.x * blockDim.x reaches 2^32 threads: 64 GiB less one tile for this kernel (bench.py
    // copies its 8 GiB workload); beyond that the caller gets an argument error instead of a launch error
    if (want * 256u > 0xFFFFFFFFull) return GPUAR_ERR_ARGUMENT;
    const uint32_t blocks = static_cast<uint32_t>(want);
    gpuar::copy_kernel<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const uint4 *>(d_src), reinterpret_cast<uint4 *>(d_dst), n_quads);
    return check_launch();
}

int gpuar_hip_clock_samples(int which, uint64_t *ticks, int reset) {
    if ((which != 0 && which != 1) || !ticks) return GPUAR_ERR_ARGUMENT;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return static_cast<int>(e);
    const size_t bytes = sizeof(unsigned long long) * gpuar::kClockSlots * 4u, at = static_cast<size_t>(which) * bytes;
    e = hipMemcpyFromSymbol(ticks, HIP_SYMBOL(gpuar::g_clock_samples), bytes, at);
    if (e != hipSuccess) return static_cast<int>(e);
    if (reset) {
        static const unsigned long long zeros[gpuar::kClockSlots * 4u] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(gpuar::g_clock_samples), zeros, bytes, at);
    }
    return e == hipSuccess ? GPUAR_OK : static_cast<int>(e);
}

// ---- reference-named shims (src/gpuar.h:74,77,78) --------------------------
void initConstantRange(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        t_last_error = GPUAR_ERR_NO_DEVICE;
        return;
    }
    (void)hipFree(nullptr);  // forces context creation on the current device
}

void garCompressExecutor(const uint8_t *source, size_t size, uint8_t *destination, uint32_t numBlocks) {
    (void)numBlocks;
    const int e = gpuar_hip_encode(source, size, destination, nullptr, nullptr);
    if (e != GPUAR_OK) {
        t_last_error = e;
        fprintf(stderr, "garCompressExecutor: %s\n", gpuar_hip_error_string(e));
    }
}

void garDecompressExecutor(const uint8_t *source, size_t size, uint8_t *destination, uint32_t numBlocks) {
    (void)numBlocks;
    // the reference's kernel decodes every packet whose slot STARTS inside `size` (index * 8704 < size,
    // src/gpuar_kernel.cu:916-934): a ceiling, not a floor
    const int e = launch_decode_slots(source, (size + GPUAR_SLOT_BYTES - 1) / GPUAR_SLOT_BYTES, size, destination, nullptr, nullptr);
    if (e != GPUAR_OK) {
        t_last_error = e;
        fprintf(stderr, "garDecompressExecutor: %s\n", gpuar_hip_error_string(e));
    }
}

}  // extern "C"
