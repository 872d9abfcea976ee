// tests/encode_table_emulation.cpp -- TEST HARNESS (CPU).  The table walk of encode_kernel_t16 (lane_codec.h: PickTable,
// TableTopModeler / TableLowModeler) one packet at a time on the host, beside the modelers the host CLI runs today
// (TopModeler / LowModeler).  Built by tests/test_encode_table.py into tests/_build/; never linked into a product library.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../gpuar_amd/csrc/lane_codec.h"

using namespace gpuar;

static const RecipTable kRecip = RecipTable();

// One packet after the other through a top modeler, a low modeler and the carry-form coder, each symbol with a look at its
// successor (PartialModeler::step).  slots: ceil(n / 8192) * 8704 bytes.  Returns the OR of the per-packet overflow flags.
template <typename Top, typename Low>
static int encode_slots_straight(const uint8_t *in, size_t n_bytes, uint8_t *slots)
{
    int any_overflow = 0;
    const size_t np = (n_bytes + kPacket - 1) / kPacket;
    std::vector<uint16_t> table(kTreeRows);
    for (size_t p = 0; p < np; ++p) {
        const size_t off = p * kPacket;
        const uint32_t len = static_cast<uint32_t>(n_bytes - off < kPacket ? n_bytes - off : kPacket);
        Top top;
        Low low;
        top.open(reinterpret_cast<uint8_t *>(table.data()), 0, in[off]);
        low.open(reinterpret_cast<uint8_t *>(table.data()), 0, in[off]);
        CarryCoderLane coder;
        coder.open(slots, static_cast<uint32_t>(p * kSlot));
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t next = i + 1 < len ? in[off + i + 1] : 0u;
            coder.step(top.step(in[off + i], 256u + i, next) + low.step(in[off + i], 256u + i, next), kRecip.r[i]);
        }
        bool ov;
        coder.finish(len, ov);
        any_overflow |= ov ? 1 : 0;
    }
    return any_overflow;
}

extern "C" {

// the table's entry for symbol x at depth 4..7, and what account() forms by shift and mask today: from the symbol
// (paths_of_symbol) and from the GPU's row tag x << 7 (paths_of_tag)
uint32_t emu_table_pick(uint32_t x, uint32_t depth) { return kPickTable.row[x & 15u][depth - 4u]; }
uint32_t emu_table_row_offset(uint32_t x) { return TableLowModeler<7>::row_offset(x << 7); }
uint32_t emu_shift_pick_of_symbol(uint32_t x, uint32_t depth) { return (LowModeler<1>::paths_of_symbol(x) >> (7u - depth)) & 0x10001u; }
uint32_t emu_shift_pick_of_tag(uint32_t x, uint32_t depth) { return (LowModeler<7>::paths_of_tag(x << 7) >> (7u + 7u - depth)) & 0x10001u; }

// what gpuar-host runs today (4 + 3, shift and mask), and the table walk's modelers in its place
int emu_current_encode_slots(const uint8_t *in, size_t n_bytes, uint8_t *slots) { return encode_slots_straight<TopModeler<1>, LowModeler<1>>(in, n_bytes, slots); }
int emu_table_encode_slots(const uint8_t *in, size_t n_bytes, uint8_t *slots) { return encode_slots_straight<TableTopModeler<1>, TableLowModeler<1>>(in, n_bytes, slots); }

// The table walk the way encode_kernel_t16's roles run it: phases of 8 symbols, rows 128 bytes apart with the lane's column
// in the address (kRowShift = 7, lane `lane` of 64), the low modeler a phase behind on row tags without lane bits
// (prime_tag at the start of a phase, step_tag, step_last_tag for the phase's last symbol), adding onto the top one's parts.
int emu_table_encode_slots_phased(const uint8_t *in, size_t n_bytes, uint8_t *slots, uint32_t lane)
{
    int any_overflow = 0;
    const size_t np = (n_bytes + kPacket - 1) / kPacket;
    std::vector<uint8_t> tree(kTreeRows * kLanes * 2);
    const uint32_t column = 2u * (((lane & 31u) << 1) | ((lane & 63u) >> 5));
    constexpr uint32_t kPhase = 8;
    for (size_t p = 0; p < np; ++p) {
        const size_t off = p * kPacket;
        const uint32_t len = static_cast<uint32_t>(n_bytes - off < kPacket ? n_bytes - off : kPacket);
        TableTopModeler<7> top;
        TableLowModeler<7> low;
        top.open(tree.data(), column, in[off]);
        low.open(tree.data(), column, 0);
        CarryCoderLane coder;
        coder.open(slots, static_cast<uint32_t>(p * kSlot));
        for (uint32_t base = 0; base < len; base += kPhase) {
            const uint32_t count = len - base < kPhase ? len - base : kPhase;
            uint32_t sums[kPhase], tags[kPhase];
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t i = base + j;
                const uint32_t xn_tag = top.tree.tag(i + 1 < len ? in[off + i + 1] : 0u);
                sums[j] = top.step_tag(top.next_tag, 256u + i, xn_tag);
            }
            for (uint32_t j = 0; j < count; ++j) tags[j] = low.tree.tag(in[off + base + j]);
            low.prime_tag(tags[0]);
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t i = base + j;
                sums[j] = j + 1 < count ? low.step_tag(tags[j], 256u + i, tags[j + 1], sums[j]) : low.step_last_tag(tags[j], 256u + i, sums[j]);
            }
            for (uint32_t j = 0; j < count; ++j) coder.step(sums[j], kRecip.r[base + j]);
        }
        bool ov;
        coder.finish(len, ov);
        any_overflow |= ov ? 1 : 0;
    }
    return any_overflow;
}

}  // extern "C"

// The kernel's other two forms (gpuar_kernels.hip, run_top "the rest", run_low "the phases that hold a ragged tail"), and the
// hand-off from the whole-phase form to them inside one packet.  A lane of encode_kernel_t16 works in
//   * the whole-phase form while every lane of its wavefront owns the phase -- the top modeler for the first
//     (len_min / 64) * 8 phases (it leaves its chunked loop after whole chunks of eight phases), the low modeler for the first
//     len_min / 8 phases, len_min the shortest length in the wavefront (0 where the group is not full);
//   * the ragged form after that: the top modeler by the symbol form step(x, total, next), `next` 0 past the packet's end as the
//     zero-filled guarded load gives it, on the nodes it HOLDS -- next_tag and left[] cross the hand-off as the last tag-form
//     step of the chunk left them, fetched for the next chunk's first byte, and nothing is primed again; the low modeler by
//     prime_tag + step_last_tag for every symbol (its whole-phase form ends on step_last_tag, so only the tree crosses).
// top_tag_phases / low_whole_phases: how many phases each modeler spends in the whole-phase form (both within the packet's own
// whole phases).  The same coder serves throughout.
static int encode_slots_forms(const uint8_t *in, size_t n_bytes, uint8_t *slots, uint32_t lane, uint32_t len_min, bool ragged_only)
{
    int any_overflow = 0;
    const size_t np = (n_bytes + kPacket - 1) / kPacket;
    std::vector<uint8_t> tree(kTreeRows * kLanes * 2);
    const uint32_t column = 2u * (((lane & 31u) << 1) | ((lane & 63u) >> 5));
    constexpr uint32_t kPhase = 8, kChunk = 64;
    for (size_t p = 0; p < np; ++p) {
        const size_t off = p * kPacket;
        const uint32_t len = static_cast<uint32_t>(n_bytes - off < kPacket ? n_bytes - off : kPacket);
        const uint32_t shortest = ragged_only ? 0u : (len_min < len ? len_min : len);
        const uint32_t top_tag_phases = (shortest / kChunk) * (kChunk / kPhase), low_whole_phases = shortest / kPhase;
        const uint32_t n_phases = (len + kPhase - 1) / kPhase;
        auto byte_at = [&](uint32_t i) -> uint32_t { return i < len ? in[off + i] : 0u; };      // (zero-filled past the end)
        TableTopModeler<7> top;
        TableLowModeler<7> low;
        top.open(tree.data(), column, in[off]);
        low.open(tree.data(), column, 0);
        CarryCoderLane coder;
        coder.open(slots, static_cast<uint32_t>(p * kSlot));
        for (uint32_t k = 0; k < n_phases; ++k) {
            const uint32_t base = k * kPhase;
            uint32_t sums[kPhase] = {};
            // the top modeler
            if (k < top_tag_phases) {
                for (uint32_t j = 0; j < kPhase; ++j)
                    sums[j] = top.step_tag(top.next_tag, 256u + base + j, top.tree.tag(byte_at(base + j + 1u)));
            } else {
                for (uint32_t j = 0; j < kPhase; ++j)
                    if (base + j < len) sums[j] = top.step(byte_at(base + j), 256u + base + j, byte_at(base + j + 1u));
            }
            // the low modeler, a phase behind
            if (k < low_whole_phases) {
                uint32_t tags[kPhase];
                for (uint32_t j = 0; j < kPhase; ++j) tags[j] = low.tree.tag(byte_at(base + j));
                low.prime_tag(tags[0]);
                for (uint32_t j = 0; j < kPhase; ++j)
                    sums[j] = j + 1u < kPhase ? low.step_tag(tags[j], 256u + base + j, tags[j + 1u], sums[j]) : low.step_last_tag(tags[j], 256u + base + j, sums[j]);
            } else {
                for (uint32_t j = 0; j < kPhase; ++j) {
                    if (base + j >= len) continue;
                    const uint32_t t = low.tree.tag(byte_at(base + j));
                    low.prime_tag(t);
                    sums[j] = low.step_last_tag(t, 256u + base + j, sums[j]);
                }
            }
            // the coder, two phases behind
            for (uint32_t j = 0; j < kPhase; ++j)
                if (base + j < len) coder.step(sums[j], kRecip.r[base + j]);
        }
        bool ov;
        coder.finish(len, ov);
        any_overflow |= ov ? 1 : 0;
    }
    return any_overflow;
}

extern "C" {

// every packet in the ragged form from its first symbol on: a lane of a group that is not full (len_min == 0)
int emu_table_encode_slots_ragged(const uint8_t *in, size_t n_bytes, uint8_t *slots, uint32_t lane)
{
    return encode_slots_forms(in, n_bytes, slots, lane, 0u, true);
}

// every packet as a lane of a full group whose shortest lane holds len_min bytes (clamped to the packet's own length)
int emu_table_encode_slots_handoff(const uint8_t *in, size_t n_bytes, uint8_t *slots, uint32_t lane, uint32_t len_min)
{
    return encode_slots_forms(in, n_bytes, slots, lane, len_min, false);
}

}  // extern "C"
