/* gpuar_hip_mixed.h -- the mixed filter: byte planes, the delta filter or XOR against a base, at a width of
 * its own, chosen per 64 KiB supergroup of a buffer.  Exported by libgpuar_hip.so beside the calls of gpuar_hip.h and under the
 * same rules: codes, status word and stream as there, GPUAR_HIP_ABI_VERSION unchanged.
 *
 * Why a header of its own: the closed tables that pin gpuar_hip.h, gpuar_hip_gip.h and gpuar_hip_xsurvey.h are complete for
 * those headers; these calls are bound from gpuar_amd/hip.py's MIXED_SIGNATURES.
 *
 * A SUPERGROUP is 8 packets = 65536 bytes counted from the buffer's start; a buffer of n bytes has gpuar_hip_mode_count(n) =
 * ceil(n / 65536) of them, the last one maybe short.  Supergroup s carries one MODE byte m:
 *     bits 0-1: log2(w), w = 1, 2, 4, 8      bit 2: delta      bit 3: base
 * Valid modes are 0 .. 11; 12 .. 15 (delta and base together) and everything above are not.  With span(s) the supergroup's
 * bytes, split_mixed writes
 *     m = log2(w):      what gpuar_hip_split_planes(x[span], w) writes
 *     m = 4 + log2(w):  what gpuar_hip_split_delta(x[span], w) writes
 *     m = 8 + log2(w):  what gpuar_hip_split_xor(x[span], base[span], w) writes
 * each supergroup taken as a buffer of its own (the last one with its tail), and merge_mixed is the inverse.
 */
#ifndef GPUAR_HIP_MIXED_H
#define GPUAR_HIP_MIXED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ceil(n_bytes / 65536): the modes of one buffer. */
size_t gpuar_hip_mode_count(size_t n_bytes);

/* The modes of a batch: first_mode[b] = the modes of the buffers in front of b (n_buffers + 1 entries, the last one the total,
 * which is also returned).  first_mode may be NULL. */
size_t gpuar_hip_batch_mode_count(const uint64_t *bytes, size_t n_buffers, uint64_t *first_mode);

/* The mode of one supergroup from the predicted totals of its n_packets (1 .. 8) packets at widths 1, 2, 4, 8: plain (byte
 * planes alone), delta (NULL: not offered) and xored (NULL: not offered).  gpuar_hip_choose_filter(plain, delta) decides between
 * planes and delta -- without delta, gpuar_hip_choose_planes(plain) -- and the base is taken at gpuar_hip_choose_planes(xored) iff
 * that total + n_packets <= the total chosen so far (a tie goes to no base).  Returns the mode, 0 .. 11, and its total in *total
 * (may be NULL); a null plain is GPUAR_ERR_ARGUMENT.  Summed over a buffer, the chosen totals are at most the smallest
 * whole-buffer total of any candidate offered + 2 * the buffer's packets. */
int gpuar_hip_choose_mode(const uint64_t plain[4], const uint64_t *delta, const uint64_t *xored, uint64_t n_packets, uint64_t *total);

/* gpuar_hip_choose_mode for every supergroup of one buffer of n_bytes bytes, on the device, from the rows the surveys wrote
 * (gpuar_hip_survey_planes, gpuar_hip_survey_delta with all four widths, gpuar_hip_survey_xor's est rows): row j at + j * stride
 * words, entry p the buffer's packet p; d_delta and d_xored may be NULL.  d_modes: gpuar_hip_mode_count(n_bytes) bytes;
 * d_totals: as many 32-bit words, or NULL.  One lane per supergroup.
 *
 * Host-side checks, in this order: n_bytes == 0 is GPUAR_OK with no launch.  GPUAR_ERR_ARGUMENT: stride < the packet count,
 * more than 0xFFFFFFFF packets, a null d_plain or d_modes.  GPUAR_ERR_ALIGNMENT: the rows, d_totals and d_status (4).  Then the
 * status word (GPUAR_ERR_NO_DEVICE). */
int gpuar_hip_choose_modes(const uint32_t *d_plain, const uint32_t *d_delta, const uint32_t *d_xored, size_t stride, size_t n_bytes,
                           uint8_t *d_modes, uint32_t *d_totals, uint32_t *d_status, void *stream);

/* The same for a batch: entry p of every row belongs to batch packet p (the batch surveys' layout), d_bytes / d_first_packet as
 * for gpuar_hip_survey_planes_batch, d_first_mode as gpuar_hip_batch_mode_count gives it, n_modes its total.  Supergroup s of
 * buffer b gets d_modes[d_first_mode[b] + s] and d_totals[the same].  A supergroup that no buffer owns, or whose buffer does not
 * own exactly the packets its bytes make, is GPUAR_STATUS_BAD_BATCH in d_status (NULL: the fallback word) and nothing of it is
 * written.
 *
 * Host-side checks, in this order: n_modes == 0 is GPUAR_OK with no launch.  GPUAR_ERR_ARGUMENT: stride < n_packets, a null
 * descriptor array, a count above 0xFFFFFFFF, a null d_plain or d_modes.  GPUAR_ERR_ALIGNMENT: the rows, d_totals and d_status
 * (4), the descriptor arrays (8).  Then the status word. */
int gpuar_hip_choose_modes_batch(const uint32_t *d_plain, const uint32_t *d_delta, const uint32_t *d_xored, size_t stride, const uint64_t *d_bytes,
                                 const uint64_t *d_first_packet, const uint64_t *d_first_mode, size_t n_buffers, size_t n_packets, size_t n_modes,
                                 uint8_t *d_modes, uint32_t *d_totals, uint32_t *d_status, void *stream);

/* The same on the CPU, from the same source (gpuar_amd/csrc/mixed.h); no device is touched.  n_bytes == 0 is GPUAR_OK; a null
 * plain or modes, or stride < the packet count, is GPUAR_ERR_ARGUMENT. */
int gpuar_hip_choose_modes_host(const uint32_t *plain, const uint32_t *delta, const uint32_t *xored, size_t stride, size_t n_bytes, uint8_t *modes,
                                uint32_t *totals);

/* One buffer.  d_in and d_out: n_bytes each in device memory, 16-byte aligned, the same pointer (in place) or apart; d_base:
 * n_bytes, 16-byte aligned, apart from d_out, or NULL where no mode asks for a base; d_modes: gpuar_hip_mode_count(n_bytes)
 * bytes in device memory, any alignment.  Nothing is read beyond the 16-byte piece that holds the last byte and nothing written
 * beyond byte n_bytes.  A supergroup whose mode is not 0 .. 11, or asks for a base where d_base is NULL, is
 * GPUAR_STATUS_BAD_BATCH in d_status (NULL: the fallback word) and its bytes of d_out are not written; the others are.
 *
 * Host-side checks, in this order and before any device work: n_bytes == 0 is GPUAR_OK with no launch.  GPUAR_ERR_ARGUMENT: a
 * null d_in or d_out, more than 0xFFFFFFFF packets.  GPUAR_ERR_ALIGNMENT: d_in, d_out, d_base (16).  GPUAR_ERR_ARGUMENT: d_out
 * overlaps d_in without being it, or overlaps d_base; a null d_modes.  GPUAR_ERR_ALIGNMENT: d_status (4).  Then the status word. */
int gpuar_hip_split_mixed(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, const uint8_t *d_modes, uint8_t *d_out, uint32_t *d_status,
                          void *stream);
int gpuar_hip_merge_mixed(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, const uint8_t *d_modes, uint8_t *d_out, uint32_t *d_status,
                          void *stream);

/* A batch, with the descriptors of gpuar_hip_split_xor_batch except the widths: d_first_mode[b] is where buffer b's modes begin
 * in d_modes (n_buffers entries are read; gpuar_hip_batch_mode_count) and d_base_ptrs[b] its base, 0 for "no base".  A buffer
 * whose pointer, output pointer or base pointer is not 16-byte aligned, or that does not own exactly the packets its bytes make,
 * is GPUAR_STATUS_BAD_BATCH and left alone as a whole; a supergroup with a mode that is not 0 .. 11, or with a base mode in a
 * buffer without a base, is GPUAR_STATUS_BAD_BATCH and left alone, the buffer's other supergroups are moved.
 *
 * Host-side checks, in this order: n_packets == 0 is GPUAR_OK with no launch.  GPUAR_ERR_ARGUMENT: a null d_modes.
 * GPUAR_ERR_ALIGNMENT: d_base_ptrs (8).  GPUAR_ERR_ARGUMENT: a null d_first_mode, d_base_ptrs or d_out_ptrs.
 * GPUAR_ERR_ALIGNMENT: d_first_mode, d_out_ptrs (8).  Then the checks of every batch call (gpuar_hip.h). */
int gpuar_hip_split_mixed_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_first_mode, const uint8_t *d_modes, const uint8_t *const *d_base_ptrs, size_t n_buffers,
                                size_t n_packets, uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream);
int gpuar_hip_merge_mixed_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_first_mode, const uint8_t *d_modes, const uint8_t *const *d_base_ptrs, size_t n_buffers,
                                size_t n_packets, uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream);

/* The same on the CPU, from the same source; no device is touched and no alignment is asked.  base may be NULL where no mode asks
 * for it.  n_bytes == 0 is GPUAR_OK.  GPUAR_ERR_ARGUMENT, with nothing written: a null in, out or modes, an overlap as above, a
 * mode that is not 0 .. 11, a base mode with a null base. */
int gpuar_hip_split_mixed_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, const uint8_t *modes, uint8_t *out);
int gpuar_hip_merge_mixed_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, const uint8_t *modes, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* GPUAR_HIP_MIXED_H */
