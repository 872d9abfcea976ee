/* gpuar_hip_xsurvey.h -- the XOR-base survey, exported by libgpuar_hip.so beside the calls of gpuar_hip.h and
 * under the same rules: codes, status word and stream as there, GPUAR_HIP_ABI_VERSION unchanged.
 *
 * Why a header of its own: the closed tables that pin gpuar_hip.h and gpuar_hip_gip.h are complete for those headers
 * (INTEGRATION.md 3); these calls are bound from gpuar_amd/hip.py's XSURVEY_SIGNATURES, with tables of their own
 * (tests/test_capi_xsurvey_host.py).
 *
 * For a buffer x and a base b of the same n bytes, with P = gpuar_hip_packet_count(n) packets, and j = 0 .. 3 for the byte-plane
 * widths w = 1, 2, 4, 8:
 *     est[j * stride + p]  = what gpuar_hip_estimate   gives for packet p of gpuar_hip_split_xor(x, b, w)
 *     scan[j * stride + p] = what gpuar_hip_sparse_scan gives for packet p of gpuar_hip_split_xor(x, b, w)
 * from one read of x and one of b; nothing is XORed or split into memory.  The est rows are the plane survey of x ^ b
 * (gpuar_hip_survey_planes).  Totals of the est rows -- or of what gpuar_hip_sparse_rule makes of both rows -- go to
 * gpuar_hip_choose_planes for the width of the bytes that are coded, and with the plane survey's totals to
 * gpuar_hip_choose_filter(plain, xored, n_packets, &width), which decides for the base as it does for the delta filter.
 */
#ifndef GPUAR_HIP_XSURVEY_H
#define GPUAR_HIP_XSURVEY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One buffer.  d_in and d_base: n_bytes each in device memory, 16-byte aligned; nothing is read beyond the 16-byte piece that
 * holds the last byte of either.  d_est and d_scan: 4 rows of at least P words, row j at + j * stride words, 4-byte aligned;
 * either may be NULL and is then not written, but not both.  Only the P entries of each asked row are written.
 *
 * Host-side checks, in this order and before any device work: n_bytes == 0 is GPUAR_OK with no launch (nothing else is looked
 * at).  GPUAR_ERR_ARGUMENT: stride < P, a null d_base, d_est and d_scan both null, a null d_in, more than 0xFFFFFFFF packets.
 * GPUAR_ERR_ALIGNMENT: d_in (16), the first output that is not null (4), then d_base (16) and d_scan (4).  Then the fallback
 * status word (GPUAR_ERR_NO_DEVICE). */
int gpuar_hip_survey_xor(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, uint32_t *d_est, uint32_t *d_scan, size_t stride,
                         void *stream);

/* A batch, with the descriptors of gpuar_hip_survey_planes_batch and d_base_ptrs[b] the base of buffer b (n_buffers pointers in
 * device memory, the array 8-byte aligned).  Entry p of every row belongs to batch packet p.  d_base_ptrs[b] == 0 means "no
 * base": the buffer's est entries are the plane survey's and its scan entries the scan of its plane splits.  A buffer whose
 * pointer or base pointer is not 16-byte aligned, or that does not own exactly the packets its bytes make, is
 * GPUAR_STATUS_BAD_BATCH in d_status (NULL: the fallback word) and none of its entries is written in either output; so is a
 * packet nobody owns.
 *
 * Host-side checks, in this order: n_packets == 0 is GPUAR_OK with no launch.  GPUAR_ERR_ARGUMENT: stride < n_packets, a null
 * d_base_ptrs, d_est and d_scan both null, a null descriptor array, n_packets or n_buffers above 0xFFFFFFFF.
 * GPUAR_ERR_ALIGNMENT: the first output that is not null (4), the descriptor arrays (8), d_status (4), then d_base_ptrs (8) and
 * d_scan (4).  Then the status word. */
int gpuar_hip_survey_xor_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                               const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets, uint32_t *d_est, uint32_t *d_scan,
                               size_t stride, uint32_t *d_status, void *stream);

/* The same on the CPU, from the same source as the kernel (gpuar_amd/csrc/xor_survey.h); no device is touched.  n_bytes == 0 is
 * GPUAR_OK; a null in or base, est and scan both null, or stride < P is GPUAR_ERR_ARGUMENT. */
int gpuar_hip_survey_xor_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, uint32_t *est, uint32_t *scan, size_t stride);

#ifdef __cplusplus
}
#endif
#endif /* GPUAR_HIP_XSURVEY_H */
