/* gpuar_hip_gip.h -- the device call behind batch.from_gip, exported by libgpuar_hip.so beside the calls of
 * gpuar_hip.h and under the same rules: codes, status word and stream as there, GPUAR_HIP_ABI_VERSION unchanged.
 *
 * Why a header of its own: the closed tables that pin gpuar_hip.h (the set of its names, and for every device call of it the
 * code of each defect) are complete for that header; a device call added later is declared here and bound from
 * gpuar_amd/hip.py's GIP_SIGNATURES, with tables of its own (tests/test_capi_gip_host.py).  The host-only readers that go with
 * this call, gpuar_hip_gip_read_host and gpuar_hip_gip_tables_host, are in gpuar_hip.h.
 */
#ifndef GPUAR_HIP_GIP_H
#define GPUAR_HIP_GIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Copies n_regions regions: d_bytes[r] bytes (1 .. 8704; 0 moves nothing) from d_src_ptrs[r] to d_dst_ptrs[r].  Both pointers
 * may have ANY byte alignment; the three arrays are in device memory and 8-byte aligned.  This is what takes the packets of a
 * version-6 .gip stream -- coded, raw and sparse, interleaved at byte alignment -- apart into the three regions of a
 * batch.Compressed, in one launch.
 *
 * Nothing is read outside [d_src_ptrs[r], d_src_ptrs[r] + d_bytes[r]) and nothing is written outside [d_dst_ptrs[r],
 * d_dst_ptrs[r] + d_bytes[r]): destination regions may stand back to back at byte grain, and a region that ends inside a
 * 16-byte piece of memory leaves the rest of the piece to its neighbour.  Regions must not overlap one another (a destination
 * with any other region); the order in which regions are moved is unspecified.
 *
 * A region with a null pointer or more than 8704 bytes is GPUAR_STATUS_BAD_BATCH in d_status (NULL: the fallback word) and is
 * skipped: its destination is left untouched.
 *
 * Host-side checks, in the order of gpuar_hip_move_packets and before any device work: n_regions == 0 is GPUAR_OK with no
 * launch (the pointers are not looked at); a null array, or n_regions above 0xFFFFFFFF, is GPUAR_ERR_ARGUMENT; an array that is
 * not 8-byte aligned, or a d_status that is not 4-byte aligned, is GPUAR_ERR_ALIGNMENT. */
int gpuar_hip_move_bytes(const uint8_t *const *d_src_ptrs, uint8_t *const *d_dst_ptrs, const uint64_t *d_bytes, size_t n_regions,
                         uint32_t *d_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPUAR_HIP_GIP_H */
