/*
 * gpuar_hip.h -- C ABI of the MI355X-native (gfx950) arithmetic-coding path.
 *
 * This is the drop-in boundary for the GPU encode/decode path of
 * jiahansu/GPUAR.  The first three entry points carry the reference's own
 * names and signatures, so the reference's GPUCompressor
 * (src/gpu_compressor.cpp:19,185,357) links against libgpuar_hip.so unchanged;
 * the gpuar_hip_* entry points are the stream- and device-explicit native ABI
 * the rest of this repository (C++ host classes, Python bindings, bench) uses.
 *
 * Plain pointers and sizes only.  All `d_*` / `source` / `destination`
 * pointers are DEVICE pointers owned by the caller (hipMalloc, or any
 * allocator that yields HIP device memory, e.g. a torch CUDA tensor).
 * Nothing here allocates device memory, and nothing throws across the boundary.
 * State kept between calls, all of it per device and none of it affecting
 * results: a fallback status word (used only by launches that were given no
 * status word of their own, i.e. the reference-named executors) and an arrival
 * counter per compute unit the encoder uses to place its wavefronts.
 *
 * Packet geometry (reference: src/gpu.h:8-14):
 *   input  is cut into 8192-byte packets, packet p = bytes [p*8192, ...)
 *   output packet p lives in the 8704-byte slot at p*8704; only its first
 *          `clen` bytes are defined: u16 LE clen (incl. this 4-byte header),
 *          u16 LE ulen, then the MSB-first arithmetic-coded bitstream
 *          (src/gpuar_kernel.cu:523-528).
 */
#ifndef GPUAR_HIP_H
#define GPUAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPUAR_PACKET_BYTES        8192u  /* UNCOMPRESSED_PACKET_SIZE, src/gpu.h:13 */
#ifndef GPUAR_SLOT_BYTES                 /* only tests/lane_emulation.cpp ever overrides it (to drive a lane into overflow) */
#define GPUAR_SLOT_BYTES          8704u  /* COMPRESSED_PACKET_SIZE,   src/gpu.h:12 */
#endif
#define GPUAR_PACKET_HEADER_BYTES 4u     /* PACKET_HEADER_LENGTH,     src/gpu.h:14 */

/* Error codes returned by the gpuar_hip_* calls (0 = ok).  Positive values
 * are hipError_t codes passed through unchanged. */
#define GPUAR_OK                 0
#define GPUAR_ERR_ALIGNMENT     (-1)  /* device pointer not 16-byte aligned            */
#define GPUAR_ERR_ARGUMENT      (-2)  /* null pointer / size out of range              */
#define GPUAR_ERR_NO_DEVICE     (-3)  /* no HIP device visible                         */

/* Bits a launch ORs into its status word (the caller's `d_status`, or the
 * device's fallback word that gpuar_hip_status reads). */
#define GPUAR_STATUS_SLOT_OVERFLOW  0x1u /* a packet outgrew its 8704-byte slot; its slot is truncated
                                            (the reference would write past the slot, SURVEY.md s.7 risk 3) */
#define GPUAR_STATUS_BAD_PACKET     0x2u /* decode met a header it refuses (ulen > 8192 or clen < 4); that
                                            packet's output is left unwritten.  Any other damage is decoded as
                                            the reference decodes it: its third exit, a code value no symbol
                                            owns (src/gpuar_kernel.cu:873-877), cannot be reached            */

#define GPUAR_STATUS_BAD_BATCH      0x4u /* batch calls only: a packet whose descriptor is unusable -- no buffer owns it, it
                                            starts at or past its buffer's end (the buffer's d_in_bytes / d_out_bytes), or its
                                            buffer's pointer is not 16-byte aligned.  That packet is skipped: its slot (encode)
                                            or output (decode) is left untouched */

#define GPUAR_STATUS_CHECKSUM       0x8u /* verify calls only: a packet's bytes do not match its stored CRC-32 (see there) */

/* ------------------------------------------------------------------------
 * Reference-named entry points (the reference's kernel object exports these;
 * declarations: /root/reference/src/gpuar.h:74,77,78).
 * ---------------------------------------------------------------------- */

/* Replaces initConstantRange (src/gpuar_kernel.cu:453-460), which uploads the
 * initial uniform model to __constant__ memory.  The HIP kernels build the
 * initial model in LDS themselves and read their reciprocal table from a
 * compile-time constant, so this only selects/initialises the current device
 * context; calling it is optional and idempotent. */
void initConstantRange(void);

/* Replaces garCompressExecutor (src/gpuar_kernel.cu:936-944): encodes the
 * `size` bytes at `source` into ceil(size/8192) slots at `destination`.
 * Asynchronous on the NULL stream, like the reference's <<<>>> launch; errors
 * surface at the caller's next synchronising HIP call and through
 * gpuar_hip_last_error().  `numBlocks` (the reference's grid size for
 * 32-thread blocks) is accepted and ignored: the launch shape is derived
 * from `size`. */
void garCompressExecutor(const uint8_t *source, size_t size, uint8_t *destination, uint32_t numBlocks);

/* Replaces garDecompressExecutor (src/gpuar_kernel.cu:946-954): `size` is
 * numPackets*8704 (src/gpu_compressor.cpp:357); every slot that STARTS inside
 * `size` is decoded (index*8704 < size, src/gpuar_kernel.cu:916-934); slot p
 * decodes to destination + p*8192.  Bytes behind source + size may be loaded
 * from the 16-byte-aligned piece of memory that holds its last byte, and no
 * further: a packet whose decoding runs past the end gets unspecified bytes
 * within its own ulen (the reference would read zeros there; a packet shorter
 * than 64 bytes does read zeros), and bytes more than 15 behind the end never
 * change any output.  A slot whose 4-byte header does not lie in front of the
 * end is flagged GPUAR_STATUS_BAD_PACKET and writes nothing. */
void garDecompressExecutor(const uint8_t *source, size_t size, uint8_t *destination, uint32_t numBlocks);

/* ------------------------------------------------------------------------
 * Native ABI: explicit stream (a hipStream_t passed as void*; NULL = the
 * NULL stream), int return codes, usable from one host thread per GPU.
 * ---------------------------------------------------------------------- */

/* Number of packets / slots for an input of n_bytes. */
size_t gpuar_hip_packet_count(size_t n_bytes);

/* `d_status` (encode, decode, decode_stream): a caller-owned 32-bit DEVICE word
 * (4-byte aligned) that this launch -- and only this launch -- ORs its
 * GPUAR_STATUS_* bits into; the caller zeroes it and copies it back on the same
 * stream, so concurrent launches on other streams never share a flag and no
 * device-wide synchronisation is needed.  NULL: the bits go to the device's
 * fallback word instead (gpuar_hip_status). */

/* Encode n_bytes at d_in (16-byte aligned) into packet slots at d_slots
 * (16-byte aligned, gpuar_hip_packet_count(n_bytes)*8704 bytes). */
int gpuar_hip_encode(const uint8_t *d_in, size_t n_bytes, uint8_t *d_slots, uint32_t *d_status, void *stream);

/* The same with the ENCODE kernel named by the caller (there is one decode kernel per input layout and no
 * decode mode).  Both encode kernels write the same bytes; they differ in how a launch is cut into wavefronts:
 *   GPUAR_MODE_THROUGHPUT  three working wavefronts (and one that carries constants) per 64 packets:
 *                          the most bytes per second from a launch that fills the chip;
 *   GPUAR_MODE_LATENCY     a finer cut -- six working wavefronts (and a seventh that carries constants) per
 *                          64 packets -- with a shorter symbol step: faster while the launch cannot fill
 *                          the chip by itself;
 *   GPUAR_MODE_TABLE       THROUGHPUT's cut with the table walk: the tree dealt 3 + 4 and the path operands of
 *                          depths 4-7 read from a 256-byte table in LDS (encode_kernel_t16), at any size;
 *   GPUAR_MODE_AUTO        what gpuar_hip_encode does: LATENCY up to 32768 packets (256 MiB of input),
 *                          TABLE above -- right for a launch that has the chip to itself; a pipeline
 *                          that keeps several launches in flight names THROUGHPUT.
 * The choice is an argument, never an environment variable: this library reads no environment.
 * Any other `mode` is GPUAR_ERR_ARGUMENT. */
#define GPUAR_MODE_AUTO        0
#define GPUAR_MODE_THROUGHPUT  1
#define GPUAR_MODE_LATENCY     2
#define GPUAR_MODE_TABLE       3       /* gpuar_hip_encode_mode only: the batch encoders have no table walk */
int gpuar_hip_encode_mode(const uint8_t *d_in, size_t n_bytes, uint8_t *d_slots, uint32_t *d_status, void *stream, int mode);

/* Decode n_packets slots at d_slots into d_out (n_packets*8192 bytes; the
 * last packet writes only its ulen bytes). */
int gpuar_hip_decode(const uint8_t *d_slots, size_t n_packets, uint8_t *d_out, uint32_t *d_status, void *stream);

/* Device-side compaction (what the reference does with one 8704-byte D2H copy
 * and one fwrite per packet, src/gpu_compressor.cpp:138,161-168):
 *   d_offsets[p]   = sum of clen of packets < p   (n_packets+1 entries, u64)
 *   d_stream       = packets back to back, exactly the bytes that follow the
 *                    20-byte header in a .gip file.
 * d_stream (8-byte aligned) needs room for the sum of clen (<= n_packets*8704);
 * its first bytes serve as scan scratch before the packets are gathered into
 * it, so the call keeps no state outside its arguments and may run
 * concurrently on different streams and devices.  At most 16 777 215 packets
 * (128 GiB of input) per call: GPUAR_ERR_ARGUMENT above. */
int gpuar_hip_compact(const uint8_t *d_slots, size_t n_packets, uint8_t *d_stream,
                      uint64_t *d_offsets, void *stream);

/* Decode straight from a back-to-back packet stream: d_offsets[p] is the byte
 * offset of packet p in d_stream (n_packets+1 entries; the host builds it by
 * walking `off += clen`, src/gpu_compressor.cpp:299-312, or keeps the array
 * gpuar_hip_compact produced).  A packet's reader may run on into the packets
 * behind it, as the reference's does, up to d_stream + d_offsets[n_packets];
 * behind that end the same holds as for garDecompressExecutor's `size`. */
int gpuar_hip_decode_stream(const uint8_t *d_stream, const uint64_t *d_offsets, size_t n_packets,
                            uint8_t *d_out, uint32_t *d_status, void *stream);

/* ------------------------------------------------------------------------
 * Batches: many independent buffers in one launch.
 *
 * A batch is n_buffers buffers; buffer b owns the batch packets first_packet[b] .. first_packet[b+1] - 1, i.e.
 * ceil(bytes[b] / 8192) of them (a zero-byte buffer owns none), back to back in batch order, and batch packet p lives
 * in slot p (d_slots + p * 8704).  Each buffer is coded EXACTLY as if it were encoded alone: its slots are the bytes
 * gpuar_hip_encode gives for it.  So gpuar_hip_compact of the batch's n_packets slots is the batch's compaction, and
 * buffer b's stream is d_stream[offsets[first_packet[b]] .. offsets[first_packet[b+1]]) -- what `gpuar c` writes for
 * that buffer behind its 20-byte header.
 *
 * All d_* arrays live in device memory: d_in_ptrs / d_out_ptrs (n_buffers device pointers), d_in_bytes / d_out_bytes
 * (n_buffers u64), d_first_packet (n_buffers + 1 u64), all three 8-byte aligned.  The host-side checks return before
 * any device work, as the single-buffer calls do: a null pointer, n_packets or n_buffers above 0xFFFFFFFF or a bad
 * `mode` is GPUAR_ERR_ARGUMENT; a misaligned d_slots (16 bytes), d_stream (4), d_status (4) or descriptor array (8)
 * GPUAR_ERR_ALIGNMENT.  n_packets == 0 is GPUAR_OK with no launch.  What the device finds wrong with a packet's
 * descriptor is GPUAR_STATUS_BAD_BATCH in d_status, per packet (see there).
 * ---------------------------------------------------------------------- */

/* Host only: first_packet[0 .. n_buffers] from bytes[0 .. n_buffers-1] (host arrays; first_packet may be NULL to count
 * only).  Returns the batch's packet count (0 if bytes is NULL while n_buffers is not 0). */
size_t gpuar_hip_batch_packet_count(const uint64_t *bytes, size_t n_buffers, uint64_t *first_packet);

/* Encode the batch's buffers (each 16-byte aligned) into n_packets slots at d_slots.  `mode` as in gpuar_hip_encode_mode,
 * with the same 32768-packet switch for GPUAR_MODE_AUTO.  Both kernels keep a lane on its whole-phase step for every whole
 * phase it owns, whatever its neighbours' lengths; only each packet's own partial phase goes symbol by symbol. */
int gpuar_hip_encode_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                           size_t n_buffers, size_t n_packets, uint8_t *d_slots, uint32_t *d_status, void *stream, int mode);

/* Decode n_packets slots of a batch: packet j of buffer b writes its header's ulen bytes at d_out_ptrs[b] + j * 8192
 * (each d_out_ptrs[b] 16-byte aligned).  A packet that starts inside its buffer (j * 8192 < d_out_bytes[b]) but has
 * j * 8192 + ulen > d_out_bytes[b] is GPUAR_STATUS_BAD_PACKET and writes nothing, so a damaged packet never writes into
 * its neighbour's buffer; one that starts at or past the end is GPUAR_STATUS_BAD_BATCH; everything else decodes as
 * gpuar_hip_decode does, with the same promises about what is read. */
int gpuar_hip_decode_batch(const uint8_t *d_slots, const uint64_t *d_first_packet, size_t n_buffers, size_t n_packets,
                           uint8_t *const *d_out_ptrs, const uint64_t *d_out_bytes, uint32_t *d_status, void *stream);

/* The same from the compacted stream of a batch: d_offsets (n_packets + 1 entries) in batch order, as gpuar_hip_compact
 * of the batch's slots produced them; reads as gpuar_hip_decode_stream does. */
int gpuar_hip_decode_stream_batch(const uint8_t *d_stream, const uint64_t *d_offsets, const uint64_t *d_first_packet,
                                  size_t n_buffers, size_t n_packets, uint8_t *const *d_out_ptrs,
                                  const uint64_t *d_out_bytes, uint32_t *d_status, void *stream);

/* ------------------------------------------------------------------------
 * Per-packet CRC-32: CRC-32/ISO-HDLC, the CRC of zlib.crc32 and gzip (crc32("123456789") = 0xCBF43926), of each packet's
 * UNCOMPRESSED bytes: crc[p] covers bytes [p * 8192, min((p + 1) * 8192, n_bytes)) of its buffer.  These are the checksums of
 * the .gip trailer version 2; computed before encoding and verified after decoding, they check the whole
 * pipeline, the codec included.
 *
 * Host-side checks as in the calls above, before any device work: a null data pointer or d_crc is GPUAR_ERR_ARGUMENT; a data
 * pointer that is not 16-byte aligned, a d_crc not 4-byte, d_first_bad or a descriptor array not 8-byte, d_status not 4-byte
 * aligned is GPUAR_ERR_ALIGNMENT.  n_bytes == 0 / n_packets == 0 is GPUAR_OK with no launch.  Nothing is read beyond the
 * 16-byte-aligned piece of memory that holds a buffer's last byte.
 * ---------------------------------------------------------------------- */

/* crc[p] for the gpuar_hip_packet_count(n_bytes) packets of the n_bytes at d_in. */
int gpuar_hip_crc32(const uint8_t *d_in, size_t n_bytes, uint32_t *d_crc, void *stream);

/* Recomputes the CRC of every packet of the n_bytes at d_out (decoded output: packet p at d_out + p * 8192) and compares it with
 * d_crc[p].  On a mismatch ORs GPUAR_STATUS_CHECKSUM into d_status (NULL: the fallback word, as for the other calls) and, if
 * d_first_bad is not NULL, takes the atomic minimum of the packet's index and *d_first_bad: the caller sets it to UINT64_MAX
 * before the call and finds the lowest failing packet there after it. */
int gpuar_hip_verify_crc32(const uint8_t *d_out, size_t n_bytes, const uint32_t *d_crc,
                           uint64_t *d_first_bad, uint32_t *d_status, void *stream);

/* The same for a batch (descriptors as for gpuar_hip_encode_batch): d_crc[p] for batch packet p.  A packet whose descriptor is
 * unusable is GPUAR_STATUS_BAD_BATCH in d_status, by the encoder's rules, and its d_crc[p] is left untouched. */
int gpuar_hip_crc32_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                          size_t n_buffers, size_t n_packets, uint32_t *d_crc, uint32_t *d_status, void *stream);

/* Verify for a batch: d_out_bytes holds each buffer's ORIGINAL size (what was compressed), not its room; d_first_bad receives the
 * lowest failing BATCH packet index.  Unusable descriptors: GPUAR_STATUS_BAD_BATCH, that packet is not compared. */
int gpuar_hip_verify_crc32_batch(const uint8_t *const *d_out_ptrs, const uint64_t *d_out_bytes,
                                 const uint64_t *d_first_packet, size_t n_buffers, size_t n_packets,
                                 const uint32_t *d_crc, uint64_t *d_first_bad, uint32_t *d_status, void *stream);

/* ------------------------------------------------------------------------
 * Byte planes: regrouping typed data in front of the codec.  For elements of elem_bytes = w bytes (2, 4 or 8; 1 = no
 * transform) a GROUP is G = w * 8192 bytes = w whole packets, counted from the buffer's start, and for a buffer of n bytes
 *     every full group at base B = g * G:   out[B + k * 8192 + i] = in[B + i * w + k]     0 <= i < 8192, 0 <= k < w
 *     the tail of r = n mod G bytes at base B = n - r, with e = r div w:
 *                                           out[B + k * e + i]    = in[B + i * w + k]     0 <= i < e;  the last r mod w
 *                                           bytes are copied as they are.
 * That is SPLIT: packet k of a group is byte plane k of its 8192 elements, which one adaptive model codes better than
 * the mixture.  MERGE is the inverse.  The output has n bytes; packet counts, slots, compaction and
 * first_packet are untouched, and a chunk that starts on a multiple of 8 packets can be transformed alone.  Separate
 * launches in front of encode / behind decode; `out` may be `in` (every group is read whole before it is written).
 * Nothing is read beyond the 16-byte piece that holds a buffer's last byte and nothing written beyond byte n.
 * ---------------------------------------------------------------------- */

/* One buffer.  elem_bytes outside {1, 2, 4, 8} or (with n_bytes != 0) a null pointer: GPUAR_ERR_ARGUMENT; a pointer that is not
 * 16-byte aligned: GPUAR_ERR_ALIGNMENT; d_in and d_out overlapping without being equal: GPUAR_ERR_ARGUMENT.  n_bytes == 0,
 * or elem_bytes == 1 with d_in == d_out, is GPUAR_OK with no launch (elem_bytes == 1 otherwise copies). */
int gpuar_hip_split_planes(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream);
int gpuar_hip_merge_planes(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream);

/* A batch (descriptors as for gpuar_hip_encode_batch, with the same host-side checks before any device work): buffer b's
 * d_bytes[b] bytes at d_in_ptrs[b] go to d_out_ptrs[b] (which may be the same pointer), as elements of d_elem_bytes[b] bytes
 * (n_buffers u64, 8-byte aligned, like d_out_ptrs).  An unusable descriptor is GPUAR_STATUS_BAD_BATCH in d_status for each of
 * its packets, by the encoders' rules; here a width outside {1, 2, 4, 8}, a misaligned d_out_ptrs[b] and a buffer whose
 * first_packet range is not exactly the packets its bytes make count as unusable too, and such a buffer is left untouched. */
int gpuar_hip_split_planes_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                 const uint64_t *d_elem_bytes, size_t n_buffers, size_t n_packets, uint8_t *const *d_out_ptrs,
                                 uint32_t *d_status, void *stream);
int gpuar_hip_merge_planes_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                 const uint64_t *d_elem_bytes, size_t n_buffers, size_t n_packets, uint8_t *const *d_out_ptrs,
                                 uint32_t *d_status, void *stream);

/* Host only: the same maps on host memory, from the same definition (gpuar_amd/csrc/planes.h) -- no device is touched.
 * `out` may be `in`; any other overlap, a bad width or (with n_bytes != 0) a null pointer is GPUAR_ERR_ARGUMENT. */
int gpuar_hip_split_planes_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out);
int gpuar_hip_merge_planes_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out);

/* ------------------------------------------------------------------------
 * Delta filter in front of the byte planes (gpuar_amd/csrc/delta.h).  Inside every group of the byte-plane
 * layout above (G = w * 8192 bytes), and inside the e = r div w elements of the tail, the elements are read as little-endian
 * unsigned w-byte integers v[] and replaced by
 *     d[0] = v[0]      d[i] = v[i] - v[i - 1]   (mod 2^(8 w));      the tail's last r mod w bytes stay as they are.
 * SPLIT_DELTA is gpuar_hip_split_planes of that, MERGE_DELTA its inverse: gpuar_hip_merge_planes, then the prefix sum inside
 * every group.  The predictor resets at every group, so groups stay independent of each other.  One fused pass: the same
 * launches, access rules and overlap rule as the planes calls.  elem_bytes == 1 is a byte delta per packet and does work, in
 * place too.  Ordered integers (offsets, sorted indices, timestamps, samples) compress 2 - 15 x smaller behind it; unordered
 * data and floats grow: the filter is for the caller to ask for.
 * ---------------------------------------------------------------------- */

/* One buffer: arguments and error codes of gpuar_hip_split_planes (n_bytes == 0 is GPUAR_OK with no launch). */
int gpuar_hip_split_delta(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream);
int gpuar_hip_merge_delta(const uint8_t *d_in, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream);

/* A batch: arguments of gpuar_hip_split_planes_batch plus d_filter (n_buffers u64, 8-byte aligned): 0 = byte planes alone
 * (that buffer's output is gpuar_hip_split_planes_batch's), 1 = delta.  Any other value makes the buffer unusable
 * (GPUAR_STATUS_BAD_BATCH) and it is left untouched, like the other unusable descriptors. */
int gpuar_hip_split_delta_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_elem_bytes, const uint64_t *d_filter, size_t n_buffers, size_t n_packets,
                                uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream);
int gpuar_hip_merge_delta_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_bytes, const uint64_t *d_first_packet,
                                const uint64_t *d_elem_bytes, const uint64_t *d_filter, size_t n_buffers, size_t n_packets,
                                uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream);

/* Host only, from the same definition; rules of gpuar_hip_split_planes_host. */
int gpuar_hip_split_delta_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out);
int gpuar_hip_merge_delta_host(const uint8_t *in, size_t n_bytes, uint32_t elem_bytes, uint8_t *out);

/* Host only, for tests: the kernels' register transform of one block of 16 elements (mixed: 4 * elem_bytes dwords, in place).
 * undo == 0: the differences, `carried` being the element in front of the block; undo != 0: the inclusive prefix sums plus
 * `carried`, and in *total (may be null) the block's sum without it. */
int gpuar_hip_delta_block_host(uint32_t *mixed, uint32_t elem_bytes, int undo, uint64_t carried, uint64_t *total);

/* ------------------------------------------------------------------------
 * XOR against a base in front of the byte planes (gpuar_amd/csrc/xorbase.h).  For a buffer x and a base b of
 * the same n_bytes, y[i] = x[i] ^ b[i] for every i < n_bytes; SPLIT_XOR is gpuar_hip_split_planes of y, MERGE_XOR is
 * gpuar_hip_merge_planes followed by the XOR with b.  The XOR covers every byte, the tail's last r mod w included.  One fused
 * pass: the same launches, access rules and overlap rule as the planes calls; the base is read by the same rules (never beyond
 * the 16-byte piece that holds its last byte) and never written.  elem_bytes == 1 is a plain XOR and does work, in place too.
 * A tensor that is close to its base (the next checkpoint of a model) compresses 0.06 - 0.72 of its size behind it; against
 * an unrelated base it grows: the filter is for the caller to ask for.
 * Left out: a base together with the delta filter, a base of another length, a base chosen per region of a buffer.
 * ---------------------------------------------------------------------- */

/* One buffer: arguments and error codes of gpuar_hip_split_planes, in the same order of checks (n_bytes == 0 is GPUAR_OK with
 * no launch).  A null d_base is GPUAR_ERR_ARGUMENT, a d_base that is not 16-byte aligned GPUAR_ERR_ALIGNMENT, a d_base whose
 * n_bytes overlap those of d_out (d_out == d_in included) GPUAR_ERR_ARGUMENT. */
int gpuar_hip_split_xor(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream);
int gpuar_hip_merge_xor(const uint8_t *d_in, const uint8_t *d_base, size_t n_bytes, uint32_t elem_bytes, uint8_t *d_out, void *stream);

/* A batch: arguments of gpuar_hip_split_planes_batch plus d_base_ptrs (n_buffers device pointers, 8-byte aligned): 0 = byte
 * planes alone (that buffer's output is gpuar_hip_split_planes_batch's), otherwise the buffer's base, d_in_bytes[b] bytes that
 * overlap no output.  A base pointer that is not 16-byte aligned makes the buffer unusable (GPUAR_STATUS_BAD_BATCH) and it is
 * left untouched, like the other unusable descriptors. */
int gpuar_hip_split_xor_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                              const uint64_t *d_elem_bytes, const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets,
                              uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream);
int gpuar_hip_merge_xor_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                              const uint64_t *d_elem_bytes, const uint8_t *const *d_base_ptrs, size_t n_buffers, size_t n_packets,
                              uint8_t *const *d_out_ptrs, uint32_t *d_status, void *stream);

/* Host only, from the same definition; rules of gpuar_hip_split_planes_host, and a null or overlapping base as above. */
int gpuar_hip_split_xor_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, uint32_t elem_bytes, uint8_t *out);
int gpuar_hip_merge_xor_host(const uint8_t *in, const uint8_t *base, size_t n_bytes, uint32_t elem_bytes, uint8_t *out);

/* ------------------------------------------------------------------------
 * Packet size estimate and raw packets.  The codec's model starts every symbol at count 1, adds 1 per occurrence and never
 * rescales inside a packet, so a packet's ideal code length depends on its byte histogram h alone.  With
 *     lg16(k) = floor(2^16 log2 k),   LF[c] = sum of lg16(k) for k = 2 .. c   (LF[0] = LF[1] = 0)
 *     cost16  = LF[n + 255] - LF[255] - sum over the 256 symbols s of LF[h[s]]
 * the estimate of a packet of n bytes (1 .. 8192) is
 *     est = 4 + ((cost16 + 2^19 - 1) >> 19)
 * (gpuar_amd/csrc/estimate.h: one integer definition for the host and the kernels).  est[p] is the predicted clen of packet p,
 * its 4-byte header included; against the reference codec's real clen it was within +-1 byte on every packet measured
 * (INTEGRATION.md).  A packet is worth STORING raw instead of coding iff  est[p] >= 4 + ulen[p]  (ulen[p]: the packet's
 * uncompressed bytes): its coded form would then be at least 3 bytes longer than the bytes themselves.
 *
 * Host-side checks as for the CRC calls, in the same order and before any device work: n_bytes == 0 / n_packets == 0 /
 * n_regions == 0 is GPUAR_OK with no launch; a null pointer is GPUAR_ERR_ARGUMENT; a data pointer that is not 16-byte
 * aligned, a d_est not 4-byte, a descriptor array not 8-byte, d_status not 4-byte aligned is GPUAR_ERR_ALIGNMENT.  Nothing
 * is read beyond the 16-byte-aligned piece of memory that holds a buffer's (a region's) last byte.
 * ---------------------------------------------------------------------- */

/* est[p] for the gpuar_hip_packet_count(n_bytes) packets of the n_bytes at d_in. */
int gpuar_hip_estimate(const uint8_t *d_in, size_t n_bytes, uint32_t *d_est, void *stream);

/* The same for a batch (descriptors as for gpuar_hip_encode_batch): d_est[p] for batch packet p.  A packet whose descriptor is
 * unusable is GPUAR_STATUS_BAD_BATCH in d_status, by the encoders' rules, and its d_est[p] is left untouched. */
int gpuar_hip_estimate_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                             size_t n_buffers, size_t n_packets, uint32_t *d_est, uint32_t *d_status, void *stream);

/* Host only: the same values for host memory, from the same definition -- no device is touched. */
int gpuar_hip_estimate_host(const uint8_t *in, size_t n_bytes, uint32_t *est);

/* Copies n_regions regions: d_bytes[r] bytes (1 .. 8192; 0 moves nothing) from d_src_ptrs[r] to d_dst_ptrs[r], both 16-byte
 * aligned, the three arrays in device memory and 8-byte aligned.  This is what moves the packets that are stored raw.  Nothing
 * is written beyond a region's last byte.  A region with a misaligned pointer or more than 8192 bytes is
 * GPUAR_STATUS_BAD_BATCH in d_status and is skipped: its destination is left untouched. */
int gpuar_hip_move_packets(const uint8_t *const *d_src_ptrs, uint8_t *const *d_dst_ptrs, const uint64_t *d_bytes,
                           size_t n_regions, uint32_t *d_status, void *stream);

/* ------------------------------------------------------------------------
 * Plane-width survey: what a buffer would compress to at each byte-plane width, from one read of its bytes.  For a buffer of
 * P packets and j = 0 .. 3 (the widths w = 1, 2, 4, 8),
 *     d_est[j * est_stride + p]  =  the gpuar_hip_estimate value of packet p of gpuar_hip_split_planes(buffer, w)
 * for every p < P, by definition (gpuar_amd/csrc/survey.h); no split is made and nothing but d_est is written.  The sum of row
 * j is the size predicted for width w; gpuar_hip_choose_planes picks a width from the four sums.
 *
 * Host-side checks as for gpuar_hip_estimate, in the same order; in addition est_stride must be at least the packet count
 * (GPUAR_ERR_ARGUMENT).  Nothing is read beyond the 16-byte-aligned piece of memory that holds a buffer's last byte.
 * ---------------------------------------------------------------------- */

/* The four rows for the n_bytes at d_in. */
int gpuar_hip_survey_planes(const uint8_t *d_in, size_t n_bytes, uint32_t *d_est, size_t est_stride, void *stream);

/* The same for a batch (descriptors as for gpuar_hip_encode_batch): column p of d_est is batch packet p.  A buffer whose pointer
 * is not 16-byte aligned or that does not own exactly the packets its bytes make is GPUAR_STATUS_BAD_BATCH in d_status, and
 * its columns are left untouched in all four rows; a packet that no buffer owns likewise. */
int gpuar_hip_survey_planes_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                                  size_t n_buffers, size_t n_packets, uint32_t *d_est, size_t est_stride, uint32_t *d_status,
                                  void *stream);

/* Host only: the same values for host memory, from the same definition -- no device is touched. */
int gpuar_hip_survey_planes_host(const uint8_t *in, size_t n_bytes, uint32_t *est, size_t est_stride);

/* Host only, pure: the width to split by, from the four predicted totals (bytes at w = 1, 2, 4, 8) of a buffer of n_packets
 * packets: the SMALLEST w whose total is at most the lowest total + n_packets.  One byte per packet is the estimate's
 * resolution; on data of element width w every multiple of w ties within it, and the smallest is the cheapest to split. */
uint32_t gpuar_hip_choose_planes(const uint64_t total[4], uint64_t n_packets);

/* ------------------------------------------------------------------------
 * Delta survey: what a buffer would compress to WITH the delta filter at each byte-plane width, from one read of its bytes.
 * For a buffer of P packets and every j = 0 .. 3 (the widths w = 1, 2, 4, 8) whose bit is set in widths_mask,
 *     d_est[j * est_stride + p]  =  the gpuar_hip_estimate value of packet p of gpuar_hip_split_delta(buffer, w)
 * for every p < P, by definition (gpuar_amd/csrc/delta_survey.h); nothing is filtered or split into memory, nothing but d_est
 * is written, and the rows that were not asked for are left untouched.  The input is read once however many rows are asked for.
 *
 * Host-side checks as for gpuar_hip_survey_planes, in the same order; in addition widths_mask must be 1 .. 15
 * (GPUAR_ERR_ARGUMENT).  Nothing is read beyond the 16-byte-aligned piece of memory that holds a buffer's last byte.
 * ---------------------------------------------------------------------- */

/* The rows asked for, for the n_bytes at d_in. */
int gpuar_hip_survey_delta(const uint8_t *d_in, size_t n_bytes, uint32_t widths_mask, uint32_t *d_est, size_t est_stride, void *stream);

/* The same for a batch (descriptors as for gpuar_hip_encode_batch): column p of d_est is batch packet p.  Unusable buffers and
 * packets are GPUAR_STATUS_BAD_BATCH exactly as in gpuar_hip_survey_planes_batch: their columns are left untouched in every row. */
int gpuar_hip_survey_delta_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                                 size_t n_buffers, size_t n_packets, uint32_t widths_mask, uint32_t *d_est, size_t est_stride,
                                 uint32_t *d_status, void *stream);

/* Host only: the same values for host memory, from the same definition -- no device is touched. */
int gpuar_hip_survey_delta_host(const uint8_t *in, size_t n_bytes, uint32_t widths_mask, uint32_t *est, size_t est_stride);

/* Host only, pure: width and filter from the four totals of the plane survey (`plain`) and the four of the delta survey
 * (`filtered`) of a buffer of n_packets packets.  With wp = gpuar_hip_choose_planes(plain) and wd = gpuar_hip_choose_planes(filtered):
 * the filter at wd iff filtered[wd] + n_packets <= plain[wp] (it has to win by more than the estimate's resolution of one byte
 * per packet: a tie goes to no filter, and so does n_packets = 0), else no filter at wp.  Returns 1 (the filter) or 0 and writes the width to *width. */
int gpuar_hip_choose_filter(const uint64_t plain[4], const uint64_t filtered[4], uint64_t n_packets, uint32_t *width);

/* ------------------------------------------------------------------------
 * Sparse packets: a packet that is one byte value almost everywhere, kept as that byte and a list of exceptions instead of being
 * coded (gpuar_amd/csrc/sparse.h: one integer definition for the host and the kernels).  The codec cannot code
 * 8192 equal bytes below 210 bytes; their record here is 4.
 *     scan  A packet of n bytes (1 .. 8192) has a majority byte f iff 2 count(f) > n; then scan = (k << 8) | f with
 *           k = n - count(f), else scan = GPUAR_SPARSE_NONE.
 *     record, little-endian, at a 4-byte-aligned address:
 *           u8 fill | u8 0 | u16 k | u16 pos[k] | u8 val[k] | zero bytes up to a multiple of 4
 *           pos strictly ascending and < n, val[i] the byte at pos[i] and != fill; gpuar_hip_sparse_len(k) = (4 + 3 k + 3) & ~3
 *           bytes, the pad bytes included: a packet has exactly one record.
 *     A record of rec_bytes for a packet of n bytes is valid iff rec_bytes >= 4, byte 1 is 0, 2 k < n,
 *           gpuar_hip_sparse_len(k) <= rec_bytes, the positions are strictly ascending and < n and no val[i] equals the fill.
 *
 * Host-side checks as for gpuar_hip_estimate and gpuar_hip_move_packets, in the same order and before any device work.  Nothing is
 * read beyond the 16-byte-aligned piece of memory that holds a packet's last byte, nor beyond a record's rec_bytes.
 * In a .gip file a sparse packet is its record behind the packet's 4-byte header (below: raw and sparse packets in a stream).
 * ---------------------------------------------------------------------- */
#define GPUAR_SPARSE_NONE 0xFFFFFFFFu

/* Host only, pure: the bytes of a record with k exceptions. */
uint32_t gpuar_hip_sparse_len(uint32_t k);

/* Host only, pure: what to keep a packet of ulen bytes as, from its scan word and its estimate: 0 coded, 1 raw, 2 sparse.  With
 * s = gpuar_hip_sparse_len(scan >> 8) (infinite for GPUAR_SPARSE_NONE) and raw_ok = stored_on && est >= 4 + ulen:  2 iff
 * s + 1 < est && (!raw_ok || s < ulen), else 1 iff raw_ok, else 0.  The + 1 is the estimate's resolution; a tie with raw goes to raw. */
int gpuar_hip_sparse_rule(uint32_t scan, uint32_t est, uint32_t ulen, int stored_on);

/* d_scan[p] for the gpuar_hip_packet_count(n_bytes) packets of the n_bytes at d_in: arguments and checks of gpuar_hip_estimate. */
int gpuar_hip_sparse_scan(const uint8_t *d_in, size_t n_bytes, uint32_t *d_scan, void *stream);

/* The same for a batch: arguments and checks of gpuar_hip_estimate_batch.  A packet whose descriptor is unusable is
 * GPUAR_STATUS_BAD_BATCH in d_status and its d_scan[p] is left untouched. */
int gpuar_hip_sparse_scan_batch(const uint8_t *const *d_in_ptrs, const uint64_t *d_in_bytes, const uint64_t *d_first_packet,
                                size_t n_buffers, size_t n_packets, uint32_t *d_scan, uint32_t *d_status, void *stream);

/* Host only: the same values for host memory, from the same definition -- no device is touched. */
int gpuar_hip_sparse_scan_host(const uint8_t *in, size_t n_bytes, uint32_t *scan);

/* Writes the records of n_regions packets: region r is the d_bytes[r] (1 .. 8192) bytes at d_src_ptrs[r] (16-byte aligned) with
 * the scan word d_scan[r]; its record, exactly gpuar_hip_sparse_len(d_scan[r] >> 8) bytes, goes to d_dst_ptrs[r] (4-byte
 * aligned) and nothing is written behind it.  The pointer and size arrays are in device memory and 8-byte aligned, d_scan
 * 4-byte.  A region whose scan word is GPUAR_SPARSE_NONE or is not that of its bytes (another count of exceptions, or a fill
 * that is no majority), with a misaligned pointer, or of 0 or more than 8192 bytes is GPUAR_STATUS_BAD_BATCH in d_status and
 * nothing is written for it. */
int gpuar_hip_sparse_pack(const uint8_t *const *d_src_ptrs, const uint64_t *d_bytes, const uint32_t *d_scan, uint8_t *const *d_dst_ptrs,
                          size_t n_regions, uint32_t *d_status, void *stream);

/* Rebuilds n_regions packets from their records: region r is the record of d_rec_bytes[r] bytes at d_rec_ptrs[r] (4-byte
 * aligned); its packet of d_bytes[r] (1 .. 8192) bytes goes to d_dst_ptrs[r] (16-byte aligned).  The four arrays are in device
 * memory and 8-byte aligned.  A record that is not valid is GPUAR_STATUS_BAD_PACKET in d_status: what the packet's own
 * d_bytes[r] bytes then hold is unspecified, nothing outside them is written and nothing is read beyond the record.  A
 * misaligned pointer or a packet of 0 or more than 8192 bytes is GPUAR_STATUS_BAD_BATCH and the region is skipped. */
int gpuar_hip_sparse_unpack(const uint8_t *const *d_rec_ptrs, const uint64_t *d_rec_bytes, uint8_t *const *d_dst_ptrs,
                            const uint64_t *d_bytes, size_t n_regions, uint32_t *d_status, void *stream);

/* Host only: the record of the packet in[0 .. n_bytes) (1 .. 8192 bytes) into rec[0 .. rec_room), its length into *rec_len.
 * GPUAR_ERR_ARGUMENT (nothing written) for a null pointer, another n_bytes, a packet without a majority byte, or a record
 * longer than rec_room. */
int gpuar_hip_sparse_pack_host(const uint8_t *in, size_t n_bytes, uint8_t *rec, size_t rec_room, size_t *rec_len);

/* Host only: the packet out[0 .. n_bytes) from the record rec[0 .. rec_bytes).  GPUAR_ERR_ARGUMENT for a null pointer, another
 * n_bytes, or a record that is not valid (out[0 .. n_bytes) is then unspecified; nothing is read beyond rec_bytes). */
int gpuar_hip_sparse_unpack_host(const uint8_t *rec, size_t rec_bytes, uint8_t *out, size_t n_bytes);

/* ------------------------------------------------------------------------
 * Raw and sparse packets in a packet stream (gpuar_amd/csrc/kinds.h: one integer definition for the host and the kernels;
 * DESIGN.md 4.13).  In a stream -- the slots gpuar_hip_encode fills, what gpuar_hip_compact makes of them, a .gip file -- a packet
 * of any kind starts with the 4-byte header of a coded one, u16 clen (these 4 bytes included) | u16 ulen:
 *     kind 0 coded    the bitstream                                 clen as ever
 *     kind 1 raw      the packet's ulen bytes                       clen = 4 + ulen  (<= 8196)
 *     kind 2 sparse   the record above, pads included               clen = 4 + gpuar_hip_sparse_len(k)
 * so `off += clen` walks the stream, every packet fits its 8704-byte slot and gpuar_hip_compact works unchanged.  The kind is
 * gpuar_hip_sparse_rule(scan, est, ulen, stored_on), scan = GPUAR_SPARSE_NONE where sparse is off: what batch.compress applies
 * (not re-tuned for the 4 header bytes: at the tie a sparse packet may be up to 3 bytes longer than its coded form).  Which
 * packet is which is kept beside the stream, one byte per packet (the version-6 trailer of a .gip file).
 * Left out: counting kinds in the surveys, one read for scan and estimate, skipping the encode of non-coded packets.
 * ---------------------------------------------------------------------- */

/* Behind gpuar_hip_encode* on the same stream, over the gpuar_hip_packet_count(n_bytes) packets of the n_bytes at d_in (the bytes
 * that were coded; 16-byte aligned) and their slots at d_slots (16-byte aligned): writes d_kind[p] (one byte per packet) from
 * d_est[p] (gpuar_hip_estimate) and d_scan[p] (gpuar_hip_sparse_scan; NULL: sparse is off) and overwrites the slot of a raw
 * packet with header + bytes and of a sparse packet with header + record.  A coded packet's slot is not touched, and nothing
 * is written beyond slot + clen.  A scan word that is not that of the packet's bytes (another count of exceptions, a fill that
 * is no majority) is GPUAR_STATUS_BAD_BATCH in d_status: the slot stays the encoder's and d_kind[p] = 0, so the stream is
 * still a valid one.  Host-side checks as for gpuar_hip_estimate, then d_slots and d_kind (NULL: GPUAR_ERR_ARGUMENT) and the
 * alignment of d_slots (16) and d_scan (4).  Nothing is read beyond the 16-byte piece that holds the buffer's last byte. */
int gpuar_hip_kinds_store(const uint8_t *d_in, size_t n_bytes, const uint32_t *d_est, const uint32_t *d_scan, int stored_on,
                          uint8_t *d_slots, uint8_t *d_kind, uint32_t *d_status, void *stream);

/* Takes the raw and sparse packets out of a compacted stream: packet p of kind d_kind[p] = 1 or 2 at d_stream + d_offsets[p]
 * (any alignment; d_offsets: n_packets + 1 values, 8-byte aligned) goes to d_out + p * 8192 (d_out 16-byte aligned), n_bytes
 * being the bytes of the whole output: gpuar_hip_packet_count(n_bytes) == n_packets, or GPUAR_ERR_ARGUMENT.  Packets of kind 0
 * are the decoder's and are skipped.  The header is checked first: clen == d_offsets[p + 1] - d_offsets[p], ulen == the bytes
 * packet p has in n_bytes, raw: clen == 4 + ulen, sparse: a valid record.  A packet that fails, or a kind above 2, is
 * GPUAR_STATUS_BAD_PACKET in d_status: a raw packet's destination is left as it was, a sparse packet's own bytes are
 * unspecified; nothing outside the packet's bytes is written, and nothing before d_offsets[p] or from d_offsets[p + 1] on is
 * read. */
int gpuar_hip_kinds_expand(const uint8_t *d_stream, const uint64_t *d_offsets, const uint8_t *d_kind, size_t n_packets, uint8_t *d_out,
                           size_t n_bytes, uint32_t *d_status, void *stream);

/* Host only: ONE packet in[0 .. n_bytes) (1 .. 8192 bytes) in its stream form.  *kind is what the rule gives with the two
 * options; for a raw or sparse packet pkt[0 .. *clen) is written; for a coded one nothing is written and *clen = 0 (the
 * encoder's packet stands).  GPUAR_ERR_ARGUMENT (nothing written) for a null pointer, another n_bytes, or a packet longer
 * than room. */
int gpuar_hip_kinds_store_host(const uint8_t *in, size_t n_bytes, int stored_on, int sparse_on, uint8_t *pkt, size_t room, uint32_t *kind,
                               size_t *clen);

/* Host only: the packet out[0 .. n_bytes) from the raw (kind 1) or sparse (kind 2) packet pkt[0 .. pkt_bytes).
 * GPUAR_ERR_ARGUMENT for a null pointer, another n_bytes, any other kind, or a packet that is not valid (a raw packet's out is
 * then untouched, a sparse packet's out[0 .. n_bytes) unspecified; nothing is read beyond pkt_bytes). */
int gpuar_hip_kinds_expand_host(const uint8_t *pkt, size_t pkt_bytes, uint32_t kind, uint8_t *out, size_t n_bytes);

/* ------------------------------------------------------------------------
 * Host only: a whole .gip file in memory, read by the CLI's own reader (FileHeader::getInfo, Trailer::load of
 * gpuar_amd/csrc/host) and checked packet by packet -- what batch.read_gip and batch.from_gip stand on (the
 * device call that goes with them is in gpuar_hip_gip.h).  No device is touched.
 *
 * info[] (GPUAR_GIP_INFO_WORDS values) is filled as far as the reader got:
 *     [0] uncompressed bytes (a reference-written header's garbage upper bytes dropped, as getInfo drops them)
 *     [1] where the packet stream begins in the file (20)   [2] where it ends
 *     [3] the usable trailer's version, 0 where there is none (an unusable version 1, a malformed version 2 and unknown
 *         versions included, as in the CLI); with GPUAR_GIP_TRAILER the version the unusable trailer claims (3 .. 6)
 *     [4] packets   [5] elem_bytes (1 without a trailer that says)   [6] the trailer's flags (bit 0: CRCs, bit 1: delta, bit 2:
 *         base, bit 3: kinds; version 2: 1)   [7] Trailer::Status as a number (0 none, 1 ok, 2 malformed, 3 .. 6 unusable)
 *     [8] the packet and [9] the file offset a defect was found at (0 where it has none)
 * The lengths come from the trailer, and without a usable one from walking the headers; EVERY packet's header is then checked
 * against them.  Returns GPUAR_OK, GPUAR_ERR_ARGUMENT (a null pointer) or the first defect met, in this order:
 * ---------------------------------------------------------------------- */
#define GPUAR_GIP_INFO_WORDS 10
#define GPUAR_GIP_SHORT    1   /* fewer than 20 bytes                                                                    */
#define GPUAR_GIP_VERSION  2   /* bytes 0 .. 2 are not 0.1.0                                                              */
#define GPUAR_GIP_SIZE     3   /* the header's compressed size is below 20 or beyond the file                             */
#define GPUAR_GIP_TRAILER  4   /* a trailer that says version 3 .. 6 and cannot be used: not a file to read without it    */
#define GPUAR_GIP_COUNT    5   /* the packets are not the ceil(uncompressed / 8192) the header's size needs               */
#define GPUAR_GIP_CUT      6   /* the stream ends inside packet [8] (its header included)                                 */
#define GPUAR_GIP_CLEN     7   /* packet [8]: clen below 4 or above 8704                                                  */
#define GPUAR_GIP_TABLE    8   /* packet [8]: the header's clen is not the trailer's                                      */
#define GPUAR_GIP_ULEN     9   /* packet [8]: ulen is not the bytes it has in the file (8192; the last one the rest)      */
#define GPUAR_GIP_KIND    10   /* packet [8]: a kind above 2                                                              */
#define GPUAR_GIP_RAW     11   /* packet [8]: raw and clen != 4 + ulen                                                    */
#define GPUAR_GIP_SPARSE  12   /* packet [8]: sparse and the record's head fails sparse_head_ok, or clen != 4 + sparse_len(k) */
#define GPUAR_GIP_SUM     13   /* the lengths do not sum to the stream                                                    */
int gpuar_hip_gip_read_host(const uint8_t *file, size_t file_bytes, uint64_t info[GPUAR_GIP_INFO_WORDS]);

/* The per-packet tables of the same file: clen[n_packets], and where the pointer is not null crc[n_packets] (the trailer's
 * CRC-32s; GPUAR_ERR_ARGUMENT where it has none) and kind[n_packets] (version 6: the trailer's; else zeros).  n_packets must be
 * info[4].  The same checks are made again and the same code returned; the arrays are written only with GPUAR_OK.  What is NOT
 * checked here: the exceptions of a sparse record (gpuar_hip_sparse_unpack: GPUAR_STATUS_BAD_PACKET) and the inside of a coded
 * packet (the decoder and the CRCs). */
int gpuar_hip_gip_tables_host(const uint8_t *file, size_t file_bytes, uint16_t *clen, uint32_t *crc, uint8_t *kind, size_t n_packets);

/* Reads and clears the FALLBACK status word of the current device: what
 * launches without a `d_status` of their own reported (the reference-named
 * executors above).  Synchronises the whole device -- meant for that
 * single-stream legacy use, not for pipelines (pass `d_status` there).
 * The read and the clear are one atomic exchange on the device, so every bit
 * a launch ORs into the word is reported by exactly one gpuar_hip_status call,
 * even while other host threads launch into it: a bit that arrives during a
 * call is either in that call's *flags or left for the next call. */
int gpuar_hip_status(uint32_t *flags);

/* Last error recorded by a void-returning reference-named entry point on this
 * host thread (0 = none); cleared by the call. */
int gpuar_hip_last_error(void);

const char *gpuar_hip_error_string(int code);

/* Build identification: "gpuar-hip 0.2 gfx950". */
const char *gpuar_hip_version(void);

/* The number of this header's ABI, GPUAR_HIP_ABI_VERSION at the time the library was built.  It changes whenever
 * the signature of an existing entry point does (2: encode / decode / decode_stream take `d_status` in front of
 * `stream`), so a caller built against another header can refuse to go on instead of passing a stream handle
 * where a status word is expected:  if (gpuar_hip_abi_version() != GPUAR_HIP_ABI_VERSION) ...  */
#define GPUAR_HIP_ABI_VERSION 2
int gpuar_hip_abi_version(void);

/* Synthetic streams of SURVEY.md section 8(d), generated on the device so
 * multi-GiB benchmark inputs never cross PCIe.  kind: 0 uniform, 1 zipf,
 * 2 text.  Fills d_out[0..n) with bytes [offset, offset+n) of the stream.
 * d_out must be 8-byte aligned (the kernels store 8 bytes at a time; every allocator's first byte is): GPUAR_ERR_ALIGNMENT
 * otherwise, before any device work.  `offset` must be a multiple of 8 and `kind` 0 .. 2: GPUAR_ERR_ARGUMENT.  n == 0 is
 * GPUAR_OK with no launch. */
int gpuar_hip_generate(int kind, uint64_t seed, uint64_t offset, size_t n, uint8_t *d_out, void *stream);

/* Measurement support: a plain device-to-device copy of n_bytes (a multiple of 16; both pointers 16-byte aligned),
 * 16 bytes per lane -- the practical HBM roof bench.py measures on the box and quotes next to the datasheet's
 * 8 TB/s.  Moves 2 * n_bytes through HBM.  n_bytes < 64 GiB: GPUAR_ERR_ARGUMENT above. */
int gpuar_hip_copy(const uint8_t *d_src, uint8_t *d_dst, size_t n_bytes, void *stream);

/* Measurement support: the shader clock while the throughput kernels ran.  Every 64th workgroup of encode_kernel
 * (which = 0) and of the two decode kernels (which = 1) notes, in a slot of its own on the current device, the
 * shader clock's counter and the constant 100 MHz clock's counter at its start and at its end.
 * Copies the GPUAR_CLOCK_SLOTS records {shader at start, 100 MHz at start, shader at end, 100 MHz at end} into
 * ticks[4 * GPUAR_CLOCK_SLOTS] (slots no sampled workgroup has written since the last reset are 0) and, if `reset`,
 * zeroes them.  Synchronises the device.  sum(shader end - start) / sum(100 MHz end - start) x 100 MHz = the clock
 * the vector pipes ran at -- under this load not the data sheet's 2.4 GHz, which is why bench.py quotes its
 * vector-issue roof against both. */
#define GPUAR_CLOCK_SLOTS 256
int gpuar_hip_clock_samples(int which, uint64_t *ticks, int reset);

#ifdef __cplusplus
}
#endif
#endif /* GPUAR_HIP_H */
