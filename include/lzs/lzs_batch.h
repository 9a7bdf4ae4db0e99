/*
 * lzs/lzs_batch.h -- additive entry points of the MI355X build of liblzs: many
 * independent blocks per call, host or device buffers.
 *
 * The reference has no batch interface: its unit of work is one call of
 * lzs_compress()/lzs_decompress() (c/src/liblzs/lzs.h:218,229) per buffer, and the
 * way to process many buffers is a loop of such calls (c/src/test/test-lzs.c:111-114,
 * c/src/utils/lzs-compress.c:207).  Every function below is defined as exactly that
 * loop -- block b of a batch produces the bytes and the length that one reference call
 * on block b alone would -- executed by one GPU workgroup (compression) or wavefront
 * (decompression) per block.
 *
 * All functions return LZS_OK (0) or a negative LZS_E_* code; lzs_last_error() gives
 * the message of the calling thread's most recent failure.  Plain C types only.
 */
#ifndef LZS_MI355X_LZS_BATCH_H
#define LZS_MI355X_LZS_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZS_OK            0
#define LZS_E_NO_DEVICE  (-1)   /* no usable HIP device / runtime                      */
#define LZS_E_HIP        (-2)   /* a HIP call failed (message in lzs_last_error())     */
#define LZS_E_ARG        (-3)   /* invalid argument                                    */
#define LZS_E_NOMEM      (-4)   /* device or host allocation failed                    */

/* Largest single block (bytes) one launch addresses: the limit of the batch and device-pointer calls
 * below.  The plain lzs_compress() / lzs_decompress() take any size_t (longer buffers go in pieces). */
#define LZS_BLOCK_MAX    (3u << 30)

/* Message for the calling thread's most recent failure ("" if none). Never NULL. */
const char *lzs_last_error(void);

/*
 * What the library keeps between calls, and how to get it back.  The reference keeps nothing after return (lzs.h:218,229:
 * the caller's two buffers and some stack).  This build's host-buffer and one-shot calls stage through device memory, a
 * stream and pinned pieces that belong to the CALLING THREAD and stay for its next call (a hipMalloc of gigabytes can
 * take a second): at most LZS_KEEP_MAX_MB MiB of device memory in sum per thread (environment, read once per process;
 * default: 1/32 of the device's memory, at least 640 MiB -- what is above it is freed before the call returns), released
 * when the thread exits -- or now, by this call, from the thread that owns it.  The device-pointer calls
 * (lzs_*_batch_device, lzs_compact_device) allocate nothing and keep nothing.
 */
void lzs_release_thread_cache(void);

/* Human-readable description of the backend ("hip gfx950 ... 256 CUs ...") into buf.
 * Returns LZS_OK, or LZS_E_NO_DEVICE when there is no device (buf then holds the reason). */
int lzs_backend_info(char *buf, size_t cap);

/*
 * Device-pointer batch compression, asynchronous on `hip_stream`.
 *
 *   block b input  : d_in  + b * in_stride ,  length d_in_len ? d_in_len[b] : in_len
 *   block b output : d_out + b * out_stride,  capacity out_cap (same rule as
 *                    a_outBufferSize of lzs_compress(): the stream is cut there)
 *   d_out_len[b]   : bytes written for block b
 *
 * Each block is an independent LZS stream with its own end marker, i.e. the result of
 * lzs_compress(d_out + b*out_stride, out_cap, d_in + b*in_stride, len_b)
 * (reference lzs-compression.c:249-467).  All pointers are device pointers;
 * d_in_len may be NULL; it must not be the array d_out_len (LZS_E_ARG: d_out_len[] is
 * scratch of the launch until a block's length lands there).  `hip_stream` is a hipStream_t passed as void* (NULL = the
 * default stream).  Fastest when d_in, in_stride are multiples of 16 and d_out,
 * out_stride multiples of 4; any alignment is accepted.  No allocation, no
 * synchronisation: safe to capture into a hipGraph.  (Once per device and process the
 * library asks the device how it orders same-address LDS exchanges -- a 0.1 ms kernel on a
 * stream of its own, at the first entry into the library on that device; `hip_stream` is not
 * touched by it.  Call lzs_backend_info() first if the very first call is to be captured.)
 */
int lzs_compress_batch_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                              const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                              size_t in_len, size_t nblocks, void *hip_stream);

/*
 * Device-pointer batch decompression, asynchronous on `hip_stream`; block b is
 * lzs_decompress(d_out + b*out_stride, out_cap, d_in + b*in_stride, len_b)
 * (reference lzs-decompression.c:156-412).  Arguments as above.
 */
int lzs_decompress_batch_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                                size_t in_len, size_t nblocks, void *hip_stream);

/*
 * The same for a batch too small to fill the device with one wavefront per block (a wavefront
 * needs 8-9 ms for a 64 KiB block whatever the batch): every block is cut into segments for many
 * wavefronts (4 blocks 0.7 ms, 64 blocks 1.5 ms).  Buffers in device memory, but
 * the lengths in HOST memory (in_len_each may be NULL: every block in_len bytes; out_len receives
 * the results), and the call is synchronous: it runs on the calling thread's own stream, takes
 * scratch memory from the thread's staging and returns when d_out is complete.  Batches beyond
 * 64 MiB of output (or with blocks under 1 KiB on average) are handed to the one-wavefront-per-
 * block kernel.
 */
int lzs_decompress_batch_device_sync(void *d_out, size_t out_stride, size_t out_cap, uint32_t *out_len,
                                     const void *d_in, size_t in_stride, const uint32_t *in_len_each,
                                     size_t in_len, size_t nblocks);

/*
 * The compressing twin: lzs_compress_batch_device() for a batch of FEW LONG blocks, which does not fill the device with one
 * workgroup per block (a workgroup alone takes 15 ms for 1 MiB of text, whatever the batch).  Every block is cut into segments,
 * one workgroup each, as lzs_compress_stream_device() cuts one stream, with the entry rounds and the stitch over all blocks at
 * once (profiles/r24/batch_compress.txt has the rows).  Buffers in device memory, the lengths in HOST memory
 * (in_len_each may be NULL: every block in_len bytes; out_len receives the results).
 *   out_len[b], bytes [0, out_len[b]) of slot b : byte for byte what lzs_compress_batch_device() gives at the same out_cap
 *   the rest of slot b                          : unspecified, as that call leaves it; nothing outside slot b's out_stride bytes
 *                                                 is stored to on b's behalf
 * The segments are taken when out_cap <= out_stride and d_out, out_stride are multiples of 4, and the batch is of the shape for
 * which they are faster; every other batch is one launch of the workgroup-per-block kernel, with the same results.
 * Synchronous, on the calling thread's own stream: it returns when d_out is complete, and it is NOT capturable into a hipGraph
 * (the entry rounds are decided on the host).  Scratch from the calling thread's staging, as the one-stream call takes it:
 * LZS_COMPRESSED_MAX(segment) a segment, about 1.14 times the input, for at most LZS_BLOCK_MAX bytes of input at a time (longer
 * batches go group by group), and 37 bytes a segment of tables.  LZS_E_ARG as lzs_compress_batch_device(), and for a block above
 * LZS_BLOCK_MAX; nblocks == 0 is LZS_OK and touches nothing.
 */
int lzs_compress_batch_device_sync(void *d_out, size_t out_stride, size_t out_cap, uint32_t *out_len,
                                   const void *d_in, size_t in_stride, const uint32_t *in_len_each,
                                   size_t in_len, size_t nblocks);

/*
 * How long every block of a batch decodes to, and how its decoding ends, WITHOUT decoding it: what a caller needs to choose
 * out_cap or to allocate the output before any of the decode calls (LZS_DECOMPRESSED_MAX() is no bound: see lzs.h).
 *
 *   block b    : d_in + b * in_stride, length d_in_len ? d_in_len[b] : in_len, as above
 *   d_size[b]  : exactly what lzs_decompress_batch_device() writes to d_out_len[b] when called with out_cap = limit -- and what
 *                lzs_decompress_channels_device() (lzs_channels.h) writes for the same bytes on any valid channel, whatever
 *                its history: a stream's length depends on its tokens and the capacity, never on the bytes it copies
 *   d_status[b]: (d_status may be NULL) the LZS_D_STATUS_* byte lzs_decompress_channels_device() writes with out_cap = limit:
 *                END_MARKER if an end marker was reached -- it needs no room, and it does not count after a copy that `limit`
 *                cut short, also not behind that copy's closing length nibble 0 --, otherwise NO_OUTPUT_BUFFER_SPACE if
 *                d_size[b] >= limit, otherwise INPUT_STARVED | INPUT_FINISHED.  Never ERROR: the call sees no channel slot.
 *
 * A long offset of 0 has no length field and copies nothing, bytes after the end marker are ignored: the decoders' rules.
 * limit <= 0xFFFFFFFF (LZS_E_ARG above it).  limit = 0xFFFFFFFF asks for the true size; a block that decodes to more reports
 * limit and NO_OUTPUT_BUFFER_SPACE.  limit = 0 is out_cap = 0: size 0, END_MARKER for a stream that begins with its marker.
 * d_size and d_in (with nblocks > 0) are required, d_size must not be the array d_in_len, in_len and nblocks are bounded as
 * for lzs_decompress_batch_device(); nblocks == 0 is LZS_OK and touches nothing.
 *
 * A token walk, one GPU lane a block: no output traffic, no window, no allocation, no synchronisation -- asynchronous on
 * `hip_stream` and safe to capture into a hipGraph (the note on the very first call into the library applies).  Any
 * alignment of d_in and in_stride; nothing is read outside the aligned 32-bit words that hold a block's own bytes, and a
 * block's result depends on nothing outside [block start, block start + length).
 *
 * The call is sized for MANY blocks.  On an MI355X 65 536 packets of 1500 bytes of text take 0.51 ms (decoding them into
 * scratch memory: 0.80 ms) and 16 384 blocks of 64 KiB of text 18.6 ms (decoding: 7.5 ms); DESIGN.md 3.13 has every
 * row.  One block is one lane's serial walk however large it is, so a few huge blocks get no help from it: a single block of
 * 1 MiB of text takes 157 ms.  Long streams and batches of long blocks are what lzs_decompressed_size_stream_device(),
 * lzs_decompressed_size_stream() and lzs_decompressed_size_batch_device_sync() below are for: the same answers from a
 * segmented walk over the whole device.
 */
int lzs_decompressed_size_batch_device(uint32_t *d_size, uint8_t *d_status,
                                       const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                       size_t limit, size_t nblocks, void *hip_stream);

/*
 * The same question for ONE LONG stream, answered by the whole device: the stream is cut into segments as
 * lzs_decompress_stream_device() cuts it, every segment is walked without copying a byte and reports how many bytes it
 * produces, the host sums, and one short walk finds the status where the room runs out or the stream ends.
 * What the decode calls make their callers guess -- out_cap -- is one call away.
 *
 *   flags == 0, the plain rule:
 *     *size   : what lzs_decompress(out, limit, in, in_len) returns
 *     *status : (status may be NULL) the LZS_D_STATUS_* byte lzs_decompressed_size_batch_device() writes for the same bytes
 *               and the same limit, by the rules stated there -- END_MARKER 0x04, NO_OUTPUT_BUFFER_SPACE 0x08, or
 *               INPUT_STARVED | INPUT_FINISHED 0x03 -- in every corner: an empty stream is 0x03, or 0x08 with limit == 0
 *   flags == LZS_SIZE_CONCAT, the file rule of lzs_decompress_concat(): the walk goes on behind every end marker
 *     *size   : what lzs_decompress_concat(out, limit, in, in_len) returns
 *     *status : NO_OUTPUT_BUFFER_SPACE if *size == limit, otherwise INPUT_STARVED | INPUT_FINISHED; never END_MARKER -- a
 *               marker ends nothing here
 *
 * limit is any uint64_t; UINT64_MAX asks for the true size.  LZS_E_ARG, with the call's name in lzs_last_error() and before
 * the device is asked: size NULL, an unknown bit in flags, in_len > LZS_BLOCK_MAX, NULL input with in_len > 0.  in_len == 0 is
 * LZS_OK without a device; a valid call without one is LZS_E_NO_DEVICE.
 *
 * *size and *status are in HOST memory.  Synchronous, on the calling thread's own stream with scratch from the thread's
 * staging, like lzs_decompress_stream_device(): not capturable, no output allocated, d_in must be complete when the call is
 * made.  Any alignment of d_in; nothing is read outside the aligned 32-bit words that hold the stream's own bytes.
 * lzs_decompressed_size_stream() is the same from a host buffer, staged through the calling thread's device memory.
 */
#define LZS_SIZE_CONCAT 1u    /* the file rule of lzs_decompress_concat(): go on behind every end marker */
int lzs_decompressed_size_stream_device(uint64_t *size, uint8_t *status, const void *d_in, size_t in_len,
                                        uint64_t limit, unsigned flags);
int lzs_decompressed_size_stream(uint64_t *size, uint8_t *status, const uint8_t *in, size_t in_len,
                                 uint64_t limit, unsigned flags);

/*
 * The size-query twin of lzs_decompress_batch_device_sync(): a batch of blocks in device memory, the lengths (in_len_each may
 * be NULL: every block in_len bytes) and the results in HOST memory.  size[b] and status[b] (status may be NULL) are exactly
 * what lzs_decompressed_size_batch_device() gives block b at the same limit (the plain rule; limit <= 0xFFFFFFFF).  Batches
 * of long blocks -- 10 167 bytes and more on average (the crossover measured on an MI355X), in an extent that
 * 32-bit positions reach -- go by segments like one long
 * stream, all blocks at once; the others by one lane a block.  Synchronous, on the calling thread's own stream and staging.
 * LZS_E_ARG: size NULL, in_len or a block's length > LZS_BLOCK_MAX, nblocks > 0x7FFFFFFF, limit > 0xFFFFFFFF, NULL input
 * with a length above 0.  nblocks == 0 is LZS_OK and touches nothing.
 */
int lzs_decompressed_size_batch_device_sync(uint32_t *size, uint8_t *status, const void *d_in, size_t in_stride,
                                            const uint32_t *in_len_each, size_t in_len, size_t limit, size_t nblocks);

/*
 * ONE stream from device memory, on the whole device: the result of
 * lzs_compress(d_out, out_cap, d_in, in_len) (reference lzs-compression.c:249-467) for buffers
 * already in HBM.  The stream is cut into segments (0.5 KiB .. 64 KiB), one workgroup each; where each
 * segment's first token starts is agreed in a few rounds and the segments' bits are shifted to
 * their global offsets, so the bytes are those of the one-shot call.
 * The 4-argument lzs_compress() takes the same route for inputs of 6 KiB and more.
 *
 * d_out must be 4-byte aligned and hold LZS_COMPRESSED_MAX(in_len) + 1024 bytes; ALL of that is
 * overwritten (cleared first).  The result is cut at out_cap as lzs_compress() does.  The call
 * synchronises with the device several times (not capturable into a graph) and runs on this thread's
 * own staging stream: d_in must be complete when the call is made (work queued on other streams is
 * not waited for).  Returns the byte count in *out_len.
 */
int lzs_compress_stream_device(void *d_out, size_t out_cap, size_t *out_len,
                               const void *d_in, size_t in_len);

/*
 * The reverse: ONE stream in device memory decompressed by many wavefronts -- the result of
 * lzs_decompress(d_out, out_cap, d_in, in_len) (reference lzs-decompression.c:156-412: stops at
 * the first end marker, at out_cap, or when the bits run out).  The stream is cut into segments
 * (256 bytes .. 8 KiB) that agree on the decoder state at their borders in a few rounds, decode with per-byte
 * origins for copies reaching into another segment's output, and resolve those by pointer jumping
 * (DESIGN.md 3.6).  The 4-argument lzs_decompress() takes the same route from 4 KiB of input on.  Output
 * below 4 GiB; allocates 4 * produced bytes of scratch on this thread's staging; synchronous, on
 * this thread's own stream (d_in must be complete when the call is made).
 */
int lzs_decompress_stream_device(void *d_out, size_t out_cap, size_t *out_len,
                                 const void *d_in, size_t in_len);

/*
 * Gather the variable-length results of a batch into one dense byte string:
 * d_offsets[b] = sum of d_len[0..b) for b = 0..nblocks (nblocks+1 entries, uint64),
 * d_dense[d_offsets[b] .. d_offsets[b+1]) = slot b's first d_len[b] bytes.
 * d_dense must hold sum(d_len) bytes (at most nblocks*max len).  Concatenated
 * independent streams are what the reference's file decompressor consumes
 * (c/src/liblzs/lzs-decompression.c:564-576 realigns after each end marker).
 * Asynchronous on `hip_stream`, no allocation.
 */
int lzs_compact_device(void *d_dense, uint64_t *d_offsets, const void *d_slots, size_t slot_stride,
                       const uint32_t *d_len, size_t nblocks, void *hip_stream);

/*
 * PACKED streams and packed outputs: blocks addressed by OFFSETS instead of a stride -- what lzs_compact_device() produces, how
 * a shard arrives over RCCL, how a file of concatenated streams with a length table or a drained packet queue lies in memory.
 * ("Ragged" in this library means per-block lengths in a strided array; this is the other thing.)  The calls below,
 * lzs_decompress_channels_packed_device() and lzs_compress_channels_packed_device() (lzs_channels.h) share their addressing:
 *
 *   input   block b starts at d_in + d_in_off[b].  With d_in_len NULL its length is d_in_off[b + 1] - d_in_off[b]: nblocks + 1
 *           entries are read and must not decrease.  With d_in_len given its length is d_in_len[b]: only nblocks entries of
 *           d_in_off are read, in any order.  Any alignment; nothing is read outside the aligned 32-bit words that hold the
 *           block's own bytes -- by the size query and by the decoders.
 *   output  block b is written at d_out + d_out_off[b]; its room -- its out_cap -- is d_out_off[b + 1] - d_out_off[b], clamped
 *           to 0xFFFFFFFF.  nblocks + 1 entries are always read.  Any alignment.
 *   result  bytes [0, d_out_len[b]) of the block's room, d_out_len[b], d_status[b] (and the channel's slot) are byte for byte
 *           what the strided call gives for that stream alone with out_cap = its room: lzs_decompressed_size_batch_device()
 *           with the same limit, lzs_decompress_batch_device(), lzs_decompress_channels_device().
 *   containment  block b stores to d_out[d_out_off[b] .. d_out_off[b] + d_out_len[b]) and to NO other byte of d_out: not to
 *           the rest of its room, not to its neighbours' first and last bytes, which lie right beside its own here.
 *   not a block  an entry whose input or output offsets decrease, or whose length exceeds LZS_BLOCK_MAX: d_out_len[b] = 0
 *           (d_size[b] = 0), status ERROR (0x10) where there is a status array, nothing of it is read or written, its channel's
 *           slot is untouched, and the other blocks are unaffected.
 *
 * All of them are asynchronous on `hip_stream`, allocate nothing, do not synchronise and may be captured into a hipGraph (the
 * note on the very first call into the library applies).  Checked before the device is asked (LZS_E_ARG, the call's name in
 * lzs_last_error()): a required pointer that is NULL, an offset array that is not 8-byte aligned, d_out_len / d_size being the
 * array d_in_len, nblocks > 0x7FFFFFFF, limit > 0xFFFFFFFF, a bad align.  Offsets are uint64_t; a torch int64 tensor holds the
 * same bits.  Not offered: host-buffer entries.  Many packets
 * per channel in one packed call: lzs_*_channels_burst_packed_device (lzs_channels.h).
 *
 * lzs_offsets_from_sizes_device: d_offsets[0] = 0, d_offsets[b + 1] = d_offsets[b] + round_up(d_size[b], align); nblocks + 1
 * entries, the total in d_offsets[nblocks]; nblocks == 0 writes d_offsets[0] = 0.  `align`: a power of two from 1 to 256 -- 16
 * gives every block a 16-byte-aligned start.  The scan of lzs_compact_device() with padding.
 */
int lzs_offsets_from_sizes_device(uint64_t *d_offsets, const uint32_t *d_size, size_t align, size_t nblocks, void *hip_stream);

/* lzs_decompressed_size_batch_device() for packed streams: `limit` as there, d_status may be NULL (ERROR only for an entry
 * that is not a block); nblocks == 0 is LZS_OK and touches nothing. */
int lzs_decompressed_size_packed_device(uint32_t *d_size, uint8_t *d_status, const void *d_in, const uint64_t *d_in_off,
                                        const uint32_t *d_in_len, size_t limit, size_t nblocks, void *hip_stream);

/* lzs_decompress_batch_device() from packed streams to packed outputs.  Sizes from the call above, offsets from
 * lzs_offsets_from_sizes_device(), one allocation of d_offsets[nblocks] bytes, this call: the decoded batch costs its own
 * bytes of device memory and no slots (INTEGRATION.md has the lines).  Eight streams share a wavefront; where their input lies
 * more than 4 GiB apart they are decoded one after the other, which is slow and right. */
int lzs_decompress_batch_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                       const uint64_t *d_in_off, const uint32_t *d_in_len, size_t nblocks, void *hip_stream);

/*
 * PACKED COMPRESSION: lzs_compress_batch_device() from packed blocks to packed rooms, with the addressing, the
 * rule for entries that are not blocks and the argument checks of "PACKED streams" above; nblocks == 0 is LZS_OK and touches nothing.
 * A drained packet queue, a shard with its offset table or the output of lzs_decompress_batch_packed_device() is compressed where it
 * lies, into rooms sized on the device: no input slots, no nblocks x LZS_COMPRESSED_MAX(largest) of output slots.
 *
 * lzs_compressed_bound_packed_device: d_bound[b] = LZS_COMPRESSED_MAX(length of block b) -- it fits 32 bits for every length up to
 * LZS_BLOCK_MAX --, 0 for an entry that is not a block (input offsets that decrease where d_in_len is NULL, a length above
 * LZS_BLOCK_MAX).  lzs_offsets_from_sizes_device() makes the rooms of it.  d_in_off is required and 8-byte aligned (with d_in_len
 * given it is not read), d_bound must not be the array d_in_len.
 *
 * lzs_compress_batch_packed_device: block b is written at d_out + d_out_off[b]; its room is its out_cap.  d_out_len[b] and bytes
 * [0, d_out_len[b]) of the room are byte for byte what lzs_compress_batch_device() gives for that block alone with out_cap = its
 * room, the cut included.  Containment: a block stores only inside its own room; the bytes of the room past d_out_len[b] are
 * unspecified, as the strided call leaves them.  Nothing is read outside the aligned 32-bit words that hold the block's own bytes.
 * An entry that is not a block: d_out_len[b] = 0, nothing of it read or written, the others unaffected.  d_in and d_out must not
 * overlap; d_out_len must not be the array d_in_len (LZS_E_ARG: it carries the blocks' class codes during the launch).  LZS_VERIFY's
 * sampled self-check covers the strided call only.
 *
 * lzs_compact_packed_device: lzs_compact_device() with slot b at d_src + d_src_off[b] (only nblocks entries are read) -- the scan of
 * d_len into d_offsets (nblocks + 1 entries), then the gather.  d_dense must hold sum(d_len) bytes and must not overlap d_src.
 * Unlike lzs_compact_device() an empty call writes nothing, not even d_offsets[0].
 */
int lzs_compressed_bound_packed_device(uint32_t *d_bound, const uint64_t *d_in_off, const uint32_t *d_in_len, size_t nblocks,
                                       void *hip_stream);
int lzs_compress_batch_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                     const uint64_t *d_in_off, const uint32_t *d_in_len, size_t nblocks, void *hip_stream);
int lzs_compact_packed_device(void *d_dense, uint64_t *d_offsets, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_len,
                              size_t nblocks, void *hip_stream);

/*
 * Host-buffer batches: same per-block contract, buffers in host memory.  The call
 * stages through device memory it allocates and frees itself and returns when the
 * results are in `out` / `out_len`.  in_len_each may be NULL (every block in_len bytes).
 * A batch to decompress that is too small to fill the device with a wavefront per block (up to
 * 64 MiB of output) is cut into segments for many wavefronts, block by block:
 * 4 blocks of 64 KiB take 0.7 ms instead of 8.
 */
int lzs_compress_batch(uint8_t *out, size_t out_stride, size_t out_cap, uint32_t *out_len,
                       const uint8_t *in, size_t in_stride, const uint32_t *in_len_each,
                       size_t in_len, size_t nblocks);
int lzs_decompress_batch(uint8_t *out, size_t out_stride, size_t out_cap, uint32_t *out_len,
                         const uint8_t *in, size_t in_stride, const uint32_t *in_len_each,
                         size_t in_len, size_t nblocks);

/*
 * Decode a FILE of concatenated streams as the reference's file decompressor does
 * (c/src/utils/lzs-decompress.c drives the incremental decoder, which after an end marker
 * drops the pad bits to the byte boundary and carries on: lzs-decompression.c:564-576).
 * Same arguments, return value and failure mode as lzs_decompress(); decoding stops at the
 * end of the input or when the output is full.  From 4 KiB on the file is spread over many
 * wavefronts like one long stream (256 MiB of text in 0.45 s with the file I/O);
 * lzs_decompress_batch() with per-block lengths, when they are known, is faster still.
 */
size_t lzs_decompress_concat(uint8_t *out, size_t out_cap, const uint8_t *in, size_t in_len);

#ifdef __cplusplus
}
#endif

#endif /* LZS_MI355X_LZS_BATCH_H */
