/*
 * lzs_hip_shim.h -- the thin extern-"C" seam between the C host library
 * (lzs_host.c, lzs_stream.c, lzs_incremental.c) and the HIP translation unit (lzs_kernels.hip).  Internal: not
 * installed, not part of the public ABI (that is include/lzs/).
 *
 * Every function returns a hipError_t value as int (0 = hipSuccess) unless noted.
 */
#ifndef LZS_HIP_SHIM_H
#define LZS_HIP_SHIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int         lzs_hip_device_count(int *count);
int         lzs_hip_describe(char *buf, size_t cap);          /* "hip gfx950 ..., N CUs, ..." */
const char *lzs_hip_strerror(int hip_error);

int lzs_hip_total_memory(size_t *bytes);             /* the current device's memory */
int lzs_hip_malloc(void **p, size_t bytes);
int lzs_hip_free(void *p);
int lzs_hip_stream_create(void **stream);
int lzs_hip_stream_destroy(void *stream);
int lzs_hip_stream_sync(void *stream);
int lzs_hip_event_create(void **event);              /* (no timing) */
int lzs_hip_event_destroy(void *event);
int lzs_hip_event_record(void *event, void *stream);
int lzs_hip_event_sync(void *event);
int lzs_hip_event_done(void *event);                 /* 1: complete, 0: not yet, < 0: minus a hipError_t */
int lzs_hip_stream_wait_event(void *stream, void *event);
int lzs_hip_host_malloc(void **p, size_t bytes);      /* pinned host memory */
int lzs_hip_host_malloc_staging(void **p, size_t bytes);   /* pinned, hipHostMallocNonCoherent: pieces only the copy engines and the
                                                             * host touch, handed over at events (56 instead of 35-39 GB/s on a quiet
                                                             * device: tools/probes/pipe_copy_probe.hip) */
int lzs_hip_host_free(void *p);
/* Fetch and drop the runtime's sticky "last error" (a failed hipMalloc stays the answer of hipGetLastError() until it is
 * fetched, and the launchers below return hipGetLastError() after their launch). */
void lzs_hip_clear_error(void);
/* `nwords` 32-bit words from device memory to PINNED, COHERENT host memory (lzs_hip_host_malloc) by a kernel on `stream`
 * (not by a copy engine: an engine runs its queue in order, and a small copy waiting for a kernel would hold up the large
 * copies queued behind it); the kernel ends with a system-scope fence */
int lzs_hip_words_to_host(uint32_t *h_dst, const uint32_t *d_src, size_t nwords, void *stream);
int lzs_hip_h2d(void *dst, const void *src, size_t bytes, void *stream);
int lzs_hip_d2h(void *dst, const void *src, size_t bytes, void *stream);
int lzs_hip_d2d(void *dst, const void *src, size_t bytes, void *stream);
int lzs_hip_memset(void *dst, int value, size_t bytes, void *stream);

/* How CHAIN links the positions of a batch on the current device: 0 = by one ordered LDS exchange
 * (the device was asked and applies same-address lanes in lane order), 1 = the order-independent
 * form (the device failed the check, or LZS_CHAIN_FALLBACK=1).  The first call per device runs
 * lzs_lds_order_check_kernel on `stream` and waits for it. */
int lzs_hip_chain_mode(void *stream, int *mode);

/* Kernel launches (asynchronous on `stream`). */
/* The LDS ordering check once more beside the first compress launch (under load): 0 not started yet, 1 in flight,
 * 2 read (a failure switches the device to the order-independent chain build, loudly).  LZS_VERIFY=N in the
 * environment: every N-th compress launch is re-run in the order-independent form and compared on the device. */
int lzs_hip_load_check_state(int dev);
/* What LZS_VARIANT (development, read once per process) forces on every block of a compress launch: 0 nothing -- the blocks'
 * classes decide --, 1 the default (text) variant, 2 few distinct grams, 3 nearly all literals.  For tests: proof of what ran. */
int lzs_hip_forced_variant(void);
int lzs_hip_launch_compress(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                            const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                            uint32_t in_len, uint32_t nblocks, void *stream);
/* lzs_hip_launch_compress() on a device that applies LDS exchanges in lane order launches one variant of the kernel per
 * class of block over the same grid, and the blocks say which is theirs (lzs_classify_blocks_kernel leaves a code in
 * d_out_len[b] until the block's length replaces it).  This runs the classifier alone: d_codes[b] = 0xFFFFFFF0 | 1 the default
 * variant, | 2 few distinct grams (small tables, six workgroups per CU), | 3 nearly all literals (one full step per pass). */
int lzs_hip_classify_blocks(uint32_t *d_codes, const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                            uint32_t nblocks, void *stream);
int lzs_hip_launch_decompress(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                              const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                              uint32_t in_len, uint32_t nblocks, void *stream);
int lzs_hip_launch_decompress_concat(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                     const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                                     uint32_t in_len, uint32_t nblocks, void *stream);
/* One long stream in segments of `seg` bytes (lzs_compress_segments_kernel): segment k, entered
 * at d_entry[k], writes its bits to slot k and reports where its last token ends and its bit
 * count; only segments with d_dirty[k] != 0 run (NULL: all).  lzs_stitch_segments_kernel then ORs
 * the slots into the zeroed, 4-aligned d_out at d_bit_at[k] and appends the end marker.  A segment
 * whose bits did not fit its slot (d_nbits[k] > 8 * slot_stride: a very long match) is run once more
 * with d_out / d_bit_at set and ORs its bits in directly.
 * A piece of a stream that will go on (the incremental interface): no token starts at or after
 * `lim` (= n for a whole stream), d_open[2k..] receives {offset, start} of segment k's last token
 * if that is a match reaching n (it may still grow), and no end marker is written.  A piece that
 * begins inside such a match has lzs_extend_resume_kernel write its length nibbles first
 * (d_result: next position, still open, bits written low/high). */
int lzs_hip_launch_compress_segments(void *d_slots, size_t slot_stride, const void *d_in, uint32_t n,
                                     uint32_t seg, uint32_t nseg, const uint32_t *d_entry,
                                     const uint8_t *d_dirty, uint32_t *d_exit, uint64_t *d_nbits,
                                     void *d_out, const uint64_t *d_bit_at, uint32_t lim, uint32_t *d_open,
                                     void *stream);
int lzs_hip_launch_stitch_segments(void *d_out, const void *d_slots, size_t slot_stride,
                                   const uint64_t *d_bit_at, const uint64_t *d_nbits, uint32_t nseg,
                                   int end_marker, void *stream);
int lzs_hip_launch_extend_resume(void *d_out, uint32_t bit0, const void *d_in, uint32_t n, uint32_t c0,
                                 uint32_t off, int last, uint32_t *d_result, void *stream);
/* The same two for the segments of MANY streams, the blocks of a batch (lzs_batch_compress.c).  Block b is the
 * d_blk_len[b] bytes at d_in + d_blk_at[b] (a 64-bit byte offset) and is compressed as a whole stream of its own: nothing in
 * front of it or behind it is read, whatever its address.  Segment k belongs to block d_seg_block[k] and starts d_seg_start[k]
 * bytes into it (a multiple of `seg`; a block of length 0 has one segment, at 0, without a bit); d_entry, d_exit are positions in
 * the block; slots, d_dirty, d_nbits as above, indexed by k.
 * lzs_hip_launch_stitch_segments_batch() ORs segment k's slot into bit d_bit_at[k] of ITS BLOCK's output, d_out + b out_stride --
 * 4-aligned and zeroed as far as the block's stream reaches -- and puts the end marker behind the last segment of every block.
 * With d_out / d_bit_at set, lzs_hip_launch_compress_segments_batch() is the second pass of the segments with d_dirty[k] != 0
 * (those that did not fit their slot), ORed into the same place.
 * Neither stores outside [d_out + b out_stride, + out_cap rounded up to 4) for any block b; the caller sees to it that this lies
 * within the block's out_stride bytes (out_cap <= out_stride, out_stride a multiple of 4).  What would lie behind is dropped. */
int lzs_hip_launch_compress_segments_batch(void *d_slots, size_t slot_stride, const void *d_in, const uint64_t *d_blk_at,
                                           const uint32_t *d_blk_len, const uint32_t *d_seg_block, const uint32_t *d_seg_start,
                                           uint32_t seg, uint32_t nseg, const uint32_t *d_entry, const uint8_t *d_dirty,
                                           uint32_t *d_exit, uint64_t *d_nbits, void *d_out, size_t out_stride, uint32_t out_cap,
                                           const uint64_t *d_bit_at, void *stream);
int lzs_hip_launch_stitch_segments_batch(void *d_out, size_t out_stride, uint32_t out_cap, const void *d_slots, size_t slot_stride,
                                         const uint64_t *d_bit_at, const uint64_t *d_nbits, const uint32_t *d_seg_block,
                                         const uint32_t *d_seg_start, const uint32_t *d_blk_len, uint32_t seg, uint32_t nseg, void *stream);
/* `rows` rows of `width` bytes, `pitch` bytes apart, set to `value`; what lies between the rows is not touched */
int lzs_hip_memset_rows(void *d, size_t pitch, int value, size_t width, size_t rows, void *stream);
/* One long stream decompressed by many wavefronts (lzs_scan_stream_kernel, lzs_decode_stream_kernel,
 * lzs_resolve_stream_kernel; state words and the scheme are described at the kernels).  With the
 * tables (all NULL for one stream) the segments belong to many streams in one buffer -- a batch of
 * blocks: segment k starts at d_in[d_seg_base[k]], its stream ends at d_in[d_seg_end[k]], copies
 * reaching before d_out[d_out_floor[k]] yield zeros and nothing is written at or past
 * d_out[d_out_limit[k]]. */
#define LZS_SEG_STOP (1u << 30)
unsigned lzs_hip_dec_segment_bytes(void);             /* the largest segment (long streams) */
#define LZS_SCAN_MARK_WORDS 140u     /* per segment in d_marks: what a full walk leaves for repeated ones */
int lzs_hip_launch_scan_stream(const void *d_in, uint32_t n, uint32_t nseg, const uint32_t *d_entry,
                               const uint8_t *d_dirty, uint32_t *d_exit, uint32_t *d_count,
                               uint8_t *d_all_ones /* or NULL */, uint32_t *d_marks, int compare,
                               uint32_t seg, int concat /* go on after end markers */,
                               const uint32_t *d_seg_base, const uint32_t *d_seg_end /* or NULL, NULL */, uint32_t in_extent, void *stream);
int lzs_hip_launch_decode_stream(void *d_out, uint32_t cap, uint32_t *d_origin, uint32_t *d_tainted,
                                 const void *d_in, uint32_t n, uint32_t in_extent /* readable bytes at d_in */,
                                 uint32_t nseg, const uint32_t *d_entry,
                                 const uint32_t *d_out_start, uint32_t seg, int concat,
                                 const uint32_t *d_seg_base, const uint32_t *d_seg_end,
                                 const uint32_t *d_out_floor, const uint32_t *d_out_limit, void *stream);
int lzs_hip_launch_resolve_blocks(void *d_out, uint32_t *d_origin, size_t out_stride, const uint32_t *d_len,
                                  uint32_t nblocks, void *stream);   /* a batch: one workgroup per block, to the end */
int lzs_hip_launch_resolve_stream(void *d_out, uint32_t *d_origin, uint32_t total, uint32_t round,
                                  uint32_t *d_left, int last /* expected to finish: finished groups keep their origins */,
                                  void *stream);
/* The rounds of the same on tails alone: the groups of four bytes in front of the starts
 * d_seg_start[0], [stride], [2 stride] ... (positions in d_out) of `nseg` segments.  d_out must
 * be 4-byte and d_origin 16-byte aligned. */
int lzs_hip_launch_resolve_tails(void *d_out, uint32_t *d_origin, uint32_t total, const uint32_t *d_seg_start,
                                 uint32_t nseg, uint32_t stride, uint32_t round, uint32_t *d_left, void *stream);
/* Without rounds: a workgroup per `per_chunk` consecutive segments takes their tails in order;
 * what is left open afterwards is a copy of a byte in the tail in front of its chunk. */
int lzs_hip_launch_resolve_chunks(void *d_out, uint32_t *d_origin, uint32_t total, const uint32_t *d_seg_start,
                                  uint32_t nseg, uint32_t per_chunk, uint32_t round, void *stream);
/* The incremental entry points (lzs_incremental.c).  Status bits as in the reference's
 * LzsCompressStatus_t / LzsDecompressStatus_t (lzs.h:90-98, 168-176). */
#define LZS_INC_INPUT_STARVED   0x01u
#define LZS_INC_INPUT_FINISHED  0x02u
#define LZS_INC_END_MARKER      0x04u
#define LZS_INC_NO_OUTPUT_SPACE 0x08u
#define LZS_INC_ERROR           0x10u
/* What the incremental decoder carries from call to call (lzs_decode_resume_kernel reads and
 * rewrites it in device memory; the host keeps it in the caller's LzsDecompressParameters_t). */
typedef struct {
    uint32_t bitq, qlen;            /* bits of an unfinished token, left-aligned; how many */
    uint32_t off, rem, extended;    /* copy in progress: offset, bytes left, a nibble follows */
    uint32_t hist_len;              /* bytes of history in hist[] (oldest first), <= 2047 */
    uint32_t in_used, out_made, status, reserved;   /* results of the call */
    uint8_t  hist[2048];
} lzs_dec_resume_t;
int lzs_hip_launch_decode_resume(lzs_dec_resume_t *d_state, const void *d_in, uint32_t n,
                                 void *d_out, uint32_t cap, void *stream);
/* Many channels, one packet each (include/lzs/lzs_channels.h; lzs_channels.c checks the arguments): packet b is compressed /
 * decompressed on channel d_channel[b] (b if NULL) with the history in that channel's LZS_CHANNEL_STATE_BYTES-byte slot of
 * d_states, which is advanced; d_status[b] (or NULL) receives the LZS_C_STATUS_* / LZS_D_STATUS_* bits. */
int lzs_hip_launch_compress_channels(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                     const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                                     const uint32_t *d_channel, void *d_states, uint8_t *d_status, uint32_t npackets, void *stream);
int lzs_hip_launch_decompress_channels(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                       const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                                       const uint32_t *d_channel, void *d_states, uint8_t *d_status, uint32_t npackets, void *stream);
/* Many packets per channel (lzs_channels_burst.hip): the runs of a burst, one per group of a wavefront, longest first --
 * d_run_key[r] (1 + compressed bytes, 0: no run r; descending) and d_run_at[r] (its first position in the order by channel),
 * d_run_end[position of a run's first packet] (one past its last), d_skey / d_sidx (channel, nchannels if out of range, and
 * packet at each position).  A call with packet flags has a run per reset as well: d_rmark[position] says where
 * runs start and which start from an empty history, d_rkey[position] is the run's id, d_stage the staging slots of the channels with
 * several runs (kernels/common.inc, RunTables); all three NULL without flags. */
int lzs_hip_launch_decompress_runs(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                   const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                                   const uint32_t *d_run_key, const uint32_t *d_run_at, const uint32_t *d_run_end,
                                   const uint32_t *d_skey, const uint32_t *d_sidx, uint32_t nchannels, void *d_states,
                                   uint8_t *d_status, uint32_t npackets, const uint32_t *d_rkey, const uint32_t *d_rmark, void *d_stage,
                                   void *stream);
/* Many packets per channel (lzs_channels_burst.hip; lzs_channels.c checks the arguments; the work area's layout and size, and
 * `split` and `split_min`, are lzs_burst_plan.h's): one burst through compression (decompress 0) or decompression (1) -- the
 * grouping, then the kernels above.  `split` (decompression; the work area then holds the split size): the
 * runs of at least `split_min` compressed bytes are decoded by all their packets at once with per-byte origins and resolved
 * afterwards (lzs_burst_parse_kernel, lzs_burst_resolve_kernel), the others by lzs_hip_launch_decompress_runs.  d_flags: a byte a
 * packet, bit 0 a history reset in front of it (lzs_channels.h, LZS_PACKET_RESET), or NULL. */
int lzs_hip_burst(int decompress, void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                  const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                  const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, uint32_t nchannels, uint8_t *d_status,
                  void *d_work, uint32_t npackets, int split, uint32_t split_min, void *stream);
int lzs_hip_launch_compact(void *d_dense, uint64_t *d_offsets, const void *d_slots,
                           size_t slot_stride, const uint32_t *d_len, uint32_t nblocks,
                           void *stream);
/* The size query (lzs_decoded_size.hip; lzs_size_query.c checks the arguments): d_size[b] / d_status[b] (or NULL) = the length
 * and the LZS_D_STATUS_* bits the decoders give stream b at a capacity of `limit`, by a token walk, one lane a stream. */
int lzs_hip_launch_decoded_size(uint32_t *d_size, uint8_t *d_status, const void *d_in, size_t in_stride,
                                const uint32_t *d_in_len, uint32_t in_len, uint32_t limit, uint32_t nblocks,
                                void *stream);
/* The finishing walk of the size query for long streams (lzs_size_stream.hip; lzs_size_stream.c has the route):
 * stream i is walked from d_in[d_from[i]], entered in the state word d_entry[i] that SCAN settled for the segment that starts
 * there (above), to d_in[d_end[i]], its stream's end, with d_room[i] bytes of room: d_counted[i] = the bytes counted,
 * d_status[i] the LZS_D_STATUS_* bits -- lzs_hip_launch_decoded_size's walk and rules from another start.  One lane a stream. */
int lzs_hip_launch_size_finish(uint32_t *d_counted, uint8_t *d_status, const void *d_in, const uint32_t *d_from,
                               const uint32_t *d_end, const uint32_t *d_entry, const uint32_t *d_room, uint32_t nstreams,
                               void *stream);
/* The packed calls (lzs_packed.c checks the arguments): stream b lies at d_in + d_in_off[b] -- d_in_len[b] bytes,
 * or up to d_in_off[b + 1] with d_in_len NULL -- and decodes to d_out + d_out_off[b] with d_out_off[b + 1] - d_out_off[b] bytes
 * of room.  lzs_hip_launch_scan_sizes: d_offsets[b + 1] = d_offsets[b] + d_size[b] rounded up to `align` (a power of two),
 * nblocks + 1 entries from 0 -- also for nblocks = 0. */
int lzs_hip_launch_decoded_size_packed(uint32_t *d_size, uint8_t *d_status, const void *d_in, const uint64_t *d_in_off,
                                       const uint32_t *d_in_len, uint32_t limit, uint32_t nblocks, void *stream);
int lzs_hip_launch_decompress_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                     const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t nblocks, void *stream);
int lzs_hip_launch_decompress_channels_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                              const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                              void *d_states, uint8_t *d_status, uint32_t npackets, void *stream);
int lzs_hip_launch_scan_sizes(uint64_t *d_offsets, const uint32_t *d_size, uint32_t align, uint32_t nblocks, void *stream);
/* Packed compression (lzs_packed.c checks the arguments): block b lies at d_in + d_in_off[b] and is compressed to
 * d_out + d_out_off[b] with d_out_off[b + 1] - d_out_off[b] bytes of room, its capacity.  lzs_hip_launch_compress_packed takes the
 * decisions of lzs_hip_launch_compress (the variants by class; LZS_VERIFY does not cover it); d_bound[b] = LZS_COMPRESSED_MAX of
 * block b's length, 0 for an entry that is not a block; lzs_hip_launch_compact_packed is lzs_hip_launch_compact from rooms. */
int lzs_hip_launch_compressed_bound_packed(uint32_t *d_bound, const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t nblocks,
                                           void *stream);
int lzs_hip_launch_compress_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                   const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t nblocks, void *stream);
int lzs_hip_launch_compress_channels_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                            const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                            void *d_states, uint8_t *d_status, uint32_t npackets, void *stream);
int lzs_hip_launch_compact_packed(void *d_dense, uint64_t *d_offsets, const void *d_src, const uint64_t *d_src_off,
                                  const uint32_t *d_len, uint32_t nblocks, void *stream);
/* Packed bursts (lzs_channels_burst.hip; lzs_packed.c checks the arguments): lzs_hip_burst with the packets and their
 * rooms addressed as in the packed calls above.  split, origin_cap (lzs_burst_plan_split_packed): the work area holds origin_cap
 * 16-bit origins behind the burst size; the long runs are split if the sum of the rooms, found on the device, fits them.
 * lzs_hip_launch_decompress_runs_packed is lzs_hip_launch_decompress_runs on such packets; d_room_ends[i] = the sum of the
 * rooms of the packets at sorted positions 0 .. i. */
int lzs_hip_launch_decompress_runs_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                          const uint64_t *d_in_off, const uint32_t *d_in_len, const uint64_t *d_room_ends,
                                          const uint32_t *d_run_key, const uint32_t *d_run_at, const uint32_t *d_run_end,
                                          const uint32_t *d_skey, const uint32_t *d_sidx, uint32_t nchannels, void *d_states,
                                          uint8_t *d_status, uint32_t npackets, const uint32_t *d_rkey, const uint32_t *d_rmark,
                                          void *d_stage, void *stream);
int lzs_hip_burst_packed(int decompress, void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                         const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel, const uint8_t *d_flags,
                         void *d_states, uint32_t nchannels, uint8_t *d_status, void *d_work, uint32_t npackets, int split,
                         uint64_t origin_cap, uint32_t split_min, void *stream);

#ifdef __cplusplus
}
#endif
#endif
