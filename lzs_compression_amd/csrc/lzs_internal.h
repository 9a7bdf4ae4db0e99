/*
 * lzs_internal.h -- what the host-side translation units of liblzs share (not installed).
 *   lzs_host.c         errors, device batches, per-thread staging, host batches (their route, and the one-after-the-other
 *                      route: copy in, run, copy out), the one-shot calls
 *   lzs_pipeline.c     large host batches with the three stages overlapped: the plan, the ring, a function per stage
 *   lzs_stream.c       one stream (or a small batch) spread over the device: segments + stitch,
 *                      scan / decode / resolve
 *   lzs_incremental.c  the reference's incremental interface on top of both: one loop over a call's stages per direction
 *   lzs_hostcodec.c    the small calls' host route: the calling thread's own codec
 *   lzs_batch_compress.c  a batch in device memory compressed by segments over all blocks at once, or by workgroups
 */
#ifndef LZS_INTERNAL_H
#define LZS_INTERNAL_H

#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "lzs/lzs.h"
#include "lzs/lzs_batch.h"
#include "lzs_hip_shim.h"

#define LZS_HIDDEN __attribute__((visibility("hidden")))

/* errors (lzs_host.c) */
LZS_HIDDEN extern _Thread_local char tls_error[512];
LZS_HIDDEN int fail(int code, const char *fmt, ...);
LZS_HIDDEN int hip_fail(int hip_error, const char *what);
LZS_HIDDEN int require_device(void);
/* A HIP call of the shim in a function with `int e, rc`: on an error its message is recorded, rc is the LZS_E_* code and the
 * function goes on at `label`. */
#define HIP_TRY_OR(label, call, what) do { e = (call); if (e) { rc = hip_fail(e, what); goto label; } } while (0)
/* ... in a function with NOTHING TO UNDO (the stages of lzs_pipeline.c: all they touch belongs to the run, which
 * host_batch_pipelined() cleans up; those of lzs_stream.c's compressor, whose call ends in one place): it returns the LZS_E_* code at once.  A function that owns something takes HIP_TRY_OR. */
#define HIP_TRY_RET(call, what) do { const int e_ = (call); if (e_) return hip_fail(e_, what); } while (0)

/* The development switches of the environment (tools/README.md), read ONCE per process by lzs_env() -- the
 * entry points ask a struct, not getenv().  LZS_DEV_ENV=1 (set before the first call: the test suites do)
 * makes every lzs_env() read the environment afresh, so a test can flip a switch between two calls. */
typedef struct {
    size_t   keep_max;              /* LZS_KEEP_MAX_MB: staging buffers above it are released after the call; 0: the default (lzs_host.c) */
    int      one_wave, one_workgroup, force_stream;
    uint32_t stream_seg, dec_seg;   /* LZS_STREAM_SEG, LZS_DEC_SEG (0: by size) */
    int      stream_debug, no_marks, no_ones, verify_scan, no_tails, no_chunks;
    int      overlap_off;           /* LZS_HOST_SERIAL: host-buffer batches copy, run and copy back one after the other */
    int      pipe_trace;            /* LZS_PIPE_TRACE (with LZS_STREAM_DEBUG): a line per step of those batches' pipeline */
    int      batch_seg_mb;          /* LZS_BATCH_SEG_MB: host-buffer batches to decompress go by segments up to this extent (0: the default) */
    int      pipe_group, pipe_chunk_mb;   /* LZS_PIPE_GROUP, LZS_PIPE_CHUNK_MB: chunks per launch / chunk size of those batches (0: the defaults) */
    int      pipe_min_mb;           /* LZS_PIPE_MIN_MB: the smallest batch (MiB of the wider side) that takes the overlapped route (0: the default) */
    int      copy_threads;          /* LZS_COPY_THREADS: host threads that fill / empty the pinned pieces of a large batch (default 4) */
    int      staging_fail_mb;       /* LZS_STAGING_FAIL_MB (tests): device reservations above this many MiB fail like a full device */
    int      route;                 /* LZS_ROUTE: 0 by size (the default), 1 "device": every call on the device, 2 "host": the small
                                     * calls' host route for every size it can take, and no device needed (lzs_hostcodec.c) */
    int      burst_split_set;       /* LZS_BURST_SPLIT_MIN is given: the burst decoder splits the runs of at least ... */
    uint32_t burst_split_min;       /* ... this many compressed bytes over the device (0: every run; unset: the default of lzs_burst_plan.h) */
} lzs_env_t;
LZS_HIDDEN const lzs_env_t *lzs_env(void);
/* Checks that the channel calls of lzs_channels.c and lzs_packed.c share: the states; a burst's ids and work area (lzs_channels.c). */
static inline int check_states(const char *who, const void *d_states)
{
    if (!d_states) return fail(LZS_E_ARG, "%s: states is NULL", who);
    if ((uintptr_t)d_states & 3u) return fail(LZS_E_ARG, "%s: states is not 4-byte aligned", who);
    return LZS_OK;
}
LZS_HIDDEN int check_burst(const char *who, const uint32_t *d_channel, size_t nchannels, const void *d_work, size_t work_bytes, size_t npackets);

#define PIPE_STREAMS 4               /* copy in, copy out, two run streams (lzs_pipeline.c) */
#define PIPE_EVENTS  14              /* lzs_pipeline.c: EV_COUNT */

/* per-thread staging (lzs_host.c): one HIP stream and grow-only device buffers per host thread */
enum { BUF_IN, BUF_OUT, BUF_LEN, BUF_INLEN, BUF_AUX, BUF_KEEP, BUF_MARKS, BUF_COUNT };
/* the thread's pinned pieces: lzs_pipeline.c fills PIN_IN0 + (k & 1) and drains PIN_OUT0 + k % 3 for chunk k; the
 * one-after-the-other route of host_batch() lays ragged blocks out in PIN_IN0 (in) and PIN_OUT0, PIN_OUT1 (out) */
enum { PIN_IN0, PIN_IN1, PIN_OUT0, PIN_OUT1, PIN_OUT2, PIN_LENGTHS, PIN_COUNT };
typedef struct {
    void  *stream;
    void  *buf[BUF_COUNT];
    size_t cap[BUF_COUNT];
    uint8_t *host_box;              /* host side of the small incremental calls' single copies */
    void  *host_tab;                /* PINNED host memory for the per-segment tables of the stream paths: their */
    size_t host_tab_cap;            /* copies are small and many (five a round), and pageable ones cost ~150 us each */
    /* the overlapped host-buffer batches (lzs_pipeline.c): copy-in, two compute and copy-out streams, events, pinned pieces */
    void  *pipe_stream[PIPE_STREAMS];
    void  *pipe_event[PIPE_EVENTS];
    void  *pin[PIN_COUNT];
    size_t pin_cap[PIN_COUNT];
    void  *hostcodec;               /* the host route's match-finder tables (lzs_hostcodec.c), made on first use */
} staging_t;
LZS_HIDDEN staging_t *staging_get(void);
LZS_HIDDEN int staging_reserve(staging_t *st, int which, size_t bytes, void **out);   /* 0 or a hipError_t */
LZS_HIDDEN void staging_trim(staging_t *st);
LZS_HIDDEN void *staging_host_tables(staging_t *st, size_t bytes);   /* grow-only, pinned; NULL: out of memory */
/* one of the thread's pinned pieces (hipHostMallocNonCoherent: only the copy engines and the host touch them -- except
 * PIN_LENGTHS, which a kernel writes and which is coherent), grown to `bytes` if it is smaller; 0 or a HIP error. */
LZS_HIDDEN int staging_pin_reserve(staging_t *st, int which, size_t bytes, uint8_t **out);
LZS_HIDDEN double now_ms(void);

/* ---- host-buffer batches (lzs_host.c, lzs_pipeline.c).  `launch` names the operation: lzs_hip_launch_compress or
 * lzs_hip_launch_decompress (the one-shot calls also pass lzs_hip_launch_decompress_concat, one block). */
typedef int (*launch_fn)(void *, size_t, uint32_t, uint32_t *, const void *, size_t, const uint32_t *, uint32_t, uint32_t, void *);
static inline size_t round16(size_t v) { return (v + 15u) & ~(size_t)15u; }
/* blocks b0 .. b0 + nb - 1 of the caller's array laid out in `piece` at the device stride */
static inline void lay_blocks_in(uint8_t *piece, size_t d_in_stride, const uint8_t *in, size_t in_stride, const uint32_t *in_len_each,
                                 size_t in_len, size_t b0, size_t nb)
{
    for (size_t b = 0; b < nb; b++)
        memcpy(piece + b * d_in_stride, in + (b0 + b) * in_stride, in_len_each ? in_len_each[b0 + b] : in_len);
}
/* The way a batch goes, decided from its sizes alone (no device, no staging): decompressed in segments by many wavefronts
 * (lzs_stream.c), offered to the overlapped pipeline first -- pipe_plan() says whether that takes it --, or copied in, run and
 * copied back one after the other.  The strides are those of the blocks in DEVICE memory. */
typedef enum { ROUTE_SERIAL, ROUTE_SEGMENTS, ROUTE_PIPELINE } batch_route_t;
LZS_HIDDEN batch_route_t host_batch_route(launch_fn launch, uint32_t cap32, size_t nblocks, size_t d_in_stride, size_t d_out_stride,
                                          size_t total_in, const lzs_env_t *env);
/* the overlapped route's plan: K chunks of `chunk` blocks, G chunks a launch, J launches, a ring of `slots` launches' worth of
 * device memory, `threads` host threads; taken = 0: not this batch's route.  `in_len` is the longest block. */
typedef struct { int taken, threads; size_t chunk, K, G, J, slots; } pipe_plan_t;
LZS_HIDDEN pipe_plan_t pipe_plan(launch_fn launch, uint32_t cap32, size_t nblocks, size_t in_len, const lzs_env_t *env);
/* LZS_E_* or LZS_OK, *taken = 0: not this batch's route */
LZS_HIDDEN int host_batch_pipelined(const char *who, launch_fn launch, uint8_t *out, size_t out_stride, uint32_t cap32, uint32_t *out_len,
                                    const uint8_t *in, size_t in_stride, const uint32_t *in_len_each, size_t in_len, size_t nblocks,
                                    int *taken);

/* ---- the host route of the small calls (lzs_hostcodec.c).  Which call takes it: */
#define LZS_ROUTE_AUTO 0
#define LZS_ROUTE_DEVICE 1
#define LZS_ROUTE_HOST 2
/* the crossovers, measured on the GPU box (profiles/r05/route_crossover.txt, text; one core of an EPYC 9575F against the
 * MI355X): below them one host core is faster than a launch and its wait.  us a call, device / host:
 *   lzs_compress()    4 KiB 99 / 12.5, 16 KiB 118 / 48, 32 KiB 125 / 242          -> 16 KiB of input
 *   lzs_decompress()  16 KiB of output 346 / 14, 64 KiB 494 / 163, 128 KiB 502 / 361, 256 KiB 517 / 736
 *                                                                                   -> 64 KiB of compressed bytes (~115 KiB of text)
 *   lzs_decompress_incremental(), MB/s: 512-byte calls 4.5 / 204, 64 KiB 223 / 339, 256 KiB 773 / 334   -> 64 KiB a call
 *   lzs_compress_incremental(), MB/s: 512-byte calls 65 / 94, 4 KiB 87 / 109, 16 KiB 119 / 112            -> 16 KiB to decide */
#define HOST_COMPRESS_MAX    16384u     /* lzs_compress(): input bytes */
#define HOST_DECOMPRESS_MAX  65536u     /* lzs_decompress(): compressed bytes */
#define INC_DEC_HOST_MAX     65536u     /* lzs_decompress_incremental(): a call's input bytes */
#define INC_ENC_HOST_MAX     16384u     /* lzs_*compress_incremental(): bytes a piece has to decide */
static inline int route_on_host(size_t n, size_t crossover)
{
    const int r = lzs_env()->route;
    return r == LZS_ROUTE_HOST || (r == LZS_ROUTE_AUTO && n <= crossover);
}
LZS_HIDDEN size_t hostcodec_compress(uint8_t *out, size_t cap, const uint8_t *in, size_t n);      /* SIZE_MAX: out of memory */
LZS_HIDDEN size_t hostcodec_decompress(uint8_t *out, size_t cap, const uint8_t *in, size_t n);
LZS_HIDDEN void hostcodec_free(void *tables);            /* a thread's tables and scratch (staging_destroy) */

/* thresholds of the one-shot calls */
#define STREAM_MIN     6144u        /* shorter inputs are compressed by one workgroup (4 KiB: 0.109 ms alone, 0.127 in segments; 8 KiB: 0.167 / 0.127) */
#define STREAM_DEC_MIN 4096u        /* shorter streams are decompressed by one wavefront */

/* Batches up to this much output are decompressed in segments; larger ones fill the device with a
 * wavefront per block.  Measured (text, 64 KiB blocks, host buffers, ms; segments / wavefront per
 * block), round 2: 4 blocks 0.74 / 8.3, 64 blocks 1.5 / 8.5, 256 blocks 4.2 / 9.4, 512 blocks 11.4 / 13.4,
 * 1024 blocks 25.5 / 24.8; round 4 (the segment decoder at six wavefronts per CU, the copies through pinned
 * pieces; against the overlapped route with the block decoder): 768 blocks 6.2 / 8.6, 1024 blocks 7.3 / 8.9,
 * 1536 blocks 9.9 / 10.2, 2048 blocks 12.4 / 12.4, 4096 blocks 22.2 / 17.8 (profiles/r04/hostbatch_small_routes.txt). */
#define BATCH_SEG_MAX_BLOCKS 4096u
#define BATCH_SEG_MAX_EXTENT ((unsigned long long)64 << 20)

/* one stream on the whole device (lzs_stream.c) */
typedef struct {                    /* a piece of a stream for lzs_compress_incremental(): see stream_compress_piece() */
    const uint8_t *prefix;
    uint32_t prefix_len;
    uint32_t c0, ext_off, bit0;
    uint8_t  first;
    int      last;
    uint32_t stop;          /* != 0: no token starts at or after this position (the data still ends at n: a piece that knows
                             * where the stream ends but must not produce more than its caller has room for) */
    /* results */
    uint32_t c_exit;        /* everything before it is encoded */
    uint32_t ext_exit;      /* != 0: still inside a long match at this offset */
    uint64_t nbits;         /* bits in the output (bit0 included, end marker not) */
} piece_t;
typedef struct {                    /* a piece of a stream for lzs_decompress_incremental(): see stream_decompress() */
    const uint8_t *prefix;
    uint32_t prefix_len;
    uint32_t entry0;
    const uint8_t *hist;
    uint32_t hist_len;
    /* results */
    uint32_t seg, segs_done;    /* segment size used; segments decoded */
    uint32_t next_entry;        /* state word at the start of segment segs_done */
} dec_piece_t;
LZS_HIDDEN size_t stream_compress_piece(uint8_t *out, size_t cap, const uint8_t *in, size_t n, int dev, int *status, piece_t *pc);
/* two of its stages, host code only (tests/cpu_shim/san_driver.c asks them directly) */
LZS_HIDDEN uint32_t settle_compress_entries(uint32_t *entry, uint8_t *dirty, const uint32_t *exits, uint32_t nseg);
LZS_HIDDEN int open_match_take_back(const uint32_t *open, uint64_t *nbits, uint32_t nseg, uint32_t n, uint32_t c_first, uint32_t *c_exit,
                                    uint32_t *ext_exit);
LZS_HIDDEN size_t hostcodec_compress_piece(uint8_t *out, size_t cap, const uint8_t *in, size_t n, piece_t *pc);   /* the same on the host; SIZE_MAX: out of memory */
LZS_HIDDEN void hostcodec_decode_resume(lzs_dec_resume_t *st, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap);   /* lzs_decode_resume_kernel's contract */
LZS_HIDDEN void hostcodec_decode_resume_fields(uint32_t *bitq, uint32_t *qlen, uint32_t *off, uint32_t *rem, uint32_t *extended,
                                               uint8_t *hist, uint32_t *hist_len, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap,
                                               uint32_t *in_used, uint32_t *out_made, uint32_t *status_out);
LZS_HIDDEN size_t stream_compress(uint8_t *out, size_t cap, const uint8_t *in, size_t n, int dev, int *status);
LZS_HIDDEN size_t stream_decompress(uint8_t *out, size_t cap, const uint8_t *in, size_t n, int dev, int *status, int concat,
                                    dec_piece_t *dp);
LZS_HIDDEN int batch_decompress_segments(staging_t *st, void *stream, const char *who, void *d_out, size_t d_out_stride,
                                         uint32_t cap32, uint32_t *out_len, uint32_t *d_len, const void *d_in, size_t d_in_stride,
                                         const uint32_t *in_len_each, uint32_t in_len, size_t nblocks);

/* ---- what the size query for long streams (lzs_size_stream.c) shares with the many-wavefront decompressor */
/* The segments of one stream, or of all the blocks of a batch, as SCAN, DECODE and RESOLVE see them.  One stream needs no
 * range tables -- segment k is bytes [k seg, (k + 1) seg) of it -- and only its segment 0 is a first segment: one entered in
 * a state that is given, not taken over from the segment before.  A batch says for every segment where it starts, where its
 * block's stream ends, where its block's output begins and must end, and whether it is its block's first. */
typedef struct {
    const char *label;              /* "stream decode" or "batch decode": the LZS_STREAM_DEBUG lines */
    size_t   nblocks;               /* 0: one stream */
    uint32_t seg, nseg;
    uint32_t *seen, *entry, *exits, *count, *start;      /* host side; exits and count lie one behind the other */
    uint32_t *base, *end, *floor_, *limit;               /* the range tables, or NULL */
    uint8_t  *dirty, *ones, *first;                      /* (first: or NULL) */
    /* device side, in this order; then two counters, dirty, ones */
    uint32_t *d_entry, *d_exit, *d_count, *d_start, *d_base, *d_end, *d_floor, *d_limit, *d_counters;
    uint8_t  *d_dirty, *d_ones;
} seg_table_t;
LZS_HIDDEN int stream_call_begins(const char *who, size_t tab_bytes, staging_t **st, void **tables);
LZS_HIDDEN int stream_copy_in(void *d_in, const uint8_t *prefix, size_t pre, const uint8_t *in, size_t n, void *stream);
LZS_HIDDEN size_t stream_call_ends(size_t result, int rc, int dev, const char *who, int *status);
LZS_HIDDEN uint32_t stream_dec_seg(size_t n);
LZS_HIDDEN uint32_t stream_seg(size_t n);              /* the segment compressor's segment size for n bytes of input (LZS_STREAM_SEG forces it) */

/* ---- a batch in device memory compressed by segments (lzs_batch_compress.c) */
/* After a round over the segments of many blocks: settle_compress_entries() with a first segment (seg_start[k] == 0) wherever a
 * block begins -- entered at 0, never dirty again.  Host code only.  Returns how many are dirty now. */
LZS_HIDDEN uint32_t settle_compress_entries_batch(uint32_t *entry, uint8_t *dirty, const uint32_t *exits, const uint32_t *seg_start,
                                                  uint32_t nseg);
LZS_HIDDEN void segtab_lay_out(seg_table_t *t, uint32_t *h, uint32_t *d, int ranges);
LZS_HIDDEN uint32_t settle_entries(seg_table_t *t, int use_ones, int *host_made);
LZS_HIDDEN int scan_rounds(seg_table_t *t, void *stream, const char *who, const void *d_in, uint32_t n, uint32_t in_extent,
                           uint32_t entry0, int concat, uint32_t *d_marks, double *t0);

#endif
