/* lzs_launch_plan.h -- which kernels a call of the launchers in lzs_kernels.hip runs, as plain functions of what the launcher knows.
 *
 * Plain C that also compiles as C++: no HIP, no globals, no getenv.  Every environment flag and every piece of device state
 * comes in as an argument, so the rules stand where a CPU test reaches them: tests/cpu_shim/plan_check.c holds each of them
 * to a table of literal rows (tests/test_launch_plan.py).  A launcher asks its plan and then launches; none keeps a copy of a rule.
 */
#ifndef LZS_LAUNCH_PLAN_H
#define LZS_LAUNCH_PLAN_H

#include <stdint.h>

/* What lzs_kernels.hip holds equal to its kernels' constants with static_assert. */
#define LZS_PLAN_DEC_GROUPS 8u             /* kDecGroups: streams per wavefront of the grouped decoders */
/* A compress launch of this many blocks fills the device: the LDS ordering check may start beside it. */
#define LZS_PLAN_LOAD_CHECK_BLOCKS 256u

/* ---- compress: which variants of the kernel a classified launch runs ------------------------------------------------------
 * seen[c], c = 1..3: the id of the last launch whose classifier met a block of class c (0: never; ids are never 0 and wrap).
 * allow: bit c set = variant c is launched; a block of another class goes to catch_all -- the default variant (1) if that
 * runs, else the first that does.  All three while nothing is known (no words, or no class seen yet), and while the stream is
 * being captured into a graph: the guess would be frozen with it.  Otherwise the classes one of the last three classifiers met.
 * An id is a launch counter with bit 31 set, so after 0xFFFFFFFF comes 0x80000000: ids are compared as serial numbers of 31 bits
 * (a is later than b when it is ahead by less than 2^30), and an age is a difference of 31 bits. */
typedef struct { uint32_t allow, catch_all; } lzs_plan_variants_t;

static inline lzs_plan_variants_t lzs_plan_variants(const uint32_t seen[4], int have_seen, int capturing)
{
    lzs_plan_variants_t p = { 0xEu, 1u };
    uint32_t newest = 0;
    int c;
    if (!have_seen || capturing) return p;
    for (c = 1; c <= 3; c++)
        if (seen[c] && (newest == 0 || (int32_t)((seen[c] - newest) << 1) > 0)) newest = seen[c];
    if (newest == 0) return p;
    p.allow = 0;
    for (c = 1; c <= 3; c++)
        if (seen[c] && ((newest - seen[c]) & 0x7FFFFFFFu) <= 2u) p.allow |= 1u << c;
    p.catch_all = (p.allow & 2u) ? 1u : ((p.allow & 4u) ? 2u : 3u);
    return p;
}

/* ---- compress: one variant for every block (serve 0), or the classifier and then the allowed variants ----------------------
 * chain_mode != 0: the order-independent CHAIN for all blocks.  forced: LZS_VARIANT, 0 none, 1 text, 2 few, 3 lit.  A launch
 * of fewer than classify_min blocks takes the default alone.  one_variant: a build with the default and the safe form only.
 * The load check steps beside launches of the ordered form, and may start beside one that fills the device. */
enum { LZS_RUN_SAFE = 0, LZS_RUN_FEW = 1, LZS_RUN_LIT = 2, LZS_RUN_TEXT = 3, LZS_RUN_CLASSIFY = 4 };
typedef struct { int run; int load_check; int load_check_start; } lzs_plan_compress_t;

static inline lzs_plan_compress_t lzs_plan_compress(int chain_mode, int forced, uint32_t nblocks, uint32_t classify_min, int one_variant)
{
    lzs_plan_compress_t p;
    if (chain_mode != 0) p.run = LZS_RUN_SAFE;
    else if (one_variant) p.run = LZS_RUN_TEXT;
    else if (forced == 2) p.run = LZS_RUN_FEW;
    else if (forced == 3) p.run = LZS_RUN_LIT;
    else if (forced == 0 && nblocks >= classify_min) p.run = LZS_RUN_CLASSIFY;
    else p.run = LZS_RUN_TEXT;
    p.load_check = chain_mode == 0;
    p.load_check_start = p.load_check && nblocks >= LZS_PLAN_LOAD_CHECK_BLOCKS;
    return p;
}

/* ---- grouped decoders: streams per wavefront --------------------------------------------------------------------------------
 * The kernels bound a wavefront's input loads by one 32-bit extent over its streams: eight streams to a wavefront unless
 * `span` strides and the longest stream do not fit one (have_lens: lengths on the device, the longest a stream may be). */
static inline uint32_t lzs_plan_dec_per_wave(uint64_t in_stride, uint32_t span, int have_lens, uint32_t in_len)
{
    const uint64_t longest = have_lens ? 0xC0000400ull : in_len;
    return in_stride * span + longest < 0xFFFFFF00ull ? LZS_PLAN_DEC_GROUPS : 1u;
}
/* blocks and channel packets: a wavefront takes eight neighbours */
static inline uint32_t lzs_plan_dec_per_wave_blocks(uint64_t in_stride, int have_lens, uint32_t in_len)
{
    return lzs_plan_dec_per_wave(in_stride, LZS_PLAN_DEC_GROUPS - 1u, have_lens, in_len);
}
/* runs of channel packets: a wavefront's runs take packets from anywhere in the input (npackets >= 1) */
static inline uint32_t lzs_plan_dec_per_wave_runs(uint64_t in_stride, uint32_t npackets, int have_lens, uint32_t in_len)
{
    return lzs_plan_dec_per_wave(in_stride, npackets - 1u, have_lens, in_len);
}

/* ---- segments of a stream: the decode kernel's form -------------------------------------------------------------------------
 * n bytes of input decode to at most cap (n == 0: a batch of blocks with segment tables, the expansion is not known).
 * Streams that expand more than sixfold are runs: one wavefront per segment.  Otherwise eight segments per wavefront:
 * between a quarter and nine tenths of its output a stream is mostly short matches (a second token per trip), from nine
 * tenths mostly literals (the 96-bit buffer).  old_decode: LZS_SEG_DECODE=wave; one_token: LZS_DEC_ONE_TOKEN. */
enum { LZS_DECODE_WAVE = 0, LZS_DECODE_G8_PLAIN = 1, LZS_DECODE_G8_TWO = 2, LZS_DECODE_G8_WIDE = 3 };

static inline int lzs_plan_decode_stream(uint32_t n, uint32_t cap, int old_decode, int one_token)
{
    const uint64_t n64 = n, cap64 = cap;
    if (old_decode || !(n == 0u || cap64 <= 6u * n64)) return LZS_DECODE_WAVE;
    if (one_token || n == 0u) return LZS_DECODE_G8_PLAIN;
    if (4u * n64 > cap64 && 10u * n64 < 9u * cap64) return LZS_DECODE_G8_TWO;
    if (10u * n64 >= 9u * cap64) return LZS_DECODE_G8_WIDE;
    return LZS_DECODE_G8_PLAIN;
}

/* ---- segments of a stream: the scan kernel's form ---------------------------------------------------------------------------
 * scan_env: LZS_SCAN, 0 not set, 1 wave, 2 g8.  A lane per segment (lanes = 1; LZS_SCAN=g8: eight lanes) in the first round,
 * which has the all-0xFF flags to fill first, and in the later ones, which compare against its marks; the wave kernel when
 * neither holds or LZS_SCAN=wave asks for it.  With a lane per segment the marks start from 0xFF when there are none yet. */
typedef struct { int lanes; int concat; int all_ones_first; int clear_marks; } lzs_plan_scan_t;    /* lanes 0: the wave kernel */

static inline lzs_plan_scan_t lzs_plan_scan(int have_all_ones, int compare, int have_marks, int concat, int scan_env)
{
    lzs_plan_scan_t p = { 0, concat ? 1 : 0, 0, 0 };
    if (scan_env == 1 || !(have_all_ones || compare)) return p;
    p.lanes = scan_env == 2 ? 8 : 1;
    p.all_ones_first = have_all_ones ? 1 : 0;
    p.clear_marks = p.lanes == 1 && have_marks && !compare;
    return p;
}

/* ---- origins resolved everywhere: four bytes a thread, 256 threads a workgroup, one workgroup more, 65536 at the most --------- */
static inline uint32_t lzs_plan_resolve_grid(uint32_t total)
{
    const uint32_t grid = (total / 4u + 255u) / 256u + 1u;
    return grid > 65536u ? 65536u : grid;
}

/* ---- size query of a batch with its lengths on the host (lzs_size_stream.c): by lanes or by segments -----------
 * By lanes: lzs_decoded_size_kernel, one lane a block.  By segments: SCAN over every block's segments and one finishing walk a
 * block -- its tables hold 32-bit positions, so `extent`, nblocks strides plus the longest block, must fit 32 bits, and it pays
 * only where a block is many segments: from LZS_PLAN_SIZE_SEG_MIN_AVG bytes a block on average (total_in / nblocks) on -- the
 * smallest average length of the sweep in profiles/r20/size_stream.txt from which every class's rows are faster by segments
 * (low entropy: 2.35 ms against 2.76 at 10 167 bytes, 1.70 against 0.80 at 2545; text turns between 2460 and 9432, high
 * entropy between 1721 and 4570).
 * forced: LZS_SIZE_ROUTE, 0 not set, 1 lanes, 2 segments -- which an extent beyond 32 bits still cannot take. */
#define LZS_PLAN_SIZE_SEG_MIN_AVG 10167u
enum { LZS_SIZE_BY_LANES = 0, LZS_SIZE_BY_SEGMENTS = 1 };

static inline int lzs_plan_size_route(uint64_t extent, uint64_t total_in, uint64_t nblocks, int forced)
{
    if (extent > 0xFFFFFFFFull || nblocks == 0u || total_in == 0u || forced == 1) return LZS_SIZE_BY_LANES;
    if (forced == 2) return LZS_SIZE_BY_SEGMENTS;
    return total_in / nblocks >= LZS_PLAN_SIZE_SEG_MIN_AVG ? LZS_SIZE_BY_SEGMENTS : LZS_SIZE_BY_LANES;
}

/* ---- compressing a batch in device memory with its lengths on the host (lzs_batch_compress.c) ------------------
 * By workgroups: lzs_hip_launch_compress, one workgroup a block.  By segments: every block cut into segments, one workgroup each,
 * entry rounds over all blocks at once, one stitch.  The segments write through 32-bit words into the caller's slots, so
 * d_out (out_align: its address, or its low bits) and out_stride must be multiples of 4, and out_cap must not exceed out_stride:
 * then a block's capacity rounded up to a word lies within its own slot.  Everything else goes by workgroups.
 * Where it pays (profiles/r24/batch_compress.txt: MI355X, medians, ms, by workgroups / by segments; text, low entropy, high
 * entropy; run-to-run spread of the medians 3.8 % at the most).  By workgroups a batch takes as long as its longest block --
 * 1, 8 and 64 blocks of 16 MiB of text all take 210 ms -- and by segments as long as its bytes in all:
 *     64 x 16 MiB   210.4 / 16.1    44.7 / 4.60    163.0 / 15.6        64 x 1 MiB   13.21 / 2.19    2.88 / 0.66    10.22 / 1.98
 *    256 x 1 MiB    13.23 / 5.09    3.01 / 1.44    10.25 / 4.90      1024 x 1 MiB   16.72 / 16.03   3.69 / 4.66    12.48 / 15.58
 *    256 x 64 KiB   0.885 / 0.616   0.258 / 0.399  0.675 / 0.466
 * Blocks of 1 MiB win by segments in every class up to 256 of them and lose in two classes at 1024; blocks of 64 KiB lose in one
 * class at 256 already, the smallest batch measured.  So: by segments when the longest block has LZS_PLAN_BC_SEG_MIN_LONGEST
 * bytes and the batch holds at most LZS_PLAN_BC_SEG_MAX_BLOCKS times that in all -- for uniform blocks, at most that many blocks;
 * a ragged batch is measured by what it would be in blocks of its longest.  Nothing between the measured rows is claimed.
 * forced: LZS_BATCH_COMPRESS_ROUTE, 0 not set, 1 workgroups, 2 segments -- which the preconditions still bind. */
#define LZS_PLAN_BC_SEG_MIN_LONGEST 1048576u    /* the longest block, bytes */
#define LZS_PLAN_BC_SEG_MAX_BLOCKS  256u        /* total input / longest block */
enum { LZS_BATCH_COMPRESS_BY_WORKGROUPS = 0, LZS_BATCH_COMPRESS_BY_SEGMENTS = 1 };

static inline int lzs_plan_batch_compress_route(uint64_t nblocks, uint64_t total_in, uint64_t longest, uint64_t out_cap,
                                                uint64_t out_stride, uint64_t out_align, int forced)
{
    if (nblocks == 0u || nblocks > 0x7FFFFFFFull || out_cap > out_stride || (out_stride & 3u) || (out_align & 3u) || forced == 1)
        return LZS_BATCH_COMPRESS_BY_WORKGROUPS;
    if (forced == 2) return LZS_BATCH_COMPRESS_BY_SEGMENTS;
    return longest >= LZS_PLAN_BC_SEG_MIN_LONGEST && total_in <= (uint64_t)LZS_PLAN_BC_SEG_MAX_BLOCKS * longest ? LZS_BATCH_COMPRESS_BY_SEGMENTS
                                                                                                                 : LZS_BATCH_COMPRESS_BY_WORKGROUPS;
}

/* The segment route takes consecutive blocks in groups, so that the slots of a group -- about 1.14 times its input -- stay within
 * what one stream of `bound` bytes takes: the blocks b0, b0 + 1, ... whose lengths sum to `bound` at the most, and never fewer
 * than one (a block longer than the bound is a group of its own), nor more than LZS_PLAN_BC_GROUP_MAX_BLOCKS: blocks without a
 * byte add nothing to the sum but a segment each to the tables.  len_each NULL: every block has len_all bytes.  Returns how
 * many blocks the group at b0 has (0 only if b0 >= nblocks). */
#define LZS_PLAN_BC_GROUP_MAX_BLOCKS 1048576u
static inline uint64_t lzs_plan_batch_compress_group(const uint32_t *len_each, uint32_t len_all, uint64_t nblocks, uint64_t b0, uint64_t bound)
{
    uint64_t sum = 0, b = b0;
    for (; b < nblocks && b - b0 < LZS_PLAN_BC_GROUP_MAX_BLOCKS; b++) {
        const uint64_t len = len_each ? len_each[b] : len_all;
        if (b > b0 && sum + len > bound) break;
        sum += len;
    }
    return b - b0;
}

/* A block of len bytes in segments of seg: one for every seg bytes begun, and one for a block without a byte (it carries the
 * block's end marker). */
static inline uint64_t lzs_plan_batch_compress_nseg(uint32_t len, uint32_t seg) { return len ? ((uint64_t)len + seg - 1u) / seg : 1u; }

/* The segment table of the blocks b0 .. b0 + nb - 1: for every segment the block it belongs to, counted from b0, and where in
 * the block it starts.  seg_block, seg_start NULL: only counted.  Returns the number of segments. */
static inline uint64_t lzs_plan_batch_compress_segments(uint32_t *seg_block, uint32_t *seg_start, const uint32_t *len_each, uint32_t len_all,
                                                        uint64_t b0, uint64_t nb, uint32_t seg)
{
    uint64_t k = 0;
    for (uint64_t b = 0; b < nb; b++) {
        const uint32_t len = len_each ? len_each[b0 + b] : len_all;
        const uint64_t ns = lzs_plan_batch_compress_nseg(len, seg);
        for (uint64_t j = 0; j < ns; j++, k++)
            if (seg_block) { seg_block[k] = (uint32_t)b; seg_start[k] = (uint32_t)(j * seg); }
    }
    return k;
}

#endif
