/*
 * lzs_batch_compress.c -- a batch of blocks in device memory compressed with its lengths on the host
 * (include/lzs/lzs_batch.h: lzs_compress_batch_device_sync).
 *
 * One workgroup a block (lzs_hip_launch_compress) is the right shape for many short blocks and the wrong one for a few long
 * ones: eight blocks use eight of the device's 1536 places, however long they are.  Those go by segments, as one long stream
 * does (lzs_stream.c: stream_compress_piece()), only over all blocks at once: every block is cut into segments of one size, one
 * workgroup each (lzs_compress_segments_batch_kernel); the entry rounds run over the segments of all blocks in one launch a
 * round; a block's first segment is entered at 0 and every other where its predecessor's last token ended; the bit offsets are
 * a prefix sum that restarts with every block; one stitch shifts every slot into its block's output and ends every block with
 * its marker.  Same bytes as a workgroup a block produces.
 *
 * A file of its own: the sanitizer programs of tests/cpu_shim link lzs_host.c and lzs_stream.c against a CPU shim that has not
 * got the two launchers.
 */
#include "lzs_internal.h"
#include "lzs_launch_plan.h"

/* LZS_BATCH_COMPRESS_ROUTE=1|workgroups, 2|segments (development: the tests and the sweep force either route); 0: not set, or
 * another word.  Read at every call, as LZS_SIZE_ROUTE is (lzs_size_stream.c). */
static int batch_compress_route_forced(void)
{
    const char *v = getenv("LZS_BATCH_COMPRESS_ROUTE");
    return !v ? 0 : (!strcmp(v, "1") || !strcmp(v, "workgroups")) ? 1 : (!strcmp(v, "2") || !strcmp(v, "segments")) ? 2 : 0;
}

LZS_HIDDEN uint32_t settle_compress_entries_batch(uint32_t *entry, uint8_t *dirty, const uint32_t *exits, const uint32_t *seg_start,
                                                  uint32_t nseg)
{
    uint32_t ndirty = 0;
    for (uint32_t k = 0; k < nseg; k++) {
        dirty[k] = seg_start[k] != 0 && exits[k - 1] != entry[k];
        if (dirty[k]) { entry[k] = exits[k - 1]; ndirty++; }
    }
    return ndirty;
}

/* The blocks and the segments of one group as the two kernels see them.  Host side (pinned) and device side in the same order:
 * 64-bit tables first, then the words, then the flags; what never changes after the cutting -- blk_at .. blk_len -- lies together
 * and travels in one copy. */
typedef struct {
    uint32_t seg, nseg, nb;
    size_t   slot_stride;
    uint64_t *nbits, *bit_at, *blk_at;     uint32_t *seg_block, *seg_start, *blk_len, *entry, *exits;           uint8_t *dirty;
    uint64_t *d_nbits, *d_bit_at, *d_blk_at; uint32_t *d_seg_block, *d_seg_start, *d_blk_len, *d_entry, *d_exit; uint8_t *d_dirty;
    void     *d_slots;
} bseg_table_t;
static size_t bsegtab_bytes(size_t nseg, size_t nb) { return nseg * (2 * 8 + 4 * 4 + 1) + nb * (8 + 4) + 64; }

static void bsegtab_lay_out(bseg_table_t *t, void *h, void *d)
{
    const size_t n = t->nseg, nb = t->nb;
    t->nbits = (uint64_t *)h; t->bit_at = t->nbits + n; t->blk_at = t->bit_at + n;
    t->seg_block = (uint32_t *)(t->blk_at + nb); t->seg_start = t->seg_block + n; t->blk_len = t->seg_start + n;
    t->entry = t->blk_len + nb; t->exits = t->entry + n; t->dirty = (uint8_t *)(t->exits + n);
    t->d_nbits = (uint64_t *)d; t->d_bit_at = t->d_nbits + n; t->d_blk_at = t->d_bit_at + n;
    t->d_seg_block = (uint32_t *)(t->d_blk_at + nb); t->d_seg_start = t->d_seg_block + n; t->d_blk_len = t->d_seg_start + n;
    t->d_entry = t->d_blk_len + nb; t->d_exit = t->d_entry + n; t->d_dirty = (uint8_t *)(t->d_exit + n);
}
static size_t bsegtab_fixed_bytes(const bseg_table_t *t) { return (size_t)((uint8_t *)t->entry - (uint8_t *)t->blk_at); }

/* The entry rounds over all blocks of the group: every segment entered at its own start, then those whose predecessor in the
 * same block ended elsewhere again from there, until all agree; then the bit counts are fetched. */
static int batch_entry_rounds(bseg_table_t *t, void *stream, const char *who, const void *d_in, double *t0)
{
    const int debug = lzs_env()->stream_debug;
    const uint32_t nseg = t->nseg;
    for (uint32_t k = 0; k < nseg; k++) { t->entry[k] = t->exits[k] = t->seg_start[k]; t->dirty[k] = 1; t->nbits[k] = 0; }
    for (uint32_t round = 0, ndirty = nseg; ndirty; round++) {
        HIP_TRY_RET(lzs_hip_h2d(t->d_entry, t->entry, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
        HIP_TRY_RET(lzs_hip_h2d(t->d_dirty, t->dirty, nseg, stream), "hipMemcpy H2D");
        HIP_TRY_RET(lzs_hip_launch_compress_segments_batch(t->d_slots, t->slot_stride, d_in, t->d_blk_at, t->d_blk_len, t->d_seg_block,
                                                           t->d_seg_start, t->seg, nseg, t->d_entry, t->d_dirty, t->d_exit, t->d_nbits,
                                                           NULL, 0, 0, NULL, stream), who);
        HIP_TRY_RET(lzs_hip_d2h(t->exits, t->d_exit, sizeof(uint32_t) * nseg, stream), "hipMemcpy D2H");
        HIP_TRY_RET(lzs_hip_stream_sync(stream), "hipStreamSynchronize");
        const uint32_t was = ndirty;
        ndirty = settle_compress_entries_batch(t->entry, t->dirty, t->exits, t->seg_start, nseg);
        if (debug) { const double t1 = now_ms(); fprintf(stderr, "liblzs stream: round %u compressed %u segments in %.2f ms; %u to redo\n", round, was, t1 - *t0, ndirty); *t0 = t1; }
    }
    HIP_TRY_RET(lzs_hip_d2h(t->nbits, t->d_nbits, sizeof(uint64_t) * nseg, stream), "hipMemcpy D2H");
    HIP_TRY_RET(lzs_hip_stream_sync(stream), "hipStreamSynchronize");
    return LZS_OK;
}

/* Where every segment's bits go -- a prefix sum of the bit counts that restarts with every block -- and what every block gives:
 * out_len[b] = its stream with the marker, cut at the capacity.  The outputs are cleared as far as any of them is written, the
 * stitch shifts the slots into place, and the segments whose bits did not fit their slot are compressed once more, ORed in. */
static int batch_place_and_stitch(bseg_table_t *t, void *stream, const char *who, void *d_out, size_t out_stride, uint32_t cap32,
                                  uint32_t *out_len, const void *d_in, double *t0)
{
    const uint32_t nseg = t->nseg;
    const uint64_t cap4 = ((uint64_t)cap32 + 3u) & ~(uint64_t)3u;
    uint64_t at = 0, widest = 0;
    uint32_t nbig = 0;
    for (uint32_t k = 0; k < nseg; k++) {
        if (t->seg_start[k] == 0) at = 0;
        t->bit_at[k] = at;
        at += t->nbits[k];
        if (k + 1 == nseg || t->seg_start[k + 1] == 0) {       /* the block's last segment: the end marker, padded to a byte */
            const uint64_t bytes = (at + 9 + 7) / 8, words = (bytes + 3u) & ~(uint64_t)3u;
            out_len[t->seg_block[k]] = bytes > cap32 ? cap32 : (uint32_t)bytes;
            if (words > widest) widest = words;
        }
        t->dirty[k] = t->nbits[k] > 8u * (uint64_t)t->slot_stride;
        nbig += t->dirty[k];
    }
    if (widest > cap4) widest = cap4;
    HIP_TRY_RET(lzs_hip_h2d(t->d_bit_at, t->bit_at, sizeof(uint64_t) * nseg, stream), "hipMemcpy H2D");
    HIP_TRY_RET(lzs_hip_memset_rows(d_out, out_stride, 0, (size_t)widest, t->nb, stream), "hipMemset");
    HIP_TRY_RET(lzs_hip_launch_stitch_segments_batch(d_out, out_stride, cap32, t->d_slots, t->slot_stride, t->d_bit_at, t->d_nbits,
                                                     t->d_seg_block, t->d_seg_start, t->d_blk_len, t->seg, nseg, stream), who);
    if (nbig) {
        HIP_TRY_RET(lzs_hip_h2d(t->d_dirty, t->dirty, nseg, stream), "hipMemcpy H2D");
        HIP_TRY_RET(lzs_hip_launch_compress_segments_batch(t->d_slots, t->slot_stride, d_in, t->d_blk_at, t->d_blk_len, t->d_seg_block,
                                                           t->d_seg_start, t->seg, nseg, t->d_entry, t->d_dirty, t->d_exit, t->d_nbits,
                                                           d_out, out_stride, cap32, t->d_bit_at, stream), who);
    }
    HIP_TRY_RET(lzs_hip_stream_sync(stream), "hipStreamSynchronize");      /* (the tables are the next group's) */
    if (lzs_env()->stream_debug) { const double t1 = now_ms(); fprintf(stderr, "liblzs stream: stitch %.2f ms\n", t1 - *t0); *t0 = t1; }
    return LZS_OK;
}

/* The batch by segments, group by group. */
static int batch_compress_segments(const char *who, void *d_out, size_t out_stride, uint32_t cap32, uint32_t *out_len, const void *d_in,
                                   size_t in_stride, const uint32_t *in_len_each, uint32_t in_len, size_t nblocks, size_t total_in)
{
    bseg_table_t t = { .seg = stream_seg(total_in) };
    t.slot_stride = round16(LZS_COMPRESSED_MAX((size_t)t.seg));
    const int debug = lzs_env()->stream_debug;
    int e = 0, rc = LZS_OK;
    staging_t *st = NULL;
    void *tables = NULL, *d_aux = NULL;
    double t0 = debug ? now_ms() : 0;
    for (size_t b0 = 0, nb; b0 < nblocks; b0 += nb) {
        nb = (size_t)lzs_plan_batch_compress_group(in_len_each, in_len, nblocks, b0, LZS_BLOCK_MAX);
        const uint64_t nseg = lzs_plan_batch_compress_segments(NULL, NULL, in_len_each, in_len, b0, nb, t.seg);
        t.nb = (uint32_t)nb; t.nseg = (uint32_t)nseg;
        if ((rc = stream_call_begins(who, bsegtab_bytes(nseg, nb), &st, &tables)) != LZS_OK) goto done;
        void *stream = st->stream;
        e = staging_reserve(st, BUF_AUX, bsegtab_bytes(nseg, nb), &d_aux);
        if (!e) e = staging_reserve(st, BUF_KEEP, t.slot_stride * nseg + 64, &t.d_slots);
        if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto done; }
        bsegtab_lay_out(&t, tables, d_aux);
        /* ---- cutting: the group's input is counted from its first block, so the offsets are the group's own */
        lzs_plan_batch_compress_segments(t.seg_block, t.seg_start, in_len_each, in_len, b0, nb, t.seg);
        for (size_t b = 0; b < nb; b++) { t.blk_at[b] = (uint64_t)b * in_stride; t.blk_len[b] = in_len_each ? in_len_each[b0 + b] : in_len; }
        const uint8_t *g_in = (const uint8_t *)d_in + b0 * in_stride;
        uint8_t *g_out = (uint8_t *)d_out + b0 * out_stride;
        HIP_TRY_OR(done, lzs_hip_h2d(t.d_blk_at, t.blk_at, bsegtab_fixed_bytes(&t), stream), "hipMemcpy H2D");
        if (debug) fprintf(stderr, "liblzs stream: batch of %zu blocks from %zu, %u segments of %u\n", nb, b0, t.nseg, t.seg);
        if ((rc = batch_entry_rounds(&t, stream, who, g_in, &t0)) != LZS_OK) goto done;
        if ((rc = batch_place_and_stitch(&t, stream, who, g_out, out_stride, cap32, out_len + b0, g_in, &t0)) != LZS_OK) goto done;
    }
done:
    stream_call_ends(0, rc, 1, who, NULL);
    return rc;
}

/* The batch by workgroups: the lengths in, one launch, the lengths out. */
static int batch_compress_workgroups(const char *who, void *d_out, size_t out_stride, uint32_t cap32, uint32_t *out_len, const void *d_in,
                                     size_t in_stride, const uint32_t *in_len_each, uint32_t in_len, size_t nblocks)
{
    int e = 0, rc;
    void *d_len = NULL, *d_in_len = NULL, *tables = NULL;
    staging_t *st = NULL;
    if ((rc = stream_call_begins(who, 64, &st, &tables)) != LZS_OK) goto done;
    void *stream = st->stream;
    e = staging_reserve(st, BUF_LEN, sizeof(uint32_t) * nblocks, &d_len);
    if (!e && in_len_each) e = staging_reserve(st, BUF_INLEN, sizeof(uint32_t) * nblocks, &d_in_len);
    if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto done; }
    if (in_len_each) HIP_TRY_OR(done, lzs_hip_h2d(d_in_len, in_len_each, sizeof(uint32_t) * nblocks, stream), "hipMemcpy H2D");
    HIP_TRY_OR(done, lzs_hip_launch_compress(d_out, out_stride, cap32, (uint32_t *)d_len, d_in, in_stride, (const uint32_t *)d_in_len, in_len,
                                             (uint32_t)nblocks, stream), who);
    HIP_TRY_OR(done, lzs_hip_d2h(out_len, d_len, sizeof(uint32_t) * nblocks, stream), "hipMemcpy D2H");
    HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
done:
    stream_call_ends(0, rc, 1, who, NULL);
    return rc;
}

int lzs_compress_batch_device_sync(void *d_out, size_t out_stride, size_t out_cap, uint32_t *out_len,
                                   const void *d_in, size_t in_stride, const uint32_t *in_len_each,
                                   size_t in_len, size_t nblocks)
{
    const char *who = "lzs_compress_batch_device_sync";
    if (nblocks == 0) return LZS_OK;
    if (!out_len) return fail(LZS_E_ARG, "%s: out_len is NULL", who);
    if (!d_in && in_len) return fail(LZS_E_ARG, "%s: input is NULL", who);
    if (in_len > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "%s: block of %zu bytes exceeds LZS_BLOCK_MAX", who, in_len);
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    if (!d_out && out_cap) return fail(LZS_E_ARG, "%s: output is NULL", who);
    size_t total_in = 0, longest = 0;
    for (size_t b = 0; b < nblocks; b++) {
        const size_t len = in_len_each ? in_len_each[b] : in_len;
        total_in += len;
        if (len > longest) longest = len;
    }
    if (longest > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "%s: block exceeds LZS_BLOCK_MAX", who);
    if (!d_in && longest) return fail(LZS_E_ARG, "%s: input is NULL", who);
    const int rc = require_device();
    if (rc != LZS_OK) return rc;
    const uint32_t cap32 = out_cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)out_cap;
    if (lzs_plan_batch_compress_route(nblocks, total_in, longest, cap32, out_stride, (uintptr_t)d_out, batch_compress_route_forced()) ==
        LZS_BATCH_COMPRESS_BY_SEGMENTS)
        return batch_compress_segments(who, d_out, out_stride, cap32, out_len, d_in, in_stride, in_len_each, (uint32_t)in_len, nblocks, total_in);
    return batch_compress_workgroups(who, d_out, out_stride, cap32, out_len, d_in, in_stride, in_len_each, (uint32_t)in_len, nblocks);
}
