/*
 * lzs_stream.c -- one stream (or a small batch of blocks) spread over the whole device: the host
 * side of the segment compressor (lzs_compress_segments_kernel + lzs_stitch_segments_kernel,
 * DESIGN.md 3.5) and of the many-wavefront decompressor (scan / decode / resolve),
 * including their "piece" forms that the incremental interface drives.
 */
#include "lzs_internal.h"

/* (the clock of the LZS_STREAM_DEBUG lines) */
LZS_HIDDEN double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

/* ------------------------------------------------ how a one-stream call begins and ends, compressing or decompressing */
/* It begins with the device, this thread's staging, `tab_bytes` of its pinned memory for the per-segment tables (they travel every
 * round) and its stream.  LZS_OK or the code reported. */
LZS_HIDDEN int stream_call_begins(const char *who, size_t tab_bytes, staging_t **st, void **tables)
{
    tls_error[0] = 0;
    if (require_device() != LZS_OK) return LZS_E_HIP;
    if (!(*st = staging_get()) || !(*tables = staging_host_tables(*st, tab_bytes))) return fail(LZS_E_NOMEM, "%s: out of host memory", who);
    if (!(*st)->stream) HIP_TRY_RET(lzs_hip_stream_create(&(*st)->stream), "hipStreamCreate");
    return LZS_OK;
}

/* in on the host: the prefix of a piece (pre bytes, or none) and the caller's input behind it make the n bytes at d_in */
LZS_HIDDEN int stream_copy_in(void *d_in, const uint8_t *prefix, size_t pre, const uint8_t *in, size_t n, void *stream)
{
    if (pre) HIP_TRY_RET(lzs_hip_h2d(d_in, prefix, pre, stream), "hipMemcpy H2D");
    HIP_TRY_RET(lzs_hip_h2d((uint8_t *)d_in + pre, in, n - pre, stream), "hipMemcpy H2D");
    return LZS_OK;
}

/* It ends: a failed one (rc) gives 0 bytes, says so on stderr (host buffers: the reference's calls have no other way) and leaves
 * nothing of its own in flight; the thread's staging is trimmed to what it may keep. */
LZS_HIDDEN size_t stream_call_ends(size_t result, int rc, int dev, const char *who, int *status)
{
    staging_t *st = staging_get();
    if (rc != LZS_OK) {
        if (!dev) fprintf(stderr, "liblzs: %s failed: %s\n", who, tls_error);
        if (st && st->stream) lzs_hip_stream_sync(st->stream);
        /* (the runtime keeps a failed allocation as its "last error" until somebody fetches it, and every launcher returns the
         * last error after its launch: fetched here, or this thread's next call reports this out-of-memory as its own) */
        if (rc == LZS_E_NOMEM) lzs_hip_clear_error();
    }
    if (st) staging_trim(st);
    if (status) *status = rc;
    return rc != LZS_OK ? 0 : result;
}

/* ------------------------------------------------ one long stream on the whole device */
/* lzs_compress() of a buffer too long for one workgroup to be worth waiting for.  The search is a
 * pure function of (input, position), so the stream is cut into segments (stream_seg()), one workgroup
 * each (lzs_compress_segments_kernel), every one writing its bits into a slot of its own.  What a
 * segment cannot know by itself is where its first token starts -- the last token of the segment
 * before usually reaches a few bytes into it -- and at which bit its output begins.  So: (1)
 * every segment is compressed entered at its own start and reports where its last token ends;
 * (2) segments whose predecessor ended elsewhere are compressed again from there, until all
 * entries agree (the greedy parses from two nearby entries merge after a few tokens, so a second
 * round changes almost no exit; a long run simply skips the segments it covers); (3) prefix sum
 * of the bit counts on the host; (4) lzs_stitch_segments_kernel shifts every slot to its bit
 * offset in the zeroed output and appends the end marker.  Same bytes as one workgroup (or the
 * reference) produces. */
#define STREAM_SEG_MAX 65536u

/* Segment size for a stream of n bytes: 64 KiB for long streams, much smaller for shorter ones so
 * that they too spread over the device -- a workgroup alone on a CU takes 15 us per KiB, and every
 * segment pays for a 2.2 KB warm-up of its chains (HASH and CHAIN only).  Measured in round 3 (text,
 * host buffers, ms; tests/dev/seg_small_sweep.py, seg_mid_sweep.py):
 *            one workgroup   512 B   1 KiB   2 KiB   4 KiB   16 KiB   64 KiB
 *     8 KiB      0.167       0.127   0.141   0.169   0.227
 *    64 KiB      0.971       0.138   0.151   0.184   0.248
 *   256 KiB      3.749       0.169   0.178   0.212   0.275
 *     1 MiB     15.08        0.357   0.340   0.358   0.417   0.777    1.233
 *     4 MiB                          0.985   0.916   0.925   1.230    2.684
 *    16 MiB                          4.032   3.854   3.785   3.961    5.132
 * (round 2 used 4 KiB up to 2 MiB: 64 KiB in 0.29 ms).  A short piece of the incremental interface, whose block collects
 * ~10 KiB, is all latency too: at 512-byte calls 41 MB/s in 4 KiB segments, 62 in 1 KiB, 67 in 512 B. */
LZS_HIDDEN uint32_t stream_seg(size_t n)
{
    const uint32_t v = lzs_env()->stream_seg;
    size_t seg = v ? v
               : n <= ((size_t)256 << 10) ? 512u : n <= ((size_t)1 << 20) ? 1024u : n <= ((size_t)4 << 20) ? 2048u
               : n <= ((size_t)32 << 20) ? 4096u : (n / 512u + 4095u) & ~(size_t)4095u;
    if (seg < 256u) seg = 256u;
    if (seg > STREAM_SEG_MAX) seg = STREAM_SEG_MAX;
    return (uint32_t)(seg & ~(size_t)63u);
}

/* The segments of one stream as the segment compressor and the stitch see them: segment k is bytes [k seg, (k + 1) seg), and its
 * bits go to slot k of d_slots (slot_stride bytes each) first.  A segment's share of either side: the bits it gave and the bit at
 * which they begin in the output (64-bit), where it is entered and where its last token ends, the open-match report of a piece
 * (two words: offset, start), a flag. */
typedef struct {
    uint32_t seg, nseg;
    size_t   slot_stride;
    uint64_t *nbits, *bit_at;   uint32_t *entry, *exits, *open;     uint8_t *dirty;         /* host side, in this order */
    uint64_t *d_bit_at, *d_nbits; uint32_t *d_entry, *d_exit, *d_open; uint8_t *d_dirty;    /* device side, in this order */
    void     *d_slots;
} cseg_table_t;
enum { CSEG_BYTES = 2 * 8 + 2 * 4 + 8 + 1 };
static size_t csegtab_host_bytes(uint32_t nseg) { return ((size_t)nseg + 16u) * CSEG_BYTES; }
static size_t csegtab_dev_bytes(uint32_t nseg) { return (size_t)nseg * CSEG_BYTES + 64; }

/* (t->nseg is set; h: csegtab_host_bytes() of pinned memory, d: csegtab_dev_bytes() of device memory) */
static void csegtab_lay_out(cseg_table_t *t, void *h, void *d)
{
    const size_t n = t->nseg;
    t->nbits = (uint64_t *)h; t->bit_at = t->nbits + n; t->entry = (uint32_t *)(t->bit_at + n); t->exits = t->entry + n; t->open = t->exits + n;
    t->dirty = (uint8_t *)(t->open + 2 * n);
    t->d_bit_at = (uint64_t *)d; t->d_nbits = t->d_bit_at + n; t->d_entry = (uint32_t *)(t->d_nbits + n); t->d_exit = t->d_entry + n; t->d_open = t->d_exit + n;
    t->d_dirty = (uint8_t *)(t->d_open + 2 * n);
}

/* A piece that begins inside a long match (pc->ext_off): its length nibbles first, behind bit *total of d_out (d_exit as scratch).
 * *c_first: where the tokens start behind them; *ext_now: the match is still open -- it covers all the data there is; *total
 * grows by the bits written.  LZS_OK or the error reported. */
static int resume_open_match(const cseg_table_t *t, const piece_t *pc, void *d_out, const void *d_in, uint32_t n, void *stream,
                             const char *who, uint32_t *c_first, uint32_t *ext_now, uint64_t *total)
{
    uint32_t res[4];
    /* (pc->stop: the data is known to end at n -- the run is closed like in a last piece, only the marker waits) */
    HIP_TRY_RET(lzs_hip_launch_extend_resume(d_out, pc->bit0, d_in, n, pc->c0, pc->ext_off, pc->last || pc->stop, t->d_exit, stream), who);
    HIP_TRY_RET(lzs_hip_d2h(res, t->d_exit, sizeof(res), stream), "hipMemcpy D2H");
    HIP_TRY_RET(lzs_hip_stream_sync(stream), "hipStreamSynchronize");
    *c_first = res[0];
    *ext_now = res[1] ? pc->ext_off : 0;
    *total += ((uint64_t)res[3] << 32) | res[2];
    return LZS_OK;
}

/* After a round: a segment is entered where the one before stopped (segment 0 where the call says), and those for which that is
 * news are compressed again.  Host code only.  Returns how many are dirty now. */
LZS_HIDDEN uint32_t settle_compress_entries(uint32_t *entry, uint8_t *dirty, const uint32_t *exits, uint32_t nseg)
{
    uint32_t ndirty = 0;
    dirty[0] = 0;
    for (uint32_t k = 1; k < nseg; k++) {
        dirty[k] = exits[k - 1] != entry[k];
        if (dirty[k]) { entry[k] = exits[k - 1]; ndirty++; }
    }
    return ndirty;
}

/* The entry rounds: every segment entered at its own start (no token starts before c_first), then those whose predecessor ended
 * elsewhere again from there, until all agree.  `lim`: no token starts at or behind it; `open_info`: a piece wants the open-match
 * reports; `ext_now`: a match still open after its nibbles covers all the data -- the tables are set for the stages behind, but
 * this piece has no tokens and no round.  Then the bit counts (and reports) are fetched.  LZS_OK or the error reported. */
static int entry_rounds(cseg_table_t *t, void *stream, const char *who, const void *d_in, uint32_t n, uint32_t c_first, uint32_t lim,
                        int open_info, uint32_t ext_now, double *t0)
{
    const int debug = lzs_env()->stream_debug;
    const uint32_t nseg = t->nseg;
    for (uint32_t k = 0; k < nseg; k++) {
        t->entry[k] = k * t->seg > c_first ? k * t->seg : c_first;
        t->dirty[k] = 1; t->exits[k] = t->entry[k]; t->nbits[k] = 0; t->open[2 * k] = t->open[2 * k + 1] = 0;
    }
    for (uint32_t round = 0, ndirty = ext_now ? 0 : nseg; ndirty; round++) {
        HIP_TRY_RET(lzs_hip_h2d(t->d_entry, t->entry, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
        HIP_TRY_RET(lzs_hip_h2d(t->d_dirty, t->dirty, nseg, stream), "hipMemcpy H2D");
        HIP_TRY_RET(lzs_hip_launch_compress_segments(t->d_slots, t->slot_stride, d_in, n, t->seg, nseg, t->d_entry, t->d_dirty, t->d_exit, t->d_nbits,
                                                     NULL, NULL, lim, open_info ? t->d_open : NULL, stream), who);
        HIP_TRY_RET(lzs_hip_d2h(t->exits, t->d_exit, sizeof(uint32_t) * nseg, stream), "hipMemcpy D2H");
        HIP_TRY_RET(lzs_hip_stream_sync(stream), "hipStreamSynchronize");
        const uint32_t was = ndirty;
        ndirty = settle_compress_entries(t->entry, t->dirty, t->exits, nseg);
        if (debug) { const double t1 = now_ms(); fprintf(stderr, "liblzs stream: round %u compressed %u segments in %.2f ms; %u to redo\n", round, was, t1 - *t0, ndirty); *t0 = t1; }
    }
    if (ext_now) return LZS_OK;
    /* what every segment gave */
    HIP_TRY_RET(lzs_hip_d2h(t->nbits, t->d_nbits, sizeof(uint64_t) * nseg, stream), "hipMemcpy D2H");
    if (open_info) HIP_TRY_RET(lzs_hip_d2h(t->open, t->d_open, sizeof(uint32_t) * 2 * nseg, stream), "hipMemcpy D2H");
    HIP_TRY_RET(lzs_hip_stream_sync(stream), "hipStreamSynchronize");
    return LZS_OK;
}

/* The last token of a piece that is not the last may be a match that reaches the end of the data so far (c_exit >= n, in a piece
 * that had tokens: n > c_first): it may go on in the next piece.  Its full groups of 15 stand; the closing nibble is taken back
 * and the bytes it covered wait for more data (state COMPRESS_EXTENDED, :750-758).  Host code only.  0: no such match.  1: four
 * bits less for the last segment that reports an open match -- nbits[] has changed --, *c_exit and *ext_exit say from where and
 * at which offset the match goes on.  -1: no segment reports one, or that one has no nibble to give. */
LZS_HIDDEN int open_match_take_back(const uint32_t *open, uint64_t *nbits, uint32_t nseg, uint32_t n, uint32_t c_first, uint32_t *c_exit,
                                    uint32_t *ext_exit)
{
    if (*c_exit < n || n <= c_first) return 0;
    uint32_t k = nseg;
    while (k > 0 && open[2 * (k - 1)] == 0) k--;
    if (k == 0 || nbits[k - 1] < 4) return -1;
    const uint32_t off = open[2 * (k - 1)], start = open[2 * (k - 1) + 1];
    nbits[k - 1] -= 4;
    *c_exit = n - (n - start - 8u) % 15u;
    *ext_exit = off;
    return 1;
}

/* Where every segment's bits go -- the prefix sum of the bit counts from bit *total on, which it leaves at the end of them -- and
 * the stitch that shifts the slots there (none if the piece had no tokens: ext_now).  Segments whose bits did not fit their slot
 * (a match running on for more than ~120 KB past the segment) are compressed once more, ORed straight into place. */
static int place_and_stitch(cseg_table_t *t, void *stream, const char *who, void *d_out, const void *d_in, uint32_t n, uint32_t lim,
                            uint32_t ext_now, int end_marker, uint64_t *total, double *t0)
{
    const uint32_t nseg = t->nseg;
    uint32_t nbig = 0;
    for (uint32_t k = 0; k < nseg; k++) { t->bit_at[k] = *total; *total += t->nbits[k]; }
    HIP_TRY_RET(lzs_hip_h2d(t->d_bit_at, t->bit_at, sizeof(uint64_t) * nseg, stream), "hipMemcpy H2D");
    if (!ext_now)
        HIP_TRY_RET(lzs_hip_launch_stitch_segments(d_out, t->d_slots, t->slot_stride, t->d_bit_at, t->d_nbits, nseg, end_marker, stream), who);
    for (uint32_t k = 0; k < nseg; k++) { t->dirty[k] = t->nbits[k] > 8u * (uint64_t)t->slot_stride; nbig += t->dirty[k]; }
    if (nbig) {
        HIP_TRY_RET(lzs_hip_h2d(t->d_dirty, t->dirty, nseg, stream), "hipMemcpy H2D");
        HIP_TRY_RET(lzs_hip_launch_compress_segments(t->d_slots, t->slot_stride, d_in, n, t->seg, nseg, t->d_entry, t->d_dirty, t->d_exit, t->d_nbits,
                                                     d_out, t->d_bit_at, lim, NULL, stream), who);
    }
    if (lzs_env()->stream_debug) { lzs_hip_stream_sync(stream); const double t1 = now_ms(); fprintf(stderr, "liblzs stream: stitch %.2f ms\n", t1 - *t0); *t0 = t1; }
    return LZS_OK;
}

/* in/out on the host (dev == 0: staged through this thread's device buffers) or on the device.
 * With pc, a piece of a stream for lzs_compress_incremental(): the data is `prefix` (history and the
 * bytes the call before could not encode yet) followed by `in`; encoding starts at c0, inside a
 * long match if ext_off is set, at bit bit0 of the first output byte (whose earlier bits are in
 * `first`).  Unless `last`, it stops where the tokens are no longer decided by the data so far. */
LZS_HIDDEN size_t stream_compress_piece(uint8_t *out, size_t cap, const uint8_t *in, size_t n, int dev, int *status, piece_t *pc)
{
    const char *who = pc ? "lzs_compress_incremental" : dev ? "lzs_compress_stream_device" : "lzs_compress";
    cseg_table_t t = { .seg = stream_seg(n) };
    const uint32_t nseg = t.nseg = n ? (uint32_t)((n + t.seg - 1) / t.seg) : 1u;
    t.slot_stride = (LZS_COMPRESSED_MAX((size_t)t.seg) + 15u) & ~(size_t)15u;
    const size_t worst = LZS_COMPRESSED_MAX(n - (pc ? pc->c0 : 0)) + 8;
    const int end_marker = !pc || pc->last, debug = lzs_env()->stream_debug;      /* LZS_STREAM_DEBUG: stage times on stderr */
    uint32_t lim = end_marker ? (uint32_t)n : (n > LZS_MAX_LOOK_AHEAD_LEN ? (uint32_t)n - LZS_MAX_LOOK_AHEAD_LEN : 0u);
    if (pc && !pc->last && pc->stop) lim = pc->stop < n ? pc->stop : (uint32_t)n;       /* (the caller vouches that the data ends at n) */
    uint32_t c_first = pc ? pc->c0 : 0, ext_now = 0;
    uint64_t total = pc ? pc->bit0 : 0;
    size_t result = 0;
    int e = 0, rc, took = 0;
    void *d_in = NULL, *d_out = NULL, *d_aux = NULL, *tables = NULL;
    staging_t *st = NULL;
    /* ---- set-up: the stream and its output on the device, the segment table; in, and the output cleared */
    if ((rc = stream_call_begins(who, csegtab_host_bytes(nseg), &st, &tables)) != LZS_OK) goto done;
    void *stream = st->stream;
    if (dev) { d_in = (void *)in; d_out = out; } else e = staging_reserve(st, BUF_IN, n + 64, &d_in);
    if (!e && !dev) e = staging_reserve(st, BUF_OUT, worst + 1024, &d_out);
    if (!e) e = staging_reserve(st, BUF_AUX, csegtab_dev_bytes(nseg), &d_aux);
    if (!e) e = staging_reserve(st, BUF_KEEP, t.slot_stride * nseg + 64, &t.d_slots);
    if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto done; }
    csegtab_lay_out(&t, tables, d_aux);
    double t0 = debug ? now_ms() : 0, t1;
    if (!dev && (rc = stream_copy_in(d_in, pc ? pc->prefix : NULL, pc ? pc->prefix_len : 0, in, n, stream)) != LZS_OK) goto done;
    /* (a caller's device buffer is cleared only as far as it was promised: LZS_COMPRESSED_MAX(n) + 1024) */
    HIP_TRY_OR(done, lzs_hip_memset(d_out, 0, dev && worst + 1024 > cap ? cap : worst + 1024, stream), "hipMemset");
    if (debug) { lzs_hip_stream_sync(stream); t1 = now_ms(); fprintf(stderr, "liblzs stream: %zu B, %u segments; H2D + memset %.2f ms\n", n, nseg, t1 - t0); t0 = t1; }
    /* ---- the tokens: behind the bits of the call before, [the nibbles of the match it left open], the entry rounds */
    if (pc && pc->bit0) HIP_TRY_OR(done, lzs_hip_h2d(d_out, &pc->first, 1, stream), "hipMemcpy H2D");
    if (pc && pc->ext_off && (rc = resume_open_match(&t, pc, d_out, d_in, (uint32_t)n, stream, who, &c_first, &ext_now, &total)) != LZS_OK) goto done;
    if ((rc = entry_rounds(&t, stream, who, d_in, (uint32_t)n, c_first, lim, pc != NULL, ext_now, &t0)) != LZS_OK) goto done;
    if (pc) {
        pc->c_exit = ext_now ? c_first : t.exits[nseg - 1];
        pc->ext_exit = ext_now;
        if (!pc->last && !pc->stop && !ext_now) took = open_match_take_back(t.open, t.nbits, nseg, (uint32_t)n, c_first, &pc->c_exit, &pc->ext_exit);
    }
    if (took < 0) { rc = fail(LZS_E_HIP, "%s: inconsistent state from the device (piece of %zu bytes from %u ends at %u, no open match reported)", who, n, c_first, pc->c_exit); goto done; }
    if (took > 0) HIP_TRY_OR(done, lzs_hip_h2d(t.d_nbits, t.nbits, sizeof(uint64_t) * nseg, stream), "hipMemcpy H2D");
    if ((rc = place_and_stitch(&t, stream, who, d_out, d_in, (uint32_t)n, lim, ext_now, end_marker, &total, &t0)) != LZS_OK) goto done;
    if (pc) pc->nbits = total;
    result = (size_t)((total + (end_marker ? 9 : 0) + 7) / 8);  /* (the end marker, padded to a byte; a piece: the last byte may be partial) */
    if (result > cap) result = cap;                            /* cut at the capacity, prefix unchanged */
    if (!dev) HIP_TRY_OR(done, lzs_hip_d2h(out, d_out, result, stream), "hipMemcpy D2H");
    HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
done:
    return stream_call_ends(result, rc, dev, who, status);
}

LZS_HIDDEN size_t stream_compress(uint8_t *out, size_t cap, const uint8_t *in, size_t n, int dev, int *status)
{
    return stream_compress_piece(out, cap, in, n, dev, status, NULL);
}

int lzs_compress_stream_device(void *d_out, size_t out_cap, size_t *out_len, const void *d_in, size_t in_len)
{
    if (!out_len) return fail(LZS_E_ARG, "lzs_compress_stream_device: out_len is NULL");
    *out_len = 0;
    if (!d_out || (!d_in && in_len)) return fail(LZS_E_ARG, "lzs_compress_stream_device: NULL buffer");
    if (((uintptr_t)d_out & 3u) != 0) return fail(LZS_E_ARG, "lzs_compress_stream_device: d_out is not 4-byte aligned");
    if (in_len == 0 || in_len > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "lzs_compress_stream_device: length must be 1..LZS_BLOCK_MAX");
    int rc = LZS_OK;
    *out_len = stream_compress((uint8_t *)d_out, out_cap, (const uint8_t *)d_in, in_len, 1, &rc);
    return rc;
}

/* Segment size for decompressing a stream of n compressed bytes: 4 KiB for long streams (1 GiB of
 * output, ms: text 53.7 / 51.8 / 53.9 at 2 / 4 / 8 KiB, high-entropy 56.1 / 51.8 / 51.1, low-entropy
 * 8.1 / 9.7 / 11.2 -- smaller segments scan and decode a little faster, and since the copies across
 * their borders are settled by chunks of segments their number costs little), smaller
 * for short ones so that they too are spread over many wavefronts (one wavefront decodes ~7 MB/s).
 * Measured (text, host buffers, ms; output size): 64 KiB 7.7 with one wavefront, 0.67 in 256-byte
 * segments; 256 KiB 30.8 / 1.0; 1 MiB 122.8 / 2.4 (6.3 in 8 KiB segments); 4 MiB 8.2 in 1 KiB
 * segments, 10.1 in 8 KiB ones. */
LZS_HIDDEN uint32_t stream_dec_seg(size_t n)
{
    const uint32_t v = lzs_env()->dec_seg;
    size_t seg = v ? v : (n / 2048u + 255u) & ~(size_t)255u;
    if (!v && seg > 4096u) seg = 4096u;
    const size_t most = lzs_hip_dec_segment_bytes();
    if (seg < 256u) seg = 256u;
    if (seg > most) seg = most;
    return (uint32_t)(seg & ~(size_t)63u);
}

/* (seg_table_t, the segments as SCAN, DECODE and RESOLVE see them: lzs_internal.h) */

/* (t->nseg is set; host: 5 words and 2 bytes a segment, with range tables 9 and 3; device: 4 words and 2 bytes, or 8 and 2, and 8 bytes) */
LZS_HIDDEN void segtab_lay_out(seg_table_t *t, uint32_t *h, uint32_t *d, int ranges)
{
    const size_t n = t->nseg;
    t->seen = h; t->entry = h + n; t->exits = h + 2 * n; t->count = h + 3 * n; t->start = h + 4 * n; h += 5 * n;
    t->d_entry = d; t->d_exit = d + n; t->d_count = d + 2 * n; t->d_start = d + 3 * n; d += 4 * n;
    if (ranges) {
        t->base = h; t->end = h + n; t->floor_ = h + 2 * n; t->limit = h + 3 * n; h += 4 * n;
        t->d_base = d; t->d_end = d + n; t->d_floor = d + 2 * n; t->d_limit = d + 3 * n; d += 4 * n;
    }
    t->dirty = (uint8_t *)h; t->ones = t->dirty + n; t->first = ranges ? t->ones + n : NULL;
    t->d_counters = d; t->d_dirty = (uint8_t *)(d + 2); t->d_ones = t->d_dirty + n;      /* counters: [0] bytes with an origin, [1] left open */
}

/* After a SCAN round: every segment is to be entered in the state in which the one before it left (a first segment in its
 * own), and those for which that is news are walked again.  Host code only.  Returns how many are dirty now; *host_made:
 * some exits / counts were worked out here, not on the device. */
LZS_HIDDEN uint32_t settle_entries(seg_table_t *t, int use_ones, int *host_made)
{
    const uint32_t seg = t->seg;
    uint32_t *entry = t->entry, *exits = t->exits, *count = t->count, *seen = t->seen;
    uint32_t ndirty = 0;
    int ended = 0, settled = 1;     /* settled: every segment of this stream before k has been walked from its final entry */
    *host_made = 0;
    for (uint32_t k = 0; k < t->nseg; k++) {
        if (t->dirty[k]) seen[k] = entry[k];                    /* exits[k], count[k] belong to this entry */
        t->dirty[k] = 0;
        if (t->first ? t->first[k] : k == 0) { ended = 0; settled = 1; continue; }
        uint32_t want = exits[k - 1];
        if (want & LZS_SEG_STOP) {
            /* end marker or end of input before k -- believed only from a settled walk: one that
             * was entered at a guessed bit reads end markers into the data now and then */
            if (settled) ended = 1; else want = entry[k];
        }
        if (ended) want = LZS_SEG_STOP;
        if (want != entry[k]) settled = 0;
        entry[k] = want;
        /* a segment behind the (current) end of the stream keeps what it reported for its last
         * entry: the end may turn out to be a misread of a walk that had not fallen in step */
        if (ended || want == seen[k]) continue;
        if (use_ones && ((want >> 8) & 1u) && (t->ones[k] == 2 || (t->ones[k] && (want & 3u) == 0))) {
            /* all 0xFF inside a running extension: nothing but nibbles of 15, one every 4 bits
             * from the cursor on (which is up to 20 bits in if the match token itself straddles
             * the border) for as long as they start inside the segment -- provided the last of
             * them is all ones too, which reaches up to 3 bits into the next segment unless the
             * cursor is a multiple of 4.  No need to walk it then. */
            const uint32_t r = want & 0xFFu;
            const uint32_t nibbles = (seg * 8u - r + 3u) / 4u;
            exits[k] = (want & ~0xFFu) | (r + 4u * nibbles - seg * 8u);
            count[k] = 15u * nibbles;
            seen[k] = want;
            *host_made = 1;
            continue;
        }
        t->dirty[k] = 1;
        ndirty++;
    }
    return ndirty;
}

/* The SCAN rounds: every segment entered at its first bit in the normal state (segment 0 of one stream: in `entry0`), then
 * those whose predecessor left in another state again, until all agree.  `n`: the stream's length (0 with range tables),
 * `in_extent`: the readable bytes at d_in, `d_marks`: what full walks leave for repeated ones.  LZS_OK or the error reported. */
LZS_HIDDEN int scan_rounds(seg_table_t *t, void *stream, const char *who, const void *d_in, uint32_t n, uint32_t in_extent,
                       uint32_t entry0, int concat, uint32_t *d_marks, double *t0)
{
    const lzs_env_t env = *lzs_env();
    const uint32_t nseg = t->nseg;
    uint32_t *again = NULL;
    int e = 0, rc = LZS_OK;
    for (uint32_t k = 0; k < nseg; k++) { t->entry[k] = 0; t->dirty[k] = 1; t->seen[k] = 0xFFFFFFFFu; }
    t->entry[0] = entry0;
    for (uint32_t round = 0, ndirty = nseg; ndirty; round++) {
        HIP_TRY_OR(done, lzs_hip_h2d(t->d_entry, t->entry, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
        HIP_TRY_OR(done, lzs_hip_h2d(t->d_dirty, t->dirty, nseg, stream), "hipMemcpy H2D");
        HIP_TRY_OR(done, lzs_hip_launch_scan_stream(d_in, n, nseg, t->d_entry, t->d_dirty, t->d_exit, t->d_count, round == 0 ? t->d_ones : NULL,
                                                    d_marks, round != 0 && !env.no_marks, t->seg, concat, t->d_base, t->d_end, in_extent, stream), who);
        /* (exits and count lie one behind the other on both sides: one copy) */
        HIP_TRY_OR(done, lzs_hip_d2h(t->exits, t->d_exit, 2 * sizeof(uint32_t) * nseg, stream), "hipMemcpy D2H");
        if (round == 0) HIP_TRY_OR(done, lzs_hip_d2h(t->ones, t->d_ones, nseg, stream), "hipMemcpy D2H");
        HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
        const uint32_t was = ndirty;
        int host_made = 0;
        ndirty = settle_entries(t, !env.no_ones, &host_made);
        /* what the host worked out itself must survive the next round's copy back */
        if (ndirty && host_made)
            HIP_TRY_OR(done, lzs_hip_h2d(t->d_exit, t->exits, 2 * sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
        const double t1 = env.stream_debug ? now_ms() : 0;
        if (env.stream_debug && t->nblocks) fprintf(stderr, "liblzs %s: %zu blocks, %u segments of %u; round %u in %.2f ms, %u to redo\n", t->label, t->nblocks, nseg, t->seg, round, t1 - *t0, ndirty);
        else if (env.stream_debug) fprintf(stderr, "liblzs %s: round %u scanned %u of %u segments in %.2f ms; %u to redo\n", t->label, round, was, nseg, t1 - *t0, ndirty);
        *t0 = t1;
    }
    if (env.verify_scan && (again = (uint32_t *)malloc(2 * sizeof(uint32_t) * nseg)) != NULL) {
        /* development check: every segment walked in full from its final entry must report what
         * the rounds arrived at (merged walks and the all-0xFF shortcut included) */
        memset(t->dirty, 1, nseg);
        HIP_TRY_OR(done, lzs_hip_h2d(t->d_entry, t->entry, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
        HIP_TRY_OR(done, lzs_hip_h2d(t->d_dirty, t->dirty, nseg, stream), "hipMemcpy H2D");
        HIP_TRY_OR(done, lzs_hip_launch_scan_stream(d_in, n, nseg, t->d_entry, t->d_dirty, t->d_exit, t->d_count, NULL, NULL, 0, t->seg, concat,
                                                    t->d_base, t->d_end, in_extent, stream), who);
        HIP_TRY_OR(done, lzs_hip_d2h(again, t->d_exit, 2 * sizeof(uint32_t) * nseg, stream), "hipMemcpy D2H");
        HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
        for (uint32_t k = 0; k < nseg; k++) {
            if (t->entry[k] & LZS_SEG_STOP) continue;
            if (again[k] != t->exits[k] || again[nseg + k] != t->count[k])
                fprintf(stderr, "liblzs verify: segment %u entry %08x: rounds say exit %08x count %u, a full walk says %08x %u (all-ones %u)\n",
                        k, t->entry[k], t->exits[k], t->count[k], again[k], again[nseg + k], t->ones[k]);
        }
    }
done:
    free(again);
    return rc;
}

/* RESOLVE for one stream: `left` bytes of d_out[0, total) still carry an origin.  All origins lie in the 2047 bytes in front of
 * a segment start (the tails).  So: (1) a workgroup per chunk of consecutive segments settles their tails in order, up to
 * copies of bytes in front of the chunk; (2) rounds of pointer jumping on the tails in front of the chunks alone; (3) one pass
 * over everything.  (3) alone, repeated, does the job too: (1) and (2) are shortcuts, not conditions. */
static int resolve_origins(const seg_table_t *t, uint32_t ndec, void *stream, const char *who, void *d_out, uint32_t *d_origin,
                           uint32_t total, uint32_t left, double *t0)
{
    const lzs_env_t env = *lzs_env();
    const int debug = env.stream_debug;
    uint32_t *d_left = t->d_counters + 1;
    int e = 0, rc = LZS_OK;
    double t1;
    const int aligned = ((uintptr_t)d_out & 3u) == 0 && ((uintptr_t)d_origin & 15u) == 0;
    int tails = left && ndec > 1 && aligned && !env.no_tails;
    const int had_tails = tails;
    uint32_t stride = 1, round = 1;
    if (tails && ndec >= 64 && !env.no_chunks) {
        stride = (ndec + 2047u) / 2048u;                    /* <= 2048 workgroups: all resident at once */
        if (stride < 16u) stride = 16u;
        HIP_TRY_OR(failed, lzs_hip_launch_resolve_chunks(d_out, d_origin, total, t->d_start, ndec, stride, round++, stream), who);
        if (debug) { HIP_TRY_OR(failed, lzs_hip_stream_sync(stream), "hipStreamSynchronize"); t1 = now_ms(); fprintf(stderr, "liblzs %s: tails by chunks of %u segments in %.2f ms\n", t->label, stride, t1 - *t0); *t0 = t1; }
    }
    for (; left && round < 250; round++) {
        HIP_TRY_OR(failed, lzs_hip_memset(d_left, 0, 4, stream), "hipMemset");
        if (tails) {
            /* three rounds to a look at the counter: a round on the tails is 30 - 130 us, the look costs as much */
            HIP_TRY_OR(failed, lzs_hip_launch_resolve_tails(d_out, d_origin, total, t->d_start, ndec, stride, round, d_left, stream), who);
            for (int more = 0; more < 2; more++) {
                round++;
                HIP_TRY_OR(failed, lzs_hip_memset(d_left, 0, 4, stream), "hipMemset");
                HIP_TRY_OR(failed, lzs_hip_launch_resolve_tails(d_out, d_origin, total, t->d_start, ndec, stride, round, d_left, stream), who);
            }
        } else
            HIP_TRY_OR(failed, lzs_hip_launch_resolve_stream(d_out, d_origin, total, round, d_left, had_tails, stream), who);
        HIP_TRY_OR(failed, lzs_hip_d2h(&left, d_left, 4, stream), "hipMemcpy D2H");
        HIP_TRY_OR(failed, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
        if (debug) { t1 = now_ms(); fprintf(stderr, "liblzs %s: resolve round %u (%s, stride %u) in %.2f ms, %u left\n", t->label, round, tails ? "tails" : "all", stride, t1 - *t0, left); *t0 = t1; }
        if (tails && !left) {                               /* the tails in front of the chunks are final: now everything */
            tails = 0;                                      /* else -- a tail byte is one jump from its value, any other */
            left = 1;                                       /* byte two (the pass stores no marks on what it finishes, so */
        }                                                   /* a tail byte still shows its origin to whoever comes by) */
    }
    if (left) return fail(LZS_E_HIP, "%s: origins did not resolve", who);
failed:
    return rc;
}

/* lzs_decompress() of one long stream by many wavefronts: see lzs_scan_stream_kernel.  Returns
 * SIZE_MAX if this path does not apply (output of 4 GiB or more) and the caller should decode
 * with one wavefront. */
/* A piece of a stream for lzs_decompress_incremental(): the input is `prefix` (the bytes that hold
 * the bits left over from the call before) followed by `in`; the walk starts in state `entry0`
 * (bit offset into the first byte, extension running, offset: the kernels' state word); copies may
 * reach back into `hist`, the last bytes produced before.  Only whole segments are decoded, and
 * only those before the first one in which the stream stops (end marker, unfinished token) or
 * which would overflow the output: the rest is the one wavefront's (lzs_decode_resume_kernel). */

LZS_HIDDEN size_t stream_decompress(uint8_t *out, size_t cap, const uint8_t *in, size_t n, int dev, int *status, int concat,
                                dec_piece_t *dp)
{
    const char *who = dp ? "lzs_decompress_incremental" : dev ? "lzs_decompress_stream_device" : concat ? "lzs_decompress_concat" : "lzs_decompress";
    seg_table_t t = { .label = "stream decode", .seg = stream_dec_seg(n) };
    const uint32_t nseg = t.nseg = (uint32_t)((n + t.seg - 1) / t.seg);
    int e = 0, rc;
    void *d_in = NULL, *d_out = NULL, *d_aux = NULL, *d_origin = NULL, *d_marks = NULL, *tables = NULL;
    staging_t *st = NULL;
    /* ---- set-up: the stream on the device, the segment table */
    if ((rc = stream_call_begins(who, ((size_t)nseg + 16u) * (5u * 4u + 2u), &st, &tables)) != LZS_OK) goto failed;
    void *stream = st->stream;
    if (dev) d_in = (void *)in; else e = staging_reserve(st, BUF_IN, n + 64, &d_in);
    if (!e) e = staging_reserve(st, BUF_AUX, (size_t)nseg * (4 * 4 + 2) + 128, &d_aux);
    if (!e) e = staging_reserve(st, BUF_MARKS, (size_t)nseg * LZS_SCAN_MARK_WORDS * 4u, &d_marks);
    if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto failed; }
    segtab_lay_out(&t, (uint32_t *)tables, (uint32_t *)d_aux, 0);
    const int debug = lzs_env()->stream_debug;
    double t0 = debug ? now_ms() : 0, t1;
    if (!dev && (rc = stream_copy_in(d_in, dp ? dp->prefix : NULL, dp ? dp->prefix_len : 0, in, n, stream)) != LZS_OK) goto failed;
    /* ---- SCAN */
    if ((rc = scan_rounds(&t, stream, who, d_in, (uint32_t)n, (uint32_t)n, dp ? dp->entry0 : 0u, concat, (uint32_t *)d_marks, &t0)) != LZS_OK) goto failed;
    /* ---- placement: where every segment's output begins; how many segments a piece decodes, and in which state it goes on */
    uint64_t total = 0;
    uint32_t ndec = nseg;                                      /* segments to decode */
    const uint32_t before = dp ? dp->hist_len : 0;             /* bytes in front of out[0] that copies may reach */
    for (uint32_t k = 0; k < nseg; k++) {
        if (dp && ((t.exits[k] & LZS_SEG_STOP) || (t.entry[k] & LZS_SEG_STOP) || total + t.count[k] > cap)) { ndec = k; break; }
        t.start[k] = (uint32_t)total + before;
        if (!(t.entry[k] & LZS_SEG_STOP)) total += t.count[k];
        if (total >= 0xFFFFFF00ull - 0x100000ull) break;
    }
    if (total >= 0xFFFFFF00ull - 0x100000ull) return stream_call_ends(SIZE_MAX, LZS_OK, dev, who, status);   /* positions are 32-bit here */
    if (dp) { dp->seg = t.seg; dp->segs_done = ndec; dp->next_entry = ndec < nseg ? t.entry[ndec] : t.exits[nseg - 1]; }
    const uint32_t produce = (uint32_t)(total < cap ? total : cap);
    if (produce) {
        /* ---- DECODE, behind the history (final bytes: origin "clean" = all ones) */
        if (dev) d_out = out; else e = staging_reserve(st, BUF_OUT, (size_t)before + produce + 64, &d_out);
        if (!e) e = staging_reserve(st, BUF_KEEP, 4 * ((size_t)before + produce) + 64, &d_origin);
        if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto failed; }
        if (before) {
            HIP_TRY_OR(failed, lzs_hip_h2d(d_out, dp->hist, before, stream), "hipMemcpy H2D");
            HIP_TRY_OR(failed, lzs_hip_memset(d_origin, 0xFF, 4 * (size_t)before, stream), "hipMemset");
        }
        HIP_TRY_OR(failed, lzs_hip_h2d(t.d_entry, t.entry, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
        HIP_TRY_OR(failed, lzs_hip_h2d(t.d_start, t.start, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
        HIP_TRY_OR(failed, lzs_hip_memset(t.d_counters, 0, 8, stream), "hipMemset");
        HIP_TRY_OR(failed, lzs_hip_launch_decode_stream(d_out, before + produce, (uint32_t *)d_origin, t.d_counters, d_in, (uint32_t)n, (uint32_t)n,
                                                        ndec, t.d_entry, t.d_start, t.seg, concat, NULL, NULL, NULL, NULL, stream), who);
        uint32_t open[2] = {0, 0};
        HIP_TRY_OR(failed, lzs_hip_d2h(open, t.d_counters, 8, stream), "hipMemcpy D2H");
        HIP_TRY_OR(failed, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
        if (debug) { t1 = now_ms(); fprintf(stderr, "liblzs stream decode: %u bytes decoded in %.2f ms, %u with an origin in another segment\n", produce, t1 - t0, open[0]); t0 = t1; }
        /* ---- RESOLVE, and out */
        if ((rc = resolve_origins(&t, ndec, stream, who, d_out, (uint32_t *)d_origin, before + produce, open[0], &t0)) != LZS_OK) goto failed;
        if (!dev) HIP_TRY_OR(failed, lzs_hip_d2h(out, (uint8_t *)d_out + before, produce, stream), "hipMemcpy D2H");
        HIP_TRY_OR(failed, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
    }
    return stream_call_ends(produce, LZS_OK, dev, who, status);

failed:
    return stream_call_ends(0, rc, dev, who, status);
}

/* A batch of blocks decompressed like one long stream: every block is cut into segments of its
 * own (tables tell the kernels where a segment starts, where its stream ends, where its block's
 * output begins and must end), the scan rounds run over all of them at once -- a block's first
 * segment is always entered at bit 0 in the normal state -- and the origins are resolved over the
 * whole strided output.  d_in / d_out are the staged device buffers of host_batch(). */
LZS_HIDDEN int batch_decompress_segments(staging_t *st, void *stream, const char *who, void *d_out, size_t d_out_stride,
                                     uint32_t cap32, uint32_t *out_len, uint32_t *d_len, const void *d_in, size_t d_in_stride,
                                     const uint32_t *in_len_each, uint32_t in_len, size_t nblocks)
{
    int e = 0, rc = LZS_OK;
    size_t total_in = 0;
    uint32_t in_extent = 0;                                    /* the readable bytes at d_in: the kernels' loads are bounded by it */
    for (size_t b = 0; b < nblocks; b++) {
        const size_t len = in_len_each ? in_len_each[b] : in_len;
        total_in += len;
        if (b * d_in_stride + len > in_extent) in_extent = (uint32_t)(b * d_in_stride + len);
    }
    seg_table_t t = { .label = "batch decode", .nblocks = nblocks, .seg = stream_dec_seg(total_in / 4) };   /* (smaller than for one stream of that size: measured) */
    const uint32_t seg = t.seg;
    for (size_t b = 0; b < nblocks; b++) t.nseg += ((in_len_each ? in_len_each[b] : in_len) + seg - 1) / seg;
    const uint32_t nseg = t.nseg;
    const uint32_t extent = (uint32_t)(nblocks * d_out_stride);
    memset(out_len, 0, sizeof(uint32_t) * nblocks);
    if (nseg == 0) return LZS_OK;
    /* host tables: every segment's block, then the segment table -- 10 words and 3 bytes a segment */
    uint32_t *blk = (uint32_t *)malloc((size_t)nseg * (10 * 4 + 3));
    if (!blk) return fail(LZS_E_NOMEM, "%s: out of host memory", who);
    void *d_aux = NULL, *d_marks = NULL, *d_origin = NULL;
    e = staging_reserve(st, BUF_AUX, (size_t)nseg * (8 * 4 + 2) + 128, &d_aux);
    if (!e) e = staging_reserve(st, BUF_MARKS, (size_t)nseg * LZS_SCAN_MARK_WORDS * 4u, &d_marks);
    if (!e) e = staging_reserve(st, BUF_KEEP, 4 * (size_t)extent + 64, &d_origin);
    if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto done; }
    segtab_lay_out(&t, blk + nseg, (uint32_t *)d_aux, 1);
    for (size_t b = 0, k = 0; b < nblocks; b++) {
        const uint32_t len = in_len_each ? in_len_each[b] : in_len;
        for (uint32_t at = 0; at < len; at += seg, k++) {
            t.base[k] = (uint32_t)(b * d_in_stride) + at;
            t.end[k] = (uint32_t)(b * d_in_stride) + len;
            t.floor_[k] = (uint32_t)(b * d_out_stride);
            t.limit[k] = t.floor_[k] + cap32;
            blk[k] = (uint32_t)b;
            t.first[k] = at == 0;
        }
    }
    const int debug = lzs_env()->stream_debug;
    double t0 = debug ? now_ms() : 0, t1;
    HIP_TRY_OR(done, lzs_hip_h2d(t.d_base, t.base, 2 * sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");      /* (and end, behind it) */
    if ((rc = scan_rounds(&t, stream, who, d_in, 0, in_extent, 0, 0, (uint32_t *)d_marks, &t0)) != LZS_OK) goto done;
    /* placement: every block's segments one behind the other from the block's slot on, cut at the capacity */
    uint64_t total = 0;
    for (uint32_t k = 0; k < nseg; k++) {
        if (t.first[k]) total = 0;
        t.start[k] = t.floor_[k] + (uint32_t)(total < cap32 ? total : cap32);
        if (!(t.entry[k] & LZS_SEG_STOP)) total += t.count[k];
        out_len[blk[k]] = (uint32_t)(total < cap32 ? total : cap32);
    }
    HIP_TRY_OR(done, lzs_hip_h2d(t.d_entry, t.entry, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
    HIP_TRY_OR(done, lzs_hip_h2d(t.d_start, t.start, sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");
    HIP_TRY_OR(done, lzs_hip_h2d(t.d_floor, t.floor_, 2 * sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");   /* (and limit, behind it) */
    HIP_TRY_OR(done, lzs_hip_memset(t.d_counters, 0, 8, stream), "hipMemset");
    HIP_TRY_OR(done, lzs_hip_memset(d_origin, 0xFF, 4 * (size_t)extent, stream), "hipMemset");      /* everything "clean" */
    HIP_TRY_OR(done, lzs_hip_launch_decode_stream(d_out, extent, (uint32_t *)d_origin, t.d_counters, d_in, 0, in_extent, nseg, t.d_entry, t.d_start,
                                                  seg, 0, t.d_base, t.d_end, t.d_floor, t.d_limit, stream), who);
    uint32_t open[2] = {0, 0};
    HIP_TRY_OR(done, lzs_hip_d2h(open, t.d_counters, 8, stream), "hipMemcpy D2H");
    HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
    if (debug) { t1 = now_ms(); fprintf(stderr, "liblzs batch decode: tables + memset + decode in %.2f ms, %u bytes with an origin elsewhere\n", t1 - t0, open[0]); t0 = t1; }
    /* origins never leave their block: one workgroup per block resolves them to the end */
    HIP_TRY_OR(done, lzs_hip_h2d(d_len, out_len, sizeof(uint32_t) * nblocks, stream), "hipMemcpy H2D");
    if (open[0]) HIP_TRY_OR(done, lzs_hip_launch_resolve_blocks(d_out, (uint32_t *)d_origin, d_out_stride, d_len, (uint32_t)nblocks, stream), who);
    HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
    if (debug) { t1 = now_ms(); fprintf(stderr, "liblzs batch decode: resolve in %.2f ms\n", t1 - t0); t0 = t1; }
done:
    free(blk);
    return rc;
}


int lzs_decompress_stream_device(void *d_out, size_t out_cap, size_t *out_len, const void *d_in, size_t in_len)
{
    if (!out_len) return fail(LZS_E_ARG, "lzs_decompress_stream_device: out_len is NULL");
    *out_len = 0;
    if ((!d_out && out_cap) || (!d_in && in_len)) return fail(LZS_E_ARG, "lzs_decompress_stream_device: NULL buffer");
    if (in_len == 0 || out_cap == 0) return LZS_OK;
    if (in_len > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "lzs_decompress_stream_device: stream exceeds LZS_BLOCK_MAX");
    int rc = LZS_OK;
    const size_t got = stream_decompress((uint8_t *)d_out, out_cap, (const uint8_t *)d_in, in_len, 1, &rc, 0, NULL);
    if (got == SIZE_MAX) return fail(LZS_E_ARG, "lzs_decompress_stream_device: output of 4 GiB or more");
    *out_len = got;
    return rc;
}
