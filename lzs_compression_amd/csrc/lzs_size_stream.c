/*
 * lzs_size_stream.c -- the size query for LONG streams (include/lzs/lzs_batch.h: lzs_decompressed_size_stream_device,
 * lzs_decompressed_size_stream, lzs_decompressed_size_batch_device_sync): how long a stream decodes to at a
 * capacity of `limit`, and with which status, by the whole device and without decoding.
 *
 * SCAN of the many-wavefront decompressor (lzs_stream.c: scan_rounds()) walks every segment, agrees on the decoder's state at
 * every border and reports how many bytes each segment produces.  A stream's size at `limit` is min(true size, limit) -- a copy
 * the capacity cuts still takes its bits, so the tokens behind it are where they would be without a limit -- and that is the
 * prefix sum of the counts.  The status needs the few tokens around the place where the room runs out, or around the stream's
 * end: one lane a stream walks from the start of the segment in which that lies, in the state SCAN settled for it
 * (lzs_size_finish_kernel, lzs_size_stream.hip), by the rules of the lane-per-stream query (lzs_decoded_size.hip).  Under the
 * file rule (LZS_SIZE_CONCAT) a marker ends nothing and the sum is the whole answer.
 */
#include "lzs_internal.h"
#include "lzs_launch_plan.h"

#define ST_STARVED (LZS_D_STATUS_INPUT_STARVED | LZS_D_STATUS_INPUT_FINISHED)

/* LZS_SIZE_ROUTE=lanes|segments (development: the tests and the sweep force either route of the batch call); 0: not set, or
 * another word.  Read at every call, not through lzs_env(): that struct is lzs_host.c's, which the sanitizer programs of
 * tests/cpu_shim link without this file, and a getenv() is nothing beside a call that synchronises with the device. */
static int size_route_forced(void)
{
    const char *v = getenv("LZS_SIZE_ROUTE");
    return !v ? 0 : !strcmp(v, "lanes") ? 1 : !strcmp(v, "segments") ? 2 : 0;
}

/* a stream without a byte: nothing to walk */
static uint8_t empty_status(uint64_t limit) { return limit == 0 ? LZS_D_STATUS_NO_OUTPUT_BUFFER_SPACE : ST_STARVED; }

/* The streams of a call by segments: ONE stream of n bytes (nblocks == 0; from h_in, staged, or at d_in), or the nblocks blocks
 * of a batch at d_in.  size64[0], or size32[b], and status[b] (or NULL) receive the answers; `concat`: the file rule (one
 * stream only).  LZS_OK or the error reported. */
static int size_by_segments(const char *who, const void *d_in, const uint8_t *h_in, size_t n, size_t in_stride,
                            const uint32_t *in_len_each, uint32_t in_len, size_t nblocks, uint64_t limit, int concat,
                            uint64_t *size64, uint32_t *size32, uint8_t *status)
{
    const size_t ns = nblocks ? nblocks : 1;
    const int ranges = nblocks != 0;
    seg_table_t t = { .label = "size query", .nblocks = nblocks };
    uint32_t in_extent = (uint32_t)n;                          /* the readable bytes at d_in: the kernels' loads are bounded by it */
    if (ranges) {
        size_t total_in = 0;
        in_extent = 0;
        for (size_t b = 0; b < nblocks; b++) {
            const size_t len = in_len_each ? in_len_each[b] : in_len;
            total_in += len;
            if (b * in_stride + len > in_extent) in_extent = (uint32_t)(b * in_stride + len);
        }
        t.seg = stream_dec_seg(total_in / 4);                  /* (as batch_decompress_segments() cuts them) */
        for (size_t b = 0; b < nblocks; b++) t.nseg += ((in_len_each ? in_len_each[b] : in_len) + t.seg - 1) / t.seg;
    } else {
        t.seg = stream_dec_seg(n);
        t.nseg = (uint32_t)((n + t.seg - 1) / t.seg);
    }
    const uint32_t seg = t.seg, nseg = t.nseg;
    int e = 0, rc;
    void *d_stage = NULL, *d_aux = NULL, *d_marks = NULL, *d_fin = NULL, *tables = NULL;
    staging_t *st = NULL;
    /* ---- set-up.  Pinned host memory: every stream's bytes in front of its finishing segment (64-bit), the segment table, what
     * the finishing walks are told (from, end, entry, room) and what they answer (counted, status).  The same on the device. */
    const size_t tab_words = (size_t)nseg * (ranges ? 9u : 5u), tab_bytes = (tab_words * 4u + (size_t)nseg * 3u + 7u) & ~(size_t)7u;
    if ((rc = stream_call_begins(who, 8u * ns + tab_bytes + 21u * ns + 64u, &st, &tables)) != LZS_OK) goto done;
    void *stream = st->stream;
    if (h_in) { e = staging_reserve(st, BUF_IN, n + 64, &d_stage); d_in = d_stage; }
    if (!e) e = staging_reserve(st, BUF_AUX, (size_t)nseg * (8 * 4 + 2) + 128, &d_aux);
    if (!e) e = staging_reserve(st, BUF_MARKS, (size_t)nseg * LZS_SCAN_MARK_WORDS * 4u + 64, &d_marks);
    if (!e) e = staging_reserve(st, BUF_LEN, 21u * ns + 64, &d_fin);
    if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto done; }
    uint64_t *pre = (uint64_t *)tables;
    uint32_t *fin_in = (uint32_t *)((uint8_t *)tables + 8u * ns + tab_bytes), *fin_out = fin_in + 4 * ns;
    uint32_t *d_fin_in = (uint32_t *)d_fin, *d_fin_out = d_fin_in + 4 * ns;
    segtab_lay_out(&t, (uint32_t *)(pre + ns), (uint32_t *)d_aux, ranges);
    const int debug = lzs_env()->stream_debug;
    double t0 = debug ? now_ms() : 0, t1;
    if (ranges) {
        for (size_t b = 0, k = 0; b < nblocks; b++) {
            const uint32_t len = in_len_each ? in_len_each[b] : in_len;
            for (uint32_t at = 0; at < len; at += seg, k++) {
                t.base[k] = (uint32_t)(b * in_stride) + at;
                t.end[k] = (uint32_t)(b * in_stride) + len;
                t.first[k] = at == 0;
            }
        }
        if (nseg) HIP_TRY_OR(done, lzs_hip_h2d(t.d_base, t.base, 2 * sizeof(uint32_t) * nseg, stream), "hipMemcpy H2D");      /* (and end, behind it) */
    }
    if (h_in && (rc = stream_copy_in(d_stage, NULL, 0, h_in, n, stream)) != LZS_OK) goto done;
    /* ---- SCAN */
    if (nseg && (rc = scan_rounds(&t, stream, who, d_in, ranges ? 0u : (uint32_t)n, in_extent, 0u, concat, (uint32_t *)d_marks, &t0)) != LZS_OK) goto done;
    /* ---- every stream's sum, and the segment its finishing walk starts at: the first in which the room runs out, or the last
     * one the stream reaches (where the limit falls on a border either neighbour would do: the walk does not end with its
     * segment) */
    for (size_t b = 0, k = 0; b < ns; b++) {
        const uint32_t len = ranges ? (in_len_each ? in_len_each[b] : in_len) : (uint32_t)n;
        const size_t k1 = k + (len + seg - 1) / seg;
        uint64_t total = 0;
        uint32_t from = 0, end = 0, entry = 0;                 /* (a stream without a segment: a walk over nothing) */
        int found = 0;
        pre[b] = 0;
        for (; k < k1; k++) {
            if (t.entry[k] & LZS_SEG_STOP) continue;           /* behind the stream's end */
            if (!found) {
                from = ranges ? t.base[k] : (uint32_t)k * seg; end = ranges ? t.end[k] : (uint32_t)n; entry = t.entry[k];
                pre[b] = total;
                found = total + t.count[k] >= limit;
            }
            total += t.count[k];
        }
        const uint64_t room = limit - pre[b];                  /* (pre[b] <= limit: it is below the limit, or 0) */
        fin_in[b] = from; fin_in[ns + b] = end; fin_in[2 * ns + b] = entry; fin_in[3 * ns + b] = room > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)room;
        if (concat) {
            const uint64_t size = total < limit ? total : limit;
            *size64 = size;
            if (status) *status = size == limit ? LZS_D_STATUS_NO_OUTPUT_BUFFER_SPACE : ST_STARVED;
        }
    }
    /* ---- the finishing walks, one launch for all streams, and their answers in one copy */
    if (!concat) {
        HIP_TRY_OR(done, lzs_hip_h2d(d_fin_in, fin_in, 16u * ns, stream), "hipMemcpy H2D");
        HIP_TRY_OR(done, lzs_hip_launch_size_finish(d_fin_out, (uint8_t *)(d_fin_out + ns), d_in, d_fin_in, d_fin_in + ns, d_fin_in + 2 * ns,
                                                    d_fin_in + 3 * ns, (uint32_t)ns, stream), who);
        HIP_TRY_OR(done, lzs_hip_d2h(fin_out, d_fin_out, 5u * ns, stream), "hipMemcpy D2H");
        HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
        const uint8_t *fin_status = (const uint8_t *)(fin_out + ns);
        for (size_t b = 0; b < ns; b++) {
            if (ranges) size32[b] = (uint32_t)(pre[b] + fin_out[b]); else *size64 = pre[b] + fin_out[b];
            if (status) status[b] = fin_status[b];
        }
        if (debug) { t1 = now_ms(); fprintf(stderr, "liblzs size query: %zu finishing walk%s in %.2f ms\n", ns, ns == 1 ? "" : "s", t1 - t0); t0 = t1; }
    }
done:
    stream_call_ends(0, rc, 1, who, NULL);
    return rc;
}

static int size_stream(const char *who, uint64_t *size, uint8_t *status, const void *d_in, const uint8_t *h_in, size_t in_len,
                       uint64_t limit, unsigned flags)
{
    if (!size) return fail(LZS_E_ARG, "%s: size is NULL", who);
    if (flags & ~LZS_SIZE_CONCAT) return fail(LZS_E_ARG, "%s: unknown flags 0x%X", who, flags);
    if (in_len > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "%s: stream of %zu bytes exceeds LZS_BLOCK_MAX", who, in_len);
    if (!d_in && !h_in && in_len) return fail(LZS_E_ARG, "%s: input is NULL", who);
    *size = 0;
    if (in_len == 0) {
        if (status) *status = empty_status(limit);
        return LZS_OK;
    }
    const int rc = require_device();
    if (rc != LZS_OK) return rc;
    return size_by_segments(who, d_in, h_in, in_len, 0, NULL, 0, 0, limit, (flags & LZS_SIZE_CONCAT) != 0, size, NULL, status);
}

int lzs_decompressed_size_stream_device(uint64_t *size, uint8_t *status, const void *d_in, size_t in_len, uint64_t limit, unsigned flags)
{
    return size_stream("lzs_decompressed_size_stream_device", size, status, d_in, NULL, in_len, limit, flags);
}

int lzs_decompressed_size_stream(uint64_t *size, uint8_t *status, const uint8_t *in, size_t in_len, uint64_t limit, unsigned flags)
{
    return size_stream("lzs_decompressed_size_stream", size, status, NULL, in, in_len, limit, flags);
}

/* the batch by lanes: lzs_decoded_size_kernel into this thread's staging, the results copied out */
static int size_by_lanes(const char *who, uint32_t *size, uint8_t *status, const void *d_in, size_t in_stride, const uint32_t *in_len_each,
                         uint32_t in_len, uint32_t limit, size_t nblocks)
{
    int e = 0, rc;
    void *d_res = NULL, *d_in_len = NULL, *tables = NULL;
    staging_t *st = NULL;
    if ((rc = stream_call_begins(who, 64, &st, &tables)) != LZS_OK) goto done;
    void *stream = st->stream;
    e = staging_reserve(st, BUF_LEN, 5u * nblocks + 64, &d_res);
    if (!e && in_len_each) e = staging_reserve(st, BUF_INLEN, sizeof(uint32_t) * nblocks, &d_in_len);
    if (e) { rc = fail(LZS_E_NOMEM, "%s: device allocation failed: %s", who, lzs_hip_strerror(e)); goto done; }
    uint32_t *d_size = (uint32_t *)d_res;
    uint8_t *d_status = (uint8_t *)(d_size + nblocks);
    if (in_len_each) HIP_TRY_OR(done, lzs_hip_h2d(d_in_len, in_len_each, sizeof(uint32_t) * nblocks, stream), "hipMemcpy H2D");
    HIP_TRY_OR(done, lzs_hip_launch_decoded_size(d_size, d_status, d_in, in_stride, (const uint32_t *)d_in_len, in_len, limit, (uint32_t)nblocks, stream), who);
    HIP_TRY_OR(done, lzs_hip_d2h(size, d_size, sizeof(uint32_t) * nblocks, stream), "hipMemcpy D2H");
    if (status) HIP_TRY_OR(done, lzs_hip_d2h(status, d_status, nblocks, stream), "hipMemcpy D2H");
    HIP_TRY_OR(done, lzs_hip_stream_sync(stream), "hipStreamSynchronize");
done:
    stream_call_ends(0, rc, 1, who, NULL);
    return rc;
}

int lzs_decompressed_size_batch_device_sync(uint32_t *size, uint8_t *status, const void *d_in, size_t in_stride, const uint32_t *in_len_each,
                                            size_t in_len, size_t limit, size_t nblocks)
{
    const char *who = "lzs_decompressed_size_batch_device_sync";
    if (nblocks == 0) return LZS_OK;
    if (!size) return fail(LZS_E_ARG, "%s: size is NULL", who);
    if (in_len > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "%s: block of %zu bytes exceeds LZS_BLOCK_MAX", who, in_len);
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    if (limit > 0xFFFFFFFFu) return fail(LZS_E_ARG, "%s: limit %zu exceeds 0xFFFFFFFF", who, limit);
    size_t total_in = 0, longest = 0;
    for (size_t b = 0; b < nblocks; b++) {
        const size_t len = in_len_each ? in_len_each[b] : in_len;
        total_in += len;
        if (len > longest) longest = len;
    }
    if (longest > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "%s: block exceeds LZS_BLOCK_MAX", who);
    if (!d_in && longest) return fail(LZS_E_ARG, "%s: input is NULL", who);
    if (longest == 0) {                                         /* nothing but empty blocks: nothing to ask the device */
        for (size_t b = 0; b < nblocks; b++) { size[b] = 0; if (status) status[b] = empty_status(limit); }
        return LZS_OK;
    }
    const int rc = require_device();
    if (rc != LZS_OK) return rc;
    /* (products of 31- and 64-bit factors: an extent that overflows 64 bits is beyond 32 as well) */
    const uint64_t extent = in_stride > 0xFFFFFFFFull ? UINT64_MAX : (uint64_t)nblocks * in_stride + longest;
    if (lzs_plan_size_route(extent, total_in, nblocks, size_route_forced()) == LZS_SIZE_BY_SEGMENTS)
        return size_by_segments(who, d_in, NULL, 0, in_stride, in_len_each, (uint32_t)in_len, nblocks, limit, 0, NULL, size, status);
    return size_by_lanes(who, size, status, d_in, in_stride, in_len_each, (uint32_t)in_len, (uint32_t)limit, nblocks);
}
