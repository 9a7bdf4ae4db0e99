/*
 * lzs_pipeline.c -- large host-buffer batches (lzs_compress_batch / lzs_decompress_batch) with their
 * three stages overlapped.  What a drop-in caller of the reference's one-shot calls in a loop
 * (c/src/test/test-lzs.c:111-114) actually hands over are HOST buffers; round 3 copied them in, ran the
 * kernel and copied the results back one after the other on one stream: 12.1 / 15.7 GB/s at 1 GiB against
 * 64 GB/s in the kernel and 57 GB/s of pinned DMA on the same box.
 *
 * Here the batch is cut into chunks of blocks, and per chunk k
 *
 *     FILL(k)    host threads copy the caller's blocks into a pinned piece, laid out at the device stride
 *     H2D(k)     one DMA from the pinned piece                                      (one stream)
 *     RUN(j)     ONE launch for a group of G chunks: the kernel, slot compaction, the lengths to the host
 *                                                                                    (two streams in turn: two launches
 *                                                                                    on the device at once)
 *     D2H(k)     one DMA of exactly the bytes the chunk produced, into a pinned piece   (one stream)
 *     DRAIN(k)   host threads lay the blocks out in the caller's array (nothing past out_len[b] is touched)
 *
 * run as a pipeline driven by what is ready (events are asked, not waited for, as long as there is anything else to
 * do): while launches are on the device, later chunks are filled and copied in and earlier ones copied out and
 * drained.  Copies go by the chunk (~45 MiB), launches by the group: a compress launch wants 1280 blocks to fill the
 * device (G = 2), a DEcompress launch takes as long as its slowest block whatever its size (a wavefront walks eight
 * streams token by token: 7.4 ms for 88 blocks of 64 KiB, 8.2 ms for 5632 -- tests/dev/dectime_chunks.py), so only
 * thousands of blocks at once reach the rate of one big launch (G = 8, two launches in flight).  Two pinned pieces on
 * the way in, three on the way out.
 *
 * Measured (1 GiB of text in 64 KiB blocks, the caller's buffers touched beforehand, MI355X box with a 16-CPU quota;
 * tests/dev/hostbatch_time2.py, hostbatch_sweep.py; profiles/r04/hostbatch_*.txt): lzs_compress_batch 11-12.6 GB/s one
 * after the other -> 45 GB/s; lzs_decompress_batch 16-17 -> 29 GB/s (what is left: the first launch's 9 ms before any
 * byte can leave, then 1.07 GB over the copy engine).
 * Pageable memory cannot be read by the copy engines at more than 13-14 GB/s and pinning the caller's buffers
 * in place costs 79 ms per GiB (tools/probes/host_copy_probe.hip), hence the pinned pieces and the threads
 * (one thread's memcpy is 31 GB/s there: the single-thread variant of round 3 lost).
 *
 * Nothing here knows the codec: `launch` is lzs_hip_launch_compress or lzs_hip_launch_decompress.
 */
#include "lzs_internal.h"

#define PIPE_MAX_THREADS 8
#define PIPE_RUN     2              /* run streams: with the two copy streams that is four streams, what the runtime gives
                                     * hardware queues of their own (with twelve streams a 46 MB copy-out stood in line
                                     * behind another stream's 9 ms kernel) */
#define PIPE_SLOTS   3              /* launches whose blocks, slots and dense piece are on the device at once: one being
                                     * copied in, one running, one being copied out */
#define PIPE_GROUP_MAX 8            /* chunks per launch, at most */
#define PIPE_MIN_MB  24             /* the smallest batch (MiB of the wider side) and ... */
#define PIPE_MIN_BLOCKS 256         /* ... the fewest blocks that take this route (see host_batch_pipelined) */

/* events */
enum { EV_IN = 0,                   /* [2] H2D of chunk k has left pinned piece k & 1 */
       EV_INS = 2,                  /* [PIPE_SLOTS] all of launch j's chunks are on the device */
       EV_RUN = 5,                  /* [PIPE_SLOTS] launch j (kernel, compaction, lengths to the host) is through */
       EV_OUT = 8,                  /* [3] D2H of chunk k is in pinned piece k % 3 */
       EV_OUTS = 11,                /* [PIPE_SLOTS] every chunk of launch j has been copied out of its dense piece */
       EV_COUNT = 14 };
_Static_assert(2 + PIPE_RUN == PIPE_STREAMS && EV_COUNT == PIPE_EVENTS, "staging_t holds the pipeline's streams and events");

/* one batch on its way through the pipeline */
typedef struct {
    const char *who; launch_fn launch; staging_t *st; uint32_t cap32;
    uint8_t *out; size_t out_stride; uint32_t *out_len;
    const uint8_t *in; size_t in_stride; const uint32_t *in_len_each; size_t in_len;
    pipe_plan_t pl;                                     /* chunk, K chunks, G a launch, J launches */
    size_t nblocks, d_in_stride, d_out_stride;
    size_t group, dense_piece, len_piece;               /* blocks per launch; bytes of a launch's dense piece and lengths */
    /* device memory: a ring of PIPE_SLOTS launches' worth of blocks, slots, lengths and dense bytes; the pinned pieces */
    void *d_in, *d_out, *d_len, *d_in_len, *d_dense, *d_offs;
    uint8_t *pin_in[2], *pin_out[3], *pin_len;
    uint64_t *doff[3];                                  /* where a chunk's blocks begin in its pinned piece (chunk + 1 entries) */
    /* The four hands of the pipeline, each a counter of what it has done: chunks filled + copied in, launches queued,
     * chunks whose copy out is queued, chunks drained. */
    size_t n_fill, n_run, n_fin, n_drain, n_done;       /* (n_done: launches the host has seen finished) */
    size_t j_known;                                     /* the launch whose lengths the host has read */
    uint64_t chunk_at[PIPE_GROUP_MAX + 1];              /* of that launch: where its chunks begin in the dense piece */
    int progressed;                                     /* this turn of the loop */
    int debug, trace;                                   /* LZS_STREAM_DEBUG, LZS_PIPE_TRACE */
    double t_copy, t_wait, t_queue, t_mark, t_all;
    unsigned long rounds;
    /* this round of host copies: chunk numbers, or -1 */
    long fill, drain;
    /* the workers */
    pthread_t th[PIPE_MAX_THREADS];
    int nth, started;
    pthread_mutex_t mu;
    pthread_cond_t cv_work, cv_done;
    unsigned gen;
    int pending, quit;
} pipe_run_t;

/* worker w's share of this round: its slice of the blocks to fill and of the blocks to drain */
static void pipe_do_share(const pipe_run_t *p, int w)
{
    if (p->fill >= 0) {
        const size_t b0 = (size_t)p->fill * p->pl.chunk;
        const size_t nb = p->nblocks - b0 < p->pl.chunk ? p->nblocks - b0 : p->pl.chunk;
        const size_t lo = nb * (size_t)w / (size_t)p->nth, hi = nb * (size_t)(w + 1) / (size_t)p->nth;
        if (!p->in_len_each && p->in_stride == p->d_in_stride) {
            /* contiguous blocks of the device's own stride: one copy (the last block of the batch may be short of its stride) */
            if (hi > lo) {
                const size_t bytes = (hi - lo - 1) * p->d_in_stride + (b0 + hi == p->nblocks ? p->in_len : p->d_in_stride);
                memcpy(p->pin_in[p->fill & 1] + lo * p->d_in_stride, p->in + (b0 + lo) * p->in_stride, bytes);
            }
        } else {
            lay_blocks_in(p->pin_in[p->fill & 1] + lo * p->d_in_stride, p->d_in_stride, p->in, p->in_stride, p->in_len_each, p->in_len,
                          b0 + lo, hi - lo);
        }
    }
    if (p->drain >= 0) {
        const size_t b0 = (size_t)p->drain * p->pl.chunk;
        const size_t nb = p->nblocks - b0 < p->pl.chunk ? p->nblocks - b0 : p->pl.chunk;
        const size_t lo = nb * (size_t)w / (size_t)p->nth, hi = nb * (size_t)(w + 1) / (size_t)p->nth;
        const uint8_t *const piece = p->pin_out[p->drain % 3];
        const uint64_t *const off = p->doff[p->drain % 3];
        for (size_t b = lo; b < hi; b++)
            memcpy(p->out + (b0 + b) * p->out_stride, piece + off[b], p->out_len[b0 + b]);
    }
}

typedef struct { pipe_run_t *p; int w; } pipe_arg_t;

static void *pipe_worker(void *argp)
{
    pipe_arg_t *a = (pipe_arg_t *)argp;
    pipe_run_t *p = a->p;
    const int w = a->w;
    unsigned seen = 0;
    pthread_mutex_lock(&p->mu);
    for (;;) {
        while (!p->quit && p->gen == seen) pthread_cond_wait(&p->cv_work, &p->mu);
        if (p->quit) break;
        seen = p->gen;
        pthread_mutex_unlock(&p->mu);
        pipe_do_share(p, w);
        pthread_mutex_lock(&p->mu);
        if (--p->pending == 0) pthread_cond_signal(&p->cv_done);
    }
    pthread_mutex_unlock(&p->mu);
    return NULL;
}

/* one round of host copies on all workers; the calling thread takes share 0 itself */
static void pipe_round(pipe_run_t *p)
{
    if (p->fill < 0 && p->drain < 0) return;
    pthread_mutex_lock(&p->mu);
    p->pending = p->started;
    p->gen++;
    pthread_cond_broadcast(&p->cv_work);
    pthread_mutex_unlock(&p->mu);
    pipe_do_share(p, 0);
    pthread_mutex_lock(&p->mu);
    while (p->pending) pthread_cond_wait(&p->cv_done, &p->mu);
    pthread_mutex_unlock(&p->mu);
}

/* The plan: chunks of about 45 MiB of the wider side (640 blocks of 64 KiB), at least 64 blocks; worth it from four chunks on. */
LZS_HIDDEN pipe_plan_t pipe_plan(launch_fn launch, uint32_t cap32, size_t nblocks, size_t in_len, const lzs_env_t *env)
{
    pipe_plan_t pl = { 0, 0, 0, 0, 0, 0, 0 };
    const size_t d_in_stride = round16(in_len ? in_len : 1), d_out_stride = round16(cap32 ? cap32 : 1);
    const size_t widest = d_in_stride > d_out_stride ? d_in_stride : d_out_stride;
    size_t chunk = ((size_t)(env->pipe_chunk_mb > 0 ? env->pipe_chunk_mb : 46) << 20) / widest;
    chunk = chunk < 64 ? 64 : chunk & ~(size_t)63;
    /* From 24 MiB on (batches of streams up to 64 MiB of output are decompressed in segments before this is asked:
     * lzs_host.c); a batch of fewer than four chunks is cut into four all the same: pinned pieces and host threads beat
     * the runtime's path for pageable memory from there on (1024 blocks of 64 KiB: 9-28 ms -> 3.3; 384 blocks: 2.3 -> 2.0,
     * 512: 2.7 -> 2.2, equal at 256: profiles/r04/hostbatch_small_routes.txt). */
    const unsigned long long least = (unsigned long long)(env->pipe_min_mb > 0 ? env->pipe_min_mb : PIPE_MIN_MB) << 20;
    if (env->overlap_off || !cap32 || nblocks < PIPE_MIN_BLOCKS || (unsigned long long)nblocks * widest < least ||
        widest > ((size_t)4 << 20)) return pl;
    if (nblocks < 4 * chunk) chunk = ((nblocks + 3) / 4 + 63) & ~(size_t)63;
    pl.chunk = chunk;
    pl.K = (nblocks + chunk - 1) / chunk;
    pl.G = env->pipe_group > 0 && env->pipe_group <= PIPE_GROUP_MAX ? (size_t)env->pipe_group
         : launch == lzs_hip_launch_compress ? 2 : 8;                      /* chunks per launch ... */
    if (pl.G > pl.K) pl.G = pl.K;                                           /* ... of the chunks there are (a 1024-block
                                                                             * decompress batch is ONE launch of four chunks, not a ring
                                                                             * of three launches of eight) */
    pl.J = (pl.K + pl.G - 1) / pl.G;                                        /* launches */
    pl.slots = pl.J < PIPE_SLOTS ? pl.J : PIPE_SLOTS;                       /* launches' worth of device memory in the ring */
    pl.threads = env->copy_threads > 0 ? env->copy_threads : 4;
    if (pl.threads > PIPE_MAX_THREADS) pl.threads = PIPE_MAX_THREADS;
    pl.taken = (unsigned long long)pl.G * chunk * d_out_stride <= 0xF0000000ull;
    return pl;
}

enum { S_IN, S_OUT, S_RUN };        /* streams: copy in, copy out, PIPE_RUN run streams in turn */
static void *pipe_stream(const pipe_run_t *R, int which, size_t j)
{
    return R->st->pipe_stream[which + (which == S_RUN ? j % PIPE_RUN : 0)];
}
static void *pipe_event(const pipe_run_t *R, int group, size_t i) { return R->st->pipe_event[group + i % (group == EV_IN ? 2 : 3)]; }

#define TRACE(R, ...) do { if ((R)->trace) { fprintf(stderr, "  %8.2f ms  ", now_ms() - (R)->t_all); fprintf(stderr, __VA_ARGS__); \
                                             fputc('\n', stderr); } } while (0)
static void mark(pipe_run_t *R) { R->t_mark = R->debug ? now_ms() : 0; }
static void since(pipe_run_t *R, double *acc) { if (R->debug) { const double n = now_ms(); *acc += n - R->t_mark; R->t_mark = n; } }
static size_t at_most(size_t a, size_t b) { return a < b ? a : b; }

/* ---- launches whose chunks are all on their way in, and whose dense piece and length slot are free again
 * (launch j - PIPE_RUN used them: all its chunks must have been handed to the copy-out stream) */
static int pipe_queue_launches(pipe_run_t *R)
{
    const size_t G = R->pl.G, K = R->pl.K, group = R->group;
    while (R->n_run < R->pl.J && R->n_fill >= at_most((R->n_run + 1) * G, K) &&
           (R->n_run < PIPE_SLOTS || R->n_fin >= at_most((R->n_run - PIPE_SLOTS + 1) * G, K))) {
        const size_t j = R->n_run, q = j % PIPE_SLOTS, b0 = j * group, nb = at_most(R->nblocks - b0, group);
        uint8_t *const dense = (uint8_t *)R->d_dense + q * R->dense_piece;
        uint64_t *const offs = (uint64_t *)R->d_offs + q * (group + 1);
        uint8_t *const lens = R->pin_len + q * R->len_piece;
        uint8_t *const c_in = (uint8_t *)R->d_in + q * group * R->d_in_stride, *const c_out = (uint8_t *)R->d_out + q * group * R->d_out_stride;
        uint32_t *const c_len = (uint32_t *)R->d_len + q * group;
        void *const run = pipe_stream(R, S_RUN, j);
        HIP_TRY_RET(lzs_hip_stream_wait_event(run, pipe_event(R, EV_INS, j)), "hipStreamWaitEvent");
        HIP_TRY_RET(R->launch(c_out, R->d_out_stride, R->cap32, c_len, c_in, R->d_in_stride,
                              R->d_in_len ? (const uint32_t *)R->d_in_len + b0 : NULL, (uint32_t)R->in_len, (uint32_t)nb, run), R->who);
        if (j >= PIPE_SLOTS)                                             /* (the dense piece is read out) */
            HIP_TRY_RET(lzs_hip_stream_wait_event(run, pipe_event(R, EV_OUTS, j)), "hipStreamWaitEvent");
        HIP_TRY_RET(lzs_hip_launch_compact(dense, offs, c_out, R->d_out_stride, c_len, (uint32_t)nb, run), R->who);
        /* (the lengths and the byte total reach the host by a kernel, not by a copy engine: see lzs_hip_words_to_host) */
        HIP_TRY_RET(lzs_hip_words_to_host((uint32_t *)lens, c_len, nb, run), R->who);
        HIP_TRY_RET(lzs_hip_words_to_host((uint32_t *)(lens + sizeof(uint32_t) * group), (const uint32_t *)(offs + nb), 2, run), R->who);
        HIP_TRY_RET(lzs_hip_event_record(pipe_event(R, EV_RUN, j), run), "hipEventRecord");
        TRACE(R, "launch %zu queued (%zu blocks)", j, nb);
        R->n_run++;
        R->progressed = 1;
    }
    return LZS_OK;
}

/* Launch j is through (*ready) or not yet: its lengths, and where each of its chunks begins in the dense piece */
static int pipe_read_lengths(pipe_run_t *R, size_t j, int *ready)
{
    *ready = lzs_hip_event_done(pipe_event(R, EV_RUN, j));
    if (*ready < 0) return hip_fail(-*ready, "hipEventQuery");
    if (!*ready) return LZS_OK;
    const size_t group = R->group, chunk = R->pl.chunk, g0 = j * group, gn = at_most(R->nblocks - g0, group);
    const uint8_t *const lp = R->pin_len + (j % PIPE_SLOTS) * R->len_piece;
    const uint32_t *lens = (const uint32_t *)lp;
    uint64_t total = 0, at = 0;
    memcpy(&total, lp + sizeof(uint32_t) * group, sizeof total);
    for (size_t b = 0; b < gn; b++) {
        if (b % chunk == 0) R->chunk_at[b / chunk] = at;
        R->out_len[g0 + b] = lens[b];
        at += lens[b];
    }
    R->chunk_at[(gn + chunk - 1) / chunk] = at;
    if (at != total || total > (uint64_t)group * R->d_out_stride)
        return fail(LZS_E_HIP, "%s: inconsistent lengths from the device (launch %zu: %llu bytes by the lengths, %llu by the offsets)",
                    R->who, j, (unsigned long long)at, (unsigned long long)total);
    R->j_known = j;
    R->n_done = j + 1;
    TRACE(R, "launch %zu seen finished", j);
    return LZS_OK;
}

/* ---- chunks of a finished launch: exactly their bytes to a free pinned piece (three: one being drained, one
 * being copied into, one waiting) */
static int pipe_queue_copy_outs(pipe_run_t *R)
{
    const size_t G = R->pl.G, K = R->pl.K, chunk = R->pl.chunk;
    while (R->n_fin < K && R->n_fin / G < R->n_run && R->n_fin - R->n_drain < 3) {
        const size_t k = R->n_fin, j = k / G, b0 = k * chunk, nb = at_most(R->nblocks - b0, chunk);
        if (j != R->j_known) {
            int ready = 0;
            const int rc = pipe_read_lengths(R, j, &ready);
            if (rc != LZS_OK) return rc;
            if (!ready) break;
        }
        const size_t c = k - j * G;                 /* the chunk's number inside its launch */
        uint64_t *o = R->doff[k % 3], at = 0;
        for (size_t b = 0; b < nb; b++) { o[b] = at; at += R->out_len[b0 + b]; }
        o[nb] = at;
        HIP_TRY_RET(lzs_hip_d2h(R->pin_out[k % 3], (const uint8_t *)R->d_dense + (j % PIPE_SLOTS) * R->dense_piece + R->chunk_at[c],
                                (size_t)(R->chunk_at[c + 1] - R->chunk_at[c]), pipe_stream(R, S_OUT, 0)), "hipMemcpy D2H");
        HIP_TRY_RET(lzs_hip_event_record(pipe_event(R, EV_OUT, k), pipe_stream(R, S_OUT, 0)), "hipEventRecord");
        if (c + 1 == G || k + 1 == K) HIP_TRY_RET(lzs_hip_event_record(pipe_event(R, EV_OUTS, j), pipe_stream(R, S_OUT, 0)), "hipEventRecord");
        TRACE(R, "chunk %zu: copy out queued (%llu bytes)", k, (unsigned long long)(R->chunk_at[c + 1] - R->chunk_at[c]));
        R->n_fin++;
        R->progressed = 1;
    }
    return LZS_OK;
}

/* (a chunk goes where launch j - PIPE_SLOTS read its blocks from: that launch must be through) */
static int pipe_can_fill(const pipe_run_t *R)
{
    return R->n_fill < R->pl.K && (R->n_fill / R->pl.G < PIPE_SLOTS || R->n_done + PIPE_SLOTS > R->n_fill / R->pl.G);
}

/* ---- the host threads: the next chunk in (its pinned piece is free once the copy before last has left it), and
 * the oldest chunk whose bytes have arrived out; then the chunk's copy to the device */
static int pipe_host_round(pipe_run_t *R)
{
    int do_fill = pipe_can_fill(R), do_drain = 0;
    if (do_fill && R->n_fill >= 2) {
        const int ready = lzs_hip_event_done(pipe_event(R, EV_IN, R->n_fill));
        if (ready < 0) return hip_fail(-ready, "hipEventQuery");
        do_fill = ready;
    }
    if (R->n_drain < R->n_fin) {
        const int ready = lzs_hip_event_done(pipe_event(R, EV_OUT, R->n_drain));
        if (ready < 0) return hip_fail(-ready, "hipEventQuery");
        do_drain = ready;
    }
    if (!do_fill && !do_drain) return LZS_OK;
    R->fill = do_fill ? (long)R->n_fill : -1;
    R->drain = do_drain ? (long)R->n_drain : -1;
    pipe_round(R);
    since(R, &R->t_copy);
    R->rounds++;
    TRACE(R, "host copies done: fill %ld, drain %ld", R->fill, R->drain);
    if (do_fill) {
        const size_t G = R->pl.G, k = R->n_fill, b0 = k * R->pl.chunk, nb = at_most(R->nblocks - b0, R->pl.chunk);
        uint8_t *const to = (uint8_t *)R->d_in + (((k / G) % PIPE_SLOTS) * R->group + (k % G) * R->pl.chunk) * R->d_in_stride;
        HIP_TRY_RET(lzs_hip_h2d(to, R->pin_in[k & 1], nb * R->d_in_stride, pipe_stream(R, S_IN, 0)), "hipMemcpy H2D");
        HIP_TRY_RET(lzs_hip_event_record(pipe_event(R, EV_IN, k), pipe_stream(R, S_IN, 0)), "hipEventRecord");
        if ((k + 1) % G == 0 || k + 1 == R->pl.K)
            HIP_TRY_RET(lzs_hip_event_record(pipe_event(R, EV_INS, k / G), pipe_stream(R, S_IN, 0)), "hipEventRecord");
        R->n_fill++;
    }
    if (do_drain) R->n_drain++;
    since(R, &R->t_queue);
    R->progressed = 1;
    return LZS_OK;
}

/* nothing is ready: wait for what the pipeline needs next -- the copy out that is under way, else the
 * launch that is on the device; but first of all the copy in whose pinned piece the next chunk wants */
static int pipe_wait(pipe_run_t *R)
{
    void *ev;
    if (pipe_can_fill(R)) ev = pipe_event(R, EV_IN, R->n_fill);                                     /* (the shortest wait first) */
    else if (R->n_drain < R->n_fin) ev = pipe_event(R, EV_OUT, R->n_drain);
    else if (R->n_fin < R->pl.K && R->n_fin / R->pl.G < R->n_run) ev = pipe_event(R, EV_RUN, R->n_fin / R->pl.G);
    else return fail(LZS_E_HIP, "%s: the pipeline has nothing to wait for (filled %zu, launched %zu, copied out %zu, drained %zu of %zu)",
                     R->who, R->n_fill, R->n_run, R->n_fin, R->n_drain, R->pl.K);
    HIP_TRY_RET(lzs_hip_event_sync(ev), "hipEventSynchronize");
    since(R, &R->t_wait);
    return LZS_OK;
}

/* the ring on the device, the pinned pieces, the offset tables (sizes that stay with the thread between calls: no allocation
 * per call); 0, or no room */
static int pipe_reserve(pipe_run_t *R, size_t slots)
{
    staging_t *st = R->st;
    const size_t group = R->group, nblocks = R->nblocks;
    int e = staging_reserve(st, BUF_IN, slots * group * R->d_in_stride, &R->d_in);
    if (!e) e = staging_reserve(st, BUF_OUT, slots * group * R->d_out_stride, &R->d_out);
    if (!e) e = staging_reserve(st, BUF_LEN, slots * sizeof(uint32_t) * group, &R->d_len);
    if (!e && R->in_len_each) e = staging_reserve(st, BUF_INLEN, sizeof(uint32_t) * nblocks, &R->d_in_len);
    if (!e) e = staging_reserve(st, BUF_KEEP, slots * R->dense_piece + 64, &R->d_dense);
    if (!e) e = staging_reserve(st, BUF_AUX, slots * sizeof(uint64_t) * (group + 1), &R->d_offs);
    for (int i = 0; i < 2 && !e; i++) e = staging_pin_reserve(st, PIN_IN0 + i, R->pl.chunk * R->d_in_stride, &R->pin_in[i]);
    for (int i = 0; i < 3 && !e; i++) e = staging_pin_reserve(st, PIN_OUT0 + i, R->pl.chunk * R->d_out_stride, &R->pin_out[i]);
    if (!e) e = staging_pin_reserve(st, PIN_LENGTHS, slots * R->len_piece, &R->pin_len);
    /* (The runtime keeps a failed allocation as its "last error" until somebody fetches it, and every launcher returns the
     * last error after its launch: fetch it here, or the route that is to save the call reports this out-of-memory as its
     * own -- ADVICE r04) */
    if (e) { lzs_hip_clear_error(); return e; }
    for (int i = 0; i < 3; i++) R->doff[i] = (uint64_t *)malloc(sizeof(uint64_t) * (R->pl.chunk + 1));
    return !R->doff[0] || !R->doff[1] || !R->doff[2];
}

LZS_HIDDEN int host_batch_pipelined(const char *who, launch_fn launch, uint8_t *out, size_t out_stride, uint32_t cap32, uint32_t *out_len,
                                    const uint8_t *in, size_t in_stride, const uint32_t *in_len_each, size_t in_len, size_t nblocks,
                                    int *taken)
{
    const lzs_env_t *env = lzs_env();
    const pipe_plan_t pl = pipe_plan(launch, cap32, nblocks, in_len, env);
    *taken = 0;
    if (!pl.taken) return LZS_OK;
    staging_t *st = staging_get();
    if (!st) return fail(LZS_E_NOMEM, "%s: out of host memory", who);
    *taken = 1;

    int rc = LZS_OK, e = 0;
    pipe_arg_t args[PIPE_MAX_THREADS];
    pipe_run_t run, *const R = &run;
    memset(R, 0, sizeof *R);
    R->who = who; R->launch = launch; R->st = st; R->cap32 = cap32; R->nblocks = nblocks;
    R->out = out; R->out_stride = out_stride; R->out_len = out_len;
    R->in = in; R->in_stride = in_stride; R->in_len_each = in_len_each; R->in_len = in_len;
    R->pl = pl; R->group = pl.G * pl.chunk;
    R->d_in_stride = round16(in_len ? in_len : 1); R->d_out_stride = round16(cap32 ? cap32 : 1);
    R->dense_piece = R->group * R->d_out_stride + 32; R->len_piece = sizeof(uint32_t) * R->group + sizeof(uint64_t);
    R->j_known = (size_t)-1; R->fill = R->drain = -1; R->nth = pl.threads;
    pthread_mutex_init(&R->mu, NULL); pthread_cond_init(&R->cv_work, NULL); pthread_cond_init(&R->cv_done, NULL);
    for (size_t i = 0; i < PIPE_STREAMS; i++)
        if (!st->pipe_stream[i]) HIP_TRY_OR(done, lzs_hip_stream_create(&st->pipe_stream[i]), "hipStreamCreate");
    for (size_t i = 0; i < PIPE_EVENTS; i++)
        if (!st->pipe_event[i]) HIP_TRY_OR(done, lzs_hip_event_create(&st->pipe_event[i]), "hipEventCreate");
    /* (no room for the ring or the pinned pieces -- a small cgroup, many threads at once: nothing has been queued yet, the
     * batch takes the one-after-the-other route, which needs neither) */
    if (pipe_reserve(R, pl.slots)) { *taken = 0; goto done; }

    for (int w = 1; w < R->nth; w++) {
        args[w].p = R; args[w].w = w;
        if (pthread_create(&R->th[w], NULL, pipe_worker, &args[w]) != 0) { R->nth = w; break; }
        R->started++;
    }
    if (in_len_each) {
        HIP_TRY_OR(done, lzs_hip_h2d(R->d_in_len, in_len_each, sizeof(uint32_t) * nblocks, pipe_stream(R, S_IN, 0)), "hipMemcpy H2D");
        HIP_TRY_OR(done, lzs_hip_stream_sync(pipe_stream(R, S_IN, 0)), "hipStreamSynchronize");
    }
    R->debug = env->stream_debug; R->trace = env->stream_debug && env->pipe_trace; R->t_all = R->debug ? now_ms() : 0;
    while (R->n_drain < R->pl.K) {
        R->progressed = 0;
        mark(R);
        if ((rc = pipe_queue_launches(R)) != LZS_OK || (rc = pipe_queue_copy_outs(R)) != LZS_OK) goto done;
        since(R, &R->t_queue);
        if ((rc = pipe_host_round(R)) != LZS_OK) goto done;
        if (!R->progressed && (rc = pipe_wait(R)) != LZS_OK) goto done;
    }
    if (R->debug)
        fprintf(stderr, "liblzs pipeline: %s, %zu blocks in %zu chunks of %zu, %zu chunks a launch, %d host threads: %.1f ms = host copies %.1f "
                        "(%lu rounds) + waiting %.1f + queueing %.1f\n",
                who, nblocks, R->pl.K, R->pl.chunk, R->pl.G, R->started + 1, now_ms() - R->t_all, R->t_copy, R->rounds, R->t_wait, R->t_queue);

done:
    if (rc != LZS_OK)                                       /* nothing of ours may still be in flight */
        for (int i = 0; i < PIPE_STREAMS; i++) if (st->pipe_stream[i]) lzs_hip_stream_sync(st->pipe_stream[i]);
    pthread_mutex_lock(&R->mu);
    R->quit = 1;
    pthread_cond_broadcast(&R->cv_work);
    pthread_mutex_unlock(&R->mu);
    for (int w = 1; w <= R->started; w++) pthread_join(R->th[w], NULL);
    pthread_mutex_destroy(&R->mu); pthread_cond_destroy(&R->cv_work); pthread_cond_destroy(&R->cv_done);
    free(R->doff[0]); free(R->doff[1]); free(R->doff[2]);
    staging_trim(st);
    return rc;
}
