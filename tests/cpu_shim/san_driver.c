/*
 * tests/cpu_shim/san_driver.c -- drives the product's UNCHANGED host sources (linked with lzs_cpu_shim.c instead of the
 * HIP translation unit) through the cases of the GPU suite that exercise the intricate host logic, under the
 * sanitizers (tests/test_sanitizers.py builds this with -fsanitize=address,undefined and with -fsanitize=thread):
 *   ragged batches with cut capacities (one-after-the-other route); a batch of >= 24 MiB through the overlapped pipeline
 *   (pinned pieces, four worker threads, launches by the group) both ways, from two calling threads at once; the pipeline's
 *   degrade path (LZS_STAGING_FAIL_MB); one stream in segments with dirty-segment re-entry (runs and periods spanning
 *   many segments, cut capacities); the incremental interface in random pieces both ways on BOTH routes (device route:
 *   segments / stitch / extend-resume / decode-resume; host route: lzs_hostcodec.c) with 1-12 bytes of room for the
 *   low-memory block, and what each of its calls does against a table ("inctrace"); the one-shot calls on both routes; decompression by many wavefronts ("streamdec": the scan rounds with
 *   their settle rule and all-0xFF shortcut, placement, one stream / concatenated streams / batches by segments / pieces of
 *   the incremental interface, each compared with the same call by one wavefront); the route decision and the pipeline's plan
 *   against a table ("routes"); the one-after-the-other route's copy layouts where they switch ("layouts"); the segmented stream
 *   compressor's host path call by call against a table ("streamtrace": results, calls and launches of one-shot calls and pieces).
 * Every result is compared with the oracle.  Exit code 0 = all cases passed (the sanitizers make it non-zero themselves).
 * TEST INFRASTRUCTURE ONLY.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lzs/lzs.h"
#include "lzs/lzs_batch.h"
#include "lzs_internal.h"                /* "routes": host_batch_route() and pipe_plan(), asked directly */

size_t lzs_oracle_compress(uint8_t *out, size_t cap, const uint8_t *in, size_t n);
size_t lzs_oracle_decompress(uint8_t *out, size_t cap, const uint8_t *in, size_t n);
int lzs_workload_fill(uint8_t *dst, unsigned cls, uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_len, int nthreads);

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: ", __func__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 24); }
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1u); }

static uint8_t *sample(unsigned cls, size_t n, uint64_t first)
{
    const size_t nb = (n + 65535u) / 65536u;
    uint8_t *d = (uint8_t *)malloc(nb * 65536u + 1);
    lzs_workload_fill(d, cls, 0x4C5A5331ull, first, nb, 65536, 2);
    return d;
}

/* ---------------------------------------------------------------- ragged batches, cut capacities */
static void ragged_batches(void)
{
    enum { NB = 37, STRIDE = 5000 };
    uint8_t *x = sample(0, (size_t)NB * STRIDE, 3);
    uint32_t lens[NB];
    for (int b = 0; b < NB; b++) lens[b] = b % 7 == 0 ? 0 : rnd_in(1, STRIDE);
    lens[5] = STRIDE;
    for (int pass = 0; pass < 3; pass++) {
        const size_t cap = pass == 0 ? LZS_COMPRESSED_MAX(STRIDE) : pass == 1 ? 700 : 1;
        const size_t ostride = cap + 9;
        uint8_t *out = (uint8_t *)malloc(NB * ostride);
        uint32_t out_len[NB];
        memset(out, 0xA5, NB * ostride);
        const int rc = lzs_compress_batch(out, ostride, cap, out_len, x, STRIDE, lens, STRIDE, NB);
        CHECK(rc == 0, "lzs_compress_batch: %s", lzs_last_error());
        uint8_t *want = (uint8_t *)malloc(LZS_COMPRESSED_MAX(STRIDE));
        for (int b = 0; b < NB; b++) {
            const size_t w = lzs_oracle_compress(want, cap, x + (size_t)b * STRIDE, lens[b]);
            CHECK(out_len[b] == w && memcmp(out + b * ostride, want, w) == 0, "block %d differs (cap %zu)", b, cap);
            for (size_t i = w; i < ostride; i++) if (out[b * ostride + i] != 0xA5) { CHECK(0, "block %d: byte %zu past its length touched", b, i); break; }
        }
        if (pass == 0) {
            const size_t bcap = 3000, bstride = bcap + 5;           /* and back, into slots too small for some */
            uint8_t *back = (uint8_t *)malloc(NB * bstride);
            uint32_t back_len[NB];
            memset(back, 0x5A, NB * bstride);
            CHECK(lzs_decompress_batch(back, bstride, bcap, back_len, out, ostride, out_len, cap, NB) == 0, "lzs_decompress_batch: %s", lzs_last_error());
            for (int b = 0; b < NB; b++) {
                const uint32_t w = lens[b] < bcap ? lens[b] : (uint32_t)bcap;
                CHECK(back_len[b] == w && memcmp(back + b * bstride, x + (size_t)b * STRIDE, w) == 0, "block %d: round trip", b);
                CHECK(back[b * bstride + bcap] == 0x5A, "block %d: byte past the capacity touched", b);
            }
            free(back);
        }
        free(want); free(out);
    }
    free(x);
}

/* ---------------------------------------------------------------- which way a batch goes: host_batch_route() and pipe_plan() against a table
 * (every row confirmed against the code before the two functions existed: the pipeline rows by its LZS_STREAM_DEBUG line, the
 * others by the stage lines and the scan launches of the same shapes, and by reading its conditions) */
static void routes(void)
{
    lzs_env_t dflt, one_wave, seg8, serial;
    memset(&dflt, 0, sizeof dflt);                                  /* no switch set */
    one_wave = seg8 = serial = dflt;
    one_wave.one_wave = 1; seg8.batch_seg_mb = 8; serial.overlap_off = 1;
    const launch_fn C = lzs_hip_launch_compress, D = lzs_hip_launch_decompress;
    const uint32_t cmax = LZS_COMPRESSED_MAX(65536);
    enum { SEGMENTS, PIPELINE, SERIAL_OFFERED, SERIAL_NOT_OFFERED };   /* (serial: one after the other; offered: to the pipeline, which declined) */
    const struct { const char *what; launch_fn op; uint32_t cap; size_t nb, in_len; const lzs_env_t *env; int want; size_t chunk, K, G, J; } rows[] = {
        { "256 blocks", D, 65536, 256, 36000, &dflt, SEGMENTS, 0, 0, 0, 0 },
        { "1024 blocks: 64 MiB of extent exactly", D, 65536, 1024, 36000, &dflt, SEGMENTS, 0, 0, 0, 0 },
        { "1025 blocks", D, 65536, 1025, 36000, &dflt, PIPELINE, 320, 4, 4, 1 },
        { "1000 blocks, streams of 500 bytes: the preserved corner", D, 65536, 1000, 500, &dflt, SERIAL_NOT_OFFERED, 0, 0, 0, 0 },
        { "5000 blocks of 4096: over 4096 blocks, 19.5 MiB", D, 4096, 5000, 2400, &dflt, SERIAL_OFFERED, 0, 0, 0, 0 },
        { "256 blocks, LZS_ONE_WAVE", D, 65536, 256, 36000, &one_wave, SERIAL_OFFERED, 0, 0, 0, 0 },
        { "256 blocks, LZS_BATCH_SEG_MB=8: 16 MiB", D, 65536, 256, 36000, &seg8, SERIAL_OFFERED, 0, 0, 0, 0 },
        { "1024 blocks, LZS_ONE_WAVE", D, 65536, 1024, 36000, &one_wave, PIPELINE, 256, 4, 4, 1 },
        { "compress, 416 blocks: three chunks of 128 and a short fourth", C, cmax, 416, 65536, &dflt, PIPELINE, 128, 4, 2, 2 },
        { "compress, 2597 blocks", C, cmax, 2597, 65536, &dflt, PIPELINE, 640, 5, 2, 3 },
        { "compress, 37 blocks", C, cmax, 37, 65536, &dflt, SERIAL_OFFERED, 0, 0, 0, 0 },
        { "compress, 416 blocks, LZS_HOST_SERIAL", C, cmax, 416, 65536, &serial, SERIAL_OFFERED, 0, 0, 0, 0 },
        { "compress, no capacity", C, 0, 416, 65536, &dflt, SERIAL_OFFERED, 0, 0, 0, 0 },
        { "decompress, no capacity", D, 0, 1025, 36000, &dflt, SERIAL_OFFERED, 0, 0, 0, 0 },
    };
    for (unsigned i = 0; i < sizeof rows / sizeof rows[0]; i++) {
        const size_t d_in = round16(rows[i].in_len), d_out = round16(rows[i].cap ? rows[i].cap : 1);
        const batch_route_t r = host_batch_route(rows[i].op, rows[i].cap, rows[i].nb, d_in, d_out, rows[i].nb * rows[i].in_len, rows[i].env);
        const pipe_plan_t pl = pipe_plan(rows[i].op, rows[i].cap, rows[i].nb, rows[i].in_len, rows[i].env);
        const int got = r == ROUTE_SEGMENTS ? SEGMENTS : r == ROUTE_SERIAL ? SERIAL_NOT_OFFERED : pl.taken ? PIPELINE : SERIAL_OFFERED;
        CHECK(got == rows[i].want, "%s: route %d (host_batch_route %d, pipe_plan taken %d), expected %d", rows[i].what, got, (int)r, pl.taken, rows[i].want);
        if (got == PIPELINE && rows[i].want == PIPELINE)
            CHECK(pl.chunk == rows[i].chunk && pl.K == rows[i].K && pl.G == rows[i].G && pl.J == rows[i].J && pl.slots == (pl.J < 3 ? pl.J : 3) && pl.threads == 4,
                  "%s: %zu chunks of %zu, %zu a launch, %zu launches, %zu slots, %d threads", rows[i].what, pl.K, pl.chunk, pl.G, pl.J, pl.slots, pl.threads);
    }
}

/* ---------------------------------------------------------------- the one-after-the-other route's copy layouts, where they switch
 * (one copy / a copy per block below 16 blocks / pinned pieces laid out by the CPU on the way in; a copy per block / one copy of
 * full blocks / compact + pieces + layout on the way out).  `want` / `want_len`: blocks at `wstride`. */
static void lay_check(const char *what, size_t nb, const uint8_t *got, size_t stride, size_t cap, const uint32_t *got_len,
                      const uint8_t *want, size_t wstride, const uint32_t *want_len, uint8_t fill)
{
    for (size_t b = 0; b < nb; b++) {
        CHECK(got_len[b] == want_len[b] && memcmp(got + b * stride, want + b * wstride, want_len[b]) == 0, "%s, %zu blocks: block %zu differs (%u bytes, %u expected)",
              what, nb, b, got_len[b], want_len[b]);
        for (size_t i = want_len[b]; i < stride; i++)
            if (got[b * stride + i] != fill) { CHECK(0, "%s, %zu blocks: block %zu: byte %zu past its length (capacity %zu) touched", what, nb, b, i, cap); break; }
    }
    CHECK(got[nb * stride] == fill, "%s, %zu blocks: the byte past the array touched", what, nb);
}

static void layouts(void)
{
    enum { LEN = 4096, CAP = LZS_COMPRESSED_MAX(LEN), S16 = (CAP + 15) / 16 * 16, RSTRIDE = LEN + 5, NBMAX = 17 };
    uint8_t *x = sample(1, (size_t)NBMAX * LEN, 50), *xr = (uint8_t *)calloc(NBMAX, RSTRIDE);
    uint8_t *want = (uint8_t *)malloc(NBMAX * S16), *got = (uint8_t *)malloc(NBMAX * S16 + 1), *comp = (uint8_t *)malloc(NBMAX * S16 + 1);
    uint8_t *back = (uint8_t *)malloc((size_t)NBMAX * RSTRIDE + 1);
    static const size_t counts[4] = { 1, 15, 16, 17 };
    for (unsigned ci = 0; ci < 4; ci++) {
        const size_t nb = counts[ci], mid = nb / 2;
        uint32_t full[NBMAX], ragged[NBMAX], want_len[NBMAX], got_len[NBMAX], comp_len[NBMAX], back_len[NBMAX];
        for (size_t b = 0; b < nb; b++) {
            full[b] = LEN;
            ragged[b] = b % 3 == 1 ? 0 : rnd_in(1, LEN);
            memcpy(xr + b * RSTRIDE, x + b * LEN, LEN);
        }
        /* compress: (a) uniform blocks at the device stride in, into slots of a 16-aligned stride; (b) ragged and strided in */
        for (size_t b = 0; b < nb; b++) want_len[b] = (uint32_t)lzs_oracle_compress(want + b * S16, CAP, x + b * LEN, LEN);
        memset(comp, 0xA5, nb * S16 + 1);
        CHECK(lzs_compress_batch(comp, S16, CAP, comp_len, x, LEN, NULL, LEN, nb) == 0, "compress (a), %zu blocks: %s", nb, lzs_last_error());
        lay_check("compress (a)", nb, comp, S16, CAP, comp_len, want, S16, want_len, 0xA5);
        for (size_t b = 0; b < nb; b++) want_len[b] = (uint32_t)lzs_oracle_compress(want + b * S16, CAP, x + b * LEN, ragged[b]);
        memset(got, 0xA5, nb * S16 + 1);
        CHECK(lzs_compress_batch(got, CAP + 2, CAP, got_len, xr, RSTRIDE, ragged, LEN, nb) == 0, "compress (b), %zu blocks: %s", nb, lzs_last_error());
        lay_check("compress (b)", nb, got, CAP + 2, CAP, got_len, want, S16, want_len, 0xA5);
        /* ... and back: (b) ragged streams with empty ones among them, strided in and out */
        memset(back, 0x5A, nb * RSTRIDE + 1);
        CHECK(lzs_decompress_batch(back, RSTRIDE, LEN, back_len, got, CAP + 2, got_len, CAP, nb) == 0, "decompress (b), %zu blocks: %s", nb, lzs_last_error());
        lay_check("decompress (b)", nb, back, RSTRIDE, LEN, back_len, x, LEN, ragged, 0x5A);
        /* compress (c): capacity = stride = 16 and every block full, the one-copy way out; (d) the middle block short */
        for (int d = 0; d < 2; d++) {
            if (d) full[mid] = 3;
            for (size_t b = 0; b < nb; b++) want_len[b] = (uint32_t)lzs_oracle_compress(want + b * S16, 16, x + b * LEN, full[b]);
            CHECK(d ? want_len[mid] < 16 : want_len[mid] == 16, "compress (%c): the middle block gives %u bytes", "cd"[d], want_len[mid]);
            memset(got, 0xA5, nb * S16 + 1);
            CHECK(lzs_compress_batch(got, 16, 16, got_len, x, LEN, d ? full : NULL, LEN, nb) == 0, "compress (%c), %zu blocks: %s", "cd"[d], nb, lzs_last_error());
            lay_check(d ? "compress (d)" : "compress (c)", nb, got, 16, 16, got_len, want, S16, want_len, 0xA5);
            full[mid] = LEN;
        }
        /* decompress: (a) uniform lengths at the device stride in (the streams end before their slots do), (c) capacity = stride
         * and every block full out; (d) the middle block's stream that of a shorter block */
        for (int d = 0; d < 2; d++) {
            if (d) {
                full[mid] = 1000;
                memset(comp + mid * S16, 0xA5, S16);
                lzs_oracle_compress(comp + mid * S16, CAP, x + mid * LEN, 1000);
            }
            memset(back, 0x5A, nb * RSTRIDE + 1);
            CHECK(lzs_decompress_batch(back, LEN, LEN, back_len, comp, S16, NULL, S16, nb) == 0, "decompress (%s), %zu blocks: %s", d ? "a, d" : "a, c", nb, lzs_last_error());
            lay_check(d ? "decompress (a, d)" : "decompress (a, c)", nb, back, LEN, LEN, back_len, x, LEN, full, 0x5A);
        }
    }
    free(x); free(xr); free(want); free(got); free(comp); free(back);
}

/* ---------------------------------------------------------------- the overlapped pipeline (>= 24 MiB), two threads at once */
typedef struct { unsigned cls; int id; } pipe_job_t;
static void *pipeline_once(void *argp)
{
    const pipe_job_t *job = (const pipe_job_t *)argp;
    enum { NB = 416 };                                              /* 26 MiB of input: four chunks of 128 and a short fifth */
    const size_t cap = LZS_COMPRESSED_MAX(65536), ostride = cap + 13;
    uint8_t *x = sample(job->cls, (size_t)NB * 65536, 100 * (uint64_t)job->id);
    uint8_t *out = (uint8_t *)malloc(NB * ostride), *want = (uint8_t *)malloc(cap);
    uint32_t *out_len = (uint32_t *)calloc(NB, 4), *lens = (uint32_t *)malloc(NB * 4);
    for (int b = 0; b < NB; b++) lens[b] = b % 5 == 0 ? 65536 : 1 + (uint32_t)((b * 2654435761u) % 65536u);
    for (int ragged = 0; ragged < 2; ragged++) {
        memset(out, 0xA5, NB * ostride);
        const int rc = lzs_compress_batch(out, ostride, cap, out_len, x, 65536, ragged ? lens : NULL, 65536, NB);
        CHECK(rc == 0, "thread %d: lzs_compress_batch: %s", job->id, lzs_last_error());
        for (int b = 0; b < NB; b += (b < 8 ? 1 : 23)) {
            const size_t w = lzs_oracle_compress(want, cap, x + (size_t)b * 65536, ragged ? lens[b] : 65536);
            CHECK(out_len[b] == w && memcmp(out + b * ostride, want, w) == 0, "thread %d: block %d differs", job->id, b);
            CHECK(out[b * ostride + w] == 0xA5, "thread %d: block %d: byte past its length touched", job->id, b);
        }
        uint8_t *back = (uint8_t *)malloc((size_t)NB * 65540);
        uint32_t *back_len = (uint32_t *)calloc(NB, 4);
        memset(back, 0x5A, (size_t)NB * 65540);
        CHECK(lzs_decompress_batch(back, 65540, 65536, back_len, out, ostride, out_len, cap, NB) == 0, "thread %d: lzs_decompress_batch: %s", job->id, lzs_last_error());
        for (int b = 0; b < NB; b++) {
            const uint32_t n = ragged ? lens[b] : 65536;
            if (back_len[b] != n || memcmp(back + (size_t)b * 65540, x + (size_t)b * 65536, n) != 0) { CHECK(0, "thread %d: block %d: round trip", job->id, b); break; }
            if (back[(size_t)b * 65540 + 65536] != 0x5A) { CHECK(0, "thread %d: block %d: past the capacity", job->id, b); break; }
        }
        free(back); free(back_len);
    }
    free(x); free(out); free(want); free(out_len); free(lens);
    return NULL;
}
static void pipeline(void)
{
    pthread_t th[2];
    pipe_job_t jobs[2] = { { 1, 0 }, { 1, 1 } };                    /* (low-entropy blocks: the oracle behind the launches is fast on them) */
    for (int i = 0; i < 2; i++) pthread_create(&th[i], NULL, pipeline_once, &jobs[i]);
    for (int i = 0; i < 2; i++) pthread_join(th[i], NULL);
    /* the degrade path: the ring does not fit, the batch takes the one-after-the-other route and succeeds */
    setenv("LZS_STAGING_FAIL_MB", "30", 1);
    pipe_job_t one = { 1, 2 };
    pipeline_once(&one);
    unsetenv("LZS_STAGING_FAIL_MB");
}

/* ---------------------------------------------------------------- one stream in segments (dirty re-entry), both routes */
static void one_shot_streams(void)
{
    uint8_t *t = sample(0, 300000, 7), *r = sample(2, 70000, 9);
    const size_t n_mix = 50000 + 70000 + 40000 + 80000 + 30000 + 5;
    uint8_t *mix = (uint8_t *)calloc(n_mix, 1);
    size_t at = 0;
    memcpy(mix, t, 50000); at = 50000 + 70000;                      /* 70 000 zeros: a run over many segments */
    memcpy(mix + at, t + 50000, 40000); at += 40000;
    for (size_t i = 0; i < 80000; i++) mix[at + i] = "ab"[i & 1];   /* period 2 over many segments */
    at += 80000;
    memcpy(mix + at, r, 30000); at += 30000 + 5;
    const struct { const uint8_t *d; size_t n; } cases[] = { { t, 1 }, { t, 4096 }, { t, 6145 }, { t, 20000 }, { t, 300000 }, { mix, n_mix }, { r, 70000 } };
    const char *routes[] = { "device", "host" };
    for (unsigned ri = 0; ri < 2; ri++) {
        setenv("LZS_ROUTE", routes[ri], 1);
        for (unsigned ci = 0; ci < sizeof cases / sizeof cases[0]; ci++) {
            const size_t n = cases[ci].n, cap = LZS_COMPRESSED_MAX(n);
            uint8_t *want = (uint8_t *)malloc(cap), *got = (uint8_t *)malloc(cap + 8), *back = (uint8_t *)malloc(n + 8);
            const size_t w = lzs_oracle_compress(want, cap, cases[ci].d, n);
            memset(got, 0xA5, cap + 8);
            const size_t g = lzs_compress(got, cap, cases[ci].d, n);
            CHECK(g == w && memcmp(got, want, w) == 0 && got[cap] == 0xA5, "%s route: lzs_compress of %zu bytes differs (%zu / %zu): %s", routes[ri], n, g, w, lzs_last_error());
            for (int k = 0; k < 3; k++) {                            /* cut capacities: the stream is cut, never altered */
                const size_t cut = k == 0 ? 0 : rnd_in(1, (uint32_t)w);
                memset(got, 0xA5, cap + 8);
                const size_t gc = lzs_compress(got, cut, cases[ci].d, n);
                CHECK(gc == cut && memcmp(got, want, cut) == 0 && got[cut] == 0xA5, "%s route: lzs_compress of %zu bytes into %zu differs", routes[ri], n, cut);
            }
            memset(back, 0x5A, n + 8);
            const size_t b = lzs_decompress(back, n + 3, want, w);
            CHECK(b == n && memcmp(back, cases[ci].d, n) == 0 && back[n + 3] == 0x5A, "%s route: lzs_decompress to %zu bytes differs (%zu)", routes[ri], n, b);
            const size_t half = lzs_decompress(back, n / 2, want, w);
            CHECK(half == n / 2 && memcmp(back, cases[ci].d, n / 2) == 0, "%s route: lzs_decompress into half the room", routes[ri]);
            free(want); free(got); free(back);
        }
    }
    unsetenv("LZS_ROUTE");
    free(t); free(r); free(mix);
}

/* ---------------------------------------------------------------- the incremental interface in random pieces, both routes */
/* What every call did ("inctrace"): a 64-bit FNV-1a over one record a call -- bytes returned, how far the two lengths and the two
 * pointers moved, and the caller's block from offset 32 to its end (the status byte and reserved_, private bytes included; the
 * pointers and lengths in front are left out as values because addresses differ from run to run). */
typedef struct { uint64_t h; size_t calls, bytes; } trace_t;
static trace_t *tracing;                 /* != NULL: encode_pieces() and decode_pieces() record their calls here */
static void trace_call(trace_t *t, size_t made, const size_t before[4], const size_t after[4], const void *block, size_t block_size)
{
    uint64_t rec[5] = { made, before[0] - after[0], before[1] - after[1], after[2] - before[2], after[3] - before[3] };
    const uint8_t *parts[2] = { (const uint8_t *)rec, (const uint8_t *)block + 32 };
    const size_t lens[2] = { sizeof rec, block_size - 32 };
    if (!t->calls) t->h = 0xCBF29CE484222325ull;
    for (int k = 0; k < 2; k++)
        for (size_t i = 0; i < lens[k]; i++) t->h = (t->h ^ parts[k][i]) * 0x100000001B3ull;
    t->calls++; t->bytes += made;
}
/* (inLength, outLength, inPtr, outPtr of any of the three blocks: they start alike) */
static void trace_moved(size_t v[4], const void *block)
{
    const LzsDecompressParameters_t *p = (const LzsDecompressParameters_t *)block;
    v[0] = p->inLength; v[1] = p->outLength; v[2] = (size_t)p->inPtr; v[3] = (size_t)p->outPtr;
}

static size_t encode_pieces(const uint8_t *d, size_t n, uint8_t *out, size_t out_cap, uint32_t in_lo, uint32_t in_hi, uint32_t out_lo, uint32_t out_hi, int simple)
{
    LzsCompressParameters_t *p = (LzsCompressParameters_t *)malloc(sizeof *p);
    LzsSimpleCompressParameters_t *q = (LzsSimpleCompressParameters_t *)malloc(sizeof *q);
    if (simple) lzs_simple_compress_init(q); else lzs_compress_init(p);
    size_t pos = 0, made = 0, pending = 0, calls = 0;
    const uint8_t *pend_ptr = d;
    int finish = 0;
    uint8_t status = 0;
    while (!(status & LZS_C_STATUS_END_MARKER)) {
        if (!pending && !finish) {
            if (pos < n) { pending = rnd_in(in_lo, in_hi); if (pending > n - pos) pending = n - pos; pend_ptr = d + pos; pos += pending; }
            if (!pending && pos >= n) finish = 1;
        }
        size_t room = rnd_in(out_lo, out_hi);
        if (room > out_cap - made) room = out_cap - made;
        size_t got, before[4], after[4];
        if (simple) {
            q->inPtr = pend_ptr; q->inLength = pending; q->outPtr = out + made; q->outLength = room;
            trace_moved(before, q);
            got = lzs_simple_compress_incremental(q, finish);
            pend_ptr = q->inPtr; pending = q->inLength; status = q->status;
        } else {
            p->inPtr = pend_ptr; p->inLength = pending; p->outPtr = out + made; p->outLength = room;
            trace_moved(before, p);
            got = lzs_compress_incremental(p, finish);
            pend_ptr = p->inPtr; pending = p->inLength; status = p->status;
        }
        trace_moved(after, simple ? (void *)q : (void *)p);
        if (tracing) trace_call(tracing, got, before, after, simple ? (void *)q : (void *)p, simple ? sizeof *q : sizeof *p);
        made += got;
        if (status & LZS_C_STATUS_ERROR) { CHECK(0, "incremental compression reported ERROR: %s", lzs_last_error()); break; }
        if (++calls > 4000000) { CHECK(0, "incremental compression: no progress"); break; }
    }
    free(p); free(q);
    return made;
}

/* (on a block the caller keeps: what it learnt from one buffer is there for the next) */
static size_t decode_pieces_on(LzsDecompressParameters_t *p, const uint8_t *s, size_t n, uint8_t *out, size_t out_cap, uint32_t in_lo, uint32_t in_hi, uint32_t out_lo, uint32_t out_hi)
{
    size_t pos = 0, made = 0, pending = 0, calls = 0;
    const uint8_t *pend_ptr = s;
    for (;;) {
        if (!pending && pos < n) { pending = rnd_in(in_lo, in_hi); if (pending > n - pos) pending = n - pos; pend_ptr = s + pos; pos += pending; }
        size_t room = rnd_in(out_lo, out_hi);
        if (room > out_cap - made) room = out_cap - made;
        p->inPtr = pend_ptr; p->inLength = pending; p->outPtr = out + made; p->outLength = room;
        size_t before[4], after[4];
        trace_moved(before, p);
        const size_t got = lzs_decompress_incremental(p);
        trace_moved(after, p);
        if (tracing) trace_call(tracing, got, before, after, p, sizeof *p);
        made += got;
        pend_ptr = p->inPtr; pending = p->inLength;
        if (p->status & LZS_D_STATUS_ERROR) { CHECK(0, "incremental decompression reported ERROR: %s", lzs_last_error()); break; }
        if (!pending && pos >= n && (p->status & LZS_D_STATUS_INPUT_STARVED)) break;
        if (++calls > 4000000) { CHECK(0, "incremental decompression: no progress"); break; }
    }
    return made;
}

static size_t decode_pieces(const uint8_t *s, size_t n, uint8_t *out, size_t out_cap, uint32_t in_lo, uint32_t in_hi, uint32_t out_lo, uint32_t out_hi, uint8_t *status)
{
    LzsDecompressParameters_t *p = (LzsDecompressParameters_t *)malloc(sizeof *p);
    lzs_decompress_init(p);
    const size_t made = decode_pieces_on(p, s, n, out, out_cap, in_lo, in_hi, out_lo, out_hi);
    if (status) *status = p->status;
    free(p);
    return made;
}

static void incremental(void)
{
    uint8_t *t = sample(0, 200000, 11), *low = sample(1, 200000, 12);
    const size_t n_mix = 30000 + 40000 + 30000 + 20000;
    uint8_t *mix = (uint8_t *)calloc(n_mix, 1);
    memcpy(mix, t, 30000); memcpy(mix + 70000, t + 30000, 30000);
    for (size_t i = 0; i < 20000; i++) mix[100000 + i] = "abc"[i % 3];
    const struct { const uint8_t *d; size_t n; } cases[] = { { t, 507 }, { t, 90000 }, { low, 200000 }, { mix, n_mix } };
    const char *routes[] = { "device", "host" };
    for (unsigned ri = 0; ri < 2; ri++) {
        setenv("LZS_ROUTE", routes[ri], 1);
        for (unsigned ci = 0; ci < sizeof cases / sizeof cases[0]; ci++) {
            const size_t n = cases[ci].n, cap = LZS_COMPRESSED_MAX(n) + 64;
            uint8_t *want = (uint8_t *)malloc(cap), *got = (uint8_t *)malloc(cap), *back = (uint8_t *)malloc(n + 64);
            const size_t w = lzs_oracle_compress(want, cap, cases[ci].d, n);
            const uint32_t ranges[][4] = { { 1, 60, 3, 60 }, { 100, 5000, 100, 5000 }, { 20000, 90000, 20000, 90000 }, { 512, 512, 512, 512 } };
            for (unsigned k = 0; k < 4; k++) {
                if (ranges[k][0] == 1 && n > 100000) continue;      /* (tiny pieces of the long cases: time) */
                const size_t g = encode_pieces(cases[ci].d, n, got, cap, ranges[k][0], ranges[k][1], ranges[k][2], ranges[k][3], 0);
                CHECK(g == w && memcmp(got, want, w) == 0, "%s route: incremental compression of case %u in pieces of %u..%u differs (%zu / %zu)", routes[ri], ci, ranges[k][0], ranges[k][1], g, w);
                const size_t b = decode_pieces(want, w, back, n + 64, ranges[k][0], ranges[k][1], ranges[k][2], 3 * ranges[k][3], NULL);
                CHECK(b == n && memcmp(back, cases[ci].d, n) == 0, "%s route: incremental decompression of case %u in pieces of %u..%u differs (%zu / %zu)", routes[ri], ci, ranges[k][0], ranges[k][1], b, n);
            }
            if (n <= 90000) {                                       /* the low-memory block: 1-12 bytes of room, random pieces */
                const size_t m = n < 20000 ? n : 20000;
                const size_t w2 = lzs_oracle_compress(want, cap, cases[ci].d, m);
                const size_t g = encode_pieces(cases[ci].d, m, got, cap, 1, 300, 1, 12, 1);
                CHECK(g == w2 && memcmp(got, want, w2) == 0, "%s route: lzs_simple_compress_incremental of case %u with 1..12 bytes of room differs (%zu / %zu)", routes[ri], ci, g, w2);
            }
            free(want); free(got); free(back);
        }
    }
    unsetenv("LZS_ROUTE");
    free(t); free(low); free(mix);
}

/* ---------------------------------------------------------------- what every call of the incremental interface does, against a table
 * The cases above compare the bytes of a whole stream; this one compares call by call (trace_call) how much each call produced
 * and consumed, which flags it reported and what it left in the caller's block -- every byte of it.  The rows were recorded with
 * this driver linked against lzs_incremental.c as it was BEFORE its stages became functions (both routes; the device route over
 * the shim, by many wavefronts where the code sends a piece there), never from the code under test. */
typedef struct { const char *name; size_t calls, bytes; uint64_t digest; } trace_row_t;
static const trace_row_t trace_rows[2][17] = {
    { /* LZS_ROUTE=device (with the hash of the shim calls made: on this route no row is the host route's) */
        { "full/compress 1..60 into 3..60", 4499, 51125, 0x49178E3BCB15924Bull },
        { "full/decode 1..60 into 3..180", 2226, 90000, 0xBDBE8C00F5D5B27Bull },
        { "full/compress 100..5000 into 100..5000", 53, 51125, 0xC97BF946AD0CFEC8ull },
        { "full/decode 100..5000 into 100..15000", 27, 90000, 0x2EDB536B2CE23E57ull },
        { "full/compress 512..512 into 512..512", 265, 51125, 0x4EF2F224AA12DA0Cull },
        { "full/decode 512..512 into 512..1536", 146, 90000, 0xE758CBA6C2F78E8Dull },
        { "full/compress 20000..90000 into 20000..90000", 4, 51125, 0x40C11B12FAF75C73ull },
        { "full/decode 20000..90000 into 20000..270000", 3, 90000, 0x127489AF31CBB11Aull },
        { "simple/compress 1..300 into 1..12", 2085, 11194, 0x450E4BAFC997350Eull },
        { "full/compress 30000..60000 into 1..200", 74, 7769, 0x0871EB276692A755ull },
        { "three/decode 16384..16384 into 1048576..1048576", 8, 150000, 0x1E2A9690E512B8EBull },
        { "three/decode 20000..90000 into 5000..400000", 5, 150000, 0xC51F35D97D2AC515ull },
        { "big/decode 1.5..3 MiB into 8 MiB", 3, 5600000, 0xCE1D8B18846D757Eull },
        { "shrink/decode the long stream, then three short ones and the long one in one piece", 8, 11350000, 0xCA79FAD221787533ull },
        { "fail/decode: NULL input, then a call after the ERROR", 3, 254, 0x8D3171838FFBA717ull },
        { "fail/compress: a block that was not initialised", 1, 0, 0x06E3D09CFAF921F4ull },
    },
    { /* LZS_ROUTE=host: no shim call at all; what the calls do is the device route's call by call -- the same contract -- but
       * for the pass size, which only the device route learns.  That the many wavefronts ran there is the scan count's to say. */
        { "full/compress 1..60 into 3..60", 4499, 51125, 0xE99202551398A8BEull },
        { "full/decode 1..60 into 3..180", 2226, 90000, 0x0111F10AED5FBC26ull },
        { "full/compress 100..5000 into 100..5000", 53, 51125, 0xEA740366AC5A9486ull },
        { "full/decode 100..5000 into 100..15000", 27, 90000, 0x15F072017A954CFCull },
        { "full/compress 512..512 into 512..512", 265, 51125, 0xB229E93F83AED434ull },
        { "full/decode 512..512 into 512..1536", 146, 90000, 0x783A1EED04CC0115ull },
        { "full/compress 20000..90000 into 20000..90000", 4, 51125, 0x80F021A4617DFC2Cull },
        { "full/decode 20000..90000 into 20000..270000", 3, 90000, 0x25EC1E9B8AE3D189ull },
        { "simple/compress 1..300 into 1..12", 2085, 11194, 0xAB6B967145181B1Aull },
        { "full/compress 30000..60000 into 1..200", 74, 7769, 0xBE9A74C69828BE7Eull },
        { "three/decode 16384..16384 into 1048576..1048576", 8, 150000, 0x37FBBC45D62BD9BAull },
        { "three/decode 20000..90000 into 5000..400000", 5, 150000, 0xDBF068947C9315E7ull },
        { "big/decode 1.5..3 MiB into 8 MiB", 3, 5600000, 0x8A70ED9C2EF552EAull },
        { "shrink/decode the long stream, then three short ones and the long one in one piece", 8, 11350000, 0x3A2A8552E12ECCBFull },
        { "fail/decode: NULL input, then a call after the ERROR", 3, 254, 0xFCB19CFF497AA940ull },
        { "fail/compress: a block that was not initialised", 1, 0, 0x06E3D09CFAF921F4ull },
    },
};
unsigned lzs_shim_scan_launches(void);
uint64_t lzs_shim_call_hash(int reset);
static int trace_print;                  /* "inctrace-rows": print the rows instead of comparing them */
/* (every scenario draws its piece sizes from a seed of its own: a scenario that goes wrong leaves the others' pieces alone) */
/* ... and starts with nothing kept by the thread, so that the shim's hash of the calls made -- folded into the digest at the end:
 * the same syncs, copies, launches and allocations in the same order -- does not depend on what ran before) */
static void trace_begin(trace_t *t, unsigned scenario)
{
    tracing = t; rng_state = 0x9E3779B97F4A7C15ull * (scenario + 1u);
    lzs_release_thread_cache();
    lzs_shim_call_hash(1);
}
static void trace_done(unsigned ri, const char *name, trace_t *t)
{
    tracing = NULL;
    const uint64_t calls_made = lzs_shim_call_hash(1);
    for (size_t i = 0; i < sizeof calls_made; i++) t->h = (t->h ^ ((const uint8_t *)&calls_made)[i]) * 0x100000001B3ull;
    if (trace_print) { printf("        { \"%s\", %zu, %zu, 0x%016llXull },\n", name, t->calls, t->bytes, (unsigned long long)t->h); memset(t, 0, sizeof *t); return; }
    const trace_row_t *row = NULL;
    for (unsigned i = 0; i < 17 && trace_rows[ri][i].name; i++) if (!strcmp(trace_rows[ri][i].name, name)) row = &trace_rows[ri][i];
    CHECK(row, "route %u, %s: no row in the table", ri, name);
    if (row) CHECK(row->calls == t->calls && row->bytes == t->bytes && row->digest == t->h, "route %u, %s: %zu calls, %zu bytes, digest %016llx; recorded: %zu, %zu, %016llx",
                   ri, name, t->calls, t->bytes, (unsigned long long)t->h, row->calls, row->bytes, (unsigned long long)row->digest);
    memset(t, 0, sizeof *t);
}

/* the terminal failures: a NULL input with a length, then a good call on the same block; a block that was never initialised */
static void trace_failures(unsigned ri, const uint8_t *stream, size_t n)
{
    trace_t t = { 0, 0, 0 };
    size_t before[4], after[4];
    uint8_t out[600];
    LzsDecompressParameters_t *d = (LzsDecompressParameters_t *)malloc(sizeof *d);
    lzs_decompress_init(d);
    trace_begin(&t, 14);
    for (int call = 0; call < 3; call++) {                          /* a good call, the bad one, a call after the ERROR */
        d->inPtr = call == 1 ? NULL : stream + 100 * (call / 2); d->inLength = call == 1 ? 77 : 100; d->outPtr = out; d->outLength = sizeof out;
        trace_moved(before, d);
        const size_t got = lzs_decompress_incremental(d);
        trace_moved(after, d);
        trace_call(&t, got, before, after, d, sizeof *d);
        CHECK(!(d->status & LZS_D_STATUS_ERROR) == (call != 1) && d->inLength == 0, "decode call %d: status %02x, %zu bytes of input left", call, d->status, d->inLength);
    }
    trace_done(ri, "fail/decode: NULL input, then a call after the ERROR", &t);
    free(d);
    LzsCompressParameters_t *c = (LzsCompressParameters_t *)malloc(sizeof *c);
    memset(c, 0xFF, sizeof *c);
    trace_begin(&t, 15);
    c->inPtr = stream; c->inLength = n < 3000 ? n : 3000; c->outPtr = out; c->outLength = sizeof out;
    trace_moved(before, c);
    const size_t got = lzs_compress_incremental(c, false);
    trace_moved(after, c);
    trace_call(&t, got, before, after, c, sizeof *c);
    CHECK(c->status == (LZS_C_STATUS_ERROR | LZS_C_STATUS_END_MARKER | LZS_C_STATUS_INPUT_STARVED | LZS_C_STATUS_INPUT_FINISHED) && c->inLength == 0 && c->inPtr == stream + (n < 3000 ? n : 3000),
          "a block that was not initialised: status %02x", c->status);
    trace_done(ri, "fail/compress: a block that was not initialised", &t);
    free(c);
}

static void inctrace(void)
{
    enum { N_TEXT = 90000, N_SIMPLE = 20000, N_LOW = 200000, N_BIG = 5600000 };
    uint8_t *text = sample(0, N_BIG, 61), *low = sample(1, N_LOW, 62), *rnd3 = sample(2, 30000, 63);
    const size_t cap = LZS_COMPRESSED_MAX(N_BIG) + 64;
    uint8_t *want = (uint8_t *)malloc(cap), *got = (uint8_t *)malloc(cap), *back = (uint8_t *)malloc(150000 + N_BIG + 64);
    /* three streams back to back, each with its end marker: text, zeros and then text, random bytes */
    uint8_t *three_plain = (uint8_t *)calloc(40000 + 80000 + 30000, 1), *three = (uint8_t *)malloc(LZS_COMPRESSED_MAX(150000) + 64);
    memcpy(three_plain, text + 100000, 40000); memcpy(three_plain + 100000, text + 140000, 20000); memcpy(three_plain + 120000, rnd3, 30000);
    size_t n_three = lzs_oracle_compress(three, LZS_COMPRESSED_MAX(40000), three_plain, 40000);
    n_three += lzs_oracle_compress(three + n_three, LZS_COMPRESSED_MAX(80000), three_plain + 40000, 80000);
    n_three += lzs_oracle_compress(three + n_three, LZS_COMPRESSED_MAX(30000), three_plain + 120000, 30000);
    uint8_t *big = (uint8_t *)malloc(cap);
    const size_t n_big = lzs_oracle_compress(big, cap, text, N_BIG);            /* ~3 MiB of compressed text */
    CHECK(n_big > 2900000 && n_big < 3400000, "the long stream has %zu bytes", n_big);
    uint8_t *mixed = (uint8_t *)malloc(n_three + n_big);
    memcpy(mixed, three, n_three); memcpy(mixed + n_three, big, n_big);
    const char *routes[] = { "device", "host" };
    const uint64_t rng_before = rng_state;
    unsetenv("LZS_ONE_WAVE");                                       /* the device route as a caller gets it: large pieces by many wavefronts */
    for (unsigned ri = 0; ri < 2; ri++) {
        setenv("LZS_ROUTE", routes[ri], 1);
        if (trace_print) printf("    { /* LZS_ROUTE=%s */\n", routes[ri]);
        trace_t t = { 0, 0, 0 };
        char name[96];
        /* the full block, 90 000 bytes of text: the ranges of "incremental" (on the device route: the box, staged copies, many wavefronts) */
        const size_t w = lzs_oracle_compress(want, cap, text, N_TEXT);
        const uint32_t ranges[][4] = { { 1, 60, 3, 60 }, { 100, 5000, 100, 5000 }, { 512, 512, 512, 512 }, { 20000, 90000, 20000, 90000 } };
        for (unsigned k = 0; k < 4; k++) {
            trace_begin(&t, 2 * k);
            const size_t g = encode_pieces(text, N_TEXT, got, cap, ranges[k][0], ranges[k][1], ranges[k][2], ranges[k][3], 0);
            CHECK(g == w && memcmp(got, want, w) == 0, "%s route: pieces of %u..%u: the stream differs", routes[ri], ranges[k][0], ranges[k][1]);
            snprintf(name, sizeof name, "full/compress %u..%u into %u..%u", ranges[k][0], ranges[k][1], ranges[k][2], ranges[k][3]);
            trace_done(ri, name, &t);
            trace_begin(&t, 2 * k + 1);
            const size_t b = decode_pieces(want, w, back, N_TEXT + 64, ranges[k][0], ranges[k][1], ranges[k][2], 3 * ranges[k][3], NULL);
            CHECK(b == N_TEXT && memcmp(back, text, N_TEXT) == 0, "%s route: pieces of %u..%u: the text differs", routes[ri], ranges[k][0], ranges[k][1]);
            snprintf(name, sizeof name, "full/decode %u..%u into %u..%u", ranges[k][0], ranges[k][1], ranges[k][2], 3 * ranges[k][3]);
            trace_done(ri, name, &t);
        }
        /* the low-memory block, 1-12 bytes of room: the token-counted take, `stop`, the marker behind parked output */
        const size_t w2 = lzs_oracle_compress(want, cap, text, N_SIMPLE);
        trace_begin(&t, 8);
        const size_t g2 = encode_pieces(text, N_SIMPLE, got, cap, 1, 300, 1, 12, 1);
        CHECK(g2 == w2 && memcmp(got, want, w2) == 0, "%s route: the low-memory block: the stream differs", routes[ri]);
        trace_done(ri, "simple/compress 1..300 into 1..12", &t);
        /* the full block with less room than output: parked in the block, drained over several calls, the marker waiting */
        const size_t w3 = lzs_oracle_compress(want, cap, low, N_LOW);
        trace_begin(&t, 9);
        const size_t g3 = encode_pieces(low, N_LOW, got, cap, 30000, 60000, 1, 200, 0);
        CHECK(g3 == w3 && memcmp(got, want, w3) == 0, "%s route: little room: the stream differs", routes[ri]);
        trace_done(ri, "full/compress 30000..60000 into 1..200", &t);
        /* three streams back to back: markers inside pieces, a copy running at a piece border (short: the pass size stays) */
        const uint32_t three_ranges[2][4] = { { 16384, 16384, 1u << 20, 1u << 20 }, { 20000, 90000, 5000, 400000 } };
        const unsigned scans = lzs_shim_scan_launches();
        for (unsigned k = 0; k < 2; k++) {
            trace_begin(&t, 10 + k);
            const size_t b = decode_pieces(three, n_three, back, 150000 + 64, three_ranges[k][0], three_ranges[k][1], three_ranges[k][2], three_ranges[k][3], NULL);
            CHECK(b == 150000 && memcmp(back, three_plain, 150000) == 0, "%s route: three streams in pieces of %u..%u: %zu bytes", routes[ri], three_ranges[k][0], three_ranges[k][1], b);
            snprintf(name, sizeof name, "three/decode %u..%u into %u..%u", three_ranges[k][0], three_ranges[k][1], three_ranges[k][2], three_ranges[k][3]);
            trace_done(ri, name, &t);
        }
        /* ~3 MiB of compressed text in pieces of 1.5-3 MiB: the pass size of the many-wavefront path goes up and is remembered */
        trace_begin(&t, 12);
        const size_t b5 = decode_pieces(big, n_big, back, N_BIG + 64, 3u << 19, 3u << 20, 8u << 20, 8u << 20, NULL);
        CHECK(b5 == N_BIG && memcmp(back, text, N_BIG) == 0, "%s route: the long stream: %zu bytes", routes[ri], b5);
        trace_done(ri, "big/decode 1.5..3 MiB into 8 MiB", &t);
        CHECK(ri == 1 ? lzs_shim_scan_launches() == scans : lzs_shim_scan_launches() >= scans + 8, "%s route: %u launches of the scan", routes[ri], lzs_shim_scan_launches() - scans);
        /* ... and down again, on the same block: a buffer of the three short streams and then the long one, whole -- a pass of the size
         * learnt meets an end marker in its first quarter, three times over; then the long stream makes it grow once more */
        LzsDecompressParameters_t *keeps = (LzsDecompressParameters_t *)malloc(sizeof *keeps);
        lzs_decompress_init(keeps);
        trace_begin(&t, 13);
        size_t b6 = decode_pieces_on(keeps, big, n_big, back, N_BIG + 64, 3u << 19, 3u << 20, 8u << 20, 8u << 20);
        CHECK(b6 == N_BIG && memcmp(back, text, N_BIG) == 0, "%s route: the long stream on the kept block: %zu bytes", routes[ri], b6);
        b6 = decode_pieces_on(keeps, mixed, n_three + n_big, back, 150000 + N_BIG + 64, 16u << 20, 16u << 20, 8u << 20, 8u << 20);
        CHECK(b6 == 150000 + N_BIG && memcmp(back, three_plain, 150000) == 0 && memcmp(back + 150000, text, N_BIG) == 0, "%s route: short streams, then the long one: %zu bytes", routes[ri], b6);
        trace_done(ri, "shrink/decode the long stream, then three short ones and the long one in one piece", &t);
        free(keeps);
        trace_failures(ri, big, n_big);
        if (trace_print) printf("    },\n");
    }
    unsetenv("LZS_ROUTE");
    setenv("LZS_ONE_WAVE", "1", 1);
    rng_state = rng_before;
    free(text); free(low); free(rnd3); free(want); free(got); free(back); free(three_plain); free(three); free(big); free(mixed);
}

/* ---------------------------------------------------------------- decompression by many wavefronts: scan rounds, settle rule, placement
 * (lzs_stream.c's stream_decompress() and batch_decompress_segments() over the shim's serial SCAN and DECODE).  Every call is
 * made under LZS_ONE_WAVE=1 first -- the one-wavefront route, the oracle behind it -- and then by many wavefronts in segments
 * of 256, 512 and 2048 bytes, plain, with LZS_NO_ONES=1 and with LZS_NO_MARKS=1: bytes, lengths and status must not differ. */
unsigned lzs_shim_scan_launches(void);
typedef size_t (*dec_fn)(uint8_t *, size_t, const uint8_t *, size_t);
static const char *const sd_segs[3] = { "256", "512", "2048" };
static const char *const sd_switches[3] = { NULL, "LZS_NO_ONES", "LZS_NO_MARKS" };
#define SD_EACH_FORM(si, wi) for (unsigned si = 0; si < 3; si++) for (unsigned wi = 0; wi < 3; wi++)
static void sd_form(unsigned si, unsigned wi, int on)
{
    if (on) { unsetenv("LZS_ONE_WAVE"); setenv("LZS_DEC_SEG", sd_segs[si], 1); if (sd_switches[wi]) setenv(sd_switches[wi], "1", 1); }
    else { setenv("LZS_ONE_WAVE", "1", 1); unsetenv("LZS_DEC_SEG"); if (sd_switches[wi]) unsetenv(sd_switches[wi]); }
}

static void sd_call(const char *what, dec_fn fn, const char *name, const uint8_t *s, size_t n, size_t cap)
{
    uint8_t *want = (uint8_t *)malloc(cap + 8), *got = (uint8_t *)malloc(cap + 8);
    const size_t w = fn(want, cap, s, n);
    const int w_failed = lzs_last_error()[0] != 0;
    SD_EACH_FORM(si, wi) {
        sd_form(si, wi, 1);
        memset(got, 0x5A, cap + 8);
        const unsigned scans = lzs_shim_scan_launches();
        const size_t g = fn(got, cap, s, n);
        CHECK(g == w && memcmp(got, want, w) == 0 && (lzs_last_error()[0] != 0) == w_failed,
              "%s: %s of %zu bytes into %zu, segments of %s, %s: %zu bytes, one wavefront %zu (%s)", what, name, n, cap, sd_segs[si],
              sd_switches[wi] ? sd_switches[wi] : "plain", g, w, lzs_last_error());
        CHECK(got[g <= cap ? g : cap] == 0x5A && got[cap] == 0x5A, "%s: %s of %zu bytes into %zu: a byte past the result touched", what, name, n, cap);
        CHECK(!n || !cap || lzs_shim_scan_launches() > scans, "%s: %s of %zu bytes did not go by segments", what, name, n);
        sd_form(si, wi, 0);
    }
    free(want); free(got);
}

/* a stream whole, into less room than it fills, cut short at random bytes, and with garbage after its end marker; `full`: its size */
static void sd_stream(const char *what, const uint8_t *s, size_t n, size_t full, int variants)
{
    const dec_fn fns[2] = { lzs_decompress, lzs_decompress_concat };
    const char *names[2] = { "lzs_decompress", "lzs_decompress_concat" };
    uint8_t *junk = (uint8_t *)malloc(n + 700);
    memcpy(junk, s, n);
    for (size_t i = n; i < n + 700; i++) junk[i] = (uint8_t)rnd();
    for (unsigned f = 0; f < 2; f++) {
        sd_call(what, fns[f], names[f], s, n, full + 3);
        if (full) sd_call(what, fns[f], names[f], s, n, rnd_in(1, (uint32_t)full));
        if (!variants) continue;
        for (int k = 0; k < 2 && n > 1; k++) sd_call(what, fns[f], names[f], s, rnd_in(1, (uint32_t)n - 1), full + 3);
        sd_call(what, fns[f], names[f], junk, n + 700, full + 3);
        sd_call(what, fns[f], names[f], junk, n + rnd_in(1, 700), full + 6000);
    }
    free(junk);
}

static void sd_put(uint8_t *buf, uint64_t *at, uint32_t value, unsigned width)     /* MSB first into zeroed memory */
{
    for (unsigned i = 0; i < width; i++, (*at)++)
        if ((value >> (width - 1u - i)) & 1u) buf[*at >> 3] |= (uint8_t)(0x80u >> (*at & 7u));
}

/* A stream made by hand: `q` literals (0..3), a match at offset 1 with as many nibbles of 15 as bring its closing nibble `c` to
 * the border of every segment size at byte 4096 -- the nibble ends there (q = 3) or has its last 1, 2, 3 bits behind it
 * (q = 0, 1, 2: the token before the nibbles is 9 q + 13 bits) --, then `tail` literals and the end marker.  *full: its size. */
static uint8_t *sd_run_to_border(unsigned q, unsigned c, const uint8_t *tail, size_t ntail, size_t *n, size_t *full)
{
    uint8_t *s = (uint8_t *)calloc(4096 + (9 * ntail + 9) / 8 + 8, 1);
    const unsigned inside = 4u - (q + 1u) % 4u, nibbles = (8u * 4096u - inside - 9u * q - 13u) / 4u;
    uint64_t at = 0;
    for (unsigned i = 0; i < q; i++) sd_put(s, &at, "xyA"[3 - q + i], 9);
    sd_put(s, &at, (3u << 7) | 1u, 9); sd_put(s, &at, 15, 4);                    /* offset 1, length 8 and more */
    for (unsigned i = 0; i < nibbles; i++) sd_put(s, &at, 15, 4);
    CHECK(at + inside == 8u * 4096u, "the closing nibble starts at bit %llu", (unsigned long long)at);
    sd_put(s, &at, c, 4);
    for (size_t i = 0; i < ntail; i++) sd_put(s, &at, tail[i], 9);
    sd_put(s, &at, 0x180u, 9);
    *n = (size_t)((at + 7) / 8);
    *full = q + 8 + 15 * (size_t)nibbles + c + ntail;
    return s;
}

typedef struct { uint8_t *s; size_t n, full; } sd_block_t;
static sd_block_t sd_compressed(const uint8_t *d, size_t n)
{
    sd_block_t b = { (uint8_t *)malloc(LZS_COMPRESSED_MAX(n) + 8), 0, n };
    b.n = lzs_oracle_compress(b.s, LZS_COMPRESSED_MAX(n), d, n);
    return b;
}

/* ragged batches that go by segments (host_batch()'s conditions: a capacity, >= 4096 bytes in all, >= 1024 a block on average) */
static void sd_batches(const uint8_t *text, const sd_block_t *run, const sd_block_t *edge, unsigned nedge)
{
    for (int pass = 0; pass < 4; pass++) {
        const uint32_t nb = pass == 0 ? 4 : pass == 1 ? 64 : rnd_in(5, 63);
        sd_block_t *blk = (sd_block_t *)calloc(nb, sizeof *blk);
        uint32_t *lens = (uint32_t *)calloc(nb, 4);
        size_t in_stride = 16, total = 0;
        for (uint32_t b = 0; b < nb; b++) {
            /* 0 the long run, 1 empty, 2 cut short, 3 a run closed across a border (the batch of 64 has them all), else text */
            const int every = nb == 64 && b >= 4 && b < 4 + nedge;
            const uint32_t kind = b < 4 ? b : every ? 3 : rnd() % 8u;
            if (kind == 0) { blk[b] = *run; lens[b] = (uint32_t)run->n; }
            else if (kind == 3) { blk[b] = edge[every ? b - 4 : rnd() % nedge]; lens[b] = (uint32_t)blk[b].n; }
            else if (kind != 1) {
                const uint32_t len = rnd_in(3000, 40000);
                blk[b] = sd_compressed(text + rnd_in(0, 200000), len);
                lens[b] = kind == 2 ? rnd_in(1, (uint32_t)blk[b].n - 1) : (uint32_t)blk[b].n;
            }
            if (lens[b] > in_stride) in_stride = lens[b];
            total += lens[b];
        }
        CHECK(total >= 4096 && total / nb >= 1024, "batch of %u blocks, %zu bytes: too small to go by segments", nb, total);
        in_stride += rnd_in(0, 40);
        uint8_t *in = (uint8_t *)malloc(nb * in_stride);
        memset(in, 0xEE, nb * in_stride);
        for (uint32_t b = 0; b < nb; b++) if (lens[b]) memcpy(in + b * in_stride, blk[b].s, lens[b]);
        for (int small = 0; small < 2; small++) {
            const size_t cap = small ? 9000 : 130000, ostride = cap + 7;        /* (room for every block; less than many blocks give) */
            uint8_t *want = (uint8_t *)malloc(nb * ostride), *got = (uint8_t *)malloc(nb * ostride);
            uint32_t *want_len = (uint32_t *)calloc(nb, 4), *got_len = (uint32_t *)calloc(nb, 4);
            const int want_rc = lzs_decompress_batch(want, ostride, cap, want_len, in, in_stride, lens, 0, nb);
            CHECK(want_rc == 0, "lzs_decompress_batch, one wavefront a block: %s", lzs_last_error());
            for (uint32_t b = 0; b < nb; b++) if (lens[b] == blk[b].n && blk[b].s) CHECK(want_len[b] == (blk[b].full < cap ? blk[b].full : cap), "block %u: %u bytes", b, want_len[b]);
            SD_EACH_FORM(si, wi) {
                const int sync = pass == 2 && !small && si == 0;       /* one batch also from "device" memory */
                sd_form(si, wi, 1);
                for (int dev = 0; dev <= sync; dev++) {
                    memset(got, 0x5A, nb * ostride);
                    memset(got_len, 0xFF, 4 * nb);
                    const unsigned scans = lzs_shim_scan_launches();
                    const int rc = dev ? lzs_decompress_batch_device_sync(got, ostride, cap, got_len, in, in_stride, lens, 0, nb)
                                       : lzs_decompress_batch(got, ostride, cap, got_len, in, in_stride, lens, 0, nb);
                    CHECK(rc == want_rc && lzs_shim_scan_launches() > scans, "batch of %u%s, segments of %s, %s: status %d, %s", nb, dev ? " (device)" : "",
                          sd_segs[si], sd_switches[wi] ? sd_switches[wi] : "plain", rc, lzs_shim_scan_launches() > scans ? lzs_last_error() : "not by segments");
                    for (uint32_t b = 0; b < nb; b++) {
                        const int same = got_len[b] == want_len[b] && memcmp(got + b * ostride, want + b * ostride, want_len[b]) == 0;
                        /* (the device form writes in place: only the byte past the capacity is surely nobody's) */
                        const int clean = got[b * ostride + cap] == 0x5A && (dev || want_len[b] == cap || got[b * ostride + want_len[b]] == 0x5A);
                        if (!same || !clean) { CHECK(0, "batch of %u%s, capacity %zu, segments of %s, %s: block %u (%u bytes in): %u bytes out, one wavefront %u%s", nb, dev ? " (device)" : "",
                                                     cap, sd_segs[si], sd_switches[wi] ? sd_switches[wi] : "plain", b, lens[b], got_len[b], want_len[b], clean ? "" : "; a byte past the result touched"); break; }
                    }
                }
                sd_form(si, wi, 0);
            }
            free(want); free(got); free(want_len); free(got_len);
        }
        for (uint32_t b = 0; b < nb; b++) {
            int own = blk[b].s != run->s;
            for (unsigned i = 0; i < nedge; i++) own &= blk[b].s != edge[i].s;
            if (own) free(blk[b].s);
        }
        free(blk); free(lens); free(in);
    }
}

static void streamdec(void)
{
    setenv("LZS_ROUTE", "device", 1);
    setenv("LZS_FORCE_STREAM", "1", 1);
    uint8_t *cls[3] = { sample(0, 420000, 21), sample(1, 420000, 22), sample(2, 420000, 23) };
    const uint32_t longest[3] = { 340000, 400000, 170000 };         /* (up to ~200 KB of stream) */
    for (unsigned c = 0; c < 3; c++) {
        const size_t lengths[] = { 0, 1, rnd_in(2, 3000), rnd_in(3000, 60000), rnd_in(longest[c] / 2, longest[c]) };
        for (unsigned i = 0; i < sizeof lengths / sizeof lengths[0]; i++) {
            sd_block_t b = sd_compressed(cls[c] + rnd_in(0, 20000), lengths[i]);
            char what[64];
            snprintf(what, sizeof what, "class %u, %zu bytes", c, lengths[i]);
            sd_stream(what, b.s, b.n, b.full, 1);
            if (i == 0) sd_call(what, lzs_decompress, "lzs_decompress", b.s, 0, 8);         /* no input at all */
            /* streams of one segment exactly, a byte less, a byte more (cut short: what their tokens give is the one wavefront's to say) */
            if (i == 4) for (unsigned k = 0; k < 9; k++) sd_stream(what, b.s, (256u << (k / 3 == 2 ? 3 : k / 3)) + k % 3 - 1, b.full, 0);
            free(b.s);
        }
    }
    /* a long run: nibbles of 15 for segments on end (all 0xFF inside an extension, the host's shortcut) */
    uint8_t *runs = (uint8_t *)malloc(70000 + 30000);
    memset(runs, 'A', 70000); memcpy(runs + 70000, cls[0] + 1000, 30000);
    sd_block_t run = sd_compressed(runs, 70000), run_text = sd_compressed(runs, 100000), border, border_text;
    border.s = sd_run_to_border(3, 6, NULL, 0, &border.n, &border.full);
    border_text.s = sd_run_to_border(3, 6, cls[0] + 5000, 700, &border_text.n, &border_text.full);
    sd_stream("a run of 70000", run.s, run.n, run.full, 1);
    sd_stream("a run of 70000, then text", run_text.s, run_text.n, run_text.full, 1);
    sd_stream("a run ending at a segment border", border.s, border.n, border.full, 1);
    sd_stream("a run ending at a segment border, then literals", border_text.s, border_text.n, border_text.full, 1);
    {   /* (the hand-made streams decode to what they were made for) */
        uint8_t *back = (uint8_t *)malloc(border_text.full + 8);
        const size_t g = lzs_oracle_decompress(back, border_text.full + 8, border_text.s, border_text.n);
        CHECK(g == border_text.full && back[2] == 'A' && back[g - 701] == 'A' && memcmp(back + g - 700, cls[0] + 5000, 700) == 0, "the hand-made run decodes to %zu bytes", g);
        free(back);
    }
    /* (the closing nibble across the border, in every phase: whether the last nibble that starts in an all-0xFF segment is one of 15
     * is the shortcut's fine print) */
    static const unsigned closing[5] = { 0, 7, 8, 12, 14 };
    sd_block_t edge[20];
    for (unsigned q = 0; q < 4; q++)
        for (unsigned ci = 0; ci < 5; ci++) {
            sd_block_t *b = &edge[5 * q + ci];
            char what[64];
            snprintf(what, sizeof what, "a run closed by nibble %u, %u bits before a border", closing[ci], 4u - (q + 1u) % 4u);
            b->s = sd_run_to_border(q, closing[ci], cls[0] + 100 * ci, 300 + q, &b->n, &b->full);
            sd_stream(what, b->s, b->n, b->full, 0);
        }
    sd_batches(cls[0], &run, edge, 20);
    for (unsigned i = 0; i < 20; i++) free(edge[i].s);
    /* the incremental interface in pieces above INC_DEC_HOST_MAX: stream_decompress() with a prefix, an entry state, a history */
    memset(runs, 'A', 100000); memcpy(runs, cls[0], 15000); memcpy(runs + 85000, cls[0] + 15000, 15000);
    const sd_block_t pieces[2] = { sd_compressed(cls[0] + 777, 340000), sd_compressed(runs, 100000) };
    for (unsigned c = 0; c < 2; c++) {
        const size_t n = pieces[c].full;
        uint8_t *want = (uint8_t *)malloc(n + 64), *got = (uint8_t *)malloc(n + 64);
        uint8_t want_status = 0, status = 0;
        const uint32_t in_lo = c ? 17000 : 66000, in_hi = c ? 20000 : 120000;     /* (the run's stream is short: pieces from INC_DEC_STREAM_MIN on) */
        const uint64_t seed = rng_state;
        const size_t w = decode_pieces(pieces[c].s, pieces[c].n, want, n + 64, in_lo, in_hi, 4096, 200000, &want_status);
        CHECK(w == n, "incremental decompression, one wavefront: %zu of %zu bytes", w, n);
        SD_EACH_FORM(si, wi) {
            sd_form(si, wi, 1);
            rng_state = seed;
            const unsigned scans = lzs_shim_scan_launches();
            const size_t g = decode_pieces(pieces[c].s, pieces[c].n, got, n + 64, in_lo, in_hi, 4096, 200000, &status);
            CHECK(g == w && memcmp(got, want, w) == 0 && status == want_status && lzs_shim_scan_launches() > scans,
                  "incremental decompression of case %u, segments of %s, %s: %zu bytes, status %02x; one wavefront %zu, %02x", c, sd_segs[si],
                  sd_switches[wi] ? sd_switches[wi] : "plain", g, status, w, want_status);
            sd_form(si, wi, 0);
        }
        free(want); free(got); free(pieces[c].s);
    }
    free(run.s); free(run_text.s); free(border.s); free(border_text.s); free(runs);
    for (unsigned c = 0; c < 3; c++) free(cls[c]);
    unsetenv("LZS_ROUTE"); unsetenv("LZS_FORCE_STREAM");
}

/* ---------------------------------------------------------------- the segmented stream compressor's host path, against a table
 * ("streamtrace": lzs_stream.c's stream_compress_piece() over the shim's segment, stitch and extend-resume launches, in segments
 * of LZS_STREAM_SEG bytes).  A row is what one call gave -- bytes returned, the FNV-1a of the whole output buffer with its 0xA5
 * guard, for a piece c_exit, ext_exit and nbits -- and what it asked of the "device": the shim's hash of its syncs, copies, fills
 * and allocations with their sizes, and the hash of its launches with their arguments, each in order.  The rows were recorded
 * with this driver linked against lzs_stream.c as it was BEFORE that function's stages became functions, never from the code
 * under test ("streamtrace-rows" prints them).  Two of the stages are pure and have tables of their own, made by hand. */
typedef struct { const char *name; size_t bytes; uint64_t out, calls, launches; uint32_t c_exit, ext_exit; uint64_t nbits; } stream_row_t;
static const stream_row_t stream_rows[] = {
    { "text of 6145, segments of the default size, into 6917", 3554, 0xA4290434FF54C793ull, 0xD2B6114263ED0D21ull, 0x70A287C3F2F5685Eull, 0, 0, 0 },
    { "text of 20000, segments of 256, into 22503", 11314, 0xBF102CA850AD6F3Cull, 0x7BDF80FCFE03493Full, 0x7BCD1CA002B66CB6ull, 0, 0, 0 },
    { "text of 20000, segments of 256, device buffers, into 23527", 11314, 0xA64C33631A17A40Full, 0x182777C91AE2A40Eull, 0x7BCD1CA002B66CB6ull, 0, 0, 0 },
    { "text of 20000, segments of 512, into 22503", 11314, 0xBF102CA850AD6F3Cull, 0x71AA4F1B9DB94543ull, 0x22C37C5692CAE833ull, 0, 0, 0 },
    { "text of 20000, segments of 512, device buffers, into 23527", 11314, 0xA64C33631A17A40Full, 0x9FA3FA37C7F6D39Aull, 0x22C37C5692CAE833ull, 0, 0, 0 },
    { "an oversized segment, segments of 256, into 851", 329, 0x31E6A36409D52830ull, 0x8CB10756D7D1089Dull, 0x23247CE7C64ED221ull, 0, 0, 0 },
    { "walks that never merge, segments of 256, into 9219", 6401, 0x94A0E5F4C80F05D7ull, 0xBE9D0FEB3D7BEC38ull, 0x167AB13B44D0D9E5ull, 0, 0, 0 },
    { "a run and a period of 2, segments of the default size, into 101259", 29967, 0x8FD66CCD7309A3F4ull, 0x5B105169EC8A6C18ull, 0x43523FFFD20C472Cull, 0, 0, 0 },
    { "text of 20000, segments of 256, into 0", 0, 0x7A1AD6AE7FF8A1F2ull, 0x902936067DECC239ull, 0x7BCD1CA002B66CB6ull, 0, 0, 0 },
    { "text of 20000, segments of 256, into 1", 1, 0xF0C34B11233D83FBull, 0x18D4B3B2152C7C18ull, 0x7BCD1CA002B66CB6ull, 0, 0, 0 },
    { "text of 20000, segments of 256, into 11313", 11313, 0xDC5CAC1E0289BAE5ull, 0x650BAE46DAFF29CCull, 0x7BCD1CA002B66CB6ull, 0, 0, 0 },
    { "text of 20000, segments of 256, device buffers, into 22603", 11314, 0xB976EC1CDD34A2BFull, 0x2B04CBCBE3B06917ull, 0x7BCD1CA002B66CB6ull, 0, 0, 0 },
    { "piece: bit0 = 3 behind a first byte, a prefix", 3071, 0xD3F0FE3DEC5509C9ull, 0x089264BD013B2837ull, 0xD8BBD6910891DD1Dull, 8986, 0, 24561 },
    { "piece: resumes a match that ends inside it", 2452, 0x5129109D32FD4966ull, 0x661CD7A5C0D55A72ull, 0x7CF9B41ECFBE7BC5ull, 8986, 0, 19612 },
    { "piece: resumes a match that covers all its data", 18, 0x281355E2FE749B6Eull, 0x6A8D477D69DDEF46ull, 0x32029BD522C3CF7Aull, 4695, 7, 137 },
    { "piece: the last token reaches the end of the data", 2336, 0x3FE56F8CA5DD0CDAull, 0x4D7FFAE2B1E9B954ull, 0x1488DC19DEE52ABDull, 9398, 7, 18681 },
    { "piece: stop below n", 1159, 0xD353C7A0709ACDE8ull, 0x7963F5598B533E62ull, 0xD1ADF9987A3E229Eull, 7003, 0, 9265 },
    { "piece: last, with an empty tail", 2, 0xF3A98A2136F64D75ull, 0xF522C94BCC875F97ull, 0x8FA7BDC35AB3D00Bull, 3000, 0, 6 },
};
uint64_t lzs_shim_launch_hash(int reset);
static uint64_t fnv1a(const uint8_t *p, size_t n)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}
/* (every call starts with nothing kept by the thread: its allocations are part of what is recorded) */
static void st_begin(const char *seg)
{
    if (seg) setenv("LZS_STREAM_SEG", seg, 1); else unsetenv("LZS_STREAM_SEG");
    lzs_release_thread_cache();
    lzs_shim_call_hash(1); lzs_shim_launch_hash(1);
}
static void st_done(const char *name, size_t bytes, const uint8_t *buf, size_t buf_len, const piece_t *pc)
{
    const stream_row_t got = { name, bytes, fnv1a(buf, buf_len), lzs_shim_call_hash(1), lzs_shim_launch_hash(1),
                               pc ? pc->c_exit : 0, pc ? pc->ext_exit : 0, pc ? pc->nbits : 0 };
    if (trace_print) {
        printf("    { \"%s\", %zu, 0x%016llXull, 0x%016llXull, 0x%016llXull, %u, %u, %llu },\n", name, got.bytes, (unsigned long long)got.out,
               (unsigned long long)got.calls, (unsigned long long)got.launches, got.c_exit, got.ext_exit, (unsigned long long)got.nbits);
        return;
    }
    const stream_row_t *row = NULL;
    for (unsigned i = 0; i < sizeof stream_rows / sizeof stream_rows[0] && stream_rows[i].name; i++) if (!strcmp(stream_rows[i].name, name)) row = &stream_rows[i];
    CHECK(row, "%s: no row in the table", name);
    if (row) CHECK(row->bytes == got.bytes && row->out == got.out && row->calls == got.calls && row->launches == got.launches &&
                   row->c_exit == got.c_exit && row->ext_exit == got.ext_exit && row->nbits == got.nbits,
                   "%s: %zu bytes, output %016llx, calls %016llx, launches %016llx, c_exit %u, ext_exit %u, %llu bits; recorded: %zu, %016llx, %016llx, %016llx, %u, %u, %llu",
                   name, got.bytes, (unsigned long long)got.out, (unsigned long long)got.calls, (unsigned long long)got.launches, got.c_exit, got.ext_exit,
                   (unsigned long long)got.nbits, row->bytes, (unsigned long long)row->out, (unsigned long long)row->calls, (unsigned long long)row->launches,
                   row->c_exit, row->ext_exit, (unsigned long long)row->nbits);
}

/* one input through lzs_compress() into `cap` bytes (SIZE_MAX: all it may need) and, `dev`, through lzs_compress_stream_device()
 * from and into "device" memory (heap memory here) of `dev_cap` bytes; both against the oracle as well */
static void st_one_shot(const char *what, const char *seg, const uint8_t *d, size_t n, size_t cap, int dev, size_t dev_cap)
{
    const size_t most = LZS_COMPRESSED_MAX(n) + 1024;
    uint8_t *want = (uint8_t *)malloc(most), *got = (uint8_t *)malloc(most + 8);
    const size_t w = lzs_oracle_compress(want, most, d, n);
    char name[128];
    if (cap == SIZE_MAX) cap = LZS_COMPRESSED_MAX(n);
    if (cap == SIZE_MAX - 1) cap = w - 1;
    if (!dev) {
        snprintf(name, sizeof name, "%s, segments of %s, into %zu", what, seg ? seg : "the default size", cap);
        memset(got, 0xA5, most + 8);
        st_begin(seg);
        const size_t g = lzs_compress(got, cap, d, n);
        st_done(name, g, got, most + 8, NULL);
        CHECK(g == (w < cap ? w : cap) && memcmp(got, want, g) == 0 && got[g] == 0xA5, "%s: %zu bytes, the oracle %zu: %s", name, g, w, lzs_last_error());
    } else {
        snprintf(name, sizeof name, "%s, segments of %s, device buffers, into %zu", what, seg ? seg : "the default size", dev_cap);
        uint8_t *room = (uint8_t *)malloc(dev_cap + 8);
        size_t g = 0;
        memset(room, 0xA5, dev_cap + 8);
        st_begin(seg);
        const int rc = lzs_compress_stream_device(room, dev_cap, &g, d, n);
        st_done(name, g, room, dev_cap + 8, NULL);
        CHECK(rc == 0 && g == w && memcmp(room, want, w) == 0 && room[dev_cap] == 0xA5, "%s: status %d, %zu bytes, the oracle %zu: %s", name, rc, g, w, lzs_last_error());
        free(room);
    }
    free(want); free(got);
}

/* one direct call of stream_compress_piece() on a hand-made piece: `data` is the prefix and then the input, n bytes in all */
static void st_piece(const char *name, const uint8_t *data, size_t n, piece_t pc)
{
    const size_t cap = LZS_COMPRESSED_MAX(n - pc.c0) + 16;
    uint8_t *got = (uint8_t *)malloc(cap + 8);
    int rc = LZS_OK;
    memset(got, 0xA5, cap + 8);
    pc.prefix = data;
    st_begin("256");
    const size_t g = stream_compress_piece(got, cap, data + pc.prefix_len, n, 0, &rc, &pc);
    st_done(name, g, got, cap + 8, &pc);
    CHECK(rc == LZS_OK && g <= cap && pc.c_exit <= n && pc.c_exit >= pc.c0 && got[cap] == 0xA5, "%s: status %d, %zu bytes, ends at %u: %s", name, rc, g, pc.c_exit, lzs_last_error());
    free(got);
}

/* B(k, 3): every 3-gram over k symbols once (Lyndon words, as tests/stream_compress_programs.py's de_bruijn) */
static void st_db(unsigned t, unsigned p, unsigned k, unsigned *a, uint8_t *seq, size_t *len)
{
    if (t > 3) { if (3 % p == 0) for (unsigned i = 1; i <= p; i++) seq[(*len)++] = (uint8_t)a[i]; return; }
    a[t] = a[t - p];
    st_db(t + 1, p, k, a, seq, len);
    for (unsigned j = a[t - p] + 1; j < k; j++) { a[t] = j; st_db(t + 1, t, k, a, seq, len); }
}

static void st_pure_tables(void)
{
    /* settle_compress_entries(): segments of 256; segment 1's last token is a match that ends at 1030, and the walks from 512 and
     * 768 are inside it: after round 0 segments 2, 3 and 4 are entered there (2 and 3 lie behind it: skipped), 5 where 4 left */
    uint32_t entry[6] = { 0, 256, 512, 768, 1024, 1280 };
    uint8_t dirty[6] = { 1, 1, 1, 1, 1, 1 };
    const uint32_t exits0[6] = { 256, 1030, 1030, 1030, 1285, 1536 }, entry1[6] = { 0, 256, 1030, 1030, 1030, 1285 };
    const uint8_t dirty1[6] = { 0, 0, 1, 1, 1, 1 }, clean[6] = { 0, 0, 0, 0, 0, 0 };
    uint32_t nd = settle_compress_entries(entry, dirty, exits0, 6);
    CHECK(nd == 4 && !memcmp(entry, entry1, sizeof entry) && !memcmp(dirty, dirty1, 6), "settle_compress_entries: a long match over two segments: %u to redo", nd);
    /* round 1: 2 and 3 entered behind their end leave where they were entered, 4 merges with its first walk: all clean */
    nd = settle_compress_entries(entry, dirty, exits0, 6);
    CHECK(nd == 0 && !memcmp(entry, entry1, sizeof entry) && !memcmp(dirty, clean, 6), "settle_compress_entries: all clean: %u to redo", nd);
    dirty[0] = 1; entry[0] = 7;                                     /* segment 0 is entered where the piece says, and never again */
    nd = settle_compress_entries(entry, dirty, exits0, 1);
    CHECK(nd == 0 && entry[0] == 7 && dirty[0] == 0, "settle_compress_entries: one segment");
    /* open_match_take_back(): the match of offset 77 that starts at 1000 -- in segment 3 of 8, empty segments behind it -- reaches
     * the end of the data at n: 8 bytes, full groups of 15 and a closing nibble of (n - 1008) % 15, which is taken back */
    for (uint32_t r = 0; r < 15; r++) {
        const uint32_t n = 1000 + 8 + 15 * (40 + r) + r, open[16] = { 0, 0, 0, 0, 5, 400, 77, 1000, 0, 0, 0, 0, 0, 0, 0, 0 };
        uint64_t nbits[8] = { 2304, 2000, 1800, 900, 0, 0, 0, 0 };
        uint32_t c_exit = n, ext_exit = 0;
        const int took = open_match_take_back(open, nbits, 8, n, 3, &c_exit, &ext_exit);
        CHECK(took == 1 && c_exit == n - r && ext_exit == 77 && nbits[3] == 896 && nbits[2] == 1800 && nbits[4] == 0, "open_match_take_back: residue %u: %d, ends at %u of %u, offset %u, %llu bits",
              r, took, c_exit, n, ext_exit, (unsigned long long)nbits[3]);
    }
    {
        const uint32_t none[4] = { 0, 0, 0, 0 }, one[4] = { 0, 0, 9, 300 };
        uint64_t nbits[2] = { 500, 3 };
        uint32_t c_exit = 600, ext_exit = 0;
        CHECK(open_match_take_back(none, nbits, 2, 600, 0, &c_exit, &ext_exit) == -1, "open_match_take_back: no open match reported");
        CHECK(open_match_take_back(one, nbits, 2, 600, 0, &c_exit, &ext_exit) == -1 && nbits[1] == 3 && c_exit == 600 && ext_exit == 0, "open_match_take_back: fewer than 4 bits");
        /* not the case at all: the last token ends before the data does; the piece had no token (it began behind its data) */
        c_exit = 599; nbits[1] = 40;
        CHECK(open_match_take_back(one, nbits, 2, 600, 0, &c_exit, &ext_exit) == 0 && nbits[1] == 40 && c_exit == 599, "open_match_take_back: a token that ends before n");
        c_exit = 600;
        CHECK(open_match_take_back(one, nbits, 2, 600, 600, &c_exit, &ext_exit) == 0 && nbits[1] == 40 && ext_exit == 0, "open_match_take_back: a piece without tokens");
    }
}

static void streamtrace(void)
{
    setenv("LZS_ROUTE", "device", 1);
    setenv("LZS_FORCE_STREAM", "1", 1);
    if (trace_print) printf("static const stream_row_t stream_rows[] = {\n");
    uint8_t *t = sample(0, 100000, 7), *r = sample(2, 10000, 9);
    st_one_shot("text of 6145", NULL, t, 6145, SIZE_MAX, 0, 0);
    for (int k = 0; k < 2; k++) {
        const char *seg = k ? "512" : "256";
        st_one_shot("text of 20000", seg, t, 20000, SIZE_MAX, 0, 0);
        st_one_shot("text of 20000", seg, t, 20000, 0, 1, LZS_COMPRESSED_MAX(20000) + 1024);
    }
    /* tests/test_stream_compress_model.py, test_model_on_three_inputs_followed_by_hand (2): segment 0 overflows its slot by four bits */
    uint8_t big[753];
    for (unsigned i = 0; i < 753; i++) big[i] = i < 255 ? (uint8_t)i : i < 733 ? 254 : (uint8_t)(100 - (i - 733));
    st_one_shot("an oversized segment", "256", big, sizeof big, SIZE_MAX, 0, 0);
    /* ... and (3): B(16, 3) twice, walks that never merge -- fourteen rounds */
    uint8_t *db = (uint8_t *)malloc(8192);
    unsigned a[8] = { 0 };
    size_t ndb = 0;
    st_db(1, 1, 16, a, db, &ndb);
    CHECK(ndb == 4096, "B(16, 3) has %zu bytes", ndb);
    memcpy(db + 4096, db, 4096);
    st_one_shot("walks that never merge", "256", db, 8192, SIZE_MAX, 0, 0);
    /* one_shot_streams' mix, at a third of its size: a run and a period of 2 over many segments */
    const size_t n_mix = 15000 + 25000 + 15000 + 25000 + 10000 + 5;
    uint8_t *mix = (uint8_t *)calloc(n_mix, 1);
    memcpy(mix, t, 15000); memcpy(mix + 40000, t + 15000, 15000);
    for (size_t i = 0; i < 25000; i++) mix[55000 + i] = "ab"[i & 1];
    memcpy(mix + 80000, r, 10000);
    st_one_shot("a run and a period of 2", NULL, mix, n_mix, SIZE_MAX, 0, 0);
    /* cut capacities: none, one byte, one byte less than the stream; a device buffer shorter than it was promised */
    st_one_shot("text of 20000", "256", t, 20000, 0, 0, 0);
    st_one_shot("text of 20000", "256", t, 20000, 1, 0, 0);
    st_one_shot("text of 20000", "256", t, 20000, SIZE_MAX - 1, 0, 0);
    st_one_shot("text of 20000", "256", t, 20000, 0, 1, LZS_COMPRESSED_MAX(20000) + 100);

    /* pieces, as lzs_compress_incremental() hands them over.  Text with planted copies at offset 7: [4000, 4700) and [9000, 9400) */
    uint8_t *p = (uint8_t *)malloc(12000);
    memcpy(p, t + 30000, 12000);
    for (unsigned i = 4000; i < 4700; i++) p[i] = p[i - 7];
    p[4700] = (uint8_t)(p[4693] ^ 0x55);
    for (unsigned i = 9000; i < 9400; i++) p[i] = p[i - 7];
    p[9400] = (uint8_t)(p[9393] ^ 0x55);
    st_piece("piece: bit0 = 3 behind a first byte, a prefix", p, 9000, (piece_t){ .prefix_len = 3000, .c0 = 2990, .bit0 = 3, .first = 0xA0 });
    st_piece("piece: resumes a match that ends inside it", p, 9000, (piece_t){ .prefix_len = 2304, .c0 = 4200, .ext_off = 7, .bit0 = 5, .first = 0xB8 });
    st_piece("piece: resumes a match that covers all its data", p, 4700, (piece_t){ .prefix_len = 2304, .c0 = 4200, .ext_off = 7, .bit0 = 5, .first = 0xB8 });
    st_piece("piece: the last token reaches the end of the data", p, 9400, (piece_t){ .prefix_len = 5000, .c0 = 4990, .bit0 = 1, .first = 0x80 });
    st_piece("piece: stop below n", p, 9000, (piece_t){ .prefix_len = 5000, .c0 = 4990, .stop = 7000 });
    st_piece("piece: last, with an empty tail", p, 3000, (piece_t){ .prefix_len = 3000, .c0 = 3000, .bit0 = 6, .first = 0xFC, .last = 1 });
    if (!trace_print) {
        st_pure_tables();
        /* a full device: both directions report LZS_E_NOMEM before any launch, and the thread's next call works */
        const size_t n = (size_t)2 << 20, most = LZS_COMPRESSED_MAX(n) + 1024;
        uint8_t *x = sample(1, n, 30), *room = (uint8_t *)malloc(most);
        size_t g = 1;
        setenv("LZS_STAGING_FAIL_MB", "1", 1);
        st_begin(NULL);
        const uint64_t no_launch = lzs_shim_launch_hash(0);
        const unsigned scans = lzs_shim_scan_launches();
        int rc = lzs_compress_stream_device(room, most, &g, x, n);
        CHECK(rc == LZS_E_NOMEM && g == 0 && lzs_shim_launch_hash(0) == no_launch, "a full device: lzs_compress_stream_device gives %d (%s)", rc, lzs_last_error());
        g = 1;
        rc = lzs_decompress_stream_device(room, most, &g, x, n);
        CHECK(rc == LZS_E_NOMEM && g == 0 && lzs_shim_scan_launches() == scans, "a full device: lzs_decompress_stream_device gives %d (%s)", rc, lzs_last_error());
        unsetenv("LZS_STAGING_FAIL_MB");
        rc = lzs_compress_stream_device(room, most, &g, t, 20000);
        uint8_t *want = (uint8_t *)malloc(most);
        const size_t w = lzs_oracle_compress(want, most, t, 20000);
        CHECK(rc == 0 && g == w && memcmp(room, want, w) == 0, "the call after a full device: status %d, %zu bytes (%zu)", rc, g, w);
        free(x); free(room); free(want);
    }
    if (trace_print) printf("};\n");
    free(t); free(r); free(db); free(mix); free(p);
    unsetenv("LZS_ROUTE"); unsetenv("LZS_FORCE_STREAM"); unsetenv("LZS_STREAM_SEG");
}

/* ---------------------------------------------------------------- what a thread keeps, and giving it back
 * The reference keeps nothing after return (lzs.h:218,229); this build keeps a thread's staging for its next call -- at most
 * LZS_KEEP_MAX_MB in sum -- until the thread exits or calls lzs_release_thread_cache(). */
void lzs_shim_outstanding(size_t *dev_bytes, size_t *host_bytes, size_t *live);
typedef struct { int releases; size_t dev_after_calls, dev_after_release, live_after_release; } keeper_t;
static void *keeper(void *arg)
{
    keeper_t *k = (keeper_t *)arg;
    const size_t n = 300000;
    uint8_t *t = sample(0, n, 40), *got = (uint8_t *)malloc(LZS_COMPRESSED_MAX(n)), *back = (uint8_t *)malloc(n + 4);
    setenv("LZS_ROUTE", "device", 1);
    const size_t g = lzs_compress(got, LZS_COMPRESSED_MAX(n), t, n);                 /* one stream in segments: staging, tables, a stream */
    const size_t b = lzs_decompress(back, n, got, g);
    CHECK(b == n && memcmp(back, t, n) == 0, "keeper: round trip of %zu bytes (%zu, %zu)", n, g, b);
    enum { NB = 24, STRIDE = 4096 };
    uint32_t lens[NB]; for (int i = 0; i < NB; i++) lens[i] = STRIDE - (uint32_t)i;
    uint8_t *out = (uint8_t *)malloc((size_t)NB * LZS_COMPRESSED_MAX(STRIDE)); uint32_t out_len[NB];
    CHECK(lzs_compress_batch(out, LZS_COMPRESSED_MAX(STRIDE), LZS_COMPRESSED_MAX(STRIDE), out_len, t, STRIDE, lens, STRIDE, NB) == 0, "keeper: batch: %s", lzs_last_error());
    lzs_shim_outstanding(&k->dev_after_calls, NULL, NULL);
    if (k->releases) {
        lzs_release_thread_cache();
        lzs_release_thread_cache();                                                  /* (twice is once) */
        lzs_shim_outstanding(&k->dev_after_release, NULL, &k->live_after_release);
        /* ... and the thread's next call starts from nothing and works */
        const size_t g2 = lzs_compress(got, LZS_COMPRESSED_MAX(n), t, 20000);
        const size_t b2 = lzs_decompress(back, n, got, g2);
        CHECK(b2 == 20000 && memcmp(back, t, 20000) == 0, "keeper: a call after the release");
        lzs_release_thread_cache();
    }
    free(t); free(got); free(back); free(out);
    return NULL;
}
static void release_cache(void)
{
    lzs_release_thread_cache();                          /* (the main thread's own, from the cases before) */
    size_t dev0, host0, live0;
    lzs_shim_outstanding(&dev0, &host0, &live0);
    for (int pass = 0; pass < 3; pass++) {
        /* pass 0: the thread gives its cache back itself; 1: it just exits; 2: a limit of 1 MiB in sum while it lives */
        if (pass == 2) setenv("LZS_KEEP_MAX_MB", "1", 1);
        keeper_t k = { pass == 0, 0, 0, 0 };
        pthread_t th;
        pthread_create(&th, NULL, keeper, &k);
        pthread_join(th, NULL);
        size_t dev1, host1, live1;
        lzs_shim_outstanding(&dev1, &host1, &live1);
        CHECK(dev1 == dev0 && host1 == host0 && live1 == live0, "pass %d: after the thread is gone %zu device bytes, %zu pinned, %zu allocations are outstanding (before: %zu, %zu, %zu)",
              pass, dev1, host1, live1, dev0, host0, live0);
        if (pass == 0) CHECK(k.dev_after_calls > dev0 && k.dev_after_release == dev0 && k.live_after_release == live0,
                             "lzs_release_thread_cache(): %zu device bytes kept after the calls, %zu after the release (before: %zu)", k.dev_after_calls, k.dev_after_release, dev0);
        if (pass == 2) CHECK(k.dev_after_calls <= dev0 + ((size_t)1 << 20) + 4096, "LZS_KEEP_MAX_MB=1: %zu device bytes kept between calls", k.dev_after_calls - dev0);
        if (pass == 1) CHECK(k.dev_after_calls > dev0 + ((size_t)1 << 20), "the default limit keeps the staging of small calls (%zu bytes)", k.dev_after_calls - dev0);
    }
    unsetenv("LZS_KEEP_MAX_MB"); unsetenv("LZS_ROUTE");
}

/* proof that the harness is alive: "device" memory is instrumented heap memory (the test expects the sanitizer to stop this) */
int lzs_hip_malloc(void **p, size_t bytes);
static void canary(void)
{
    void *d = NULL;
    lzs_hip_malloc(&d, 100);
    volatile uint8_t *q = (volatile uint8_t *)d;
    q[100] = 1;                                  /* one byte past a device buffer */
    printf("canary: the write past the buffer went unnoticed\n");
}

int main(int argc, char **argv)
{
    setenv("LZS_DEV_ENV", "1", 1);          /* the switches are read afresh on every call: this program flips them */
    setenv("LZS_ONE_WAVE", "1", 1);         /* decompression by one wavefront a stream, the oracle behind it ("streamdec" lifts this call by call) */
    const char *only = argc > 1 ? argv[1] : "";
    char info[256];
    if (lzs_backend_info(info, sizeof info) != 0 || !strstr(info, "cpu shim")) { fprintf(stderr, "not linked with the cpu shim: %s\n", info); return 2; }
    if (!*only || !strcmp(only, "routes")) routes();
    if (!*only || !strcmp(only, "ragged")) ragged_batches();
    if (!*only || !strcmp(only, "layouts")) layouts();
    if (!*only || !strcmp(only, "streams")) one_shot_streams();
    if (!*only || !strcmp(only, "incremental")) incremental();
    trace_print = !strcmp(only, "inctrace-rows");
    if (!*only || !strcmp(only, "inctrace") || trace_print) inctrace();
    trace_print = !strcmp(only, "streamtrace-rows");
    if (!*only || !strcmp(only, "streamtrace") || trace_print) streamtrace();
    trace_print = 0;
    if (!*only || !strcmp(only, "streamdec")) streamdec();
    if (!*only || !strcmp(only, "pipeline")) pipeline();
    if (!*only || !strcmp(only, "release")) release_cache();
    if (!strcmp(only, "canary")) canary();
    printf("san_driver: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
