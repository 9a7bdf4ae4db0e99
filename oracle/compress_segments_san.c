/*
 * oracle/compress_segments_san.c -- lzs_oracle_compress_segments (lzs_oracle.c: the plain model of a segment border of the
 * segmented stream compressor) in a program of its own, to be built with -fsanitize=address,undefined (oracle/Makefile:
 * san-program).  TEST INFRASTRUCTURE ONLY.
 *
 *   compress_segments_san [FILE]
 *
 * FILE holds inputs one behind the other, each as a 32-bit little-endian length and its bytes
 * (tests/test_stream_compress_model.py writes the directed inputs there); without it the program walks seeded data.  Every
 * input goes through the model in segments of 256 and 512 bytes, with the chained finder and (8 KiB and less) the written rule,
 * with and without counters, trace and rounds, and with tables shorter than the input needs.  Checked: the segments' bits add up
 * to what is returned and to lzs_oracle_compress()'s length, bit_at is their prefix sum, exits chain into entries, the rounds
 * arrive at the true exits, and nothing is written past what was handed in (exact-size heap blocks: the sanitizer's business).
 * Prints "<n> input(s), <m> walk(s), <f> failure(s)"; the exit status is 0 only with 0 failures.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

size_t lzs_oracle_compress(uint8_t *out, size_t cap, const uint8_t *in, size_t n);
size_t lzs_oracle_compress_segments(const uint8_t *in, size_t n, size_t seg, int brute,
                                    uint64_t *rec, size_t max_seg, uint32_t *rounds, size_t max_rounds, size_t *nrounds,
                                    uint64_t *counters, uint32_t *trace, size_t max_tok, size_t *ntok);
void lzs_oracle_compress_segments_layout(uint32_t *sizes);

static unsigned long failures, walks;

static void fail(const char *what, size_t input, size_t seg, int shape)
{
    failures++;
    fprintf(stderr, "input %zu, segments of %zu, shape %d: %s\n", input, seg, shape, what);
}

static void one_input(const uint8_t *data, size_t n, size_t index)
{
    static const size_t segs[2] = { 256, 512 };
    uint32_t sizes[4];
    lzs_oracle_compress_segments_layout(sizes);
    const size_t ncounters = sizes[0], fields = sizes[1];
    const size_t cap = n + (n + 7) / 8 + 3;
    uint8_t *in = (uint8_t *)malloc(n ? n : 1);                  /* exactly n bytes: a read past the input is caught */
    uint8_t *packed = (uint8_t *)malloc(cap);
    if (!in || !packed) { fail("out of memory", index, 0, 0); free(in); free(packed); return; }
    memcpy(in, data, n);
    const size_t stream = lzs_oracle_compress(packed, cap, in, n);
    for (int s = 0; s < 2; s++) {
        const size_t seg = segs[s], nseg = n ? (n + seg - 1) / seg : 1;
        /* 0: everything asked for; 1: no counters, trace or rounds; 2: tables for half the segments, three tokens, one round;
         * 3: the written rule */
        for (int shape = 0; shape < (n <= 8192 ? 4 : 3); shape++) {
            const size_t max_seg = shape == 2 ? nseg / 2 : nseg, max_tok = shape == 1 ? 0 : shape == 2 ? 3 : n;
            const size_t max_rounds = shape == 1 ? 0 : shape == 2 ? 1 : nseg + 1;
            uint64_t *rec = (uint64_t *)malloc((max_seg ? max_seg : 1) * fields * sizeof(uint64_t));
            uint64_t *counters = shape == 1 ? NULL : (uint64_t *)calloc(ncounters, sizeof(uint64_t));
            uint32_t *trace = max_tok ? (uint32_t *)malloc(max_tok * 4 * sizeof(uint32_t)) : NULL;
            uint32_t *rounds = max_rounds ? (uint32_t *)malloc(max_rounds * sizeof(uint32_t)) : NULL;
            size_t ntok = 0, nrounds = 0;
            const size_t bits = lzs_oracle_compress_segments(in, n, seg, shape == 3, rec, max_seg, rounds, max_rounds, &nrounds,
                                                             counters, trace, max_tok, shape == 1 ? NULL : &ntok);
            walks++;
            if (bits == (size_t)-1) fail("out of memory", index, seg, shape);
            else {
                if ((bits + 9 + 7) / 8 != stream) fail("bits differ from lzs_oracle_compress", index, seg, shape);
                if (shape != 2) {
                    uint64_t sum = 0, at = 0;
                    for (size_t k = 0; k < nseg; k++) {
                        const uint64_t *r = rec + k * fields;
                        if (r[4] != sum) fail("bit_at is not the prefix sum", index, seg, shape);
                        if (!r[5] && r[0] != at) fail("entry is not the exit before", index, seg, shape);
                        if (r[10] != r[1]) fail("the rounds do not arrive at the true exit", index, seg, shape);
                        sum += r[3]; at = r[1];
                    }
                    if (sum != bits) fail("segments do not add up", index, seg, shape);
                    if (n && at != n) fail("the last exit is not the end", index, seg, shape);
                }
                if (shape == 0 || shape == 3) {
                    if (ntok > max_tok && n) fail("more tokens than bytes", index, seg, shape);
                    if (nrounds > max_rounds || (nrounds && rounds[nrounds - 1] != 0)) fail("rounds", index, seg, shape);
                    size_t covered = 0;
                    for (size_t t = 0; t < ntok && t < max_tok; t++) covered += trace[4 * t + 2];
                    if (covered != n) fail("tokens do not cover the input", index, seg, shape);
                }
            }
            free(rec); free(counters); free(trace); free(rounds);
        }
    }
    if (lzs_oracle_compress_segments(in, n, 100, 0, NULL, 0, NULL, 0, NULL, NULL, NULL, 0, NULL) != (size_t)-1)
        fail("a segment size that is none was taken", index, 100, 0);
    free(in); free(packed);
}

int main(int argc, char **argv)
{
    size_t inputs = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        for (;;) {
            uint8_t head[4];
            if (fread(head, 1, 4, f) != 4) break;
            const size_t n = (size_t)head[0] | ((size_t)head[1] << 8) | ((size_t)head[2] << 16) | ((size_t)head[3] << 24);
            uint8_t *data = (uint8_t *)malloc(n ? n : 1);
            if (!data || fread(data, 1, n, f) != n) { fprintf(stderr, "%s: short read\n", argv[1]); free(data); fclose(f); return 2; }
            one_input(data, n, inputs++);
            free(data);
        }
        fclose(f);
    } else {
        /* seeded data of a small alphabet with runs in it, lengths around the segment sizes and 0 */
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (int i = 0; i < 24; i++) {
            const size_t n = i < 4 ? (size_t)i : (size_t)(i * 397 % 3000) + (size_t)(i % 5 == 0 ? 256 * i - i * 397 % 3000 : 40);
            uint8_t *data = (uint8_t *)malloc(n ? n : 1);
            if (!data) return 2;
            for (size_t j = 0; j < n; j++) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                data[j] = (i % 3 == 1 && (j / 300) % 2) ? 0x41 : (uint8_t)('a' + (x >> 32) % (i % 3 == 2 ? 4 : 20));
            }
            one_input(data, n, inputs++);
            free(data);
        }
    }
    printf("%zu input(s), %lu walk(s), %lu failure(s)\n", inputs, walks, failures);
    return failures ? 1 : 0;
}
