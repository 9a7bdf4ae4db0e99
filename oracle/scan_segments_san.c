/*
 * oracle/scan_segments_san.c -- lzs_oracle_scan_segments (lzs_oracle.c: the plain model of a segment border) in a program of
 * its own, to be built with -fsanitize=address,undefined (oracle/Makefile: san-program).  TEST INFRASTRUCTURE ONLY.
 *
 *   scan_segments_san [FILE]
 *
 * FILE holds streams one behind the other, each as a 32-bit little-endian length and its bytes
 * (tests/test_stream_border_model.py writes the directed streams there); without it the program walks seeded garbage.  Every
 * stream goes through the model under both rules, in segments of 64, 256 and 512 bytes, with room for everything and cut at
 * three capacities, with and without counters and trace, and with tables shorter than the stream needs.  Checked: the
 * segments' bytes add up to what is returned, their output starts are the prefix sums, under the one-shot rule the total is
 * lzs_oracle_decompress()'s, and nothing is written past what was handed in (exact-size heap blocks: the sanitizer's business).
 * Prints "<n> stream(s), <m> walk(s), <f> failure(s)"; the exit status is 0 only with 0 failures.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

size_t lzs_oracle_decompress(uint8_t *out, size_t cap, const uint8_t *in, size_t n);
size_t lzs_oracle_scan_segments(const uint8_t *in, size_t n, size_t seg, int file_rule, size_t cap,
                                uint32_t *rec, size_t max_seg, uint64_t *counters,
                                uint32_t *trace, size_t max_tok, size_t *ntok);
void lzs_oracle_scan_layout(uint32_t *sizes);

static unsigned long failures, walks;

static void fail(const char *what, size_t stream, size_t seg, int rule, size_t cap)
{
    failures++;
    fprintf(stderr, "stream %zu, segments of %zu, rule %d, capacity %zu: %s\n", stream, seg, rule, cap, what);
}

static void one_stream(const uint8_t *data, size_t n, size_t index)
{
    static const size_t segs[3] = { 64, 256, 512 };
    uint32_t sizes[4];
    lzs_oracle_scan_layout(sizes);
    const size_t ncounters = sizes[0], fields = sizes[1];
    uint8_t *in = (uint8_t *)malloc(n ? n : 1);                  /* exactly n bytes: a read past the stream is caught */
    uint8_t *plain = (uint8_t *)malloc(30 * n + 16);
    if (!in || !plain) { fail("out of memory", index, 0, 0, 0); free(in); free(plain); return; }
    memcpy(in, data, n);
    const size_t all = lzs_oracle_decompress(plain, 30 * n + 16, in, n);
    for (int s = 0; s < 3; s++) {
        const size_t seg = segs[s], nseg = (n + seg - 1) / seg;
        for (int rule = 0; rule < 2; rule++) {
            const size_t caps[4] = { 30 * n + 16, all / 2, 1, all ? all - 1 : 0 };
            for (int c = 0; c < 4; c++) {
                for (int shape = 0; shape < (c == 0 ? 3 : 1); shape++) {
                    /* 0: everything asked for; 1: no counters, no trace; 2: tables for half the segments and a handful of steps */
                    const size_t max_seg = shape == 2 ? nseg / 2 : nseg, max_tok = shape == 0 ? 2 * n + 1 : shape == 2 ? 5 : 0;
                    uint32_t *rec = (uint32_t *)malloc((max_seg ? max_seg : 1) * fields * sizeof(uint32_t));
                    uint64_t *counters = shape == 1 ? NULL : (uint64_t *)calloc(ncounters, sizeof(uint64_t));
                    uint32_t *trace = max_tok ? (uint32_t *)malloc(max_tok * 5 * sizeof(uint32_t)) : NULL;
                    size_t ntok = 0;
                    const size_t got = lzs_oracle_scan_segments(in, n, seg, rule, caps[c], rec, max_seg, counters, trace, max_tok, &ntok);
                    walks++;
                    if (got == (size_t)-1) fail("out of memory", index, seg, rule, caps[c]);
                    else {
                        if (got > caps[c]) fail("more bytes than the capacity", index, seg, rule, caps[c]);
                        if (!rule) {
                            const size_t want = lzs_oracle_decompress(plain, caps[c], in, n);
                            if (got != want) fail("total differs from lzs_oracle_decompress", index, seg, rule, caps[c]);
                        }
                        if (shape != 2) {
                            size_t sum = 0;
                            for (size_t k = 0; k < nseg; k++) {
                                const uint32_t *r = rec + k * fields;
                                if (r[0] != 0xFFFFFFFFu && r[4] != sum) fail("output start is not the prefix sum", index, seg, rule, caps[c]);
                                sum += r[3];
                            }
                            if (sum != got) fail("segments do not add up", index, seg, rule, caps[c]);
                        }
                        if (shape == 0) {
                            size_t sum = 0;
                            if (ntok > max_tok) fail("more steps than bits allow", index, seg, rule, caps[c]);
                            for (size_t t = 0; t < ntok && t < max_tok; t++) sum += trace[5 * t + 3];
                            if (sum != got) fail("steps do not add up", index, seg, rule, caps[c]);
                        }
                    }
                    free(rec); free(counters); free(trace);
                }
            }
        }
    }
    free(in); free(plain);
}

int main(int argc, char **argv)
{
    size_t streams = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        for (;;) {
            uint8_t head[4];
            if (fread(head, 1, 4, f) != 4) break;
            const size_t n = (size_t)head[0] | ((size_t)head[1] << 8) | ((size_t)head[2] << 16) | ((size_t)head[3] << 24);
            uint8_t *data = (uint8_t *)malloc(n ? n : 1);
            if (!data || fread(data, 1, n, f) != n) { fprintf(stderr, "%s: short read\n", argv[1]); free(data); fclose(f); return 2; }
            one_stream(data, n, streams++);
            free(data);
        }
        fclose(f);
    } else {
        /* seeded garbage, and garbage with long runs of ones (extensions) and of zeros (literals at every phase) in it */
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (int i = 0; i < 24; i++) {
            const size_t n = (size_t)(i * 397 % 3000) + (i < 3 ? (size_t)i : 40);
            uint8_t *data = (uint8_t *)malloc(n);
            if (!data) return 2;
            for (size_t j = 0; j < n; j++) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                data[j] = (i % 3 == 1 && (j / 300) % 2) ? 0xFF : (i % 3 == 2 && (j / 200) % 2) ? 0x00 : (uint8_t)(x >> 32);
            }
            one_stream(data, n, streams++);
            free(data);
        }
    }
    printf("%zu stream(s), %lu walk(s), %lu failure(s)\n", streams, walks, failures);
    return failures ? 1 : 0;
}
