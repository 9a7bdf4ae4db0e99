/*
 * oracle/channel_encode_san.c -- lzs_oracle_compress_channel (lzs_oracle.c) in a program of its own, for a build with
 * -fsanitize=address,undefined (oracle/Makefile: san-program).
 *
 * TEST INFRASTRUCTURE ONLY.  It makes its own histories and packets with a small generator: random bytes, two symbols, runs
 * that continue the history's last byte, and pieces of the history (from its first and last bytes among them); every buffer is
 * allocated at its exact size, so that a byte read or written outside it is seen.  For every packet: the chained finder gives
 * the brute finder's stream, a cut stream is a prefix of the whole one with the status and the history unchanged by the cut,
 * and lzs_oracle_decompress_channel on the same history gives the packet and the same new history back.
 * Prints "<n> failure(s)"; exit status 0 only with none.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

size_t lzs_oracle_compress_channel(uint8_t *out, size_t cap, const uint8_t *in, size_t n,
                                   const uint8_t *hist, size_t h, int brute, size_t *total,
                                   uint8_t *new_hist, size_t *new_h, uint8_t *status,
                                   uint64_t *counters, uint32_t *trace, size_t max_tok, size_t *ntok);
size_t lzs_oracle_decompress_channel(uint8_t *out, size_t cap, const uint8_t *in, size_t n,
                                     const uint8_t *hist, size_t h,
                                     uint8_t *new_hist, size_t *new_h, uint8_t *status,
                                     uint64_t *counters, uint32_t *trace, size_t max_tok, size_t *ntok,
                                     uint64_t *stop_bit);

enum { WINDOW = 2047, COUNTERS = 12 };

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)                                   /* xorshift64* */
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

static const size_t HIST_LENS[] = { 0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 2046, 2047 };
static const size_t PACKET_LENS[] = { 0, 1, 2, 3, 7, 8, 9, 23, 2046, 2047, 2048 };

static void fill(uint8_t *p, size_t n, const uint8_t *hist, size_t h, unsigned kind)
{
    size_t i = 0;
    while (i < n) {
        if (kind == 0) {
            p[i++] = (uint8_t)rnd();
        } else if (kind == 1) {
            p[i++] = (uint8_t)('a' + below(2));
        } else if (kind == 2) {
            p[i++] = h ? hist[h - 1] : 'r';
        } else {                                            /* pieces of the history, a literal between them now and then */
            size_t len = 2 + below(40), at = 0;
            if (h) {
                switch (below(4)) {
                case 0: at = 0; break;
                case 1: at = h - 1; break;
                case 2: at = h > 1 ? h - 2 : 0; break;
                default: at = below((uint32_t)h);
                }
            }
            for (size_t k = 0; k < len && i < n; k++, i++) {
                size_t q = at + k;                          /* in history | packet so far */
                p[i] = q < h ? hist[q] : (q - h < i ? p[q - h] : (uint8_t)rnd());
            }
            if (i < n && below(2))
                p[i++] = (uint8_t)rnd();
        }
    }
}

static uint8_t *exact(size_t n) { return (uint8_t *)malloc(n ? n : 1); }

int main(void)
{
    unsigned failures = 0, packets = 0;
    uint64_t counters[COUNTERS] = { 0 };

    for (unsigned ch = 0; ch < 104; ch++) {
        size_t   h = HIST_LENS[ch % 13];
        uint8_t *hist = exact(WINDOW);
        fill(hist, h, NULL, 0, ch % 2);
        for (unsigned r = 0; r < 10; r++, packets++) {
            size_t   n = below(4) ? (below(3) ? below(200) : below(3001)) : PACKET_LENS[below(11)];
            size_t   room = n + (n + 7) / 8 + 3;
            uint8_t *in = exact(n), *a = exact(room), *b = exact(room), *back = exact(n);
            uint8_t *ha = exact(WINDOW), *hb = exact(WINDOW), *hd = exact(WINDOW);
            size_t   ta = 0, tb = 0, tc = 0, na = 0, nb = 0, nc = 0, nd = 0, ntok = 0;
            uint8_t  sa = 0, sb = 0, sc = 0, sd = 0;
            uint32_t *trace = (uint32_t *)malloc((n ? n : 1) * 4 * sizeof(uint32_t));
            int      bad = 0;

            fill(in, n, hist, h, (ch + r) % 4);
            size_t la = lzs_oracle_compress_channel(a, room, in, n, hist, h, 0, &ta, ha, &na, &sa, counters, trace, n, &ntok);
            size_t lb = lzs_oracle_compress_channel(b, room, in, n, hist, h, 1, &tb, hb, &nb, &sb, NULL, NULL, 0, NULL);
            bad |= la != lb || ta != tb || la != ta || sa != 0x07 || sb != 0x07 || memcmp(a, b, la) != 0;
            bad |= na != nb || memcmp(ha, hb, na) != 0 || na != (h + n < WINDOW ? h + n : WINDOW) || ntok > n;

            size_t   cap = below((uint32_t)ta + 2);          /* 0 .. total + 1, in a buffer of exactly that size */
            uint8_t *c = exact(cap);
            size_t   lc = lzs_oracle_compress_channel(c, cap, in, n, hist, h, 0, &tc, hb, &nc, &sc, counters, NULL, 0, NULL);
            bad |= lc != (ta < cap ? ta : cap) || tc != ta || memcmp(c, a, lc) != 0 || sc != (ta <= cap ? 0x07 : 0x0B);
            bad |= nc != na || memcmp(ha, hb, na) != 0;

            size_t ld = lzs_oracle_decompress_channel(back, n, a, la, hist, h, hd, &nd, &sd, NULL, NULL, 0, NULL, NULL);
            bad |= ld != n || sd != 0x04 || memcmp(back, in, n) != 0 || nd != na || memcmp(hd, ha, na) != 0;

            if (bad) {
                failures++;
                printf("FAIL: channel %u, packet %u: hlen %zu, %zu bytes, capacity %zu\n", ch, r, h, n, cap);
            }
            memcpy(hist, ha, na);
            h = na;
            free(in); free(a); free(b); free(c); free(back); free(ha); free(hb); free(hd); free(trace);
        }
        free(hist);
    }
    printf("%u packets;", packets);
    for (unsigned i = 0; i < COUNTERS; i++)
        printf(" %llu", (unsigned long long)counters[i]);
    printf("\n%u failure(s)\n", failures);
    return failures != 0;
}
