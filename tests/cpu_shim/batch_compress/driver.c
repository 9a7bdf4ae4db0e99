/* tests/cpu_shim/batch_compress/driver.c -- lzs_compress_batch_device_sync() (csrc/lzs_batch_compress.c) over the CPU statement of
 * its launchers, as a stand-alone program under the address and undefined-behaviour sanitizers (tests/test_batch_compress_host.py).
 *
 *   batch_compress_driver <blob> <capacity> [<capacity> ...]
 *
 * The blob is ONE ragged batch: a count, the lengths (32-bit, little-endian), the blocks' bytes one behind the other.  The rows are
 * laid out at a stride of the longest block rounded up to 16, in an allocation that ends with the last block's last byte.  For
 * every capacity (0: one that holds every stream) the batch is compressed twice, into slots of the capacity rounded up to 4 -- they
 * touch -- and into slots 8 bytes longer, inside a buffer of 0xA5: out_len[b] and the bytes in front of it are
 * lzs_oracle_compress()'s at that capacity, the bytes around the slots and the last four of every longer slot are still 0xA5.
 * The segment size, the route and the debug lines are the environment's (LZS_STREAM_SEG, LZS_BATCH_COMPRESS_ROUTE,
 * LZS_STREAM_DEBUG); a line "== <capacity> <gap>" on stderr precedes every call's.  Prints "ok N calls", or what differs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lzs/lzs.h"
#include "lzs/lzs_batch.h"

size_t lzs_oracle_compress(uint8_t *out, size_t cap, const uint8_t *in, size_t n);
extern unsigned g_bc_compress_launches, g_bc_stitch_launches, g_bc_second_passes;

#define LEAD 64u

static void *need(void *p) { if (!p) { fprintf(stderr, "out of memory\n"); exit(2); } return p; }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <blob> <capacity> ...\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    uint32_t nb = 0;
    if (!f || fread(&nb, 4, 1, f) != 1 || nb == 0) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t *len = (uint32_t *)need(malloc(sizeof(uint32_t) * nb));
    if (fread(len, 4, nb, f) != nb) { fprintf(stderr, "short blob\n"); return 2; }
    size_t longest = 0;
    for (uint32_t b = 0; b < nb; b++) if (len[b] > longest) longest = len[b];
    const size_t in_stride = (longest + 15u) & ~(size_t)15u, extent = (size_t)(nb - 1) * in_stride + len[nb - 1];
    uint8_t *in = (uint8_t *)need(malloc(extent ? extent : 1));
    memset(in, 0x5A, extent);
    uint8_t **want = (uint8_t **)need(malloc(sizeof(uint8_t *) * nb));
    size_t *want_len = (size_t *)need(malloc(sizeof(size_t) * nb)), most = 0;
    for (uint32_t b = 0; b < nb; b++) {
        if (len[b] && fread(in + b * in_stride, 1, len[b], f) != len[b]) { fprintf(stderr, "short blob\n"); return 2; }
        const size_t room = LZS_COMPRESSED_MAX((size_t)len[b]);
        want[b] = (uint8_t *)need(malloc(room));
        want_len[b] = lzs_oracle_compress(want[b], room, in + b * in_stride, len[b]);
        if (want_len[b] > most) most = want_len[b];
    }
    fclose(f);
    uint32_t *got_len = (uint32_t *)need(malloc(sizeof(uint32_t) * nb));
    unsigned calls = 0, failures = 0;
    for (int a = 2; a < argc; a++) {
        const size_t asked = strtoull(argv[a], NULL, 10), cap = asked ? asked : most;
        for (size_t gap = 0; gap <= 8; gap += 8, calls++) {
            const size_t out_stride = ((cap + 3u) & ~(size_t)3u) + gap, bytes = LEAD + out_stride * nb + LEAD;
            uint8_t *buf = (uint8_t *)need(malloc(bytes));
            memset(buf, 0xA5, bytes);
            memset(got_len, 0xEE, sizeof(uint32_t) * nb);
            fprintf(stderr, "== %zu %zu\n", cap, gap);
            const int rc = lzs_compress_batch_device_sync(buf + LEAD, out_stride, cap, got_len, in, in_stride, len, longest, nb);
            if (rc != LZS_OK) { printf("FAIL capacity %zu gap %zu: rc %d (%s)\n", cap, gap, rc, lzs_last_error()); failures++; free(buf); continue; }
            for (uint32_t b = 0; b < nb; b++) {
                const size_t expect = want_len[b] < cap ? want_len[b] : cap;
                const uint8_t *slot = buf + LEAD + b * out_stride;
                if (got_len[b] != expect || memcmp(slot, want[b], expect)) {
                    if (failures++ < 10) printf("FAIL capacity %zu gap %zu block %u (%u bytes): length %u, expected %zu, or other bytes\n", cap, gap, b, len[b], got_len[b], expect);
                }
                for (size_t i = out_stride - (gap ? 4 : 0); i < out_stride; i++)
                    if (slot[i] != 0xA5 && failures++ < 10) printf("FAIL capacity %zu block %u: byte %zu of the slot's gap changed\n", cap, b, i);
            }
            for (size_t i = 0; i < LEAD; i++)
                if ((buf[i] != 0xA5 || buf[bytes - 1 - i] != 0xA5) && failures++ < 10) printf("FAIL capacity %zu gap %zu: a byte outside the slots changed\n", cap, gap);
            free(buf);
        }
    }
    fprintf(stderr, "== launches: %u compress (%u second passes), %u stitch\n", g_bc_compress_launches, g_bc_second_passes, g_bc_stitch_launches);
    lzs_release_thread_cache();
    for (uint32_t b = 0; b < nb; b++) free(want[b]);
    free(want); free(want_len); free(got_len); free(in); free(len);
    if (failures) { printf("%u failure(s)\n", failures); return 1; }
    printf("ok %u calls\n", calls);
    return 0;
}
