/* tests/cpu_shim/size_stream/driver.c -- the size query for long streams (csrc/lzs_size_stream.c) over the CPU shim, under the
 * address and undefined-behaviour sanitizers (tests/test_size_stream_host.py).  usage: driver CASES OUT
 *   CASES: uint32 ncases, then per case uint32 kind and
 *            kind 0, one stream: uint32 n, offset, flags; uint64 limit; n bytes
 *            kind 1, a batch   : uint32 nblocks, stride, offset, extent; uint64 limit; uint32 length[nblocks]; `extent` bytes -- the
 *                                blocks at their stride up to the end of the last one that has a byte
 *   OUT  : one stream: uint64 size, uint32 status, uint32 0; a batch: per block uint32 size, uint32 status
 * "Device" memory is the heap here.  Every input lies in an allocation of its own that begins `offset` bytes in front of it and ends
 * with the aligned 32-bit word that holds its last byte, so a read outside the words that hold the streams' own bytes stops the
 * run.  One stream is asked three ways -- in "device" memory, without a status, from a host buffer --, a batch by both routes
 * (LZS_SIZE_ROUTE; the shim counts SCAN launches, which tells which route a call took); all must agree, between guard words. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lzs/lzs.h"
#include "lzs/lzs_batch.h"

unsigned lzs_shim_scan_launches(void);

#define GUARD64 0xAAAAAAAAAAAAAAAAull
#define GUARD32 0xAAAAAAAAu

static uint8_t *tight(FILE *f, uint32_t offset, uint32_t n)
{
    const size_t alloc = n ? ((size_t)offset + n + 3) / 4 * 4 : offset;
    uint8_t *buf = (uint8_t *)malloc(alloc ? alloc : 1);
    if (!buf) exit(2);
    for (size_t i = 0; i < alloc; i++) buf[i] = (uint8_t)rand();
    if (n && fread(buf + offset, 1, n, f) != n) exit(2);
    return buf;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t nc;
    if (!f || !o || fread(&nc, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < nc; c++) {
        uint32_t kind;
        if (fread(&kind, 4, 1, f) != 1) return 2;
        if (kind == 0) {
            uint32_t h[3];
            uint64_t limit;
            if (fread(h, 4, 3, f) != 3 || fread(&limit, 8, 1, f) != 1) return 2;
            const uint32_t n = h[0], offset = h[1], flags = h[2];
            uint8_t *buf = tight(f, offset, n);
            uint64_t size[3] = {GUARD64, GUARD64, GUARD64}, size2 = GUARD64, size3 = GUARD64;
            uint8_t st[3] = {0xAA, 0xAA, 0xAA}, st3 = 0xAA;
            int rc = lzs_decompressed_size_stream_device(size + 1, st + 1, buf + offset, n, limit, flags);
            if (rc == LZS_OK) rc = lzs_decompressed_size_stream_device(&size2, NULL, buf + offset, n, limit, flags);
            if (rc == LZS_OK) rc = lzs_decompressed_size_stream(&size3, &st3, buf + offset, n, limit, flags);
            if (rc != LZS_OK) { printf("case %u: rc %d: %s\n", c, rc, lzs_last_error()); return 1; }
            if (size[0] != GUARD64 || size[2] != GUARD64 || st[0] != 0xAA || st[2] != 0xAA || size2 != size[1] || size3 != size[1] || st3 != st[1]) {
                printf("case %u: guard words changed, or the three ways differ: %llu/%u, %llu, %llu/%u\n", c, (unsigned long long)size[1], st[1],
                       (unsigned long long)size2, (unsigned long long)size3, st3);
                return 1;
            }
            const uint32_t r[2] = {st[1], 0};
            fwrite(size + 1, 8, 1, o);
            fwrite(r, 4, 2, o);
            free(buf);
        } else {
            uint32_t h[4];
            uint64_t limit;
            if (fread(h, 4, 4, f) != 4 || fread(&limit, 8, 1, f) != 1) return 2;
            const uint32_t nb = h[0], stride = h[1], offset = h[2], extent = h[3];
            uint32_t *len = (uint32_t *)malloc(4 * (size_t)(nb ? nb : 1));
            uint32_t *size = (uint32_t *)malloc(4 * ((size_t)nb + 2)), *size2 = (uint32_t *)malloc(4 * ((size_t)nb + 2));
            uint8_t *st = (uint8_t *)malloc((size_t)nb + 2), *st2 = (uint8_t *)malloc((size_t)nb + 2);
            if (!len || !size || !size2 || !st || !st2 || (nb && fread(len, 4, nb, f) != nb)) return 2;
            uint8_t *buf = tight(f, offset, extent);
            for (uint32_t b = 0; b < nb + 2; b++) { size[b] = size2[b] = GUARD32; st[b] = st2[b] = 0xAA; }
            setenv("LZS_SIZE_ROUTE", "segments", 1);
            const unsigned scans0 = lzs_shim_scan_launches();
            int rc = lzs_decompressed_size_batch_device_sync(size + 1, st + 1, buf + offset, stride, len, 0, (size_t)limit, nb);
            const unsigned scans1 = lzs_shim_scan_launches();
            setenv("LZS_SIZE_ROUTE", "lanes", 1);
            if (rc == LZS_OK) rc = lzs_decompressed_size_batch_device_sync(size2 + 1, st2 + 1, buf + offset, stride, len, 0, (size_t)limit, nb);
            const unsigned scans2 = lzs_shim_scan_launches();
            unsetenv("LZS_SIZE_ROUTE");
            if (rc != LZS_OK) { printf("case %u: rc %d: %s\n", c, rc, lzs_last_error()); return 1; }
            if ((extent && scans1 == scans0) || scans2 != scans1) { printf("case %u: a forced route was not taken\n", c); return 1; }
            if (size[0] != GUARD32 || size[nb + 1] != GUARD32 || st[0] != 0xAA || st[nb + 1] != 0xAA || size2[0] != GUARD32 ||
                size2[nb + 1] != GUARD32 || st2[0] != 0xAA || st2[nb + 1] != 0xAA) { printf("case %u: guard words changed\n", c); return 1; }
            for (uint32_t b = 0; b < nb; b++) {
                if (size[b + 1] != size2[b + 1] || st[b + 1] != st2[b + 1]) {
                    printf("case %u block %u: by segments %u/%u, by lanes %u/%u\n", c, b, size[b + 1], st[b + 1], size2[b + 1], st2[b + 1]);
                    return 1;
                }
                const uint32_t r[2] = {size[b + 1], st[b + 1]};
                fwrite(r, 4, 2, o);
            }
            free(buf); free(len); free(size); free(size2); free(st); free(st2);
        }
    }
    fclose(o);
    fclose(f);
    lzs_release_thread_cache();
    printf("ok %u cases\n", nc);
    return 0;
}
