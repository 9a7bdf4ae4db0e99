/* tests/cpu_shim/size_stream/route_check.c -- lzs_plan_size_route() (csrc/lzs_launch_plan.h) held to a table of literal rows
 * (tests/test_size_stream_plan.py builds this with -Werror and the address and undefined-behaviour sanitizers and runs it).  The
 * rule: by segments when the extent -- nblocks strides and the longest block -- fits 32 bits and the blocks are
 * 10 167 bytes and more on average, the threshold the sweep of profiles/r20/size_stream.txt gave; LZS_SIZE_ROUTE=lanes|segments
 * (forced 1 | 2) takes the place of the average, never of the extent.  No expected value is computed by the function under test.  Prints one line per failing row,
 * then "N rows, M failure(s)"; exit status 1 if M > 0. */
#include <stdio.h>
#include <stdint.h>
#include "lzs_launch_plan.h"

enum { LANES = 0, SEGMENTS = 1 };

static const struct { const char *name; uint64_t extent, total_in, nblocks; int forced; int route; } rows[] = {
    /* the 32-bit extent: 64 blocks of 1 MiB */
    { "extent 0xFFFFFFFF",                        0xFFFFFFFFull,  67108864ull, 64ull, 0, SEGMENTS },
    { "extent 0x100000000",                       0x100000000ull, 67108864ull, 64ull, 0, LANES },
    { "extent 0x100000000, segments forced",      0x100000000ull, 67108864ull, 64ull, 2, LANES },
    { "extent 0xFFFFFFFF, segments forced",       0xFFFFFFFFull,  67108864ull, 64ull, 2, SEGMENTS },
    { "extent 0xFFFFFFFFFFFFFFFF",                0xFFFFFFFFFFFFFFFFull, 67108864ull, 64ull, 0, LANES },
    /* the threshold, 10 167 bytes a block on average: one block, then three (30 501 = 3 * 10 167; the average rounds down) */
    { "one block of 10166",                       10166ull, 10166ull, 1ull, 0, LANES },
    { "one block of 10167",                       10167ull, 10167ull, 1ull, 0, SEGMENTS },
    { "one block of 10168",                       10168ull, 10168ull, 1ull, 0, SEGMENTS },
    { "three blocks, 30500 bytes",                3ull * 20000ull + 20000ull, 30500ull, 3ull, 0, LANES },
    { "three blocks, 30501 bytes",                3ull * 20000ull + 20000ull, 30501ull, 3ull, 0, SEGMENTS },
    { "three blocks, 30502 bytes",                3ull * 20000ull + 20000ull, 30502ull, 3ull, 0, SEGMENTS },
    /* the shapes the threshold lies between: 65 536 packets of 1500 bytes, 16 384 blocks of 64 KiB */
    { "65536 packets of 1500",                    65536ull * 1536ull + 1500ull, 98304000ull, 65536ull, 0, LANES },
    { "16384 blocks of 64 KiB",                   16384ull * 65536ull + 65536ull, 1073741824ull, 16384ull, 0, SEGMENTS },
    /* LZS_SIZE_ROUTE */
    { "lanes forced on 64 blocks of 1 MiB",       64ull * 1048576ull + 1048576ull, 67108864ull, 64ull, 1, LANES },
    { "segments forced on 65536 packets of 1500", 65536ull * 1536ull + 1500ull, 98304000ull, 65536ull, 2, SEGMENTS },
    { "segments forced on one block of 1 byte",   2ull, 1ull, 1ull, 2, SEGMENTS },
    /* nothing to cut into segments */
    { "no blocks",                                0ull, 0ull, 0ull, 0, LANES },
    { "blocks without a byte, segments forced",   4096ull, 0ull, 4ull, 2, LANES },
};

int main(void)
{
    int failures = 0;
    size_t i;
    for (i = 0; i < sizeof(rows) / sizeof(rows[0]); i++) {
        const int got = lzs_plan_size_route(rows[i].extent, rows[i].total_in, rows[i].nblocks, rows[i].forced);
        if (got != rows[i].route) {
            printf("FAIL %s: route %d, expected %d\n", rows[i].name, got, rows[i].route);
            failures++;
        }
    }
    printf("%u rows, %d failure(s)\n", (unsigned)(sizeof(rows) / sizeof(rows[0])), failures);
    return failures ? 1 : 0;
}
