/* tests/cpu_shim/batch_compress/route_check.c -- the plain functions behind lzs_compress_batch_device_sync() (csrc/lzs_launch_plan.h;
 * DESIGN.md 3.19) held to tables of literal rows: lzs_plan_batch_compress_route(), lzs_plan_batch_compress_group() and
 * lzs_plan_batch_compress_segments().  tests/test_batch_compress_plan.py builds this with -Werror and the address and
 * undefined-behaviour sanitizers and runs it.  No expected value is computed by a function under test.  Prints one line per
 * failing row, then "N rows, M failure(s)"; exit status 1 if M > 0. */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "lzs_launch_plan.h"

enum { WG = 0, SEG = 1 };
#define MiB 1048576ull

/* nblocks, total_in, longest, out_cap, out_stride, out_align (d_out's address), forced */
static const struct { const char *name; uint64_t nblocks, total_in, longest, out_cap, out_stride, out_align; int forced; int route; } routes[] = {
    /* the preconditions, each one side and the other, with the segments forced so that nothing else decides */
    { "cap == stride",                      8, 8 * MiB, MiB, 1179652, 1179652, 0x7f0000001000ull, 2, SEG },
    { "cap == stride + 1",                  8, 8 * MiB, MiB, 1179653, 1179652, 0x7f0000001000ull, 2, WG },
    { "stride a multiple of 4",             8, 8 * MiB, MiB, 1000, 1179652, 0x7f0000001000ull, 2, SEG },
    { "stride + 2",                         8, 8 * MiB, MiB, 1000, 1179654, 0x7f0000001000ull, 2, WG },
    { "stride + 1",                         8, 8 * MiB, MiB, 1000, 1179653, 0x7f0000001000ull, 2, WG },
    { "d_out at 4",                         8, 8 * MiB, MiB, 1000, 1179652, 0x7f0000001004ull, 2, SEG },
    { "d_out at 2",                         8, 8 * MiB, MiB, 1000, 1179652, 0x7f0000001002ull, 2, WG },
    { "d_out at 1",                         8, 8 * MiB, MiB, 1000, 1179652, 0x7f0000001001ull, 2, WG },
    { "0x7FFFFFFF blocks",                  0x7FFFFFFFull, 0x7FFFFFFFull, 1, 4, 4, 0, 2, SEG },
    { "0x80000000 blocks",                  0x80000000ull, 0x80000000ull, 1, 4, 4, 0, 2, WG },
    { "no blocks",                          0, 0, 0, 4, 4, 0, 2, WG },
    { "capacity 0, segments forced",        2, 2000, 1000, 0, 0, 0, 2, SEG },
    /* LZS_BATCH_COMPRESS_ROUTE */
    { "workgroups forced on 8 x 16 MiB",    8, 128 * MiB, 16 * MiB, 18874372, 18874372, 0, 1, WG },
    { "segments forced on 4096 x 64 KiB",   4096, 256 * MiB, 65536, 73732, 73732, 0, 2, SEG },
    { "segments forced on one byte",        1, 1, 1, 8, 8, 0, 2, SEG },
    /* the measured thresholds (profiles/r24/batch_compress.txt): the longest block from 1 MiB on, at most 256 times it in all */
    { "two blocks, the longest 1048575",    2, 1398100, 1048575, 1179652, 1179652, 0, 0, WG },
    { "two blocks, the longest 1048576",    2, 1398100, 1048576, 1179652, 1179652, 0, 0, SEG },
    { "two blocks, the longest 1048577",    2, 1398100, 1048577, 1179656, 1179656, 0, 0, SEG },
    { "255 blocks of 1 MiB",                255, 255 * MiB, MiB, 1179652, 1179652, 0, 0, SEG },
    { "256 blocks of 1 MiB",                256, 256 * MiB, MiB, 1179652, 1179652, 0, 0, SEG },
    { "256 blocks of 1 MiB and a byte",     257, 256 * MiB + 1, MiB, 1179652, 1179652, 0, 0, WG },
    { "257 blocks of 1 MiB",                257, 257 * MiB, MiB, 1179652, 1179652, 0, 0, WG },
    /* a ragged batch counts as what it would be in blocks of its longest: 8 x 16 MiB and 300 blocks of 1 KiB */
    { "8 x 16 MiB and 300 x 1 KiB",         308, 128 * MiB + 307200, 16 * MiB, 18874372, 18874372, 0, 0, SEG },
    /* the sweep's rows */
    { "1 block of 16 MiB",                  1, 16 * MiB, 16 * MiB, 18874372, 18874372, 0, 0, SEG },
    { "8 blocks of 16 MiB",                 8, 128 * MiB, 16 * MiB, 18874372, 18874372, 0, 0, SEG },
    { "64 blocks of 16 MiB",                64, 1024 * MiB, 16 * MiB, 18874372, 18874372, 0, 0, SEG },
    { "64 blocks of 1 MiB",                 64, 64 * MiB, MiB, 1179652, 1179652, 0, 0, SEG },
    { "1024 blocks of 1 MiB",               1024, 1024 * MiB, MiB, 1179652, 1179652, 0, 0, WG },
    { "256 blocks of 64 KiB",               256, 16 * MiB, 65536, 73732, 73732, 0, 0, WG },
    { "1024 blocks of 64 KiB",              1024, 64 * MiB, 65536, 73732, 73732, 0, 0, WG },
    { "1536 blocks of 64 KiB",              1536, 96 * MiB, 65536, 73732, 73732, 0, 0, WG },
    { "4096 blocks of 64 KiB",              4096, 256 * MiB, 65536, 73732, 73732, 0, 0, WG },
    { "16384 blocks of 64 KiB",             16384, 1024 * MiB, 65536, 73732, 73732, 0, 0, WG },
    /* nblocks x in_stride beyond 32 bits is no obstacle (the tables hold 64-bit offsets): 300 strides of 16 MiB, only 8 MiB used */
    { "300 x 16 MiB strides, by the rule",  300, 300 * 8 * MiB, 8 * MiB, 9437188, 9437188, 0, 0, WG },
    { "300 x 16 MiB strides, forced",       300, 300 * 8 * MiB, 8 * MiB, 9437188, 9437188, 0, 2, SEG },
    { "200 x 32 MiB strides, by the rule",  200, 200 * 24 * MiB, 24 * MiB, 28311556, 33554432, 0, 0, SEG },
    /* an unaligned output stays with the workgroups whatever the shape */
    { "8 x 16 MiB, stride + 1",             8, 128 * MiB, 16 * MiB, 18874372, 18874373, 0, 0, WG },
};

#define BOUND 0xC0000000ull             /* LZS_BLOCK_MAX, the bound the host path passes */
static const uint32_t g_big[]   = { 100, 0xC0000000u, 5, 5 };                   /* a block at the bound: alone (its neighbours do not fit) */
static const uint32_t g_exact[] = { 0x40000000u, 0x40000000u, 0x40000000u, 1, 0x40000000u };   /* a sum exactly at the bound, then one byte too many */
static const uint32_t g_zero[]  = { 0, 0, 7, 0, 0 };
static const uint32_t g_small[] = { 10, 20, 30, 40 };
static const struct { const char *name; const uint32_t *len; uint32_t len_all; uint64_t nblocks, b0, bound, want; } group_rows[] = {
    { "100 then a block at the bound: 100 alone",   g_big, 0, 4, 0, BOUND, 1 },
    { "the block at the bound alone",               g_big, 0, 4, 1, BOUND, 1 },
    { "what follows it",                            g_big, 0, 4, 2, BOUND, 2 },
    { "past the end",                               g_big, 0, 4, 4, BOUND, 0 },
    { "a block above a small bound, alone",         g_small, 0, 4, 3, 35, 1 },
    { "a sum exactly at the bound",                 g_exact, 0, 5, 0, BOUND, 3 },
    { "one byte too many starts the next group",    g_exact, 0, 5, 3, BOUND, 2 },
    { "a sum exactly at a small bound",             g_small, 0, 4, 0, 60, 3 },
    { "one below it",                               g_small, 0, 4, 0, 59, 2 },
    { "blocks without a byte join any group",       g_zero, 0, 5, 0, 7, 5 },
    { "blocks without a byte, bound 0",             g_zero, 0, 5, 0, 0, 2 },
    { "a block above the bound takes nothing with it", g_zero, 0, 5, 2, 0, 1 },
    { "uniform rows: 3 x 1 GiB fit",                NULL, 0x40000000u, 8, 0, BOUND, 3 },
    { "uniform rows: the last two",                 NULL, 0x40000000u, 8, 6, BOUND, 2 },
    { "uniform rows without a byte: the cap on blocks", NULL, 0, 3000000, 0, BOUND, 1048576 },
};

static const uint32_t s_ragged[] = { 700, 1, 513, 255 };            /* in segments of 256: 3, 1, 3, 1 */
static const uint32_t s_multiple[] = { 512, 256 };                  /* 2, 1: no empty segment behind a multiple */
static const uint32_t s_zero[] = { 0, 300, 0 };                     /* 1, 2, 1 */
static const struct { const char *name; const uint32_t *len; uint32_t len_all; uint64_t b0, nb; uint32_t seg; uint64_t nseg; uint32_t block[8], start[8]; } tables[] = {
    { "ragged",            s_ragged, 0, 0, 4, 256, 8, { 0, 0, 0, 1, 2, 2, 2, 3 }, { 0, 256, 512, 0, 0, 256, 512, 0 } },
    { "ragged, from 1",    s_ragged, 0, 1, 3, 256, 5, { 0, 1, 1, 1, 2 }, { 0, 0, 256, 512, 0 } },
    { "multiples of seg",  s_multiple, 0, 0, 2, 256, 3, { 0, 0, 1 }, { 0, 256, 0 } },
    { "length 0",          s_zero, 0, 0, 3, 256, 4, { 0, 1, 1, 2 }, { 0, 0, 256, 0 } },
    { "uniform 1025 / 512", NULL, 1025, 0, 2, 512, 6, { 0, 0, 0, 1, 1, 1 }, { 0, 512, 1024, 0, 512, 1024 } },
    { "uniform 0",         NULL, 0, 0, 3, 512, 3, { 0, 1, 2 }, { 0, 0, 0 } },
};

int main(void)
{
    int failures = 0;
    unsigned nrows = 0;
    size_t i;
    for (i = 0; i < sizeof(routes) / sizeof(routes[0]); i++, nrows++) {
        const int got = lzs_plan_batch_compress_route(routes[i].nblocks, routes[i].total_in, routes[i].longest, routes[i].out_cap,
                                                      routes[i].out_stride, routes[i].out_align, routes[i].forced);
        if (got != routes[i].route) { printf("FAIL route %s: %d, expected %d\n", routes[i].name, got, routes[i].route); failures++; }
    }
    for (i = 0; i < sizeof(group_rows) / sizeof(group_rows[0]); i++, nrows++) {
        const uint64_t got = lzs_plan_batch_compress_group(group_rows[i].len, group_rows[i].len_all, group_rows[i].nblocks, group_rows[i].b0, group_rows[i].bound);
        if (got != group_rows[i].want) { printf("FAIL group %s: %llu, expected %llu\n", group_rows[i].name, (unsigned long long)got, (unsigned long long)group_rows[i].want); failures++; }
    }
    for (i = 0; i < sizeof(tables) / sizeof(tables[0]); i++, nrows++) {
        uint32_t block[9], start[9];
        memset(block, 0xEE, sizeof(block)); memset(start, 0xEE, sizeof(start));
        const uint64_t counted = lzs_plan_batch_compress_segments(NULL, NULL, tables[i].len, tables[i].len_all, tables[i].b0, tables[i].nb, tables[i].seg);
        const uint64_t got = lzs_plan_batch_compress_segments(block, start, tables[i].len, tables[i].len_all, tables[i].b0, tables[i].nb, tables[i].seg);
        int bad = counted != tables[i].nseg || got != tables[i].nseg || block[tables[i].nseg] != 0xEEEEEEEEu || start[tables[i].nseg] != 0xEEEEEEEEu;
        for (uint64_t k = 0; !bad && k < tables[i].nseg; k++) bad = block[k] != tables[i].block[k] || start[k] != tables[i].start[k];
        if (bad) { printf("FAIL segments %s: %llu segments, expected %llu, or a wrong entry\n", tables[i].name, (unsigned long long)got, (unsigned long long)tables[i].nseg); failures++; }
    }
    printf("%u rows, %d failure(s)\n", nrows, failures);
    return failures ? 1 : 0;
}
