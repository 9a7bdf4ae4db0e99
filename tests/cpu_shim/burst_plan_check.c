/* tests/cpu_shim/burst_plan_check.c -- csrc/lzs_burst_plan.h held to tables of literal rows (tests/test_burst_plan.py builds this
 * with -fsanitize=address,undefined and runs it).  The layout's and the sizes' expected values are what burst_layout() of
 * lzs_channels_burst.hip and the three size functions of lzs_channels.c and lzs_packed.c gave at commit 81b9245, the last before they
 * moved into the header, compiled as host code; the decisions' are worked out by hand from that commit's lines.  None is computed by
 * the function under test.  Prints one line per failing row, then "N failure(s)"; exit status 1 if N > 0. */
#include <stdio.h>
#include <stdint.h>
#include "lzs_burst_plan.h"

static int failures;
#define ROWS(t) (sizeof(t) / sizeof((t)[0]))
#define MAXSZ 18446744073709551615u         /* SIZE_MAX of the 64-bit hosts the library is built for */

/* ---- the layout.  part[]: slots, key 0 1, val 0 1, lens, ends, weight 0 1, at 0 1, run_end, temp -- the documented order;
 * over[]: nheavy, light_w, light_at, rec, rooms, room_ends, the tables laid over the slots; room_ends_bytes: that last table's
 * aligned size.  per_packet[] / over_per_packet[]: the bytes of a part that a packet accounts for (temp: 65536 and 8 a packet;
 * nheavy: 4 bytes whatever n) -- a part must end before the next begins. */
enum { PARTS = 13, OVER = 6 };
static const size_t per_packet[PARTS] = { 2112u, 4u, 4u, 4u, 4u, 8u, 8u, 4u, 4u, 4u, 4u, 4u, 8u };
static const size_t over_per_packet[OVER] = { 0u, 4u, 4u, 8u, 8u, 8u };
static const struct { size_t n, part[PARTS], temp_bytes, total, over[OVER], room_ends_bytes; } layout_rows[] = {
    { 1u, { 0u, 2304u, 2560u, 2816u, 3072u, 3328u, 3584u, 3840u, 4096u, 4352u, 4608u, 4864u, 5120u },
      65792u, 70912u, { 0u, 256u, 512u, 768u, 1024u, 1280u }, 256u },
    { 2u, { 0u, 4352u, 4608u, 4864u, 5120u, 5376u, 5632u, 5888u, 6144u, 6400u, 6656u, 6912u, 7168u },
      65792u, 72960u, { 0u, 256u, 512u, 768u, 1024u, 1280u }, 256u },
    { 63u, { 0u, 133120u, 133376u, 133632u, 133888u, 134144u, 134656u, 135168u, 135424u, 135680u, 135936u, 136192u, 136448u },
      66048u, 202496u, { 0u, 256u, 512u, 768u, 1280u, 1792u }, 512u },
    { 64u, { 0u, 135168u, 135424u, 135680u, 135936u, 136192u, 136704u, 137216u, 137472u, 137728u, 137984u, 138240u, 138496u },
      66048u, 204544u, { 0u, 256u, 512u, 768u, 1280u, 1792u }, 512u },
    { 255u, { 0u, 538624u, 539648u, 540672u, 541696u, 542720u, 544768u, 546816u, 547840u, 548864u, 549888u, 550912u, 551936u },
      67584u, 619520u, { 0u, 256u, 1280u, 2304u, 4352u, 6400u }, 2048u },
    { 256u, { 0u, 540672u, 541696u, 542720u, 543744u, 544768u, 546816u, 548864u, 549888u, 550912u, 551936u, 552960u, 553984u },
      67584u, 621568u, { 0u, 256u, 1280u, 2304u, 4352u, 6400u }, 2048u },
    { 257u, { 0u, 542976u, 544256u, 545536u, 546816u, 548096u, 550400u, 552704u, 553984u, 555264u, 556544u, 557824u, 559104u },
      67840u, 626944u, { 0u, 256u, 1536u, 2816u, 5120u, 7424u }, 2304u },
    { 65536u, { 0u, 138412032u, 138674176u, 138936320u, 139198464u, 139460608u, 139984896u, 140509184u, 140771328u, 141033472u, 141295616u, 141557760u, 141819904u },
      589824u, 142409728u, { 0u, 256u, 262400u, 524544u, 1048832u, 1573120u }, 524288u },
    { 16777216u, { 0u, 35433480192u, 35500589056u, 35567697920u, 35634806784u, 35701915648u, 35836133376u, 35970351104u, 36037459968u, 36104568832u, 36171677696u, 36238786560u, 36305895424u },
      134283264u, 36440178688u, { 0u, 256u, 67109120u, 134217984u, 268435712u, 402653440u }, 134217728u },
    { 2147483647u, { 0u, 4535485462528u, 4544075397120u, 4552665331712u, 4561255266304u, 4569845200896u, 4587025070080u, 4604204939264u, 4612794873856u, 4621384808448u, 4629974743040u, 4638564677632u, 4647154612224u },
      17179934720u, 4664334546944u, { 0u, 256u, 8589934848u, 17179869440u, 34359738624u, 51539607808u }, 17179869184u },
};

/* ---- lzs_channels_burst_work_bytes: no packets (rocPRIM's spare alone), nchannels changes nothing, the clamp at LZS_CHANNELS_MAX */
static const struct { const char *name; size_t npackets, nchannels, bytes; } work_rows[] = {
    { "work n=0",                         0u, 0u, 65536u },
    { "work n=0, nchannels=5",            0u, 5u, 65536u },
    { "work n=1",                         1u, 1u, 70912u },
    { "work n=1, nchannels at its most",  1u, 2147483647u, 70912u },
    { "work n=100",                       100u, 10u, 284416u },
    { "work n=65536, nchannels=16384",    65536u, 16384u, 142409728u },
    { "work n=65536, nchannels=1",        65536u, 1u, 142409728u },
    { "work n one below the clamp",       2147483646u, 1u, 4664334544896u },
    { "work n at the clamp",              2147483647u, 1u, 4664334546944u },
    { "work n one above the clamp",       2147483648u, 1u, 4664334546944u },
    { "work n=SIZE_MAX",                  MAXSZ, 1u, 4664334546944u },
};

/* ---- lzs_channels_burst_split_work_bytes: the burst size + 2 * n * out_cap, out_cap clamped to 2^32 - 1, SIZE_MAX on overflow */
static const struct { const char *name; size_t npackets, nchannels, out_cap, bytes; } split_size_rows[] = {
    { "split size n=0",                                  0u, 1u, 1500u, 65536u },
    { "split size n=0 cap=0",                            0u, 1u, 0u, 65536u },
    { "split size n=1 cap=0",                            1u, 1u, 0u, 70912u },
    { "split size n=1 cap=1",                            1u, 1u, 1u, 70914u },
    { "split size n=4 cap=100 nchannels=8",              4u, 8u, 100u, 77856u },
    { "split size n=4 cap=100 nchannels=1",              4u, 1u, 100u, 77856u },
    { "split size n=3 cap=1500",                         3u, 2u, 1500u, 84008u },
    { "split size cap at its clamp",                     1u, 1u, 4294967295u, 8590005502u },
    { "split size cap one above its clamp",              1u, 1u, 4294967296u, 8590005502u },
    { "split size n at most, the largest cap that fits", 2147483647u, 1u, 4294966211u, 18446744069414649978u },
    { "split size n at most, that cap plus one",         2147483647u, 1u, 4294966212u, MAXSZ },
    { "split size cap at most, the largest n that fits", 2147483105u, 1u, 4294967295u, 18446744069413473598u },
    { "split size cap at most, that n plus one",         2147483106u, 1u, 4294967295u, MAXSZ },
    { "split size n and cap at their most",              2147483647u, 1u, 4294967295u, MAXSZ },
    { "split size n above its clamp",                    2147483648u, 1u, 4294967295u, MAXSZ },
    { "split size both SIZE_MAX",                        MAXSZ, 1u, MAXSZ, MAXSZ },
};

/* ---- lzs_channels_burst_packed_split_work_bytes: the burst size + 2 * out_bytes, SIZE_MAX on overflow (the burst size of 10
 * packets is 89856: (SIZE_MAX - 89856) / 2 = 9223372036854730879 bytes of room still fit) */
static const struct { const char *name; size_t npackets, nchannels; uint64_t out_bytes; size_t bytes; } packed_size_rows[] = {
    { "packed size nothing",                     0u, 0u, 0u, 65536u },
    { "packed size n=0, 1000 bytes",             0u, 3u, 1000u, 67536u },
    { "packed size n=3, 1000 bytes",             3u, 2u, 1000u, 77008u },
    { "packed size n=3, nchannels=9",            3u, 9u, 1000u, 77008u },
    { "packed size n=10, no room",               10u, 4u, 0u, 89856u },
    { "packed size the most room that fits",     10u, 4u, 9223372036854730879u, 18446744073709551614u },
    { "packed size that plus one",               10u, 4u, 9223372036854730880u, MAXSZ },
    { "packed size out_bytes = 2^64 - 1",        10u, 4u, 18446744073709551615u, MAXSZ },
    { "packed size n at its clamp",              2147483647u, 1u, 1u, 4664334546946u },
    { "packed size n above its clamp",           2147483648u, 1u, 1u, 4664334546946u },
};

/* ---- the channel sort's bits, lzs_channels_burst.hip:606-607: the smallest b >= 1 with nchannels >> b == 0, 32 at the most */
static const struct { uint32_t nchannels; unsigned bits; } bits_rows[] = {
    { 0u, 1u },                                          /* (refused before it gets here: the sort still has a bit) */
    { 1u, 1u }, { 2u, 2u }, { 3u, 2u }, { 4u, 3u }, { 255u, 8u }, { 256u, 9u }, { 16384u, 15u }, { 0x7FFFFFFFu, 31u },
    { 0x80000000u, 32u }, { 0xFFFFFFFFu, 32u },          /* (no call has that many channels: the loop ends at 32 without shifting by it) */
};

/* ---- RESOLVE's grid, :674: npackets <= nchannels ? npackets : nchannels + 1 */
static const struct { uint32_t npackets, nchannels, grid; } grid_rows[] = {
    { 1u, 1u, 1u }, { 1u, 8u, 1u }, { 7u, 8u, 7u }, { 8u, 8u, 8u }, { 9u, 8u, 9u }, { 10u, 8u, 9u }, { 65536u, 16384u, 16385u },
    { 2u, 1u, 2u }, { 3u, 1u, 2u },
    { 0x7FFFFFFEu, 0x7FFFFFFFu, 0x7FFFFFFEu }, { 0x7FFFFFFFu, 0x7FFFFFFFu, 0x7FFFFFFFu }, { 0x7FFFFFFFu, 0x7FFFFFFEu, 0x7FFFFFFFu },
    { 0x7FFFFFFFu, 1u, 2u },
};

/* ---- the strided split rule, lzs_channels.c:87: decompress && work_bytes >= the split size (4 packets of 100: 77856; at the
 * largest sizes the split size is SIZE_MAX, which no work area reaches -- but the rule is the comparison) */
static const struct { const char *name; int decompress; size_t work_bytes, npackets, nchannels; uint32_t out_cap; int split; } strided_rows[] = {
    { "strided burst size only",            1, 77056u, 4u, 8u, 100u, 0 },     /* the burst size of 4 packets */
    { "strided one below the split size",   1, 77855u, 4u, 8u, 100u, 0 },
    { "strided at the split size",          1, 77856u, 4u, 8u, 100u, 1 },
    { "strided above the split size",       1, 1u << 30, 4u, 8u, 100u, 1 },
    { "strided compression at the split size", 0, 77856u, 4u, 8u, 100u, 0 },
    { "strided compression, huge area",     0, MAXSZ, 4u, 8u, 100u, 0 },
    { "strided cap=0: the burst size is the split size", 1, 77056u, 4u, 8u, 0u, 1 },
    { "strided split size overflows, area below SIZE_MAX", 1, MAXSZ - 1u, 2147483647u, 1u, 4294967295u, 0 },
};

/* ---- the packed split rule, lzs_channels_burst.hip:726-728 with lzs_packed.c:187: origin_cap = origin_bytes / 2 when decompressing,
 * else 0; split when it is not 0 */
static const struct { int decompress; size_t origin_bytes; int split; uint64_t origin_cap; } packed_rows[] = {
    { 1, 0u, 0, 0u }, { 1, 1u, 0, 0u }, { 1, 2u, 1, 1u }, { 1, 3u, 1, 1u }, { 1, 12000u, 1, 6000u }, { 1, MAXSZ, 1, 9223372036854775807u },
    { 0, 0u, 0, 0u }, { 0, 2u, 0, 0u }, { 0, 12000u, 0, 0u },
};

/* ---- split_min, lzs_channels.c:89 and lzs_packed.c:185: LZS_BURST_SPLIT_MIN if it is set, else 8192 */
static const struct { int set; uint32_t value, split_min; } split_min_rows[] = {
    { 0, 0u, 8192u }, { 0, 77u, 8192u }, { 1, 0u, 0u }, { 1, 1u, 1u }, { 1, 8192u, 8192u }, { 1, 100000u, 100000u }, { 1, 0xFFFFFFFFu, 0xFFFFFFFFu },
};

static void layout_fail(size_t n, const char *what, size_t got, size_t want)
{
    printf("FAIL layout n=%zu: %s %zu, expected %zu\n", n, what, got, want);
    failures++;
}

int main(void)
{
    size_t i, k;
    for (i = 0; i < ROWS(layout_rows); i++) {
        const size_t n = layout_rows[i].n;
        const lzs_burst_layout_t L = lzs_burst_layout(n);
        const size_t part[PARTS] = { L.slots, L.key[0], L.key[1], L.val[0], L.val[1], L.lens, L.ends, L.weight[0], L.weight[1], L.at[0], L.at[1],
                                     L.run_end, L.temp };
        const size_t over[OVER] = { L.nheavy, L.light_w, L.light_at, L.rec, L.rooms, L.room_ends };
        static const char *const part_name[PARTS] = { "slots", "key[0]", "key[1]", "val[0]", "val[1]", "lens", "ends", "weight[0]", "weight[1]",
                                                      "at[0]", "at[1]", "run_end", "temp" };
        static const char *const over_name[OVER] = { "nheavy", "light_w", "light_at", "rec", "rooms", "room_ends" };
        for (k = 0; k < PARTS; k++) {
            const size_t bytes = per_packet[k] * n + (k == PARTS - 1 ? 65536u : 0u), next = k + 1 < PARTS ? part[k + 1] : L.total;
            if (part[k] != layout_rows[i].part[k]) layout_fail(n, part_name[k], part[k], layout_rows[i].part[k]);
            if (part[k] % 256u != 0) layout_fail(n, "not 256-byte aligned:", part[k], part[k] / 256u * 256u);
            if (part[k] + bytes > next) layout_fail(n, "overlaps the part behind it, ends at", part[k] + bytes, next);
        }
        for (k = 0; k < OVER; k++) {
            const size_t bytes = k == 0 ? 4u : over_per_packet[k] * n, next = k + 1 < OVER ? over[k + 1] : L.key[0];
            if (over[k] != layout_rows[i].over[k]) layout_fail(n, over_name[k], over[k], layout_rows[i].over[k]);
            if (over[k] % 256u != 0) layout_fail(n, "not 256-byte aligned:", over[k], over[k] / 256u * 256u);
            if (over[k] + bytes > next) layout_fail(n, "overlaps the table behind it, ends at", over[k] + bytes, next);
        }
        if (L.temp_bytes != layout_rows[i].temp_bytes) layout_fail(n, "temp_bytes", L.temp_bytes, layout_rows[i].temp_bytes);
        if (L.total != layout_rows[i].total) layout_fail(n, "total", L.total, layout_rows[i].total);
        if (L.total % 256u != 0) layout_fail(n, "not 256-byte aligned:", L.total, L.total / 256u * 256u);
        if (L.temp + L.temp_bytes != L.total) layout_fail(n, "temp does not end at total:", L.temp + L.temp_bytes, L.total);
        if (L.origins != L.total) layout_fail(n, "origins", L.origins, L.total);
        /* the tables of the split decode, whole, end where the slots do or before */
        if (L.room_ends + layout_rows[i].room_ends_bytes > L.key[0])
            layout_fail(n, "the overlay ends past the slots, at", L.room_ends + layout_rows[i].room_ends_bytes, L.key[0]);
    }
    for (i = 0; i < ROWS(work_rows); i++) {
        const size_t got = lzs_burst_plan_work_bytes(work_rows[i].npackets, work_rows[i].nchannels);
        if (got != work_rows[i].bytes) { printf("FAIL %s: %zu, expected %zu\n", work_rows[i].name, got, work_rows[i].bytes); failures++; }
    }
    for (i = 0; i < ROWS(split_size_rows); i++) {
        const size_t got = lzs_burst_plan_split_work_bytes(split_size_rows[i].npackets, split_size_rows[i].nchannels, split_size_rows[i].out_cap);
        if (got != split_size_rows[i].bytes) { printf("FAIL %s: %zu, expected %zu\n", split_size_rows[i].name, got, split_size_rows[i].bytes); failures++; }
    }
    for (i = 0; i < ROWS(packed_size_rows); i++) {
        const size_t got = lzs_burst_plan_packed_split_work_bytes(packed_size_rows[i].npackets, packed_size_rows[i].nchannels, packed_size_rows[i].out_bytes);
        if (got != packed_size_rows[i].bytes) { printf("FAIL %s: %zu, expected %zu\n", packed_size_rows[i].name, got, packed_size_rows[i].bytes); failures++; }
    }
    for (i = 0; i < ROWS(bits_rows); i++) {
        const unsigned got = lzs_burst_plan_sort_bits(bits_rows[i].nchannels);
        if (got != bits_rows[i].bits) { printf("FAIL sort bits nchannels=%u: %u, expected %u\n", (unsigned)bits_rows[i].nchannels, got, bits_rows[i].bits); failures++; }
    }
    for (i = 0; i < ROWS(grid_rows); i++) {
        const uint32_t got = lzs_burst_plan_resolve_grid(grid_rows[i].npackets, grid_rows[i].nchannels);
        if (got != grid_rows[i].grid) {
            printf("FAIL resolve grid npackets=%u nchannels=%u: %u, expected %u\n", (unsigned)grid_rows[i].npackets, (unsigned)grid_rows[i].nchannels,
                   (unsigned)got, (unsigned)grid_rows[i].grid);
            failures++;
        }
    }
    for (i = 0; i < ROWS(strided_rows); i++) {
        const lzs_burst_split_t got = lzs_burst_plan_split_strided(strided_rows[i].decompress, strided_rows[i].work_bytes, strided_rows[i].npackets,
                                                                   strided_rows[i].nchannels, strided_rows[i].out_cap);
        if (got.split != strided_rows[i].split || got.origin_cap != 0u) {
            printf("FAIL %s: split %d origin_cap %llu, expected %d 0\n", strided_rows[i].name, got.split, (unsigned long long)got.origin_cap, strided_rows[i].split);
            failures++;
        }
    }
    for (i = 0; i < ROWS(packed_rows); i++) {
        const lzs_burst_split_t got = lzs_burst_plan_split_packed(packed_rows[i].decompress, packed_rows[i].origin_bytes);
        if (got.split != packed_rows[i].split || got.origin_cap != packed_rows[i].origin_cap) {
            printf("FAIL packed split decompress=%d origin_bytes=%zu: split %d origin_cap %llu, expected %d %llu\n", packed_rows[i].decompress,
                   packed_rows[i].origin_bytes, got.split, (unsigned long long)got.origin_cap, packed_rows[i].split,
                   (unsigned long long)packed_rows[i].origin_cap);
            failures++;
        }
    }
    for (i = 0; i < ROWS(split_min_rows); i++) {
        const uint32_t got = lzs_burst_plan_split_min(split_min_rows[i].set, split_min_rows[i].value);
        if (got != split_min_rows[i].split_min) {
            printf("FAIL split_min set=%d value=%u: %u, expected %u\n", split_min_rows[i].set, (unsigned)split_min_rows[i].value, (unsigned)got,
                   (unsigned)split_min_rows[i].split_min);
            failures++;
        }
    }
    printf("%u rows, %d failure(s)\n", (unsigned)(ROWS(layout_rows) + ROWS(work_rows) + ROWS(split_size_rows) + ROWS(packed_size_rows) + ROWS(bits_rows) +
                                                   ROWS(grid_rows) + ROWS(strided_rows) + ROWS(packed_rows) + ROWS(split_min_rows)), failures);
    return failures ? 1 : 0;
}
