/* tests/cpu_shim/plan_check.c -- csrc/lzs_launch_plan.h held to tables of literal rows (tests/test_launch_plan.py builds this
 * with -fsanitize=address,undefined and runs it).  Every expected value below was worked out by hand from the rule the row's
 * group cites -- the line of lzs_kernels.hip at commit 1d0fe86, the last before the rules moved into the header -- and none
 * is computed by the function under test.  Prints one line per failing row, then "N failure(s)"; exit status 1 if N > 0. */
#include <stdio.h>
#include <stdint.h>
#include "lzs_launch_plan.h"

static int failures;
#define ROWS(t) (sizeof(t) / sizeof((t)[0]))

enum { S = LZS_RUN_SAFE, F = LZS_RUN_FEW, L = LZS_RUN_LIT, T = LZS_RUN_TEXT, C = LZS_RUN_CLASSIFY };

/* ---- compress, lzs_kernels.hip:452-476 (the packed copy: 505-530): chain mode gives safe; LZS_VARIANT few / lit that one; nothing
 * forced and at least kClassifyMinBlocks = 64 blocks the classifier; else text.  The load check steps when chain_mode == 0 and
 * may start from 256 blocks. */
static const struct { const char *name; int chain_mode, forced; uint32_t nblocks; int one_variant; int run, load_check, start; } compress_rows[] = {
    { "compress n=1 chain=0 forced=0",   0, 0, 1,   0, T, 1, 0 }, { "compress n=1 chain=0 forced=1",   0, 1, 1,   0, T, 1, 0 },
    { "compress n=1 chain=0 forced=2",   0, 2, 1,   0, F, 1, 0 }, { "compress n=1 chain=0 forced=3",   0, 3, 1,   0, L, 1, 0 },
    { "compress n=1 chain=1 forced=0",   1, 0, 1,   0, S, 0, 0 }, { "compress n=1 chain=1 forced=1",   1, 1, 1,   0, S, 0, 0 },
    { "compress n=1 chain=1 forced=2",   1, 2, 1,   0, S, 0, 0 }, { "compress n=1 chain=1 forced=3",   1, 3, 1,   0, S, 0, 0 },
    { "compress n=63 chain=0 forced=0",  0, 0, 63,  0, T, 1, 0 }, { "compress n=63 chain=0 forced=1",  0, 1, 63,  0, T, 1, 0 },
    { "compress n=63 chain=0 forced=2",  0, 2, 63,  0, F, 1, 0 }, { "compress n=63 chain=0 forced=3",  0, 3, 63,  0, L, 1, 0 },
    { "compress n=63 chain=1 forced=0",  1, 0, 63,  0, S, 0, 0 }, { "compress n=63 chain=1 forced=1",  1, 1, 63,  0, S, 0, 0 },
    { "compress n=63 chain=1 forced=2",  1, 2, 63,  0, S, 0, 0 }, { "compress n=63 chain=1 forced=3",  1, 3, 63,  0, S, 0, 0 },
    { "compress n=64 chain=0 forced=0",  0, 0, 64,  0, C, 1, 0 }, { "compress n=64 chain=0 forced=1",  0, 1, 64,  0, T, 1, 0 },
    { "compress n=64 chain=0 forced=2",  0, 2, 64,  0, F, 1, 0 }, { "compress n=64 chain=0 forced=3",  0, 3, 64,  0, L, 1, 0 },
    { "compress n=64 chain=1 forced=0",  1, 0, 64,  0, S, 0, 0 }, { "compress n=64 chain=1 forced=1",  1, 1, 64,  0, S, 0, 0 },
    { "compress n=64 chain=1 forced=2",  1, 2, 64,  0, S, 0, 0 }, { "compress n=64 chain=1 forced=3",  1, 3, 64,  0, S, 0, 0 },
    { "compress n=65 chain=0 forced=0",  0, 0, 65,  0, C, 1, 0 }, { "compress n=65 chain=0 forced=1",  0, 1, 65,  0, T, 1, 0 },
    { "compress n=65 chain=0 forced=2",  0, 2, 65,  0, F, 1, 0 }, { "compress n=65 chain=0 forced=3",  0, 3, 65,  0, L, 1, 0 },
    { "compress n=65 chain=1 forced=0",  1, 0, 65,  0, S, 0, 0 }, { "compress n=65 chain=1 forced=1",  1, 1, 65,  0, S, 0, 0 },
    { "compress n=65 chain=1 forced=2",  1, 2, 65,  0, S, 0, 0 }, { "compress n=65 chain=1 forced=3",  1, 3, 65,  0, S, 0, 0 },
    { "compress n=255 chain=0 forced=0", 0, 0, 255, 0, C, 1, 0 }, { "compress n=255 chain=0 forced=1", 0, 1, 255, 0, T, 1, 0 },
    { "compress n=255 chain=0 forced=2", 0, 2, 255, 0, F, 1, 0 }, { "compress n=255 chain=0 forced=3", 0, 3, 255, 0, L, 1, 0 },
    { "compress n=255 chain=1 forced=0", 1, 0, 255, 0, S, 0, 0 }, { "compress n=255 chain=1 forced=1", 1, 1, 255, 0, S, 0, 0 },
    { "compress n=255 chain=1 forced=2", 1, 2, 255, 0, S, 0, 0 }, { "compress n=255 chain=1 forced=3", 1, 3, 255, 0, S, 0, 0 },
    { "compress n=256 chain=0 forced=0", 0, 0, 256, 0, C, 1, 1 }, { "compress n=256 chain=0 forced=1", 0, 1, 256, 0, T, 1, 1 },
    { "compress n=256 chain=0 forced=2", 0, 2, 256, 0, F, 1, 1 }, { "compress n=256 chain=0 forced=3", 0, 3, 256, 0, L, 1, 1 },
    { "compress n=256 chain=1 forced=0", 1, 0, 256, 0, S, 0, 0 }, { "compress n=256 chain=1 forced=1", 1, 1, 256, 0, S, 0, 0 },
    { "compress n=256 chain=1 forced=2", 1, 2, 256, 0, S, 0, 0 }, { "compress n=256 chain=1 forced=3", 1, 3, 256, 0, S, 0, 0 },
    /* :457 and :510, #ifndef LZS_ONE_VARIANT: such a build has safe and text only, whatever is forced and however many blocks */
    { "compress one_variant forced=2",          0, 2, 1,    1, T, 1, 0 },
    { "compress one_variant forced=0 n=4096",   0, 0, 4096, 1, T, 1, 1 },
    { "compress one_variant chain=1 forced=3",  1, 3, 64,   1, S, 0, 0 },
};

/* ---- variants, lzs_kernels.hip:392-410 (variant_hint).  have_seen 0 passes no words at all. */
static const struct { const char *name; int have_seen; uint32_t seen[4]; int capturing; uint32_t allow, catch_all; } variant_rows[] = {
    /* :395, :397 -- nothing known: all three, the default catches */
    { "variants no seen words",            0, { 0, 0, 0, 0 }, 0, 0xEu, 1u },
    { "variants all seen zero",            1, { 0, 0, 0, 0 }, 0, 0xEu, 1u },
    { "variants seen[0] alone is no class", 1, { 0x80000009u, 0, 0, 0 }, 0, 0xEu, 1u },
    /* :406-407 -- one class only: that variant, and it catches */
    { "variants class 1 only",             1, { 0, 0x80000005u, 0, 0 }, 0, 0x2u, 1u },
    { "variants class 2 only",             1, { 0, 0, 0x80000005u, 0 }, 0, 0x4u, 2u },
    { "variants class 3 only",             1, { 0, 0, 0, 0x80000005u }, 0, 0x8u, 3u },
    /* :406 -- newest - seen <= 2: seen by one of the last three classifiers */
    { "variants age: 2 before newest kept",   1, { 0, 0x80000008u, 0x8000000Au, 0 }, 0, 0x6u, 1u },
    { "variants age: 3 before newest dropped", 1, { 0, 0x80000007u, 0x8000000Au, 0 }, 0, 0x4u, 2u },
    { "variants age: 1 and 2 before, all kept", 1, { 0, 0x80000009u, 0x80000008u, 0x8000000Au }, 0, 0xEu, 1u },
    { "variants age: default dropped, lit and few kept", 1, { 0, 0x80000001u, 0x80000010u, 0x8000000Fu }, 0, 0xCu, 2u },
    /* :396, :399 -- ids are counter | 0x80000000, so after 0xFFFFFFFF they go on from 0x80000000: 0x80000002 is the newest, 0xFFFFFFFF
     * lies three launches behind it (dropped), 0x80000001 one (kept).  THE ONE ROW THE PARENT'S LINE MISSES: (int32_t)(a - b) > 0 on
     * two values with bit 31 set is their plain order, which keeps 0xFFFFFFFF as the newest (allow 0x2, catch_all 1) until a
     * class is seen again; the header compares serial numbers of 31 bits instead.  The bytes of a launch never depended on it. */
    { "variants id wrap",                  1, { 0, 0xFFFFFFFFu, 0x80000001u, 0x80000002u }, 0, 0xCu, 2u },
    { "variants id wrap, ages across it",  1, { 0, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu }, 0, 0xAu, 1u },   /* 0xFFFFFFFF two behind 0x80000001 (kept), 0xFFFFFFFE three */
    /* far from the wrap both readings agree: ids 0x0FFFFFFF launches apart */
    { "variants ids far apart, no wrap",   1, { 0, 0x80000001u, 0x90000000u, 0 }, 0, 0x4u, 2u },
    /* :402-404 -- while capturing every variant is launched */
    { "variants capture with narrow seen", 1, { 0, 0, 0x80000005u, 0 }, 1, 0xEu, 1u },
    { "variants capture, nothing known",   1, { 0, 0, 0, 0 }, 1, 0xEu, 1u },
};

/* ---- streams per wavefront, lzs_kernels.hip:567-568 (blocks), 600-601 (channels), 616-617 (runs):
 * eight exactly when in_stride * span + longest < 0xFFFFFF00 = 4294967040, longest = lengths on the device ? 0xC0000400 = 3221226496 : in_len */
static const struct { const char *name; int runs; uint64_t in_stride; uint32_t npackets; int have_lens; uint32_t in_len; uint32_t per_wave; } per_wave_rows[] = {
    /* span 7, in_len 65536: 7 * 613557357 + 65536 = 4294967035; 7 * 613557358 + 65536 = 4294967042 */
    { "per-wave no lengths: largest stride for 8", 0, 613557357ull, 0, 0, 65536u, 8u },
    { "per-wave no lengths: that plus one",        0, 613557358ull, 0, 0, 65536u, 1u },
    /* span 7, lengths on the device: 7 * 153391506 + 3221226496 = 4294967038; 7 * 153391507 + 3221226496 = 4294967045 */
    { "per-wave with lengths: largest stride for 8", 0, 153391506ull, 0, 1, 65536u, 8u },
    { "per-wave with lengths: that plus one",        0, 153391507ull, 0, 1, 65536u, 1u },
    { "per-wave dense blocks of 64 KiB",             0, 65536ull, 0, 0, 65536u, 8u },
    /* runs, span npackets - 1.  npackets 1: span 0, no stride matters */
    { "per-wave runs npackets=1, huge stride",       1, 0x100000000ull, 1u, 0, 65536u, 8u },
    { "per-wave runs npackets=1, with lengths",      1, 0x100000000ull, 1u, 1, 65536u, 8u },
    /* npackets 2: span 1: 4294901503 + 65536 = 4294967039; one more is the bound itself */
    { "per-wave runs npackets=2: largest stride for 8", 1, 4294901503ull, 2u, 0, 65536u, 8u },
    { "per-wave runs npackets=2: that plus one",        1, 4294901504ull, 2u, 0, 65536u, 1u },
    /* npackets 65536: span 65535: 65535 * 65535 + 65536 = 4294901761; 65535 * 65536 + 65536 = 4294967296.  (With span 7 both strides would give 8.) */
    { "per-wave runs npackets=65536 stride 65535",   1, 65535ull, 65536u, 0, 65536u, 8u },
    { "per-wave runs npackets=65536 stride 65536",   1, 65536ull, 65536u, 0, 65536u, 1u },
    /* the same stride and lengths as the blocks' row above, but 9 packets: span 8 instead of 7: 8 * 613557357 + 65536 = 4908524392 */
    { "per-wave runs npackets=9 at the blocks' largest stride", 1, 613557357ull, 9u, 0, 65536u, 1u },
};

/* ---- decode of a stream's segments, lzs_kernels.hip:750-766: g8 when !old_decode && (n == 0 || cap <= 6n); two when !one_token &&
 * n != 0 && 4n > cap && 10n < 9cap; wide when !one_token && n != 0 && 10n >= 9cap; 64-bit arithmetic */
enum { W = LZS_DECODE_WAVE, P = LZS_DECODE_G8_PLAIN, T2 = LZS_DECODE_G8_TWO, WD = LZS_DECODE_G8_WIDE };
static const struct { const char *name; uint32_t n, cap; int old_decode, one_token; int form; } decode_rows[] = {
    { "decode n=0",                         0u, 1000000u, 0, 0, P },
    { "decode n=0 cap=0",                   0u, 0u, 0, 0, P },
    { "decode cap=6n",                      1000u, 6000u, 0, 0, P },
    { "decode cap=6n+1",                    1000u, 6001u, 0, 0, W },
    { "decode 4n=cap",                      1000u, 4000u, 0, 0, P },
    { "decode 4n=cap+1",                    1000u, 3999u, 0, 0, T2 },
    { "decode 10n=9cap-10 (n one below)",   899u, 1000u, 0, 0, T2 },
    { "decode 10n=9cap",                    900u, 1000u, 0, 0, WD },
    { "decode 10n=9cap+10 (n one above)",   901u, 1000u, 0, 0, WD },
    { "decode 10n=9cap-1",                  8999u, 9999u, 0, 0, T2 },      /* 89990 < 89991 */
    { "decode 10n=9cap+1",                  9001u, 10001u, 0, 0, WD },     /* 90010 >= 90009 */
    { "decode text (0.57)",                 570u, 1000u, 0, 0, T2 },
    { "decode old_decode, g8 range",        570u, 1000u, 1, 0, W },
    { "decode old_decode, n=0",             0u, 1000u, 1, 0, W },
    { "decode old_decode, one_token",       900u, 1000u, 1, 1, W },
    { "decode one_token in two's range",    570u, 1000u, 0, 1, P },
    { "decode one_token in wide's range",   900u, 1000u, 0, 1, P },
    { "decode one_token, expands sevenfold", 100u, 700u, 0, 1, W },
    /* 6n, 4n, 10n and 9cap all pass 2^32 here: in 32 bits 10n = 0xFFFFFFF6 < 9cap = 0xFFFFFFF7 would say "two" */
    { "decode n=cap=0xFFFFFFFF",            0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, WD },
    { "decode n=0x40000000 cap=0xFFFFFFFF", 0x40000000u, 0xFFFFFFFFu, 0, 0, T2 },   /* 4n = 2^32 > cap only in 64 bits */
    { "decode n=0x2AAAAAAA cap=0xFFFFFFFF", 0x2AAAAAAAu, 0xFFFFFFFFu, 0, 0, W },     /* 6n = 0xFFFFFFFC < cap */
};

/* ---- scan of a stream's segments, lzs_kernels.hip:714-737: the wave kernel when LZS_SCAN=wave or neither the all-ones flags nor a
 * compare round; else lzs_all_ones_kernel first if there are flags, a lane per segment with the marks cleared first when there are
 * marks and it is no compare round, or (LZS_SCAN=g8) eight lanes and no clearing.  Columns: all_ones, compare, marks, concat,
 * scan_env (0 unset, 1 wave, 2 g8) -> lanes (0: the wave kernel), concat, all_ones_first, clear_marks. */
static const struct { int all_ones, compare, marks, concat, scan_env; int lanes, concat_out, all_ones_first, clear_marks; } scan_rows[] = {
    { 0, 0, 0, 0, 0,  0, 0, 0, 0 }, { 0, 0, 0, 0, 1,  0, 0, 0, 0 }, { 0, 0, 0, 0, 2,  0, 0, 0, 0 },
    { 0, 0, 0, 1, 0,  0, 1, 0, 0 }, { 0, 0, 0, 1, 1,  0, 1, 0, 0 }, { 0, 0, 0, 1, 2,  0, 1, 0, 0 },
    { 0, 0, 1, 0, 0,  0, 0, 0, 0 }, { 0, 0, 1, 0, 1,  0, 0, 0, 0 }, { 0, 0, 1, 0, 2,  0, 0, 0, 0 },
    { 0, 0, 1, 1, 0,  0, 1, 0, 0 }, { 0, 0, 1, 1, 1,  0, 1, 0, 0 }, { 0, 0, 1, 1, 2,  0, 1, 0, 0 },
    { 0, 1, 0, 0, 0,  1, 0, 0, 0 }, { 0, 1, 0, 0, 1,  0, 0, 0, 0 }, { 0, 1, 0, 0, 2,  8, 0, 0, 0 },
    { 0, 1, 0, 1, 0,  1, 1, 0, 0 }, { 0, 1, 0, 1, 1,  0, 1, 0, 0 }, { 0, 1, 0, 1, 2,  8, 1, 0, 0 },
    { 0, 1, 1, 0, 0,  1, 0, 0, 0 }, { 0, 1, 1, 0, 1,  0, 0, 0, 0 }, { 0, 1, 1, 0, 2,  8, 0, 0, 0 },
    { 0, 1, 1, 1, 0,  1, 1, 0, 0 }, { 0, 1, 1, 1, 1,  0, 1, 0, 0 }, { 0, 1, 1, 1, 2,  8, 1, 0, 0 },
    { 1, 0, 0, 0, 0,  1, 0, 1, 0 }, { 1, 0, 0, 0, 1,  0, 0, 0, 0 }, { 1, 0, 0, 0, 2,  8, 0, 1, 0 },
    { 1, 0, 0, 1, 0,  1, 1, 1, 0 }, { 1, 0, 0, 1, 1,  0, 1, 0, 0 }, { 1, 0, 0, 1, 2,  8, 1, 1, 0 },
    { 1, 0, 1, 0, 0,  1, 0, 1, 1 }, { 1, 0, 1, 0, 1,  0, 0, 0, 0 }, { 1, 0, 1, 0, 2,  8, 0, 1, 0 },
    { 1, 0, 1, 1, 0,  1, 1, 1, 1 }, { 1, 0, 1, 1, 1,  0, 1, 0, 0 }, { 1, 0, 1, 1, 2,  8, 1, 1, 0 },
    { 1, 1, 0, 0, 0,  1, 0, 1, 0 }, { 1, 1, 0, 0, 1,  0, 0, 0, 0 }, { 1, 1, 0, 0, 2,  8, 0, 1, 0 },
    { 1, 1, 0, 1, 0,  1, 1, 1, 0 }, { 1, 1, 0, 1, 1,  0, 1, 0, 0 }, { 1, 1, 0, 1, 2,  8, 1, 1, 0 },
    { 1, 1, 1, 0, 0,  1, 0, 1, 0 }, { 1, 1, 1, 0, 1,  0, 0, 0, 0 }, { 1, 1, 1, 0, 2,  8, 0, 1, 0 },
    { 1, 1, 1, 1, 0,  1, 1, 1, 0 }, { 1, 1, 1, 1, 1,  0, 1, 0, 0 }, { 1, 1, 1, 1, 2,  8, 1, 1, 0 },
};

/* ---- resolve everywhere, lzs_kernels.hip:790-791: min((total / 4 + 255) / 256 + 1, 65536) */
static const struct { const char *name; uint32_t total, grid; } resolve_rows[] = {
    { "resolve total=1",                        1u, 1u },
    { "resolve total=1023",                     1023u, 2u },           /* (255 + 255) / 256 + 1 */
    { "resolve total=1024",                     1024u, 2u },           /* (256 + 255) / 256 + 1 */
    { "resolve total=1028",                     1028u, 3u },           /* (257 + 255) / 256 + 1 */
    { "resolve total=67104768",                 67104768u, 65533u },   /* 16776192 + 255 = 16776447 = 65532 * 256 + 255 */
    { "resolve total=67106819, last below the cap", 67106819u, 65535u },   /* 16776704 + 255 = 16776959 = 65535 * 256 - 1 */
    { "resolve total=67106820, first at the cap",   67106820u, 65536u },   /* 16776705 + 255 = 65535 * 256 */
    { "resolve total=67107844, first the cap cuts", 67107844u, 65536u },   /* 16776961 + 255 = 65536 * 256: 65537 uncut */
    { "resolve total=0xFFFFFFFF",               0xFFFFFFFFu, 65536u },
};

int main(void)
{
    size_t i;
    for (i = 0; i < ROWS(compress_rows); i++) {
        const lzs_plan_compress_t p = lzs_plan_compress(compress_rows[i].chain_mode, compress_rows[i].forced, compress_rows[i].nblocks, 64u,
                                                        compress_rows[i].one_variant);
        if (p.run != compress_rows[i].run || p.load_check != compress_rows[i].load_check || p.load_check_start != compress_rows[i].start) {
            printf("FAIL %s: run %d load check %d start %d, expected %d %d %d\n", compress_rows[i].name, p.run, p.load_check, p.load_check_start,
                   compress_rows[i].run, compress_rows[i].load_check, compress_rows[i].start);
            failures++;
        }
    }
    for (i = 0; i < ROWS(variant_rows); i++) {
        const lzs_plan_variants_t p = lzs_plan_variants(variant_rows[i].have_seen ? variant_rows[i].seen : NULL, variant_rows[i].have_seen,
                                                        variant_rows[i].capturing);
        if (p.allow != variant_rows[i].allow || p.catch_all != variant_rows[i].catch_all) {
            printf("FAIL %s: allow 0x%X catch_all %u, expected 0x%X %u\n", variant_rows[i].name, (unsigned)p.allow, (unsigned)p.catch_all,
                   (unsigned)variant_rows[i].allow, (unsigned)variant_rows[i].catch_all);
            failures++;
        }
    }
    for (i = 0; i < ROWS(per_wave_rows); i++) {
        const uint32_t got = per_wave_rows[i].runs
            ? lzs_plan_dec_per_wave_runs(per_wave_rows[i].in_stride, per_wave_rows[i].npackets, per_wave_rows[i].have_lens, per_wave_rows[i].in_len)
            : lzs_plan_dec_per_wave_blocks(per_wave_rows[i].in_stride, per_wave_rows[i].have_lens, per_wave_rows[i].in_len);
        if (got != per_wave_rows[i].per_wave) {
            printf("FAIL %s: %u to a wavefront, expected %u\n", per_wave_rows[i].name, (unsigned)got, (unsigned)per_wave_rows[i].per_wave);
            failures++;
        }
    }
    for (i = 0; i < ROWS(decode_rows); i++) {
        const int got = lzs_plan_decode_stream(decode_rows[i].n, decode_rows[i].cap, decode_rows[i].old_decode, decode_rows[i].one_token);
        if (got != decode_rows[i].form) {
            printf("FAIL %s: form %d, expected %d\n", decode_rows[i].name, got, decode_rows[i].form);
            failures++;
        }
    }
    for (i = 0; i < ROWS(scan_rows); i++) {
        const lzs_plan_scan_t p = lzs_plan_scan(scan_rows[i].all_ones, scan_rows[i].compare, scan_rows[i].marks, scan_rows[i].concat, scan_rows[i].scan_env);
        if (p.lanes != scan_rows[i].lanes || p.concat != scan_rows[i].concat_out || p.all_ones_first != scan_rows[i].all_ones_first ||
            p.clear_marks != scan_rows[i].clear_marks) {
            printf("FAIL scan all_ones=%d compare=%d marks=%d concat=%d scan_env=%d: lanes %d concat %d all_ones_first %d clear_marks %d, expected %d %d %d %d\n",
                   scan_rows[i].all_ones, scan_rows[i].compare, scan_rows[i].marks, scan_rows[i].concat, scan_rows[i].scan_env,
                   p.lanes, p.concat, p.all_ones_first, p.clear_marks,
                   scan_rows[i].lanes, scan_rows[i].concat_out, scan_rows[i].all_ones_first, scan_rows[i].clear_marks);
            failures++;
        }
    }
    for (i = 0; i < ROWS(resolve_rows); i++) {
        const uint32_t got = lzs_plan_resolve_grid(resolve_rows[i].total);
        if (got != resolve_rows[i].grid) {
            printf("FAIL %s: grid %u, expected %u\n", resolve_rows[i].name, (unsigned)got, (unsigned)resolve_rows[i].grid);
            failures++;
        }
    }
    printf("%u rows, %d failure(s)\n", (unsigned)(ROWS(compress_rows) + ROWS(variant_rows) + ROWS(per_wave_rows) + ROWS(decode_rows) + ROWS(scan_rows) +
                                                   ROWS(resolve_rows)), failures);
    return failures ? 1 : 0;
}
