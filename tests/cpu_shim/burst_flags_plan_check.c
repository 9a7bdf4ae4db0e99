/* tests/cpu_shim/burst_flags_plan_check.c -- what csrc/lzs_burst_plan.h adds for packet flags (history resets inside a burst,
 * DESIGN.md 3.18) held to tables of literal rows: the staging slots of the decoder, where the start marks lie, RESOLVE's grid with
 * flags, the staging slot of a run.  tests/test_burst_flags_plan.py builds this with -fsanitize=address,undefined and runs it.
 * The rows are worked out by hand from the documented layout -- every part rounded up to 256 bytes, the staging slots behind the six
 * tables laid over the slots, n / 2 of them --; the values of the fields the header had before are those of burst_plan_check.c's
 * rows (n = 3 by the same arithmetic): they must not have moved.  None is computed by the function under test.  Prints one line per
 * failing row, then "N failure(s)"; exit status 1 if N > 0. */
#include <stdio.h>
#include <stdint.h>
#include "lzs_burst_plan.h"

static int failures;
#define ROWS(t) (sizeof(t) / sizeof((t)[0]))

/* part[]: slots, key 0 1, val 0 1, lens, ends, weight 0 1, at 0 1, run_end, temp; over[]: nheavy, light_w, light_at, rec, rooms,
 * room_ends; then the new fields: stage, stage_slots, stage_end, marks */
enum { PARTS = 13, OVER = 6 };
static const struct { size_t n, part[PARTS], temp_bytes, total, over[OVER], stage, stage_slots, stage_end, marks; } rows[] = {
    { 1u, { 0u, 2304u, 2560u, 2816u, 3072u, 3328u, 3584u, 3840u, 4096u, 4352u, 4608u, 4864u, 5120u },
      65792u, 70912u, { 0u, 256u, 512u, 768u, 1024u, 1280u }, 1536u, 0u, 1536u, 3840u },
    { 2u, { 0u, 4352u, 4608u, 4864u, 5120u, 5376u, 5632u, 5888u, 6144u, 6400u, 6656u, 6912u, 7168u },
      65792u, 72960u, { 0u, 256u, 512u, 768u, 1024u, 1280u }, 1536u, 1u, 3840u, 5888u },
    { 3u, { 0u, 6400u, 6656u, 6912u, 7168u, 7424u, 7680u, 7936u, 8192u, 8448u, 8704u, 8960u, 9216u },
      65792u, 75008u, { 0u, 256u, 512u, 768u, 1024u, 1280u }, 1536u, 1u, 3840u, 7936u },
    { 255u, { 0u, 538624u, 539648u, 540672u, 541696u, 542720u, 544768u, 546816u, 547840u, 548864u, 549888u, 550912u, 551936u },
      67584u, 619520u, { 0u, 256u, 1280u, 2304u, 4352u, 6400u }, 8448u, 127u, 276736u, 546816u },
    { 256u, { 0u, 540672u, 541696u, 542720u, 543744u, 544768u, 546816u, 548864u, 549888u, 550912u, 551936u, 552960u, 553984u },
      67584u, 621568u, { 0u, 256u, 1280u, 2304u, 4352u, 6400u }, 8448u, 128u, 278784u, 548864u },
    { 257u, { 0u, 542976u, 544256u, 545536u, 546816u, 548096u, 550400u, 552704u, 553984u, 555264u, 556544u, 557824u, 559104u },
      67840u, 626944u, { 0u, 256u, 1536u, 2816u, 5120u, 7424u }, 9728u, 128u, 280064u, 552704u },
    { 65536u, { 0u, 138412032u, 138674176u, 138936320u, 139198464u, 139460608u, 139984896u, 140509184u, 140771328u, 141033472u, 141295616u, 141557760u, 141819904u },
      589824u, 142409728u, { 0u, 256u, 262400u, 524544u, 1048832u, 1573120u }, 2097408u, 32768u, 71303424u, 140509184u },
    { LZS_BURST_PACKETS_MAX, { 0u, 4535485462528u, 4544075397120u, 4552665331712u, 4561255266304u, 4569845200896u, 4587025070080u, 4604204939264u, 4612794873856u, 4621384808448u, 4629974743040u, 4638564677632u, 4647154612224u },
      17179934720u, 4664334546944u, { 0u, 256u, 8589934848u, 17179869440u, 34359738624u, 51539607808u }, 68719476992u, 1073741823u, 2336462207232u, 4604204939264u },
};

/* the three sizes at those n (nchannels changes nothing; out_cap 1500, 1000 bytes of room): the burst size, + 2 * n * 1500, + 2000 */
static const struct { size_t n, work, split, packed; } size_rows[] = {
    { 1u, 70912u, 73912u, 72912u }, { 2u, 72960u, 78960u, 74960u }, { 3u, 75008u, 84008u, 77008u }, { 255u, 619520u, 1384520u, 621520u },
    { 256u, 621568u, 1389568u, 623568u }, { 257u, 626944u, 1397944u, 628944u }, { 65536u, 142409728u, 339017728u, 142411728u },
    { LZS_BURST_PACKETS_MAX, 4664334546944u, 11106785487944u, 4664334548944u },
};

/* RESOLVE's grid: with flags a workgroup per packet, without them lzs_burst_plan_resolve_grid's npackets <= nchannels ? npackets : nchannels + 1 */
static const struct { uint32_t npackets, nchannels; int flags; uint32_t grid; } grid_rows[] = {
    { 1u, 1u, 0, 1u }, { 1u, 1u, 1, 1u }, { 10u, 8u, 0, 9u }, { 10u, 8u, 1, 10u }, { 4096u, 1u, 0, 2u }, { 4096u, 1u, 1, 4096u },
    { 7u, 8u, 0, 7u }, { 7u, 8u, 1, 7u }, { 65536u, 16384u, 0, 16385u }, { 65536u, 16384u, 1, 65536u },
    { 0x7FFFFFFFu, 1u, 0, 2u }, { 0x7FFFFFFFu, 1u, 1, 0x7FFFFFFFu }, { 3u, 1u, 2, 3u },
};

/* the staging slot of a channel whose last run is run `run` of the call and not the channel's first: (run - 1) / 2 */
static const struct { uint32_t run, slot; } slot_rows[] = {
    { 1u, 0u }, { 2u, 0u }, { 3u, 1u }, { 4u, 1u }, { 5u, 2u }, { 254u, 126u }, { 255u, 127u }, { 65535u, 32767u }, { 0x7FFFFFFEu, 0x3FFFFFFEu },
};

#define CHECK(what, got, want) do { \
    const unsigned long long g_ = (unsigned long long)(got), w_ = (unsigned long long)(want); \
    if (g_ != w_) { printf("n = %zu: %s is %llu, the row has %llu\n", n, what, g_, w_); failures++; } } while (0)

int main(void)
{
    size_t n = 0;
    for (size_t r = 0; r < ROWS(rows); r++) {
        n = rows[r].n;
        const lzs_burst_layout_t L = lzs_burst_layout(n);
        const size_t part[PARTS] = { L.slots, L.key[0], L.key[1], L.val[0], L.val[1], L.lens, L.ends, L.weight[0], L.weight[1], L.at[0], L.at[1],
                                     L.run_end, L.temp };
        const size_t over[OVER] = { L.nheavy, L.light_w, L.light_at, L.rec, L.rooms, L.room_ends };
        for (int k = 0; k < PARTS; k++) CHECK("a part the header had before", part[k], rows[r].part[k]);
        for (int k = 0; k < OVER; k++) CHECK("a table over the slots", over[k], rows[r].over[k]);
        CHECK("temp_bytes", L.temp_bytes, rows[r].temp_bytes);
        CHECK("total", L.total, rows[r].total);
        CHECK("origins", L.origins, rows[r].total);
        CHECK("stage", L.stage, rows[r].stage);
        CHECK("stage_slots", L.stage_slots, rows[r].stage_slots);
        CHECK("stage_end", L.stage_end, rows[r].stage_end);
        CHECK("marks", L.marks, rows[r].marks);
        /* the new parts end inside what they borrow: the staging slots begin behind room_ends' 8 bytes a packet and end before the
         * slots' region does; the marks are weight[0], 4 bytes a packet, which ends where weight[1] begins; every slot a run can be
         * given (the last run of n is run n - 1) lies below stage_slots */
        if (L.stage % LZS_BURST_ALIGN || L.stage < L.room_ends + 8u * n) { printf("n = %zu: stage %zu lies in room_ends\n", n, L.stage); failures++; }
        if (L.stage + L.stage_slots * LZS_BURST_SLOT_BYTES > L.stage_end || L.stage_end > L.key[0]) {
            printf("n = %zu: the staging slots end at %zu, the slots' region at %zu\n", n, L.stage + L.stage_slots * LZS_BURST_SLOT_BYTES, L.key[0]);
            failures++;
        }
        if (L.marks + 4u * n > L.weight[1]) { printf("n = %zu: the marks do not fit weight[0]\n", n); failures++; }
        if (n >= 2u && lzs_burst_plan_stage_slot((uint32_t)(n - 1u)) >= L.stage_slots) { printf("n = %zu: run n - 1 has no staging slot\n", n); failures++; }
    }
    for (size_t r = 0; r < ROWS(size_rows); r++) {
        n = size_rows[r].n;
        CHECK("lzs_burst_plan_work_bytes", lzs_burst_plan_work_bytes(n, 3u), size_rows[r].work);
        CHECK("lzs_burst_plan_split_work_bytes", lzs_burst_plan_split_work_bytes(n, 3u, 1500u), size_rows[r].split);
        CHECK("lzs_burst_plan_packed_split_work_bytes", lzs_burst_plan_packed_split_work_bytes(n, 3u, 1000u), size_rows[r].packed);
    }
    for (size_t r = 0; r < ROWS(grid_rows); r++) {
        n = grid_rows[r].npackets;
        CHECK("lzs_burst_plan_resolve_grid_flags", lzs_burst_plan_resolve_grid_flags(grid_rows[r].npackets, grid_rows[r].nchannels, grid_rows[r].flags),
              grid_rows[r].grid);
    }
    for (size_t r = 0; r < ROWS(slot_rows); r++) {
        n = slot_rows[r].run;
        CHECK("lzs_burst_plan_stage_slot", lzs_burst_plan_stage_slot(slot_rows[r].run), slot_rows[r].slot);
    }
    printf("%zu layout rows, %zu size rows, %zu grid rows, %zu slot rows: %d failure(s)\n", ROWS(rows), ROWS(size_rows), ROWS(grid_rows),
           ROWS(slot_rows), failures);
    return failures ? 1 : 0;
}
