/* search_lane_sim.c -- development aid (CPU only): a lane model of the text variant's SEARCH (kernels/compress_wg.inc, wg_search as
 * wgv_text runs it), priced in vector instructions per wave and pool from the instruction ledger (profiles/r06/ledger_text.txt).
 * Where search_sim.c counts steps per position, this one runs the kernel's own rules candidate by candidate -- the one-byte probe at
 * offset best-length, the hop and step rules, the restart on the 2-byte chain -- on the kernel's own tables (1152 / 512 buckets, its
 * multipliers, wg_hash3x4's scaling, HASH's not-inserted rule, the offset-1 seed, the refill pass's walk3 / walk2 / capped), with four
 * waves that pull positions from one counter, walks carried into the next pool and the kernel's rule for leaving.  The waves run their
 * loop iterations in turn (lock step); on the device they drift, which is the model's one known liberty.
 * What it does not price is latency: it counts instructions.  Timed (profiles/r07/README.md), its ranking of the shapes under one
 * rule held to about 0.5 %, except where a shape changes the number of loop trips (one sub-step a pass: predicted -0.2 %, timed
 * +2.2 %); item 2's rule, which it prices at +1.5 %, timed -1.5 %: its hop consumes each compare by a select, today's ANDs two lane masks.
 * Not part of the library, computes no compressed output.
 *   build: gcc -O2 tools/sim/search_lane_sim.c -Llzs_compression_amd -llzs_workload -Wl,-rpath,$PWD/lzs_compression_amd -o tools/sim/search_lane_sim
 *   usage: search_lane_sim [nblocks = 256] [first_block = 0] [class = 0]          prints the table of profiles/r07/search_shape_sim.txt
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int lzs_workload_fill(uint8_t *, unsigned, uint64_t, uint64_t, size_t, size_t, int);

enum { N = 65536, WINDOW = 2047, CAP = 12, NOLINK = 0xFFFF, POOL = 512, H3 = 1152, H2 = 512, H2SHIFT = 7 };
#define M3 0x897397u
#define M2 0x64EBAD33u
enum { KEY_NONE3 = 0x2000, KEY_NONE2 = 0x1000 };

/* prices, vector instructions (ledger_text.txt): a hop 10, a full step 39.5 (the pass of 2 x (2 hops + step) is 119), a loop trip 2,
 * its leave test 4 once the pool is handed out, a refill pass 7 + 45 when a lane takes a position + 12 when the offset-1 length is
 * computed.  Item 2's rule, counted in a listing of the kernel built with it (tools/isa.sh; profiles/r07/README.md): a hop 11 (the AND
 * of two lane masks, a scalar instruction, becomes a second select), a step the same (+1 v_min_u16, -1 select): the pass 119 -> 123. */
static const double PRICE_HOP = 10.0, PRICE_STEP = 39.5, PRICE_HOP_END = 11.0, PRICE_STEP_END = 39.5;
static const double PRICE_TRIP = 2.0, PRICE_LEAVE = 4.0, PRICE_PASS = 7.0, PRICE_TAKE = 45.0, PRICE_LEN1 = 12.0, PRICE_MIDCHECK = 2.0;
static const double LEDGER_TOTAL = 886.0;   /* a wave's vector instructions per pool with today's tables: 6.92 per byte x 128 */

static uint8_t *blk; static unsigned nblocks;
static uint16_t l3[N], l2[N];

static uint32_t b3(uint32_t t) { const uint32_t lo = (t & 0xFFFFFFu) * M3; return (uint32_t)(((uint64_t)lo * (4u * H3)) >> 32) >> 2; }
static uint32_t b2(uint32_t t) { return (((t & 0xFFFFu) * M2) >> H2SHIFT) & (H2 - 1); }

/* HASH + CHAIN of a whole block.  Not inserted: the five aligned words [(p - 4) & ~3, + 20) hold one byte value. */
static void build(const uint8_t *s)
{
    static uint32_t head3[H3], head2[H2];
    memset(head3, 0xFF, sizeof head3); memset(head2, 0xFF, sizeof head2);
    for (uint32_t p = 0; p < N; p++) {
        int skip = p >= 4 && ((p - 4) & ~3u) + 20 <= N;
        if (skip) { const uint32_t a = (p - 4) & ~3u; for (uint32_t k = 1; k < 20; k++) if (s[a + k] != s[a]) { skip = 0; break; } }
        l3[p] = l2[p] = NOLINK;
        if (skip) continue;
        const uint32_t t = s[p] | (p + 1 < N ? s[p + 1] << 8 : 0) | (p + 2 < N ? s[p + 2] << 16 : 0);
        uint32_t h = b3(t), o = head3[h]; head3[h] = p; if (o != ~0u && p - o < NOLINK) l3[p] = (uint16_t)(p - o);
        h = b2(t); o = head2[h]; head2[h] = p; if (o != ~0u && p - o < NOLINK) l2[p] = (uint16_t)(p - o);
    }
}
static uint32_t lcp(const uint8_t *s, uint32_t a, uint32_t b, uint32_t lim) { uint32_t l = 0; while (l < lim && s[a + l] == s[b + l]) l++; return l; }

typedef struct { uint32_t p, d, cap, first2, reach; int32_t key; int two; } Lane;     /* d: distance of the candidate to look at next; 0 = idle */

typedef struct {
    int nsub, hops[4];          /* sub-steps of a pass and the hops in front of each one's full step */
    int hop_end;                /* item 2's rule */
    int refill_lo, refill_hi;   /* kRefillMin while less / more than `split` of the pool is handed out */
    int split;                  /* positions; POOL: one threshold */
    int mid;                    /* > 0: a refill check between sub-steps from `mid` idle lanes on */
} Shape;

typedef struct {
    double trips, iters, passes, empty, len1, taken, busy, leave_tests, midchecks;
    double step_slots, hop_slots, steps_used, hops_used;       /* lane-slots offered and used */
    double step_pass, step_forced, step_ranout, step_endonly, restarts;
    double positions, wavepools;
} Count;

static void take(const uint8_t *s, Lane *L, uint32_t p, int *any_len1)
{
    const uint32_t lim = N - p < CAP ? N - p : CAP, reach = p < WINDOW ? p : WINDOW;
    const int maybe1 = p >= 1 && lim >= 2 && s[p] == s[p - 1] && s[p + 1] == s[p];
    uint32_t len1 = 0;
    if (maybe1) { *any_len1 = 1; len1 = lcp(s, p, p - 1, lim); }
    const int seeded = maybe1 && len1 >= 2, capped = seeded && len1 == lim;
    const int walk3 = lim >= 3 && !capped && l3[p] <= reach;
    const int walk2 = lim >= 2 && !capped && !seeded && l2[p] <= reach;
    L->p = p; L->reach = reach;
    L->first2 = walk2 ? l2[p] : NOLINK;
    L->d = walk3 ? l3[p] : (walk2 ? l2[p] : 0);
    L->key = seeded ? (int32_t)((len1 << 12) - 1u) : (walk3 ? KEY_NONE3 : KEY_NONE2);
    L->cap = (walk3 || walk2) ? (walk3 ? lim : 2u) : 0u;
    L->two = !walk3;
}
static int probe_differs(const uint8_t *s, const Lane *L)
{
    const uint32_t bl = ((uint32_t)L->key + 0xFFFu) >> 12;
    return s[L->p + bl - L->d] != s[L->p + bl];
}
static void hop(const uint8_t *s, Lane *L, const Shape *sh, Count *c)
{
    if (!L->d || !probe_differs(s, L)) return;
    const uint32_t nx = L->d + (L->two ? l2 : l3)[L->p - L->d];
    if (nx <= L->reach) { L->d = nx; c->hops_used++; }
    else if (sh->hop_end) { L->d = 0; c->hops_used++; }        /* to its own position; cap stays: the step that follows ends the walk */
}
static void step(const uint8_t *s, Lane *L, Count *c)
{
    const uint32_t capm = L->d ? L->cap : 0u;                   /* (today cap is 0 whenever d is: the mask changes nothing) */
    uint32_t len = 0, nnext = NOLINK;
    if (L->d) {
        const uint32_t nx = L->d + (L->two ? l2 : l3)[L->p - L->d];
        c->steps_used++;
        if (!probe_differs(s, L)) c->step_pass++; else if (nx > L->reach) c->step_forced++; else c->step_ranout++;
        len = lcp(s, L->p, L->p - L->d, capm);
        const int32_t cand = (int32_t)((len << 12) - L->d);
        if (cand > L->key) L->key = cand;
        nnext = nx;
    } else if (L->cap) c->step_endonly++;
    const int ended = len == capm || nnext > L->reach;
    if (!ended) { L->d = nnext; return; }
    if (L->key == KEY_NONE3 && L->first2 <= L->reach) {        /* nothing on the 3-byte chain: the 2-byte chain */
        L->key = KEY_NONE2; L->cap = 2; L->two = 1; L->d = L->first2; L->first2 = NOLINK + 1; c->restarts++;
        return;
    }
    L->d = 0; L->cap = 0;
}

static void run(const Shape *sh, Count *c)
{
    memset(c, 0, sizeof *c);
    for (unsigned b = 0; b < nblocks; b++) {
        const uint8_t *s = blk + (size_t)b * N;
        build(s);
        static Lane W[4][64];
        memset(W, 0, sizeof W);
        for (uint32_t Pb = 0; Pb <= N; Pb += POOL) {                          /* (the last round searches an empty pool: the walks end) */
            const uint32_t pend = Pb < N ? Pb + POOL : N;
            uint32_t nextp = Pb;
            int left[4] = {0, 0, 0, 0}, pool_done[4] = {0, 0, 0, 0};
            if (Pb < N) c->wavepools += 4;
            while (!(left[0] && left[1] && left[2] && left[3])) for (int w = 0; w < 4; w++) {
                if (left[w]) continue;
                Lane *L = W[w];
                c->trips++;
                for (int sub = -1; sub < sh->nsub; sub++) {
                    /* the refill check: at the top of the loop, and (mid) between sub-steps from more idle lanes on */
                    if (sub == -1 || (sub > 0 && sh->mid > 0)) {
                        uint32_t nidle = 0; for (int l = 0; l < 64; l++) nidle += L[l].d == 0;
                        const int thr = sub > 0 ? sh->mid : ((int)(nextp - Pb) < sh->split ? sh->refill_lo : sh->refill_hi);
                        if (sub > 0) c->midchecks++;
                        if (!pool_done[w] && (int)nidle >= thr) {
                            const uint32_t basep = nextp; nextp += nidle; pool_done[w] = basep + nidle >= pend;
                            uint32_t r = 0; int any = 0, any_len1 = 0;
                            for (int l = 0; l < 64; l++) if (L[l].d == 0) { const uint32_t np = basep + r++; if (np < pend) { take(s, &L[l], np, &any_len1); any = 1; c->taken++; c->positions++; } }
                            c->passes++; c->empty += !any; c->len1 += any_len1;
                        }
                    }
                    if (sub == -1) {
                        if (pool_done[w]) {
                            int old = 0; for (int l = 0; l < 64; l++) old += L[l].d != 0 && L[l].p < Pb;
                            c->leave_tests++;
                            if (!old) { left[w] = 1; break; }
                        }
                        c->iters++;
                        for (int l = 0; l < 64; l++) c->busy += L[l].d != 0;
                        continue;
                    }
                    for (int h = 0; h < sh->hops[sub]; h++) { c->hop_slots += 64; for (int l = 0; l < 64; l++) hop(s, &L[l], sh, c); }
                    c->step_slots += 64;
                    for (int l = 0; l < 64; l++) step(s, &L[l], c);
                }
            }
        }
    }
}


/* vector instructions of SEARCH per wave and pool: the step loop, the refill passes, the loop's control */
static void price(const Shape *sh, const Count *c, double *loop, double *refill, double *control)
{
    double pass = 0;
    for (int i = 0; i < sh->nsub; i++) pass += sh->hops[i] * (sh->hop_end ? PRICE_HOP_END : PRICE_HOP) + (sh->hop_end ? PRICE_STEP_END : PRICE_STEP);
    *loop = c->iters * pass / c->wavepools;
    *refill = (c->passes * PRICE_PASS + (c->passes - c->empty) * PRICE_TAKE + c->len1 * PRICE_LEN1) / c->wavepools;
    *control = (c->trips * PRICE_TRIP + c->leave_tests * PRICE_LEAVE + c->midchecks * PRICE_MIDCHECK) / c->wavepools;
}
static double base_total;
static void row(const Shape *sh)
{
    Count c; run(sh, &c);
    double loop, refill, control; price(sh, &c, &loop, &refill, &control);
    const double total = loop + refill + control;
    if (base_total == 0) base_total = total;
    char shape[64] = ""; for (int i = 0; i < sh->nsub; i++) { for (int h = 0; h < sh->hops[i]; h++) strcat(shape, "H"); strcat(shape, i + 1 < sh->nsub ? "S+" : "S"); }
    char ref[32]; if (sh->split < POOL) snprintf(ref, sizeof ref, "%d/%d@%d", sh->refill_lo, sh->refill_hi, sh->split); else snprintf(ref, sizeof ref, "%d", sh->refill_lo);
    printf("  %-16s %-3s refill %-10s mid %-2d | iter %5.2f pass %5.2f (empty %4.2f) busy %4.1f | slots/pos S %4.2f H %4.2f used S %4.2f H %4.2f | loop %6.1f refill %6.1f ctl %5.1f = %6.1f  %+6.1f (%+5.2f %% of the kernel)\n",
           shape, sh->hop_end ? "end" : "-", ref, sh->mid, c.iters / c.wavepools, c.passes / c.wavepools, c.empty / c.wavepools, c.busy / c.iters,
           c.step_slots / c.positions, c.hop_slots / c.positions, c.steps_used / c.positions, c.hops_used / c.positions,
           loop, refill, control, total, total - base_total, 100.0 * (total - base_total) / LEDGER_TOTAL);
}

int main(int argc, char **argv)
{
    nblocks = argc > 1 ? atoi(argv[1]) : 256;
    const unsigned first = argc > 2 ? atoi(argv[2]) : 0, cls = argc > 3 ? atoi(argv[3]) : 0;
    blk = malloc((size_t)nblocks * N);
    lzs_workload_fill(blk, cls, 0x4C5A5331ull, first, nblocks, N, 8);
    printf("search_lane_sim: class %u, blocks %u..%u of 64 KiB, %d / %d buckets, pools of %d\n", cls, first, first + nblocks - 1, H3, H2, POOL);

    /* 1. the anchor: today's shape against the product kernel's own counters (profiles/r06/prof_counts_classes.txt, class 0, mean of the four roles) */
    const Shape today = { 2, {2, 2}, 0, 32, 32, POOL, 0 };
    Count c; run(&today, &c);
    const struct { const char *what; double model, measured; } anchor[] = {
        { "step iterations per wave and pool", c.iters / c.wavepools, 3.24 },
        { "refill passes per wave and pool", c.passes / c.wavepools, 3.55 },
        { "  of which take nothing", c.empty / c.wavepools, 0.76 },
        { "  of which compute the offset-1 length", c.len1 / c.wavepools, 0.80 },
        { "positions taken per wave and pool", c.taken / c.wavepools, 128.0 },
        { "busy lanes when a pass starts", c.busy / c.iters, 53.8 },
        { "candidates a position visits", (c.steps_used + c.hops_used) / c.positions, 4.2 },
        { "  whose probe passes: a full step is needed", c.step_pass / c.positions, 1.3 },
        { "  whose probe fails: a hop would do", (c.hops_used + c.step_forced + c.step_ranout) / c.positions, 2.9 },
        { "full-step slots a position is offered", c.step_slots / c.positions, 3.2 },
        { "hop slots a position is offered", c.hop_slots / c.positions, 6.5 },
    };
    printf("anchor (shape HHS+HHS, refill from 32 idle lanes):                 model   measured  deviation\n");
    for (unsigned i = 0; i < sizeof anchor / sizeof anchor[0]; i++)
        printf("  %-62s %7.3f  %7.3f  %+6.1f %%\n", anchor[i].what, anchor[i].model, anchor[i].measured, 100.0 * (anchor[i].model - anchor[i].measured) / anchor[i].measured);
    double loop, refill, control; price(&today, &c, &loop, &refill, &control);
    printf("  priced: step loop %.1f (ledger 385.6), refill passes %.1f (160.1), loop control %.1f (13.7) vector instructions per wave and pool\n", loop, refill, control);
    printf("full steps used, by what the candidate was (share of %.3f per position):\n", c.steps_used / c.positions);
    printf("  probe passes (the compare is needed)                        %5.1f %%\n", 100.0 * c.step_pass / c.steps_used);
    printf("  probe fails, last candidate in the window (FORCED ENDING)   %5.1f %%\n", 100.0 * c.step_forced / c.steps_used);
    printf("  probe fails, not the last (the hops in front ran out)       %5.1f %%\n", 100.0 * c.step_ranout / c.steps_used);
    printf("  per position: %.3f full steps and %.3f hops used; restarts on the 2-byte chain %.3f\n", c.steps_used / c.positions, c.hops_used / c.positions, c.restarts / c.positions);

    /* 2. the grid */
    printf("shapes (vector instructions of SEARCH per wave and pool; the difference to today's shape, also as a share of the kernel's %.0f):\n", LEDGER_TOTAL);
    row(&today);
    static const int grids[][5] = {   /* nsub, hops... */
        {1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {1, 5}, {1, 6},
        {2, 0, 0}, {2, 1, 1}, {2, 1, 2}, {2, 2, 1}, {2, 2, 3}, {2, 3, 2}, {2, 3, 3}, {2, 2, 4}, {2, 4, 2}, {2, 3, 4}, {2, 4, 4}, {2, 5, 5},
        {3, 1, 1, 1}, {3, 2, 2, 2}, {3, 3, 3, 3}, {3, 2, 3, 4},
    };
    for (int he = 0; he < 2; he++) {
        if (he) { Shape s = today; s.hop_end = 1; row(&s); }
        for (unsigned g = 0; g < sizeof grids / sizeof grids[0]; g++) {
            Shape s = { grids[g][0], {grids[g][1], grids[g][2], grids[g][3], 0}, he, 32, 32, POOL, 0 };
            row(&s);
        }
    }
    printf("refill threshold, by progress through the pool, and a refill check between sub-steps (today's shape and the grid's best two, both rules):\n");
    static const int bests[][5] = { {2, 2, 2}, {2, 3, 3}, {1, 4}, {2, 2, 3} };
    for (unsigned g = 0; g < sizeof bests / sizeof bests[0]; g++) for (int he = 0; he < 2; he++) {
        static const int thr[][3] = { {24, 24, POOL}, {40, 40, POOL}, {48, 48, POOL}, {24, 40, 256}, {40, 24, 256}, {32, 16, 384}, {32, 48, 384}, {48, 24, 384} };
        for (unsigned t = 0; t < sizeof thr / sizeof thr[0]; t++) { Shape s = { bests[g][0], {bests[g][1], bests[g][2], 0, 0}, he, thr[t][0], thr[t][1], thr[t][2], 0 }; row(&s); }
        if (bests[g][0] > 1) for (int mid = 40; mid <= 56; mid += 8) { Shape s = { bests[g][0], {bests[g][1], bests[g][2], 0, 0}, he, 32, 32, POOL, mid }; row(&s); }
    }
    return 0;
}
