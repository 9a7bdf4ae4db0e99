/* lzs_burst_plan.h -- the host arithmetic of the burst calls (lzs_channels_burst.hip, lzs_channels.c, lzs_packed.c; DESIGN.md 3.11,
 * 3.12, 3.16): where the parts of the work area lie, how large it is, and what a call decides before it launches.
 *
 * Plain C that also compiles as C++: no HIP, no globals, no getenv.  tests/cpu_shim/burst_plan_check.c holds every function here
 * to a table of literal rows (tests/test_burst_plan.py).  The three files ask these functions; none keeps a copy of a rule.
 */
#ifndef LZS_BURST_PLAN_H
#define LZS_BURST_PLAN_H

#include <stddef.h>
#include <stdint.h>

/* What lzs_channels_burst.hip holds equal to its kernels' constants, and lzs_channels.c to lzs_channels.h, with static_assert. */
#define LZS_BURST_SLOT_BYTES  2112u         /* kStateBytes, LZS_CHANNEL_STATE_BYTES: a channel slot */
#define LZS_BURST_ALIGN       256u          /* kAlign: every part of the work area begins at a multiple of it */
#define LZS_BURST_SORT_SPARE  65536u        /* kSortSpareBytes: rocPRIM's temporary storage is this + 8 bytes a packet (checked at every call) */
#define LZS_BURST_PACKETS_MAX 0x7FFFFFFFu   /* LZS_CHANNELS_MAX: packets, and channels, per call */
#define LZS_BURST_SPLIT_MIN_DEFAULT 8192u   /* DESIGN.md 3.12 has the sweep: the crossover of both routes on queues with one long run */

/* ---- the work area -------------------------------------------------------------------------------------------------------------
 * In this order, each part 256-byte aligned: npackets channel slots (compression), sort keys and values twice each (the sort's
 * double buffers), the lengths and their scan (64 bit), the runs' weights and positions twice each and their ends
 * (decompression), rocPRIM's temporary storage.
 * A split decode keeps its tables where compression has its slots -- the number of heavy runs, the light runs' weights and
 * positions, {length, open bytes} of every packet by sorted position: 16 bytes a packet -- and npackets * out_cap 16-bit origins,
 * packet by packet in sorted order, behind everything else (`total` is where): the larger work area's extra part.
 * A packed decode has the rooms by sorted position and their scan there as well (16 bytes a packet more), and its origins lie
 * room by room: as many as the caller's work area holds behind `total`.
 * The six tables end before the slots do -- 256 + 32 n bytes and five roundings against 2112 n -- which the table's rows hold
 * at every n they have.
 * A call with packet flags (history resets) has more runs than channels.  Its start marks lie in weight[0] until
 * they are scanned -- no direction has written it by then --, the run ids and the runs' records in the halves of key[] and val[]
 * the channel sort left unused (which halves is the sort's to say: burst_group).  Decompression stages the final slot
 * of every channel that has a second run behind its tables, `stage_slots` slots at `stage`: a second run needs a second packet,
 * so n / 2 slots do, and they end before the slots' region does (tests/cpu_shim/burst_flags_plan_check.c). */
typedef struct {
    size_t slots, key[2], val[2], lens, ends, weight[2], at[2], run_end, temp, temp_bytes, total;
    size_t light_w, light_at, rec, nheavy, rooms, room_ends, origins;
    size_t stage, stage_slots, stage_end, marks;
} lzs_burst_layout_t;

static inline size_t lzs_burst_up(size_t x) { return (x + LZS_BURST_ALIGN - 1u) / LZS_BURST_ALIGN * LZS_BURST_ALIGN; }
static inline size_t lzs_burst_take(size_t *o, size_t bytes) { const size_t at = *o; *o += lzs_burst_up(bytes); return at; }

static inline lzs_burst_layout_t lzs_burst_layout(size_t n)
{
    lzs_burst_layout_t L;
    size_t o = 0;
    int k;
    L.slots = lzs_burst_take(&o, n * LZS_BURST_SLOT_BYTES);
    for (k = 0; k < 2; k++) L.key[k] = lzs_burst_take(&o, 4u * n);
    for (k = 0; k < 2; k++) L.val[k] = lzs_burst_take(&o, 4u * n);
    L.lens = lzs_burst_take(&o, 8u * n);
    L.ends = lzs_burst_take(&o, 8u * n);
    for (k = 0; k < 2; k++) L.weight[k] = lzs_burst_take(&o, 4u * n);
    for (k = 0; k < 2; k++) L.at[k] = lzs_burst_take(&o, 4u * n);
    L.run_end = lzs_burst_take(&o, 4u * n);
    L.temp_bytes = lzs_burst_up(LZS_BURST_SORT_SPARE + 8u * n);
    L.temp = lzs_burst_take(&o, L.temp_bytes);
    L.total = o;
    o = L.slots;
    L.nheavy = lzs_burst_take(&o, 4u);
    L.light_w = lzs_burst_take(&o, 4u * n);
    L.light_at = lzs_burst_take(&o, 4u * n);
    L.rec = lzs_burst_take(&o, 8u * n);
    L.rooms = lzs_burst_take(&o, 8u * n);
    L.room_ends = lzs_burst_take(&o, 8u * n);
    L.origins = L.total;
    L.stage_slots = n / 2u;
    L.stage = lzs_burst_take(&o, L.stage_slots * LZS_BURST_SLOT_BYTES);
    L.stage_end = o;
    L.marks = L.weight[0];
    return L;
}

/* ---- the three sizes (lzs_channels_burst_work_bytes, lzs_channels_burst_split_work_bytes,
 * lzs_channels_burst_packed_split_work_bytes).  nchannels: today's layout does not depend on it. */
static inline size_t lzs_burst_plan_work_bytes(size_t npackets, size_t nchannels)
{
    (void)nchannels;
    return lzs_burst_layout(npackets > LZS_BURST_PACKETS_MAX ? (size_t)LZS_BURST_PACKETS_MAX : npackets).total;
}

/* The strided decoder's larger work area: the burst size and a 16-bit origin for every byte a packet may produce.  SIZE_MAX where
 * that does not fit a size_t: no work area is that large, so no call splits. */
static inline size_t lzs_burst_plan_split_work_bytes(size_t npackets, size_t nchannels, size_t out_cap)
{
    const size_t n = npackets > LZS_BURST_PACKETS_MAX ? (size_t)LZS_BURST_PACKETS_MAX : npackets;
    const size_t cap = out_cap > 0xFFFFFFFFu ? (size_t)0xFFFFFFFFu : out_cap;
    const size_t base = lzs_burst_plan_work_bytes(n, nchannels);
    if (cap != 0 && n > (SIZE_MAX - base) / 2u / cap) return SIZE_MAX;
    return base + 2u * n * cap;
}

/* The packed decoder's: the burst size and a 16-bit origin for every byte of room, out_bytes in all. */
static inline size_t lzs_burst_plan_packed_split_work_bytes(size_t npackets, size_t nchannels, uint64_t out_bytes)
{
    const size_t base = lzs_burst_plan_work_bytes(npackets, nchannels);
    if (out_bytes > (uint64_t)((SIZE_MAX - base) / 2u)) return SIZE_MAX;
    return base + 2u * (size_t)out_bytes;
}

/* ---- what a call decides on the host ---------------------------------------------------------------------------------------------
 * The channel sort: a stable radix sort over the bits a channel id in range, or nchannels for one out of range, can have. */
static inline unsigned lzs_burst_plan_sort_bits(uint32_t nchannels)
{
    unsigned bits = 1;
    while (bits < 32u && (nchannels >> bits) != 0u) bits++;
    return bits;
}

/* RESOLVE's grid, a workgroup per run there can be: a run per packet or per channel, and the ids out of range are one more. */
static inline uint32_t lzs_burst_plan_resolve_grid(uint32_t npackets, uint32_t nchannels)
{
    return npackets <= nchannels ? npackets : nchannels + 1u;
}

/* With packet flags a reset starts a run: as many runs as packets there can be.  Without them the grid above. */
static inline uint32_t lzs_burst_plan_resolve_grid_flags(uint32_t npackets, uint32_t nchannels, int flags)
{
    return flags ? npackets : lzs_burst_plan_resolve_grid(npackets, nchannels);
}

/* The staging slot of a channel whose last run is run `run` of the call (0-based, in sorted order) and not its first: two such
 * channels' last runs lie at least two runs apart and none is run 0, so (run - 1) / 2 is one slot each, below npackets / 2. */
static inline uint32_t lzs_burst_plan_stage_slot(uint32_t run) { return (run - 1u) / 2u; }

/* Whether the decoder splits its long runs (PARSE and RESOLVE), and over how many 16-bit origins behind the burst part of the
 * work area (packed: whether the rooms fit them is the device's to see, lzs_burst_split_plan_packed_kernel).  The compressor
 * ignores extra room.  Strided: the caller gave the split size, so the origins fit and nothing counts them. */
typedef struct { int split; uint64_t origin_cap; } lzs_burst_split_t;

static inline lzs_burst_split_t lzs_burst_plan_split_strided(int decompress, size_t work_bytes, size_t npackets, size_t nchannels, uint32_t out_cap)
{
    lzs_burst_split_t s = { 0, 0 };
    s.split = decompress && work_bytes >= lzs_burst_plan_split_work_bytes(npackets, nchannels, out_cap);
    return s;
}

/* origin_bytes: what the work area holds behind the burst size */
static inline lzs_burst_split_t lzs_burst_plan_split_packed(int decompress, size_t origin_bytes)
{
    lzs_burst_split_t s = { 0, 0 };
    if (decompress) s.origin_cap = origin_bytes / 2u;
    s.split = s.origin_cap != 0;
    return s;
}

/* Runs of at least this many compressed bytes are split: LZS_BURST_SPLIT_MIN where it is given (0: every run), else the default. */
static inline uint32_t lzs_burst_plan_split_min(int env_set, uint32_t env_value)
{
    return env_set ? env_value : LZS_BURST_SPLIT_MIN_DEFAULT;
}

#endif
