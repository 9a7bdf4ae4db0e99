// kernels/compress_wg.inc -- the default compress kernel (one 256-thread workgroup per block) and its segment / stitch / resume forms.
// Part of lzs_kernels.hip (included there, inside its anonymous namespace); not a translation unit of its own.

// ---------------------------------------------------------------------------------
// lzs_compress() per block, variant "wg" (the default): the same algorithm as "chain",
// but ONE 256-THREAD WORKGROUP PER BLOCK.  The four waves share a single set of LDS tables
// (ring, heads, links), which quadruples the waves a CU can hold for a given LDS budget,
// and every phase is lane-parallel over 256 threads, separated by workgroup barriers:
// Pools of 512 positions are pipelined: pool k is built and searched while pool k-1 is
// parsed and packed (walks of pool k still running are carried into the next round).
//   BUILD   HASH: buckets and "inserted at all" per position, dealt over the four waves;
//           CHAIN: wave 0 / wave 1 chain the 3-byte / 2-byte buckets by ordered exchange.
//           Positions inside a run of one byte value (same byte before, 13 equal bytes
//           ahead) are not inserted -- they can only ever win as offset 1, the seed of
//           every search;
//   SEARCH  the four waves pull positions from one shared counter; one branch-free step
//           per candidate for all 64 lanes;
//   EXTEND  a match that fills the search cap is measured on to <= 59 more bytes so that
//           its token is complete (only the first of each run of such positions compares
//           bytes); longer ones are left "open";
//   PARSE   the greedy chain of token starts (lzs-compression.c:301-447) by pointer
//           doubling inside 64-position chunks (in registers, for every possible entry),
//           a walk over the 8 chunk exits, and lane m taking the m-th token of its chunk;
//   PACK    tokens are encoded by their lanes, a workgroup prefix sum of the bit widths
//           places them, and complete 256-byte quarters of the bit ring go out as
//           coalesced stores.
//   OPEN    matches longer than that (long runs, zero fill, repeated records) are finished by
//           the whole workgroup straight from the source, 4080 bytes per step; of the positions
//           run over only the last offset + 12 go into the chains (the others are dominated by
//           the position one period on), and for two rounds the pools are small and parsed in
//           the round that searches them ("run mode").
// DESIGN.md section 3.1 has the LDS table, the measurements and what bounds the kernel.
// ---------------------------------------------------------------------------------
//   LZS_WGV_WG_WAVES                waves per workgroup: 4 (256 threads, pools of 512: the shape of rounds 1-6) or 8 (512 threads, pools of 1024,
//                                   an 8 KiB ring, link rings of 4096 -- a power of two: a slot is one AND --, a 16 384-bit output ring: ~44 KB
//                                   of LDS, THREE workgroups = 24 waves per CU where four-wave workgroups with the same tables are 20)
#ifdef LZS_WGV_WG_WAVES
constexpr uint32_t kW = LZS_WGV_WG_WAVES;
#else
constexpr uint32_t kW = 4;
#endif
static_assert(kW == 4 || kW == 8, "four or eight waves per workgroup");
constexpr uint32_t kWgThreads  = 64u * kW;
constexpr uint32_t kChunkStride = 64u * kW;       // pool-relative distance between a wave's two chunks: chunk k = kW * h + wave starts at 64 k
constexpr uint32_t kWgRing      = kW == 8 ? 8192u : 4096u;   // bytes of input window: 2047 + two pools + look-ahead + one refill
constexpr uint32_t kWgRingMask  = kWgRing - 1u, kWgRingWords = kWgRing / 4u;
constexpr uint32_t kRefillUnit  = 128u * kW;      // bytes a REFILL stores at a time (16 per lane of one wave's first 32 / 64 lanes)
// 3-byte buckets: what the LDS left over at five workgroups per CU holds (round 2: 1320 = 31 988 B per workgroup; 1384 =
// 32 244 B no longer fits five and costs 12 %).  Round 4 keeps SEARCH's result per position in 16 bits and the HASH record
// in the link rings, which frees 2 KiB: measured on text 1536 / 1664 / 1728 / 1760 / 1792 / 1808 / 1824 / 1832 buckets
// = 69.6 / 69.8 / 70.3 / 70.2 / 71.1 / 69.9 / 69.9 / 70.2 GB/s (1320: 70.1; not monotonic: which grams of a text share a
// bucket is luck, and 7 x 256 is the count that was kept).  Not a power of two: the hash is scaled into the range.
// THE CONFIGURATION OF THIS INCLUSION.  lzs_kernels.hip includes this file once per variant of the kernel, each inside a
// namespace of its own, with LZS_WGV_* saying what differs (round 5: a block gets the variant its class wants, chosen on the
// device -- see lzs_classify_blocks_kernel in compress_aux.inc -- and the text kernel carries no code it never runs):
//   LZS_WGV_HEAD3 / LZS_WGV_HEAD2   bucket counts (default 1792 / 1024: rounds 2-5's, still wgv_safe's; the default variant since round 6: 1152 / 512 with
//                                   multipliers of its own and six workgroups per CU; the two class variants: no 3-byte table, 1024)
//   LZS_WGV_SUBSTEPS                full steps per pass of the SEARCH loop (default 2; high-entropy blocks: 1)
//   LZS_WGV_HOPS                    quick-reject hops in front of a full step (default LZS_HOPS = 2; high-entropy blocks: 1 -- their
//                                   candidates are hash collisions, and with twice the buckets one is passed over for a quarter of a
//                                   step; low-entropy blocks: 0 -- few candidates, long matches, the test itself is the cost: +5 %)
//   LZS_WGV_CHAIN_SAFE              CHAIN in its order-independent form (a device that fails the LDS ordering check)
//   LZS_WGV_PACK_BY_CHUNK           PACK formats a wave's two chunks one after the other (default: in one pass when their
//                                   tokens are no more than 64 together)
//   LZS_WGV_SEGMENTS                the variant also serves lzs_compress_segments_kernel
//   LZS_WGV_CHANNELS                the inclusion serves lzs_compress_channels_wg_kernel alone: the job reads a two-source view,
//                                   [a channel's history | the packet] (wg_view_* below), and nothing else is compiled in it
//   LZS_WGV_LEAN                    constants of SEARCH as literals (2.5 cycles an instruction) instead of registers (2): the
//                                   variant that runs six workgroups per CU has 80 vector registers and not one more
//   LZS_WGV_PRIO                    wave priorities by phase (s_setprio): SEARCH 0, CHAIN's two waves 3, the other phases 2
// (-DLZS_WG_HEAD3= / -DLZS_WG_HEAD2= / -DLZS_SUBSTEPS= on the command line change the defaults: tools/probes/ab.sh)
#ifndef LZS_WG_HEAD3
#define LZS_WG_HEAD3 1792
#endif
#ifndef LZS_WG_HEAD2
#define LZS_WG_HEAD2 1024
#endif
#ifdef LZS_WGV_HEAD3
constexpr uint32_t kWgHead3    = LZS_WGV_HEAD3;
#else
constexpr uint32_t kWgHead3    = LZS_WG_HEAD3;
#endif
#ifdef LZS_WGV_HEAD2
constexpr uint32_t kWgHead2    = LZS_WGV_HEAD2;      // a power of two <= 4096
#else
constexpr uint32_t kWgHead2    = LZS_WG_HEAD2;
#endif
//   LZS_WGV_NO3                     no 3-byte chain at all (round 6, the variant of blocks that are nearly all literals): every position walks
//                                   the 2-byte chain with the full rule -- that chain is complete for every match of 2 and more, the 3-byte chain
//                                   is only the shorter list for matches of 3 and more, and where grams do not repeat it holds nothing but
//                                   collisions -- so there are no head3[] / link3[], HASH and CHAIN do half the work, a step has no restart on
//                                   another chain, and the LDS they took buys 2-byte buckets (fewer collisions to step over) or a workgroup more
#ifdef LZS_WGV_NO3
constexpr bool kNo3 = true;
#else
constexpr bool kNo3 = false;
#endif
//   LZS_WGV_EXIT8                   PARSE's exit functions as one byte a position (round 6: 512 B of LDS less -- 128 three-byte buckets for the
//                                   default variant at six workgroups per CU, +0.6 %; the scalar walk over the exits decodes them, which costs
//                                   the nearly-all-literals variant 1.9 % and gives it nothing: profiles/r06/ab_s49)
#ifdef LZS_WGV_EXIT8
constexpr bool kExit8 = true;
typedef uint8_t exit_t;
#else
constexpr bool kExit8 = false;
typedef uint16_t exit_t;
#endif
#ifdef LZS_WGV_CHAIN_SAFE
constexpr bool kChainSafe = true;
#else
constexpr bool kChainSafe = false;
#endif
constexpr uint32_t kWgHead2Shift = kWgHead2 == 4096 ? 4 : kWgHead2 == 2048 ? 5 : kWgHead2 == 1024 ? 6 : kWgHead2 == 512 ? 7 : 8;   // bits 15.. of the product down
//   LZS_WGV_POOL                    positions per pool: 512 (two chunks of 64 per wave), or 256 (one; round 6's occupancy experiment:
//                                   link rings of 2560, results and exits halved -- 3.5 KiB of LDS -- for twice the rounds per byte)
#ifdef LZS_WGV_POOL
constexpr uint32_t kWgPool     = LZS_WGV_POOL;
#else
constexpr uint32_t kWgPool     = 128u * kW;
#endif
static_assert(kWgPool == 128u * kW || (kW == 4 && kWgPool == 256), "a wave parses one or two chunks of 64 positions");
constexpr int      kCh         = (int)(kWgPool / kChunkStride);   // chunks per wave
constexpr uint32_t kWgLinkN    = (2047u + 2u * kWgPool + 63u) / 64u * 64u;   // 48 x 64 = 3072 >= 2047 + 2 * 512: the pool in SEARCH and the one before
constexpr uint32_t kWgResN     = 2 * kWgPool;     // results of two consecutive pools, by position & (kWgResN - 1)
constexpr uint32_t kWgBitWords = 64u * kW;        // 8192-bit ring (16 384 with eight waves: a pool of 1024 literals is 9216 bits), quarters of 2048 bits
constexpr uint32_t kBitMask    = 32u * kWgBitWords - 1u;
constexpr uint32_t kOpen       = 0xFFFFu;         // jump code of an open match (no exit position: those end below the pool's size + 67)
constexpr uint32_t kExtOpen    = 63;              // extension code of an open match
#ifndef LZS_SUBSTEPS
#define LZS_SUBSTEPS 2               // full steps per pass of the SEARCH loop
#endif
#ifdef LZS_WGV_SUBSTEPS
constexpr int kSubsteps = LZS_WGV_SUBSTEPS;
#else
constexpr int kSubsteps = LZS_SUBSTEPS;
#endif
#ifndef LZS_HOPS
#define LZS_HOPS 2                   // quick-reject hops in front of every full step (0: none, round 1's kernel)
#endif
#ifdef LZS_WGV_HOPS                  // (a variant's own count)
#define LZS_HOPS_HERE LZS_WGV_HOPS
#else
#define LZS_HOPS_HERE LZS_HOPS
#endif
constexpr int kHops = LZS_HOPS_HERE;
//   LZS_WGV_HOP_END                 the block and packed entries' SEARCH lets a hop pass over the LAST candidate inside the window too
//                                   (wg_search<true>: the rule and why it is exact stand at the hop), and runs LZS_WGV_HOPS_LAST hops
//                                   (default: as many as the others) in front of the last full step of a pass.  The default variant
//                                   alone: 2 + 3 hops, +2 % on text (profiles/r07/README.md).  The segments entry keeps the plain rule
#ifdef LZS_WGV_HOP_END
constexpr bool kHopEnd = true;
#else
constexpr bool kHopEnd = false;
#endif
#ifdef LZS_WGV_HOPS_LAST
constexpr int kHopsLast = LZS_WGV_HOPS_LAST;
#else
constexpr int kHopsLast = kHops;
#endif
constexpr uint32_t kExtMax     = 59;              // longest extension resolved in SEARCH
constexpr uint32_t kOpenStep   = 4080;            // bytes of an open match per step: 255 threads x 16 = 272 nibbles of 15
#ifndef LZS_RUN_ROUNDS
#define LZS_RUN_ROUNDS 2             // rounds in "run mode" (small pools, parsed at once) after an open match
#endif
#ifndef LZS_RUN_POOL
#define LZS_RUN_POOL 128             // positions per pool in run mode
#endif
constexpr uint32_t kRunRounds  = LZS_RUN_ROUNDS;
constexpr uint32_t kRunPool    = LZS_RUN_POOL;

// (ring first: at LDS offset 0 the two-word reads of the ring need no base added to their addresses)
struct __attribute__((aligned(16))) BlkLds {
    uint32_t ring[kWgRingWords + 4];                // +16 B mirror of ring[0..15]
    uint32_t head3[kNo3 ? 1 : kWgHead3];
    uint32_t head2[kWgHead2];
    uint16_t link3[kNo3 ? 2 : kWgLinkN];          // (before CHAIN has been there: the LDS address HASH wants exchanged, see wg_hash_range)
    uint16_t link2[kWgLinkN];
    uint16_t res[kWgResN];                        // the running best match of SEARCH as (len << 12) - offset: 16 bits (round 4; the
                                                  // 2 KiB a 32-bit word per position took are 472 more 3-byte buckets)
    exit_t   exitfn[kExit8 && kWgPool < 2u * kWgThreads ? 2u * kWgThreads : kWgPool];   // per entry position: where the chain leaves its chunk -- 16 bits: the
                                                  // pool-relative position it goes to next, or 0x8000 | the position of an open match; LZS_WGV_EXIT8: ONE BYTE
                                                  // relative to the chunk's start (0 .. 130 the position it goes to next -- a token is 67 bytes at most --,
                                                  // 192 + i an open match at position i of the chunk).  Outside PARSE a 16-bit dummy target per thread
    uint32_t bits[kWgBitWords];                   // output bit ring
    uint32_t chunk_bits[2 * kW];
    uint32_t nextp;                               // SEARCH work counter
    uint32_t bcast[8];
#ifdef LZS_PAD_LDS
    uint32_t pad[LZS_PAD_LDS / 4];                // occupancy experiments only
#endif
};

// Bucket of the 3 bytes in the low 24 bits of t, times 4 (the byte offset of its head inside head3[]): one 24-bit
// multiply (which ignores the fourth byte) mixes, one high multiply scales into the table.
// The buckets' multipliers (round 6).  Which grams of a text share a bucket decides how many candidates a walk steps over, and on
// ASCII text the multipliers of rounds 1-5 (0x9E3779, 40503) were poor ones: tools/sim/hash_sim.c counts the candidates a walk
// visits by multiplier, on the seeded text and on real text from the build container (licences, source, prose), and the ones kept
// here are the best of 8000 for their table sizes on both.  LZS_WGV_HASH3_MUL / LZS_WGV_HASH2_MUL: a variant's own (the defaults:
// for 1792 / 1024 buckets); -DLZS_HASH3_MUL= / -DLZS_HASH2_MUL= on the command line change the defaults (tools/probes/ab.sh).
#ifndef LZS_HASH3_MUL
#define LZS_HASH3_MUL 0x1EB419u
#endif
#ifndef LZS_HASH2_MUL
#define LZS_HASH2_MUL 0xCFC8AE9Bu
#endif
#ifdef LZS_WGV_HASH3_MUL
constexpr uint32_t kHash3Mul = LZS_WGV_HASH3_MUL;
#else
constexpr uint32_t kHash3Mul = LZS_HASH3_MUL;
#endif
#ifdef LZS_WGV_HASH2_MUL
constexpr uint32_t kHash2Mul = LZS_WGV_HASH2_MUL;
#else
constexpr uint32_t kHash2Mul = LZS_HASH2_MUL;
#endif
__device__ __forceinline__ uint32_t wg_hash3x4(uint32_t t) { return __umulhi(__umul24(t, kHash3Mul), 4u * kWgHead3) & ~3u; }

__device__ __forceinline__ uint32_t wg_slot_base(uint32_t B) { return ((B >> 6) % (kWgLinkN / 64u)) * 64u; }
// Slot `at` of a link ring for at in (-kWgLinkN, kWgLinkN): what is negative wraps around to something huge, and the smaller
// of at and at + kWgLinkN is the slot.  In 16-bit arithmetic: gfx950 issues v_min_u32 (like every compare, select and left
// shift) at half the rate of an add -- profiles/r05/valu_rates.txt -- and v_min_u16 at the full rate.
__device__ __forceinline__ uint32_t wg_link_slot(uint32_t at)
{
    if constexpr ((kWgLinkN & (kWgLinkN - 1u)) == 0u) return at & (kWgLinkN - 1u);      // (eight waves: 4096 slots, one AND)
    // (as assembly: from a < b ? a : b on 16-bit values the compiler makes a compare, a select and a mask; the 16-bit
    // instructions of gfx9 write zeros to the upper half of their destination)
    uint32_t b, r;
#ifdef LZS_WGV_LEAN          // (no register for the constant: see the configuration at the top)
    asm("v_add_u16 %0, %2, %1" : "=v"(b) : "v"(at), "n"(kWgLinkN));
#else
    asm("v_add_u16 %0, %1, %2" : "=v"(b) : "v"(at), "v"(kWgLinkN));
#endif
    asm("v_min_u16 %0, %1, %2" : "=v"(r) : "v"(at), "v"(b));
    return r;
}

// Equal leading bytes of two 12-byte strings given the XOR of their little-endian words;
// 12 or more (a large number) when all are equal -- callers clamp to their own limit.
__device__ __forceinline__ uint32_t lcp12(uint32_t x0, uint32_t x1, uint32_t x2)
{
    // v_ffbl_b32 gives -1 for 0, which survives the OR: the first set bit of x2:x1:x0, or huge
    uint32_t f0, f1, f2;
    asm("v_ffbl_b32 %0, %1" : "=v"(f0) : "v"(x0));
    asm("v_ffbl_b32 %0, %1" : "=v"(f1) : "v"(x1));
    asm("v_ffbl_b32 %0, %1" : "=v"(f2) : "v"(x2));
    const uint32_t a = f1 | 32u, b = f2 | 64u;
    const uint32_t m = f0 < a ? (f0 < b ? f0 : b) : (a < b ? a : b);   // v_min3_u32
    return m >> 3;                                                      // all equal -> huge
}

// OR `width` (1..32) bits of `value`, MSB first, at bit offset `at` of a ring of `words` words.
__device__ __forceinline__ void bits_or(uint32_t *ring, uint32_t words, uint32_t at, uint32_t value, uint32_t width)
{
    const uint32_t sh = at & 31u, d = (at >> 5) & (words - 1);
    const uint64_t v = (uint64_t)value << (64u - sh - width);
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    __hip_atomic_fetch_or(&ring[d], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (lo) __hip_atomic_fetch_or(&ring[(d + 1) & (words - 1)], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Output state: wave-uniform and identical in all four waves.
struct WgOut {
    uint32_t flushed;    // bytes handed to HBM (multiple of 256)
    uint32_t head;       // bits appended past `flushed`
    uint8_t *dst;
    uint32_t cap;
    bool     aligned4;
    // Segments of one long stream only: `cap` above stays unlimited (the bits are counted to the
    // end whatever happens), stores stop at `limit` (the slot), or -- `ored` -- go to zeroed memory
    // shared with the neighbouring segments by atomic OR.  A block: limit = cap.
    uint32_t limit;
    bool     ored;
};

__device__ __forceinline__ uint32_t wg_bit_at(const WgOut &o) { return ((o.flushed << 3) + o.head) & kBitMask; }

// Store one complete quarter (2048 bits) of the ring from the calling wave and clear it.
// (BOUNDED_OR: the ORed stores stop at `limit` too -- the segments of a batch, whose neighbour in memory is another block's output;
// a parameter of the instance, so that the entries that had an instance keep their instructions)
template <bool BOUNDED_OR = false>
__device__ __forceinline__ void wg_store_quarter(const WgOut &o, BlkLds &L, uint32_t lane)
{
    const uint32_t slot = ((o.flushed >> 8) & (kWgBitWords / 64u - 1u)) * 64u + lane;
    const uint32_t v = __builtin_bswap32(L.bits[slot]);
    L.bits[slot] = 0;
    const uint32_t at = o.flushed + 4 * lane;
    if (o.ored) {                                             // o.dst is 4-aligned in this mode
        if (v && (!BOUNDED_OR || at + 4u <= o.limit)) atomicOr(reinterpret_cast<unsigned int *>(o.dst + at), v);
        return;
    }
    if (o.aligned4 && at + 4 <= o.limit) {
        *reinterpret_cast<uint32_t *>(o.dst + at) = v;
    } else {
        for (uint32_t k = 0; k < 4; k++)
            if (at + k < o.limit) o.dst[at + k] = (uint8_t)(v >> (8 * k));
    }
}

// Where an idle lane's (16-bit) stores go: a half-word of its own in exitfn[], which is only live inside PARSE.
// (halves of shared words: measured no slower than a word each -- profiles/r06/ab_s10 -- and pools of 256 have only these 512 bytes)
__device__ __forceinline__ uint16_t *wg_dummy(BlkLds &L) { return reinterpret_cast<uint16_t *>(L.exitfn) + threadIdx.x; }

// The ring's helpers with THIS inclusion's ring size (common.inc's are for the 4 KiB ring).
__device__ __forceinline__ uint32_t wg_ring_byte(const uint32_t *ring, uint32_t q) { return reinterpret_cast<const uint8_t *>(ring)[q & kWgRingMask]; }
__device__ __forceinline__ void wg_read12(const uint32_t *ring, uint32_t q, uint32_t &w0, uint32_t &w1, uint32_t &w2)
{
    const uint32_t a = (q & kWgRingMask) >> 2;   // words a..a+3 exist thanks to the mirror
    const uint32_t d0 = ring[a], d1 = ring[a + 1], d2 = ring[a + 2], d3 = ring[a + 3];
    w0 = __builtin_amdgcn_alignbyte(d1, d0, q);
    w1 = __builtin_amdgcn_alignbyte(d2, d1, q);
    w2 = __builtin_amdgcn_alignbyte(d3, d2, q);
}

// LDS byte offsets as plain integers: HASH leaves CHAIN the ADDRESS of the word to exchange with.
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) uint16_t lds_u16_t;
__device__ __forceinline__ uint32_t lds_off(const void *p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p; }
__device__ __forceinline__ lds_u32_t *lds_word(uint32_t off) { return (lds_u32_t *)(uintptr_t)off; }
__device__ __forceinline__ lds_u16_t *lds_half(uint32_t off) { return (lds_u16_t *)(uintptr_t)off; }

// BUILD in two phases, so that the arithmetic is done once per position instead of once per wave.
// HASH: the batches of [B0, Be) are dealt to the four waves; a wave computes, for each position
// of its batches, the LDS address of the word CHAIN will exchange with in each of the two bucket
// tables -- the head of the position's bucket, or, for a position that is not inserted, a dummy
// word of the lane's own -- and leaves both as two 16-bit halves of a record in the result slot of
// that position (free until SEARCH).
// Not inserted: the interior of a run of one byte value.  The test (round 4) is on the five
// aligned words around the position -- [(p - 4) & ~3, + 20) all one byte value, which covers
// p - 1 .. p + 12 wherever p sits in its word: the same byte before and 13 equal bytes ahead --
// so a lane needs nothing from its neighbours (rounds 1-3 read the run off ballots of three
// neighbouring batches: 113 vector instructions per pool and wave, now 46) and skips a few
// positions less at either end of a run, which costs nothing: inserting MORE positions never
// changes a search result.  Bytes past the end of the input (stale ring content) and before its
// start may take part in the test: a position they let through is still dominated (its real bytes
// up to the end are one value, so is everything a later position could compare), and nothing is
// searched from there.  For the same reason the last two positions need no "gram within the input"
// test: nothing is searched after them that could walk into them with a cap above 1.
// CHAIN (after a barrier): wave 0 keeps the 3-byte chain and wave 1 the 2-byte chain, so every
// bucket is chained by one wave's in-order instruction stream; waves 2 and 3 wait (the kernel is
// bound by VALU issue, and chaining four ways only repeated the record decoding).  No
// exec-masked regions and no branches inside the loops.
__device__ __forceinline__ void wg_hash_range(BlkLds &L, uint32_t B0, uint32_t Be, uint32_t lane, uint32_t wave)
{
    const uint32_t head3_at = lds_off(L.head3), head2_at = lds_off(L.head2);
    // a non-inserting lane of a CHAIN wave exchanges with word `lane` (3-byte chain) / 64 + lane (2-byte chain) of exitfn[]
    const uint32_t dummy3 = lds_off(L.exitfn) + 4u * lane, dummy2 = dummy3 + 256u;
    // two batches of the wave side by side (straight-line code: their LDS reads overlap); one
    // that lies past Be is computed all the same and stored to the dummy word
    for (uint32_t B = B0 + 64u * wave; B < Be; B += kChunkStride * kCh) {
        uint32_t e[kCh][5];
#pragma unroll
        for (int j = 0; j < kCh; j++) {
            const uint32_t p = B + kChunkStride * j + lane;
            const uint32_t a = ((p - 4u) & kWgRingMask) >> 2;            // words a .. a + 4 exist thanks to the mirror
#pragma unroll
            for (int k = 0; k < 5; k++) e[j][k] = L.ring[a + k];
        }
#pragma unroll
        for (int j = 0; j < kCh; j++) {
            const uint32_t Bj = B + kChunkStride * j, p = Bj + lane;
            const uint32_t tcur = __builtin_amdgcn_alignbyte(e[j][2], e[j][1], p);     // bytes p .. p + 3
            // Interior of a run: dominated by p + 1 as a candidate for every later position, and its
            // own search ends at offset 1 (full cap), so it is neither inserted nor does it need a
            // link (DESIGN.md 3.1).
            const uint32_t rot = __builtin_amdgcn_alignbit(e[j][0], e[j][0], 8);
            const uint32_t x = (e[j][0] ^ rot) | (e[j][1] ^ e[j][0]) | (e[j][2] ^ e[j][0]) | (e[j][3] ^ e[j][0]) | (e[j][4] ^ e[j][0]);
            const bool skip = x == 0u;
            // (bits 6.. of the product depend on the two low bytes alone)
            const uint32_t g2 = head2_at + (((tcur * kHash2Mul) >> (kWgHead2Shift - 2u)) & (4u * (kWgHead2 - 1)));
            const uint32_t a2 = skip ? dummy2 : g2;
            // (the two addresses wait for CHAIN where its links will go: the position's slot in either link ring)
            const uint32_t sl = wg_slot_base(Bj) + lane;
            uint16_t *const dummy16 = wg_dummy(L);
            if constexpr (!kNo3) {
                const uint32_t g3 = opaque(head3_at + wg_hash3x4(tcur));  // (opaque: selects, not an exec-masked region)
                const uint32_t a3 = skip ? dummy3 : g3;
                *(Bj < Be ? &L.link3[sl] : dummy16) = (uint16_t)a3;
            }
            *(Bj < Be ? &L.link2[sl] : dummy16) = (uint16_t)a2;
        }
    }
}

// CHAIN for `K` consecutive batches from B: all reads, then all exchanges, then all links, so the
// LDS latencies are paid once per group.  `half`: which 16 bits of the HASH record hold this
// chain's address (0: the 3-byte chain, 2: the 2-byte chain).  A lane that does not insert
// exchanges with its dummy word and gets a meaningless link: a position that is not inserted is
// never a candidate, and its own search never walks (it ends at offset 1 with the full cap).
template <int K>
__device__ __forceinline__ void wg_chain_group(BlkLds &L, uint32_t B, uint32_t &slot, uint32_t lane, uint32_t half, uint16_t *links)
{
    (void)half;
    uint32_t at[K], old[K];
    uint16_t *la[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        la[j] = &links[slot + lane];
        at[j] = *la[j];                                        // HASH left the address to exchange with here
        slot = slot + 64u >= kWgLinkN ? slot + 64u - kWgLinkN : slot + 64u;
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const uint32_t p = B + 64u * j + lane;
        old[j] = __hip_atomic_exchange(lds_word(at[j]), p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
        const uint32_t p = B + 64u * j + lane;
        const uint32_t d = p - old[j] < kNoLink ? p - old[j] : kNoLink;
        *la[j] = (uint16_t)d;
    }
}

// CHAIN without the ordering property (DESIGN.md 3.1): which lanes of the batch share a bucket is
// worked out with ballots over the bits of the bucket's address, a lane's predecessor is the
// nearest lower lane of its group (positions of a batch are consecutive, so its distance is the
// lane distance) or else the bucket's old head, and only the highest lane of a group stores the
// new head -- one writer per address, nothing depends on the order in which the LDS applies the
// lanes of an instruction.  ~7x the instructions of the exchange form; used when the device fails
// lzs_lds_order_check_kernel (or LZS_CHAIN_FALLBACK=1 asks for it).
__device__ __forceinline__ void wg_chain_batch_safe(BlkLds &L, uint32_t B, uint32_t &slot, uint32_t lane, uint32_t half, uint16_t *links)
{
    (void)half;
    const uint32_t at = links[slot + lane];
    const uint32_t p = B + lane;
    const bool ins = at - lds_off(L.exitfn) >= (uint32_t)sizeof(L.exitfn);   // a bucket head, not one of the dummy words (which are exitfn[]'s)
    uint64_t same = __builtin_amdgcn_ballot_w64(ins);          // lanes that insert, narrowed to my bucket
#pragma unroll
    for (uint32_t bit = 2; bit < 15u; bit++) {                 // word addresses below 32 KiB
        const bool set = (at >> bit) & 1u;
        const uint64_t bb = __builtin_amdgcn_ballot_w64(set);
        same &= set ? bb : ~bb;
    }
    const uint64_t lower = same & ((1ull << lane) - 1ull);
    const bool top = (same >> lane >> 1) == 0ull;              // no higher lane with my bucket
    const uint32_t old = ins ? *lds_word(at) : ~0u;
    __builtin_amdgcn_wave_barrier();                           // every head is read before any is replaced
    uint32_t d = kNoLink;
    if (ins) {
        if (lower) d = lane - (63u - (uint32_t)__builtin_clzll(lower));
        else       d = p - old < kNoLink ? p - old : kNoLink;
        if (top) *lds_word(at) = p;
    }
    links[slot + lane] = (uint16_t)d;
    slot = slot + 64u >= kWgLinkN ? slot + 64u - kWgLinkN : slot + 64u;
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void wg_chain_range(BlkLds &L, uint32_t B0, uint32_t Be, uint32_t lane, uint32_t wave)
{
    if (wave >= 2u) return;                                    // waves 2 and 3 only wait: the kernel is VALU-bound
    if (kNo3 && wave == 0u) return;                            // (no 3-byte chain to keep)
    const bool two = wave == 1u;                               // uniform
    uint16_t *const links = two ? L.link2 : L.link3;
    const uint32_t half = two ? 2u : 0u;
    uint32_t slot = wg_slot_base(B0);
    uint32_t B = B0;
    // (a variant of its own, lzs_kernels.hip: the order-independent form inside the default kernel cost it 39 of its 50
    // scalar-register spills and 2 % of its time on text -- profiles/r05/ab_s1.txt -- for code no device has needed so far)
    if constexpr (kChainSafe) {
        for (; B < Be; B += 64u) wg_chain_batch_safe(L, B, slot, lane, half, links);
        return;
    }
#ifdef LZS_WGV_PRIO
    __builtin_amdgcn_s_setprio(3);                             // the few waves every other wave of the workgroup waits for
#endif
    for (; B + 256u <= Be; B += 256u) wg_chain_group<4>(L, B, slot, lane, half, links);
    for (; B < Be; B += 64u) wg_chain_group<1>(L, B, slot, lane, half, links);
#ifdef LZS_WGV_PRIO
    __builtin_amdgcn_s_setprio(2);
#endif
}

// EXTEND: a match that fills the search cap (12) may run on, and its token is only complete with
// the whole length (:417-431).  SEARCH leaves bits 15.. of such results empty; this pass fills them
// for the pool about to be parsed, for both chunks of the calling wave.  Consecutive positions
// inside one long match all report 12 at the same offset, and their totals differ by one per
// position, so only the first of each such run (per 64-position chunk) compares bytes -- up to
// kTokenMax + kExtMax + 1 of them -- and the others derive theirs.  Beyond that the match is
// "open" (finished serially in PARSE), and so is everything derived from an open one.
// (the profiling build hands its counters to the phases that are functions of their own)
#ifdef LZS_PROFILE
#ifdef LZS_PROFILE_COUNTS
#define SEARCH_PROF_PARAMS , uint32_t *prof_acc
#else
#define SEARCH_PROF_PARAMS , unsigned long long *prof_acc
#endif
#define SEARCH_PROF_ARGS , prof_acc
#else
#define SEARCH_PROF_PARAMS
#define SEARCH_PROF_ARGS
#endif
__device__ __forceinline__ void wg_extend(BlkLds &L, uint32_t Pb, uint32_t entry, uint32_t npos, uint32_t n, uint32_t lane, uint32_t wave,
                                          uint32_t (&rr)[2] SEARCH_PROF_PARAMS)
{
    PROF_ITER_DECL;
    constexpr uint32_t kRoom = kTokenMax + kExtMax + 1;
#pragma unroll
    for (int h = 0; h < kCh; h++) {
        const uint32_t gi = kChunkStride * h + 64u * wave + lane;
        rr[h] = 0;
        if (64u * wave + kChunkStride * h >= npos) continue;           // chunk past the end of the pool (uniform)
        const uint32_t p = Pb + gi;
        // SEARCH stored (len << 12) - offset; offset 0 = no match
        const uint32_t k = L.res[p & (kWgResN - 1)];
        const uint32_t off = (0u - k) & 0xFFFu;
        const uint32_t len = off ? (k + 0xFFFu) >> 12 : 0u;
        const uint32_t r = off | (len << 11);
        // positions before the entry were not searched: what is stored there is stale
        const bool need = gi >= entry && gi < npos && len == kSearchCap && n - p > kSearchCap;
#ifdef LZS_ABLATE_EXTEND     // counter experiments only: no match is measured past the search cap
        const uint64_t needs = 0ull;
#else
        const uint64_t needs = __builtin_amdgcn_ballot_w64(need);
#endif
        if (needs == 0ull) {
            rr[h] = r | ((len > kTokenMax ? len - kTokenMax : 0u) << 15);
            continue;
        }
        PROF_COUNT(19, 1);
        const uint32_t left = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane - 1u) << 2), (int)r);
        // the run goes on if the position before is complete the same way: 12 at the same offset
        const bool head = need && !(lane > 0u && ((needs >> (lane - 1u)) & 1ull) != 0ull && ((left ^ r) & 0x7FFFu) == 0u);
        // A run of k + 1 such lanes from its head on is k + 12 bytes of match already (lane j of it
        // vouches for bytes j .. j + 11): the head starts comparing there, and a run that fills the
        // rest of a chunk (long runs, zero fill) is open without a single compare.
        const uint64_t heads_all = __builtin_amdgcn_ballot_w64(head);
        const uint64_t ends = (heads_all | ~needs) >> lane >> 1;             // first lane above mine that is not of my run
        const uint32_t runlen = ends ? (uint32_t)__builtin_ctzll(ends) : 63u - lane;
        uint32_t total = kSearchCap;
        if (head) {
            const uint32_t room = n - p < kRoom ? n - p : kRoom;
            total = kSearchCap + runlen < room ? kSearchCap + runlen : room;
            while (total < room) {
                PROF_ITER;
                uint32_t a0, a1, a2, b0, b1, b2;
                wg_read12(L.ring, p + total, a0, a1, a2);
                wg_read12(L.ring, p + total - off, b0, b1, b2);
                uint32_t e = lcp12(a0 ^ b0, a1 ^ b1, a2 ^ b2);
                e = e < 12u ? e : 12u;
                e = e < room - total ? e : room - total;
                total += e;
                if (e < 12u) break;
            }
        }
        PROF_ITER_DONE(27);
        const uint64_t heads = heads_all & ((2ull << lane) - 1ull);
        const uint32_t hp = heads ? 63u - (uint32_t)__builtin_clzll(heads) : lane;   // head of my run
        const uint32_t th = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(hp << 2), (int)total);
        uint32_t ext = len >= kTokenMax ? len - kTokenMax : 0u;
        if (need) ext = th >= kRoom ? kExtOpen : th - (lane - hp) - kTokenMax;
        rr[h] = r | (ext << 15);
    }
}

// One lane's SEARCH state.  It lives in registers across pools: a walk that is still going when
// its wave runs out of fresh positions is carried into the SEARCH of the next pool.
//
// The step is written for LATENCY, not instruction count: with 5 or 6 workgroups per CU a wave has at
// most four neighbours on its SIMD, and measured on gfx950 a lone wave pays 4 cycles per VALU or
// SALU instruction but ~28 for compare -> s_and -> select, ~35 for an exec-masked region and ~40
// for a branch on a vector compare (tools/probes/lat_probe.hip).  So there is no boolean algebra
// on lane masks and no branch inside a step: every predicate is one compare consumed by selects,
// conditions are folded into the data (an out-of-window candidate compares with length cap 0),
// the best match is one v_max over a packed key, and idle lanes run along harmlessly.
// (Round 5) A lane's running best stays in its register until the lane takes its next position (or SEARCH is left): rounds
// 1-4 stored it every step -- two scattered 16-bit LDS writes a pass, on the unit that is 66 % busy -- so that an idle
// lane could store to a dummy word instead; now an idle lane is one that stands on its own position (nback == 0) and
// compares with a cap of 0, which never beats a key (+0.7 % on text, profiles/r05/ab_s2.txt).
struct Walk {
    uint32_t p, t0, t1, t2;      // position and its 12 bytes
    uint32_t nreach, myslot;     // ~(window reach): a distance d is inside iff -d > ~reach; link slot of p
    uint32_t nback;              // MINUS the distance of the candidate to look at next
    // best so far as (len << 12) - offset (signed compares; it fits 16 bits: res[]): candidates come nearest first, so a
    // longer match wins and an equally long farther one does not.  0x2000 = "3-byte chain, nothing
    // yet" (only a length >= 3 beats it), 0x1000 = "2-byte chain, nothing yet".
    int32_t key;
    uint32_t cap;                // length that ends the walk: min(remaining, 12), or 2 on the 2-byte chain; 0 while the lane is idle
                                 // (wg_search<true>, LZS_WGV_HOP_END: stale while idle, and masked by the step -- see there)
    uint32_t nfirst2;            // MINUS the distance where the 2-byte chain starts (-kNoLink: nowhere)
    const uint16_t *links;       // link array being followed
    uint16_t *resp;              // where the result goes once the walk has ended; the dummy word when there is none to store
    // quick reject (LZS_HOPS): a candidate can only improve the key if it is LONGER than the best
    // so far, so its byte at offset best-length must equal mine (`probe`, at position `pb`)
    uint32_t pb, probe;
};
constexpr int32_t kKeyNone3 = 0x2000, kKeyNone2 = 0x1000;

// SEARCH: every wave pulls positions of [Pb, pend) from L.nextp.  A wave leaves when the pool has
// no fresh position left and none of its lanes still walks for a position before Pb (those belong
// to the pool that is parsed next); walks for positions of this pool may be left unfinished.
// The longest walk of a pool (about 30 steps in text, against 5.5 on average) then no longer
// holds up 255 other lanes at the end of every pool.  Results are stored as raw keys; EXTEND
// turns them into off | len << 11 | ext << 15.
template <bool HE>
__device__ __forceinline__ void wg_search(BlkLds &L, Walk &W, uint32_t Pb, uint32_t pend, uint32_t n, uint32_t lane, bool lit, bool drain SEARCH_PROF_PARAMS)
{
    const uint32_t slot0 = wg_slot_base(Pb);
    uint16_t *const dummy = wg_dummy(L);
    PROF_ITER_DECL;
    bool pool_done = false;
    uint32_t p = W.p, t0 = W.t0, t1 = W.t1, t2 = W.t2, nreach = W.nreach, myslot = W.myslot;
    uint32_t nback = W.nback, cap = W.cap, nfirst2 = W.nfirst2;
    uint32_t pb = W.pb, probe = W.probe;
    int32_t key = W.key;
    const uint16_t *links = W.links;
    uint16_t *resp = W.resp;
    // (the masks of the ring in registers: an instruction with a 32-bit literal issues in 2.5 cycles, with registers in 2)
    // (vFFF rounds a key up to its length field; vRM / vRC are the ring's masks -- with the 4 KiB ring vRM is the same number, and register)
#ifdef LZS_WGV_LEAN
    const uint32_t vFFF = 0xFFFu, vRC = kWgRingMask & ~3u, vRM = kWgRingMask;
#else
    const uint32_t vFFF = opaque(0xFFFu), vRC = opaque(kWgRingMask & ~3u);
    const uint32_t vRM = kWgRingMask == 0xFFFu ? vFFF : opaque(kWgRingMask);
#endif
    const uint8_t *const ring8 = reinterpret_cast<const uint8_t *>(L.ring);
    (void)vFFF; (void)vRM;                               // (only the quick reject uses them: a variant without hops does not)
    for (;;) {
        const uint64_t idle = __builtin_amdgcn_ballot_w64(nback == 0u);
        const uint32_t nidle = (uint32_t)__builtin_popcountll(idle);
        if (!pool_done && nidle >= kRefillMin) {
            uint32_t basep = 0;
            // (as assembly: the compiler's rewrite of a one-lane atomic -- count the active lanes, multiply,
            // add the lane's rank back -- is seven vector instructions per pass for nothing)
            if (lane == 0) asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(basep) : "v"(lds_off(&L.nextp)), "v"(nidle) : "memory");
            basep = uniform(basep);
            pool_done = basep + nidle >= pend;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                  __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            const uint32_t np = basep + rank;
            const bool take = nback == 0u && np < pend;
            PROF_COUNT(9, 1);
            PROF_COUNT(10, __builtin_popcountll(__builtin_amdgcn_ballot_w64(take)));
            PROF_COUNT(43, __builtin_amdgcn_ballot_w64(take) == 0ull);       // (a pass that finds the pool taken by the other waves)
            PROF_T0;
            if (take) {                                                  // exec-masked: direct writes, no selects
                *resp = (uint16_t)key;                                   // the result of the walk that ended here (or the dummy word)
                p = np;
                wg_read12(L.ring, p, t0, t1, t2);
                const uint32_t before = wg_ring_byte(L.ring, p - 1u);
                uint32_t sl = slot0 + (p - Pb);
                sl = sl >= kWgLinkN ? sl - kWgLinkN : sl;
                myslot = sl;
                const uint32_t l3 = kNo3 ? kNoLink : (uint32_t)L.link3[sl], l2 = L.link2[sl];
                const uint32_t lim = n - p < kSearchCap ? n - p : kSearchCap;
                // offset 1 first: common prefix of the text with itself shifted by one byte.  It
                // can only reach 2 if the byte before equals the next two, which is rare in text:
                // the 12-byte form is computed only when some lane needs it.
                const bool maybe1 = p >= 1u && ((t0 ^ ((t0 << 8) | before)) & 0xFFFFu) == 0;
                uint32_t len1 = 0;
                if (__builtin_amdgcn_ballot_w64(maybe1) != 0ull) {
                    PROF_ITER;
                    len1 = lcp12(t0 ^ ((t0 << 8) | before), t1 ^ ((t1 << 8) | (t0 >> 24)), t2 ^ ((t2 << 8) | (t1 >> 24)));
                    len1 = len1 < lim ? len1 : lim;
                }
                const bool seeded = maybe1 && len1 >= 2u;
                const bool capped = seeded && len1 == lim;               // nothing nearer or longer exists
                const uint32_t reach = p < kWindow ? p : kWindow;
                nreach = ~reach;
                // chains that are empty inside the window are skipped here, not discovered by a step
#ifdef LZS_ABLATE_STEPS      // counter experiments only: no position ever walks a chain
                const bool walk3 = false, walk2 = false;
#else
                // `lit` (wave-uniform: the pool parsed last was nearly all literals -- high-entropy data):
                // the 3-byte chain holds nothing but collisions there, so a position without a seed walks
                // the 2-byte chain alone, with the full rule (longer wins, the cap ends it) -- that chain
                // is complete for every match of 2 and more, the 3-byte chain is only the shorter list
                // for matches of 3 and more.  (Written as algebra on the lane masks, which the scalar
                // unit does: the refill pass is where every vector instruction costs text 0.3 %.)
                // (kNo3: the 2-byte chain alone, with the full rule, from the seed if there is one)
                const bool walk3 = !kNo3 && lim >= 3u && !capped && l3 <= reach && (seeded || !lit);
                const bool walk2 = lim >= 2u && !capped && (kNo3 || !seeded) && l2 <= reach;
#endif
                nfirst2 = 0u - (walk2 ? l2 : kNoLink);
                nback = walk3 ? 0u - l3 : (walk2 ? nfirst2 : 0u);       // (no chain to walk: idle, on its own position)
                // 3-byte chain: only a longer match than the seed (or than 2) counts and the cap ends
                // the walk (:337-345); 2-byte chain after it: the first verified candidate is the answer
                key = seeded ? (int32_t)((len1 << 12) - 1u) : (walk3 ? kKeyNone3 : kKeyNone2);
                cap = (walk3 || lit || kNo3) ? lim : 2u;
                links = walk3 ? L.link3 : L.link2;
                uint16_t *const slot = &L.res[p & (kWgResN - 1)];
                resp = slot;                                             // stored when the lane takes its next position, or on the way out
                cap = (walk3 || walk2) ? cap : 0u;                       // (no chain to walk: idle at once, its key is final)
#if LZS_HOPS_HERE
                pb = p + (((uint32_t)key + 0xFFFu) >> 12);               // best length so far: 2 / 1 for "nothing yet"
                probe = wg_ring_byte(L.ring, pb);
#endif
            }
            PROF_T1(14);
            PROF_ITER_DONE(18);
        }
        // (`drain`, uniform: the walks of this pool end here too -- it is parsed in this same round)
        if (pool_done && __builtin_amdgcn_ballot_w64(nback != 0u && (drain || p < Pb)) == 0ull) break;
        PROF_COUNT(11, 1);
        PROF_COUNT(8 + 4, __builtin_popcountll(__builtin_amdgcn_ballot_w64(nback != 0u)));
        PROF_T0B;
#pragma unroll
        for (int sub = 0; sub < kSubsteps; sub++) {
            // INVARIANT: the candidate a lane stands on lies inside its window (a walk starts on one:
            // the refill pass skips chains that are empty inside the window; a step or hop only
            // moves on if the next one is inside too), and an idle lane stands on its own position
            // (nback = 0): no step has to ask "is this still inside".
#if LZS_HOPS_HERE
            // Quick reject, zlib's trick in lock step: candidates come nearest first, so one only
            // counts if it is LONGER than the best so far -- its byte at offset best-length must
            // equal mine.  Up to LZS_HOPS candidates that fail this one-byte test are passed over
            // here (a link read and a byte read each, a quarter of a full step) -- but never the
            // last one inside the window: the full step below ends the walk on it.
            // HE (LZS_WGV_HOP_END, round 7): the last one inside the window is passed over as well.  Exact for the same
            // reason: a candidate whose byte at offset best-length differs cannot be strictly longer than the best, wherever
            // it stands in the window, and the nearest-first order of the others is untouched.  With no candidate left the
            // lane goes to its own position (nback = 0, the idle marker) with its cap still set, and the hop holds no end
            // logic: the full step below masks the cap of a lane that stands on its own position to 0, so that it compares
            // nothing, beats no key and satisfies len == cap -- the end logic there runs as it always did, store-on-next-take
            // and the restart on the 2-byte chain included.  What this relies on: hops are ALWAYS followed by a full step
            // before the loop looks at idle lanes again (the refill pass and the test for leaving stand at the top of a
            // pass); a lane taken between a hop and its step would lose the restart.  A later hop of the same sub-step
            // finds the lane's own byte equal to the probe and leaves it where it is.
            // The two predicates are consumed by a select each instead of an AND of lane masks (see above struct Walk): with
            // the step's cap held by a v_min_u16 instead of a select that alone is 1.5 % on text, for four vector
            // instructions a pass more (profiles/r07/ab_search_shape.txt).
            const int nhops = (HE && sub == kSubsteps - 1) ? kHopsLast : kHops;
#pragma unroll
            for (int hop = 0; hop < nhops; hop++) {
                const uint32_t cb = ring8[(pb + nback) & vRM];
                const uint32_t ax = myslot + nback;
                const uint32_t nnx = nback - links[wg_link_slot(ax)];
                if constexpr (HE) {
                    const uint32_t nto = nnx > nreach ? nnx : 0u;
                    nback = cb != probe ? nto : nback;
                } else {
                    const bool skip = cb != probe && nnx > nreach;
                    nback = skip ? nnx : nback;
                }
            }
#endif
            // One step = one candidate, for all 64 lanes alike.
            uint32_t w0, w1, w2;
            {
                const uint32_t q = p + nback;
                const uint32_t *const wp = reinterpret_cast<const uint32_t *>(ring8 + (q & vRC));   // (the mirror: words +1..+3 exist)
                const uint32_t d0 = wp[0], d1 = wp[1], d2 = wp[2], d3 = wp[3];
                w0 = __builtin_amdgcn_alignbyte(d1, d0, q);
                w1 = __builtin_amdgcn_alignbyte(d2, d1, q);
                w2 = __builtin_amdgcn_alignbyte(d3, d2, q);
            }
            const uint32_t at = myslot + nback;
            const uint32_t nd = links[wg_link_slot(at)];
            uint32_t len = lcp12(w0 ^ t0, w1 ^ t1, w2 ^ t2);
            // ("all equal" is 0x1FFFFFFF: 0xFFFF in 16 bits, still more than any cap)
            // (HE: a lane on its own position compares with a cap of 0 whatever its cap is -- nback is 0 or minus a distance of
            // 1 .. 2047: in 16 bits 0, or more than any cap)
            uint32_t capm = cap;
            if constexpr (HE) asm("v_min_u16 %0, %1, %2" : "=v"(capm) : "v"(cap), "v"(nback));
            asm("v_min_u16 %0, %1, %2" : "=v"(len) : "v"(len), "v"(capm));
            const int32_t cand = (int32_t)((len << 12) + nback);
            key = key > cand ? key : cand;
            // the walk ends at the cap, or on the last candidate inside the window (:337-345)
            const uint32_t nnext = nback - nd;
            const int32_t kend = opaque((len == capm || !(nnext > nreach)) ? key : 0);
            // nothing on the 3-byte chain: restart on the 2-byte chain, if there is one in the window
            const bool fallback = !kNo3 && kend == kKeyNone3 && nfirst2 > nreach;
            const int32_t kfin = opaque(fallback ? 0 : kend);
            key = fallback ? kKeyNone2 : key;
            cap = fallback ? 2u : cap;
            links = fallback ? L.link2 : links;
            const uint32_t nwalk = fallback ? nfirst2 : nnext;
            // (HE: the cap of a lane whose walk has ended is NOT cleared -- the step masks the cap of every lane that stands on
            // its own position itself, capm above, so such a lane compares nothing and beats no key while it stays there, and
            // struct Walk's "cap: 0 while the lane is idle" holds for the plain rule only.  Inside one call of wg_search the ring
            // does not change and every step re-reads the probe, so a hop finds an idle lane's own byte equal to its probe and
            // leaves it.  ACROSS calls the ring is refilled: an idle lane carried into the next pool may find another byte under
            // its stale probe, be moved by a hop along stale links and compare with its stale cap, where the plain rule's idle
            // lane wanders the same way with a cap of 0 and ends at once.  That is harmless for one reason only: the key of a
            // walk that has ended is stored on the way out of the call it ended in, and resp is the dummy word from then on
            // until the lane's next take, which resets all of its state; the wandering lane ends on the window like any walk.)
            if constexpr (!HE) {
                cap = kfin != 0 ? 0u : cap;                    // ended for good: the lane is idle -- what it compares with itself from now
                                                               // on is no match (its key waits to be stored) ...
            }
            nback = kfin != 0 ? 0u : nwalk;                    // ... and it stands on its own position
#if LZS_HOPS_HERE
            pb = p + (((uint32_t)key + vFFF) >> 12);
            probe = ring8[pb & vRM];
#endif
        }
        PROF_T1B(15);
    }
    // every lane leaves what it has (a walk still going: its running best, overwritten when it ends); a lane whose walk
    // has ended forgets its slot, which belongs to another position two pools on
    *resp = (uint16_t)key;
    resp = nback == 0u ? dummy : resp;
    W.p = p; W.t0 = t0; W.t1 = t1; W.t2 = t2; W.nreach = nreach; W.myslot = myslot;
    W.nback = nback; W.key = key; W.cap = cap; W.nfirst2 = nfirst2;
    W.pb = pb; W.probe = probe;
    W.links = links; W.resp = resp;
}

// What one workgroup compresses: the stream `src[0..n)` from token start `c0` up to (not
// including) the first token start >= `cend`.  A whole block: c0 = w0 = 0, cend = n.  A segment of
// a longer stream (lzs_compress_segments_kernel): the chains are first built from `w0` (a window
// before the segment), there is no end marker, and where the last token ends and how many bits
// were written is reported for the stitching.
struct WgJob {
    const uint8_t *src;
    uint32_t n, cend, c0, w0;
    bool last;                      // append the end marker
    uint32_t *out_len;              // bytes written (a block), or null
    uint32_t *exit_pos;             // a segment: first token start >= cend ...
    unsigned long long *nbits;      // ... and the bits emitted up to there; or null
    uint32_t *open_info;            // a piece of a stream that will go on (lzs_compress_incremental):
                                    // {offset, start} of the job's last token if that is a match
                                    // reaching the end of the data so far (n), {0, 0} otherwise; or null
#ifdef LZS_WGV_CHANNELS
    const uint8_t *hist;            // the view: positions [0, hlen) are hist[], [hlen, n) are src[0 .. n - hlen)
    uint32_t hlen;
    uint8_t *status;                // LZS_C_STATUS_* of the packet
#endif
};

#ifdef LZS_WGV_CHANNELS
// The two-source view of a channel's job: byte q of [history | packet], zero from n on.
__device__ __forceinline__ uint32_t wg_view_byte(const WgJob &job, uint32_t q)
{
    return q < job.hlen ? job.hist[q] : (q < job.n ? job.src[q - job.hlen] : 0u);
}
// 16 bytes of the view at p (a multiple of 16: REFILL's and OPEN's ring loads), zero from n on
__device__ __forceinline__ uint4 wg_view_load16(const WgJob &job, uint32_t p)
{
    const uint32_t h = job.hlen;
    if (p + 16u <= h) return load16(job.hist, p, h, ((uintptr_t)job.hist & 15u) == 0, ((uintptr_t)job.hist & 3u) == 0);
    if (p >= h) {
        if (p >= job.n) return make_uint4(0u, 0u, 0u, 0u);
        const uint8_t *q = job.src + (p - h);
        return load16(q, 0u, job.n - p, ((uintptr_t)q & 15u) == 0, ((uintptr_t)q & 3u) == 0);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < 16u; k++) w[k >> 2] |= wg_view_byte(job, p + k) << (8u * (k & 3u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// 16 bytes of the view at any q with q + 16 <= n (OPEN's comparisons)
__device__ __forceinline__ u32x4 wg_view_read16(const WgJob &job, uint32_t q)
{
    u32x4 v;
    if (q >= job.hlen) {
        __builtin_memcpy(&v, job.src + (q - job.hlen), 16);
    } else if (q + 16u <= job.hlen) {
        __builtin_memcpy(&v, job.hist + q, 16);
    } else {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (uint32_t k = 0; k < 16u; k++) w[k >> 2] |= wg_view_byte(job, q + k) << (8u * (k & 3u));
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    return v;
}
#endif

// (ENTRY changes nothing in the code: the packed entries below take instance 1, so that every strided entry stays the only caller
// of the instance it had -- as a second caller of that one they moved the strided kernels' instructions; DESIGN.md 3.15.  Instance 2,
// the segments of a batch, differs in one compare: its ORed stores are bounded, wg_store_quarter<true>; DESIGN.md 3.19)
// (HE: SEARCH with LZS_WGV_HOP_END's rule -- the block and packed entries of a variant that asks for it; the segments entry does not)
template <int ENTRY = 0, bool HE = false>
__device__ __forceinline__ void wg_compress_job(BlkLds &L, const WgJob &job, WgOut o)
{
    const uint32_t tid  = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = uniform(tid >> 6);
    const uint8_t *src = job.src;
    const uint32_t n   = job.n;
    const uint32_t cend = job.cend;
    const uint32_t head0 = o.head;
    const bool src16   = ((uintptr_t)src & 15u) == 0;
    const bool src4    = ((uintptr_t)src & 3u) == 0;
#ifdef LZS_WGV_CHANNELS
    (void)src16; (void)src4;                                   // (the view loads by its own rules)
#endif

    for (uint32_t i = tid; i < (kNo3 ? 1u : kWgHead3); i += kWgThreads) L.head3[i] = ~0u;
    for (uint32_t i = tid; i < kWgHead2; i += kWgThreads) L.head2[i] = ~0u;
    L.bits[tid] = 0;
    // HASH looks at the word before a position's own: in front of position 0 there is none, and what
    // it finds there must not look like the beginning of a run (wg_hash_range)
    if (tid == 0) L.ring[kWgRingWords - 1] = 0x00FF00FFu;
    __syncthreads();

    if (job.open_info && tid == 0) { job.open_info[0] = 0; job.open_info[1] = 0; }
    uint32_t c = job.c0;         // start of the next token
    uint32_t loaded = job.w0;    // ring holds [loaded-4096, loaded)
    uint32_t next = job.w0;      // next batch of 64 positions to build
#if !defined(LZS_NO_PREFETCH) && !defined(LZS_WGV_CHANNELS)
    // The half KiB a REFILL stores is requested one pool earlier (every thread asks for the 16
    // bytes its lane & 31 would store -- an unconditional bounded buffer load, straight into
    // `pre`, eight requests for the same bytes -- so that nobody stands at the barrier behind a
    // load from HBM; aligned sources only, and never the stream's last, partial half KiB).
    const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)src, 0, (int)n, 0x00020000);
    u32x4 pre = {0u, 0u, 0u, 0u};
    uint32_t pre_at = ~0u;       // the position `pre` was requested for
#endif
    PROF_DECL;

    // The pools are pipelined: while pool k is in SEARCH, pool k-1 (searched in the round before,
    // except for the walks carried over, which end in this round's SEARCH) waits for PARSE + PACK.
    Walk W;
    W.p = 0; W.t0 = W.t1 = W.t2 = 0; W.nreach = ~0u; W.myslot = 0;
    // (a lane that has not taken a position yet is idle like one whose walk has ended: it stands on its own position with a
    // cap of 0 and a key that is none -- NOT 0, which the step reads as "the walk goes on": with "idle" told by nback since
    // round 5, such a lane wandered off along garbage links and SEARCH never ended in a segment too short to give every lane
    // a position; tests/test_gpu_parity.py::test_short_segments_leave_lanes_that_never_took_a_position)
    W.nback = 0; W.key = kKeyNone2; W.cap = 0; W.nfirst2 = 0u - kNoLink;
    W.pb = 0; W.probe = 0;
    W.links = L.link2; W.resp = wg_dummy(L);
    bool pending = false;                    // a searched pool waits for PARSE
    uint32_t run_rounds = 0;                 // > 0: "run mode" (after an open match), see below
    bool lit_mode = false;                   // the pool parsed last came to more than 8 bits a position: see wg_search
    uint32_t Pb = 0, pend = 0;               // that pool
    const uint32_t nup = (cend + 63u) & ~63u;                 // no pool starts past the job's end

    for (;;) {
        if (o.flushed >= o.cap) break;
        if (!pending && (c >= cend || next >= nup)) break;
        PROF_MARK(4);
        // ---- the next pool [Sb, Se): REFILL (128 threads x 4 B per half KiB) and BUILD
        const bool fresh = next < nup;
        uint32_t Sb = next;
        if (!pending) while (Sb + 64 <= c) Sb += 64;          // batches wholly behind c: built, not searched
        // Run mode: long matches come in company (runs, records, zero fill), and what follows one is
        // mostly run over by the next -- so for kRunRounds rounds after an open match the pool is
        // small (its search is mostly thrown away) and is parsed in the round that searches it,
        // instead of a round later beside the search of the next one.
        const bool run_mode = !pending && run_rounds != 0u;
        const uint32_t pool = run_mode ? kRunPool : kWgPool;
        const uint32_t Se = fresh ? (Sb + pool < nup ? Sb + pool : nup) : Sb;
        if (fresh) {
            // Not further ahead than needed: the walks carried over still read 2047 bytes
            // back from the pool before, and the ring holds 4096.
            const uint32_t need = (Se > c ? Se : c) + 96;
            while (loaded < n && loaded < need) {
                PROF_COUNT(42, 1);
                // half a KiB by 32 lanes of one wave (the waves take turns): the kernel is bound
                // by VALU issue, and four waves computing addresses for 4 bytes each cost four times this
                if (wave == ((loaded / kRefillUnit) & (kW - 1u)) && lane < kRefillUnit / 16u) {
                    const uint32_t p = loaded + 16 * lane;
#if defined(LZS_WGV_CHANNELS)     // (no prefetch: the view has two sources)
                    const uint4 v = wg_view_load16(job, p);
#elif !defined(LZS_NO_PREFETCH)
                    const uint4 v = pre_at == loaded ? make_uint4(pre.x, pre.y, pre.z, pre.w) : load16(src, p, n, src16, src4);
#else
                    const uint4 v = load16(src, p, n, src16, src4);
#endif
                    const uint32_t at = (p & kWgRingMask) >> 2;
                    *reinterpret_cast<uint4 *>(&L.ring[at]) = v;
                    if (at == 0) *reinterpret_cast<uint4 *>(&L.ring[kWgRingWords]) = v;
                }
                loaded += kRefillUnit;
            }
#if !defined(LZS_NO_PREFETCH) && !defined(LZS_WGV_CHANNELS)
            if (src16 && loaded + kRefillUnit <= n) {
                pre = __builtin_amdgcn_raw_buffer_load_b128(src_rsrc, (int)(loaded + 16u * (lane & (kRefillUnit / 16u - 1u))), 0, 0);
                pre_at = loaded;
            }
#endif
            PROF_SYNC(32);
            PROF_MARK(0);
            // Normally one pool; after an open match also the batches it ran over (at most the
            // 2112 positions that can still be candidates, see below), half a KiB at a time (the
            // HASH records wait for CHAIN in the positions' own slots of the link rings).
            { PROF_T0; PROF_COUNT(17, (Se - next) >> 6);
              for (uint32_t R = next; R < Se; R += kWgPool) {
                  const uint32_t R2 = R + kWgPool < Se ? R + kWgPool : Se;
                  if (R != next) PROF_SYNC(33);
#ifndef LZS_ABLATE_BUILD     // counter experiments only
                  wg_hash_range(L, R, R2, lane, wave);
                  PROF_SYNC(34);
                  // (which waves chain rotates with the block, so that no SIMD is always the one with the extra work: +0.25 %)
                  wg_chain_range(L, R, R2, lane, (wave + blockIdx.x) & (kW - 1u));
#endif
              }
              PROF_T1(16); }
            next = Se;
        }
        const uint32_t send = Se < cend ? Se : cend;             // (cend <= n; tokens start before it)
        if (tid == 0) L.nextp = (!pending && c > Sb) ? c : Sb;
        PROF_SYNC(35);
        PROF_MARK(1);

        // ---- SEARCH the new pool; ends every walk for the pending one
#ifdef LZS_WGV_PRIO          // SEARCH is where the time goes and every wave has work in it; the short phases between barriers, where
        __builtin_amdgcn_s_setprio(0);   // some waves of the workgroup wait for others, go first on their SIMD (+0.9 % on text, ab_s13)
#endif
        wg_search<HE>(L, W, Sb, send, n, lane, lit_mode, run_mode && fresh SEARCH_PROF_ARGS);
#ifdef LZS_WGV_PRIO
        __builtin_amdgcn_s_setprio(2);
#endif
        PROF_MARK(2);
        PROF_SYNC(36);
        PROF_MARK(5);

        bool at_once = false;
        if (!pending) {                                        // nothing to parse yet
            Pb = Sb; pend = send; pending = fresh;
            if (!(run_mode && fresh)) continue;
            at_once = true;                                    // run mode: every walk of this pool has ended (`drain`)
            run_rounds--;
        }

        // ---- PARSE + PACK; repeated after each open match that ends inside the pool.
        // The greedy chain of token starts is resolved hierarchically.  Inside each 64-position
        // chunk (two per wave, lane = position) pointer doubling over next[i] = i + bytes
        // consumed at i runs in registers (ds_bpermute, no barrier) and yields, for EVERY
        // possible entry position, where the chain leaves the chunk.  One short walk over the
        // 8 published exit functions then tells each chunk its actual entry, and lane m finds
        // the m-th token start of its chunk from the kept doubling tables -- so lane order is
        // token order and the bit offsets are a prefix sum.
#ifdef LZS_ABLATE_PARSE      // counter experiments only: the pool is dropped instead of parsed and packed
        c = pend;
        Pb = Sb; pend = send; pending = fresh;
        continue;
#endif
        const uint32_t npos = pend - Pb;
        PROF_STAMP0;
        uint32_t rr[2];                                        // results of this thread's two positions, complete
        wg_extend(L, Pb, c - Pb, npos, n, lane, wave, rr SEARCH_PROF_ARGS);
        PROF_STAMP(20);
        while (c < pend && o.flushed < o.cap) {
            const uint32_t entry = c - Pb;
            PROF_COUNT(31, 1);
            // Written for latency (see Walk): the two chunks of a wave go through every
            // dependent cross-lane step side by side, predicates are single compares consumed
            // by selects, and nothing is exec-masked.
            // (Round 4) A position whose token ends the chain inside the chunk -- it leaves the chunk
            // or the pool, or is an open match -- points at ITSELF, so doubling needs no "is this still
            // a lane" test: six plain ds_bpermute rounds end on the chain's last token start in the
            // chunk, and one more fetches that position's exit code.  Pointers are kept times 4, as
            // ds_bpermute wants them.
            uint32_t T4[2][6], t4[2], xc[2];
#pragma unroll
            for (int h = 0; h < kCh; h++) {
                const uint32_t cb = kChunkStride * h + 64u * wave;         // pool-relative start of the chunk
                const uint32_t inside = cb < npos ? (npos - cb < 64u ? npos - cb : 64u) : 0u;   // its positions in the pool
                const uint32_t r = rr[h];
                const uint32_t len = (r >> 11) & 15u, ext = r >> 15;
                uint32_t step = len < kTokenMax ? len : kTokenMax + ext;
                step = len < 2u ? 1u : step;
                const uint32_t land = lane + step;
                // exit code of a position that ends the chain here: the pool-relative position the chain goes to next
                // (>= npos: the pool is done), or 0x8000 | the position of an open match; with one-byte exits both relative
                // to the chunk's start (<= 63 + 67, or 192 + the position)
                const uint32_t xb = kExit8 ? 0u : cb;
                uint32_t to = land < inside ? land : lane;
                uint32_t ex = xb + land;
                to = ext == kExtOpen ? lane : to;                          // ext is 63 only for an open match
                ex = ext == kExtOpen ? (kExit8 ? 192u + lane : (0x8000u | (cb + lane))) : ex;
                to = lane < inside ? to : lane;
                ex = lane < inside ? ex : xb + lane;
                t4[h] = to << 2;
                xc[h] = ex;
            }
#pragma unroll
            for (int d = 0; d < 6; d++) {
#pragma unroll
                for (int h = 0; h < kCh; h++) {
                    T4[h][d] = t4[h];
                    t4[h] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)t4[h], (int)t4[h]);
                }
            }
#pragma unroll
            for (int h = 0; h < kCh; h++) {
                const uint32_t cb = kChunkStride * h + 64u * wave;
                L.exitfn[cb + lane] = (exit_t)__builtin_amdgcn_ds_bpermute((int)t4[h], (int)xc[h]);
            }
            PROF_STAMP(21);
            PROF_SYNC(37);
            PROF_STAMP(22);
            // complete quarters of the bit ring go out, one wave each: the bits of the round before
            // are all in (barrier above), and nothing is added before the next barrier
            while (o.head >= 2048u) {
                PROF_COUNT(29, 1);
                if (wave == ((o.flushed >> 8) & (kW - 1u))) wg_store_quarter<ENTRY == 2>(o, L, lane);
                o.flushed += 256u;
                o.head -= 2048u;
            }
            // follow the published exits from the entry, one hop per chunk, in every lane alike
            // (on the scalar unit: the kernel is VALU-bound, and this walk is the same in all four waves)
            uint32_t enter[2] = {0x100u, 0x100u};                          // where the chain enters my chunks; >= 64: not at all
            uint32_t last = entry;
            while (last < npos) {
                const uint32_t k = last >> 6;
                if (k == wave) enter[0] = last & 63u;
                if (kCh > 1 && k == wave + kW) enter[1] = last & 63u;
                PROF_COUNT(28, 1);
                const uint32_t v = uniform((uint32_t)L.exitfn[last]), from = last & ~63u;
                last = !kExit8 ? v : v < 192u ? from + v : (0x8000u | (from + v - 192u));
            }
            const uint32_t chain_end = (last & 0x8000u) ? kOpen : last;
            const uint32_t open_at = last & 0x7FFFu;
            PROF_STAMP(23);
            PROF_MARK(3);
            // ---- PACK: lane m takes the m-th token of its chunk (formats: lzs-compression.c:365-431):
            // m steps from the entry by the bits of m; past the chain's last token the steps stand
            // still, so a lane has a token iff it stands elsewhere than the lane before it
            uint32_t n4[2];
            bool tok[2];
#pragma unroll
            for (int h = 0; h < kCh; h++) n4[h] = (enter[h] & 63u) << 2;
#pragma unroll
            for (int d = 0; d < 6; d++) {
                uint32_t via[2];
#pragma unroll
                for (int h = 0; h < kCh; h++)
                    via[h] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)n4[h], (int)T4[h][d]);
#pragma unroll
                for (int h = 0; h < kCh; h++) n4[h] = ((lane >> d) & 1u) ? via[h] : n4[h];
            }
#pragma unroll
            for (int h = 0; h < kCh; h++) {
                // (wave_shr:1 -- lane 0 keeps `old`, which no pointer equals)
                const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp((int)~0u, (int)n4[h], 0x138, 0xf, 0xf, false);
                tok[h] = enter[h] < 64u && n4[h] != before;
            }
#if !defined(LZS_WGV_PACK_BY_CHUNK) && !(defined(LZS_WGV_POOL) && LZS_WGV_POOL == 256)
            // (Round 5) The tokens of a wave's two chunks formatted, summed and placed in ONE pass when they are no more than
            // 64 together (text: ~43 of 128 positions start a token), in a second pass of the same shape for the rest
            // otherwise: lane L of pass p takes token 64 p + L of chunk 0's tokens followed by chunk 1's (chunk 1's come across
            // the lanes by one ds_bpermute).  Text 72.9 -> 73.6 GB/s; blocks that are nearly all literals always need the second
            // pass and lose 3.5 % to the bookkeeping, so their variant (LZS_WGV_PACK_BY_CHUNK) formats chunk by chunk as
            // rounds 1-4 did (profiles/r05/ab_s8_pack_in_one_pass.txt; round 3's attempt at this had no such choice).
            const uint32_t nt0 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(tok[0]));
            const uint32_t nt1 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(tok[1]));
            uint32_t rec[2];                                               // a token's result and its position in its chunk
#pragma unroll
            for (int h = 0; h < 2; h++) rec[h] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)n4[h], (int)rr[h]) | (n4[h] << 19);
            uint32_t valhi[2] = {0u, 0u}, vallo[2] = {0u, 0u}, width[2] = {0u, 0u}, incl[2] = {0u, 0u}, from1[2] = {0u, 0u};
            const uint32_t npass = nt0 + nt1 > 64u ? 2u : 1u;              // (uniform)
            PROF_COUNT(30, npass - 1u);
#pragma unroll
            for (int ps = 0; ps < 2; ps++) {
                if ((uint32_t)ps >= npass) break;
                const uint32_t t = 64u * ps + lane;
                const uint32_t idx1 = t - nt0;                             // which of chunk 1's tokens, if t >= nt0
                const uint32_t pulled = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((idx1 & 63u) << 2), (int)rec[1]);
                const bool f1 = t >= nt0;
                const bool valid = t < nt0 + nt1;
                const uint32_t rc = (ps == 0 && !f1) ? rec[0] : pulled;
                const uint32_t r = rc & 0x1FFFFFu, posc = rc >> 21;
                const uint32_t byte = wg_ring_byte(L.ring, Pb + (f1 ? kChunkStride : 0u) + 64u * wave + posc) & 0xFFu;
                const uint32_t len = (r >> 11) & 15u, ext = r >> 15, off = r & kWindow;
                const uint32_t ov = off <= kShortMax ? ((3u << 7) | off) : ((2u << 11) | off);
                const uint32_t ow = off <= kShortMax ? 9u : 13u;
                const uint32_t first = len < kTokenMax ? len : kTokenMax;
                const uint32_t lv = first <= 4u ? first - 2u : first + 7u;
                const uint32_t lw = first <= 4u ? 2u : 4u;
                const uint32_t full = (ext * 137u) >> 11;                  // ext / 15 for ext < 64
                uint32_t tv = (((1u << (4u * full)) - 1u) << 4) | (ext - kNibbleMax * full);
                uint32_t tw = 4u * (full + 1u);
                tw = len < kTokenMax ? 0u : tw;
                tv = len < kTokenMax ? 0u : tv;
                uint32_t hv = (ov << lw) | lv, hw = ow + lw;
                hv = len < 2u ? byte : hv;                                 // literal: 0 bbbbbbbb
                hw = len < 2u ? 9u : hw;
                uint32_t w = hw + tw;
                w = ext == kExtOpen ? 0u : w;                              // the open match: finished by the whole workgroup below
                w = valid ? w : 0u;
                const uint64_t v = w ? (((uint64_t)hv << tw) | tv) : 0ull;
                valhi[ps] = (uint32_t)(v >> 32); vallo[ps] = (uint32_t)v; width[ps] = w; from1[ps] = f1 ? 1u : 0u;
                if (job.open_info) {                                       // (wave-uniform; null for whole blocks)
                    const uint32_t pos = Pb + (f1 ? kChunkStride : 0u) + 64u * wave + posc;
                    if (w && len >= kTokenMax && pos + kTokenMax + ext == n) { job.open_info[0] = off; job.open_info[1] = pos; }
                }
                incl[ps] = wave_inclusive_sum(w);
            }
            // the bits of either chunk: chunk 0's tokens are the first nt0 of pass 0
            const uint32_t sum0 = (uint32_t)__builtin_amdgcn_readlane((int)incl[0], 63);
            const uint32_t bits0 = nt0 ? (uint32_t)__builtin_amdgcn_readlane((int)incl[0], (int)((nt0 - 1u) & 63u)) : 0u;
            const uint32_t sum_all = sum0 + (npass > 1u ? (uint32_t)__builtin_amdgcn_readlane((int)incl[1], 63) : 0u);
            if (lane == 63u) { L.chunk_bits[wave] = bits0; L.chunk_bits[kW + wave] = sum_all - bits0; }
            PROF_STAMP(24);
            PROF_SYNC(38);
            PROF_STAMP(25);
            const uint32_t cbits = lane < 2u * kW ? L.chunk_bits[lane & (2u * kW - 1u)] : 0u;
            const uint32_t cincl = wave_inclusive_sum(cbits);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)cincl, (int)(2u * kW - 1u));
            const uint32_t cexcl = cincl - cbits;
            const uint32_t at0 = wg_bit_at(o);
            const uint32_t before0 = (uint32_t)__builtin_amdgcn_readlane((int)cexcl, (int)wave);
            const uint32_t before1 = (uint32_t)__builtin_amdgcn_readlane((int)cexcl, (int)(kW + wave));
#pragma unroll
            for (int ps = 0; ps < 2; ps++) {
                if ((uint32_t)ps >= npass) break;
                const uint32_t carry = ps ? sum0 : 0u;                     // bits of the tokens in the pass before
                const uint32_t rel = carry + incl[ps] - width[ps];         // bits of the wave's tokens before this one
                const uint32_t at = (at0 + (from1[ps] ? before1 + rel - bits0 : before0 + rel)) & kBitMask;
                const uint64_t v = (((uint64_t)valhi[ps] << 32) | vallo[ps]) << ((64u - (at & 31u) - width[ps]) & 63u);
                const uint32_t vh = (uint32_t)(v >> 32), vl = (uint32_t)v;
                const uint32_t d = at >> 5;
                const uint32_t dh = vh ? d : tid, dl = vl ? (d + 1u) & (kWgBitWords - 1) : tid;
                __hip_atomic_fetch_or(&L.bits[dh], vh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_or(&L.bits[dl], vl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
#else
            uint32_t valhi[2], vallo[2], width[2], incl[2], rtok[2], btok[2];
#pragma unroll
            for (int h = 0; h < kCh; h++) {
                rtok[h] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)n4[h], (int)rr[h]);
                btok[h] = wg_ring_byte(L.ring, Pb + kChunkStride * h + 64u * wave + (n4[h] >> 2)) & 0xFFu;
            }
#pragma unroll
            for (int h = 0; h < kCh; h++) {
                const uint32_t r = rtok[h];
                const uint32_t len = (r >> 11) & 15u, ext = r >> 15, off = r & kWindow;
                // match: offset field, first length code, extension nibbles 15 15 .. last
                const uint32_t ov = off <= kShortMax ? ((3u << 7) | off) : ((2u << 11) | off);
                const uint32_t ow = off <= kShortMax ? 9u : 13u;
                const uint32_t first = len < kTokenMax ? len : kTokenMax;
                const uint32_t lv = first <= 4u ? first - 2u : first + 7u;
                const uint32_t lw = first <= 4u ? 2u : 4u;
                const uint32_t full = (ext * 137u) >> 11;                  // ext / 15 for ext < 64
                uint32_t tv = (((1u << (4u * full)) - 1u) << 4) | (ext - kNibbleMax * full);
                uint32_t tw = 4u * (full + 1u);
                tw = len < kTokenMax ? 0u : tw;
                tv = len < kTokenMax ? 0u : tv;
                uint32_t hv = (ov << lw) | lv, hw = ow + lw;
                hv = len < 2u ? btok[h] : hv;                              // literal: 0 bbbbbbbb
                hw = len < 2u ? 9u : hw;
                // not a token of this round: no node, or the open match (finished by wave 0 below)
                uint32_t w = hw + tw;
                w = ext == kExtOpen ? 0u : w;
                w = tok[h] ? w : 0u;
                const uint64_t v = w ? (((uint64_t)hv << tw) | tv) : 0ull;
                valhi[h] = (uint32_t)(v >> 32); vallo[h] = (uint32_t)v; width[h] = w;
                if (job.open_info) {                                       // (wave-uniform; null for whole blocks)
                    const uint32_t pos = Pb + kChunkStride * h + 64u * wave + (n4[h] >> 2);
                    if (w && len >= kTokenMax && pos + kTokenMax + ext == n) { job.open_info[0] = off; job.open_info[1] = pos; }
                }
                incl[h] = wave_inclusive_sum(w);
                if (lane == 63u) L.chunk_bits[kW * h + wave] = incl[h];     // (exitfn is live: no dummy stores here)
            }
            PROF_STAMP(24);
            PROF_SYNC(38);
            PROF_STAMP(25);
            // bits of the chunks before mine: a scan over the 8 chunk sums in lanes 0..7
            const uint32_t cbits = lane < kW * kCh ? L.chunk_bits[lane & (2u * kW - 1u)] : 0u;
            const uint32_t cincl = wave_inclusive_sum(cbits);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)cincl, (int)(2u * kW - 1u));
            const uint32_t cexcl = cincl - cbits;
            const uint32_t at0 = wg_bit_at(o);
#pragma unroll
            for (int h = 0; h < kCh; h++) {
                const uint32_t before = (uint32_t)__builtin_amdgcn_readlane((int)cexcl, (int)(kW * h + wave));
                const uint32_t at = (at0 + before + incl[h] - width[h]) & kBitMask;
                // OR the token (<= 33 bits), MSB first, at bit `at`; a lane without one ORs zeros
                const uint64_t v = (((uint64_t)valhi[h] << 32) | vallo[h]) << ((64u - (at & 31u) - width[h]) & 63u);
                // zeros go to a word of the thread's own: many lanes ORing into one word serialize
                const uint32_t vh = (uint32_t)(v >> 32), vl = (uint32_t)v;
                const uint32_t d = at >> 5;
                const uint32_t dh = vh ? d : tid, dl = vl ? (d + 1u) & (kWgBitWords - 1) : tid;
                __hip_atomic_fetch_or(&L.bits[dh], vh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_or(&L.bits[dl], vl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
#endif
            o.head += total;
#ifndef LZS_NO_LIT_MODE
            lit_mode = total > 8u * (npos - entry);
#endif
            PROF_STAMP(26);

            PROF_MARK(6);
            if (chain_end != kOpen) {
                c = Pb + chain_end;                            // >= pend
            } else {
                // ---- open match at Pb + open_at: finished by the whole workgroup (:417-431)
                PROF_SYNC(39);                               // every wave's bits of this round are in
                const uint32_t off = uniform((0u - (uint32_t)L.res[(Pb + open_at) & (kWgResN - 1)]) & kWindow);   // raw key: (len << 12) - offset
                if (tid == 0) {
                    if (off <= kShortMax) bits_or(L.bits, kWgBitWords, wg_bit_at(o), (((3u << 7) | off) << 4) | 0xFu, 13);
                    else                  bits_or(L.bits, kWgBitWords, wg_bit_at(o), (((2u << 11) | off) << 4) | 0xFu, 17);
                }
                o.head += off <= kShortMax ? 13u : 17u;
                c = Pb + open_at + kTokenMax;
                // Up to 4080 bytes = 272 nibbles per step: thread t compares the 16 bytes at c + 16 t
                // with those `off` before, straight from the source (the bytes of a long match never
                // pass through the ring: what the chains need of them is loaded in one go below).
                // A wave's count goes to the others through L.bcast (two sets, used in turn: one
                // barrier per step).  Nothing is inserted into the chains here.
                uint32_t par = 0;
                for (;;) {
                    const uint32_t rem = n - c;
                    const uint32_t span = rem < kOpenStep ? rem : kOpenStep;
                    const uint32_t q = c + 16u * tid;
                    const uint32_t mine = span > 16u * tid ? (span - 16u * tid < 16u ? span - 16u * tid : 16u) : 0u;   // bytes of the span in my 16
                    uint32_t eq = 0;
                    if (mine == 16u) {
                        u32x4 va, vb;
#ifdef LZS_WGV_CHANNELS
                        va = wg_view_read16(job, q);
                        vb = wg_view_read16(job, q - off);
#else
                        __builtin_memcpy(&va, src + q, 16);
                        __builtin_memcpy(&vb, src + q - off, 16);
#endif
                        const uint32_t e = lcp12(va.x ^ vb.x, va.y ^ vb.y, va.z ^ vb.z);
                        const uint32_t x3 = va.w ^ vb.w;
                        const uint32_t e3 = x3 ? (uint32_t)__builtin_ctz(x3) >> 3 : 4u;
                        eq = e < 12u ? e : 12u + e3;
                    } else {
#ifdef LZS_WGV_CHANNELS
                        while (eq < mine && wg_view_byte(job, q + eq) == wg_view_byte(job, q + eq - off)) eq++;
#else
                        while (eq < mine && src[q + eq] == src[q + eq - off]) eq++;
#endif
                    }
                    const uint64_t stops = __builtin_amdgcn_ballot_w64(eq < 16u);
                    const uint32_t l = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;
                    const uint32_t mw = l < 64u ? 16u * l + (uint32_t)__builtin_amdgcn_readlane((int)eq, (int)(l & 63u)) : 1024u;
                    if (lane == 0 && wave < 4u) L.bcast[4u * par + wave] = mw;   // (a step is 255 threads' worth whatever the workgroup's size)
                    PROF_SYNC(40);                           // the counts are there; the bits of the step before are in
                    while (o.head >= 2048u) {
                        if (wave == ((o.flushed >> 8) & (kW - 1u))) wg_store_quarter<ENTRY == 2>(o, L, lane);
                        o.flushed += 256u;
                        o.head -= 2048u;
                    }
                    if (o.flushed >= o.cap) break;
                    const uint32_t m0 = L.bcast[4u * par], m1 = L.bcast[4u * par + 1u], m2 = L.bcast[4u * par + 2u], m3 = L.bcast[4u * par + 3u];
                    const uint32_t m = uniform(m0 < 1024u ? m0 : 1024u + (m1 < 1024u ? m1 : 1024u + (m2 < 1024u ? m2 : 1024u + m3)));
                    par ^= 1u;
                    c += m;
                    const bool more = m == kOpenStep;
                    // m / 15 nibbles of 15, then (unless the whole step matched and the run may go
                    // on) the closing nibble 0..14: up to 1092 bits, 32 per lane of wave 0
                    const uint32_t full = m / kNibbleMax;
                    const uint32_t ones = 4u * full, seq = more ? ones : ones + 4u;
                    if (wave == 0 && 32u * lane < seq) {
                        const uint32_t a = 32u * lane;
                        const uint32_t n1 = ones > a ? (ones - a < 32u ? ones - a : 32u) : 0u;         // ones in my piece
                        const bool closes = !more && ones >= a && ones < a + 32u;                      // the nibble is in my piece
                        const uint32_t width = n1 + (closes ? 4u : 0u);
                        uint32_t v = n1 >= 32u ? ~0u : (1u << n1) - 1u;
                        if (closes) v = (v << 4) | (m - kNibbleMax * full);
                        if (width) bits_or(L.bits, kWgBitWords, (wg_bit_at(o) + a) & kBitMask, v, width);
                    }
                    o.head += seq;
                    if (!more) break;
                }
                // Which of the positions the match ran over still go into the chains:
                // * none that lie more than a window before c (nothing searched from here on looks
                //   back further than 2047; chains only lead from built positions to older built ones);
                // * none whose 12 bytes repeat `off` further on INSIDE the match, q + off + 12 <= c:
                //   the position q + off is nearer to everything searched later and has the same
                //   capped common prefix with it, so q is never the nearest-longest (the argument of
                //   the period-1 rule in HASH, for any period); what remains is the last off + 12.
                if (c > next + 2176u) next = (c - 2112u) & ~63u;
#ifndef LZS_NO_DOMINATED_SKIP
                if (c > off + kSearchCap) {
                    const uint32_t dom = (c - off - kSearchCap + 1u) & ~63u;
                    next = dom > next ? dom : next;
                }
#endif
                if (job.open_info && tid == 0 && c == n) { job.open_info[0] = off; job.open_info[1] = Pb + open_at; }
                // the ring, in one go: what the next pools read (2047 back from c, and BUILD one batch
                // more) -- 16 bytes per thread, up to c + 1 KiB in steps of half a KiB
                if (c + 1024u > loaded && loaded < n) {
                    uint32_t upto = loaded + ((c + 1024u - loaded + 511u) & ~511u);
                    while (upto >= n + 512u) upto -= 512u;     // (as far as REFILL would go: one half KiB holds the end)
                    const uint32_t from = upto - loaded > kWgRing ? upto - kWgRing : loaded;
                    const uint32_t p = from + 16u * tid;
                    if (p < upto) {
#ifdef LZS_WGV_CHANNELS
                        const uint4 v = wg_view_load16(job, p);
#else
                        const uint4 v = load16(src, p, n, src16, src4);
#endif
                        const uint32_t at = (p & kWgRingMask) >> 2;
                        *reinterpret_cast<uint4 *>(&L.ring[at]) = v;
                        if (at == 0) *reinterpret_cast<uint4 *>(&L.ring[kWgRingWords]) = v;
                    }
                    loaded = upto;
                }
                run_rounds = kRunRounds;
                PROF_SYNC(41);                               // the match's bits and the ring are in
                PROF_MARK(7);
            }
        }
        PROF_COUNT(13, 1);
        if (at_once) {                                         // nothing is in flight: every walk has ended
            pending = false;
            continue;
        }
        // the pool just searched is parsed next, unless an open match ran past all of it
        Pb = Sb; pend = send; pending = fresh;
        if (pending && c >= pend) { pending = false; W.resp = wg_dummy(L); W.nback = 0; W.cap = 0; }
    }
    PROF_DONE;
    __syncthreads();                                           // the last round's bits are in

    if (wave == 0) {
        if (job.exit_pos && lane == 0) {
            *job.exit_pos = c;
            *job.nbits = 8ull * o.flushed + o.head - head0;        // without an end marker
        }
        // ---- end marker 1 1 0000000, zero pad to a byte, drain (:449-466)
        if (job.last) {
            if (lane == 0) bits_or(L.bits, kWgBitWords, wg_bit_at(o), 0x180u, 9);
            o.head = (o.head + 9u + 7u) & ~7u;
        }
        while (o.head >= 2048u) { wg_store_quarter<ENTRY == 2>(o, L, lane); o.flushed += 256u; o.head -= 2048u; }
        __builtin_amdgcn_wave_barrier();
        const uint32_t nbytes = (o.head + 7u) >> 3;                // a segment may end inside a byte
        if (o.ored) {
            if (32u * lane < o.head) wg_store_quarter<ENTRY == 2>(o, L, lane);     // the words the last bits reach into
        } else {
            for (uint32_t i = lane; i < nbytes; i += 64) {
                const uint32_t bit = ((o.flushed << 3) + 8 * i) & kBitMask;
                const uint32_t v = (L.bits[bit >> 5] >> (24u - (bit & 24u))) & 0xFFu;
                if (o.flushed + i < o.limit) o.dst[o.flushed + i] = (uint8_t)v;
            }
        }
        const uint32_t total = o.flushed + nbytes;
        if (job.out_len && lane == 0) *job.out_len = total < o.cap ? total : o.cap;
#ifdef LZS_WGV_CHANNELS
        // all of the packet was taken; cut at the capacity, the stream lacks its end (lzs_compress_incremental's flags)
        if (job.status && lane == 0) *job.status = (uint8_t)(total <= o.cap ? 0x07u : 0x0Bu);
#endif
    }
}

#ifndef LZS_WGV_CHANNELS
#ifdef LZS_WGV_WAVES          // (waves per SIMD the register allocation is held to: an occupancy experiment of round 6)
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(LZS_WGV_WAVES, LZS_WGV_WAVES)))
#else
__global__ __launch_bounds__(kWgThreads)
#endif
void lzs_compress_blocks_wg_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                   uint32_t *__restrict__ out_len,
                                   const uint8_t *__restrict__ in, size_t in_stride,
                                   const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                   uint32_t nblocks, uint32_t serve)
{
    __shared__ BlkLds L;
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    // `serve` != 0: this launch is one of several over the same grid, one per variant of the kernel, and a block belongs to
    // the variant whose code lzs_classify_blocks_kernel left in out_len[b] (nothing that could be a length); the workgroups
    // of the others return at once.  Whichever variant compresses a block, its bytes are the same (tests force each on all).
    if (serve != 0u) {
        // (a scalar load: the workgroups of the other variants' blocks live as long as this takes, five or six to a CU)
        uint32_t code;
        asm volatile("s_load_dword %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(code) : "s"(out_len + b) : "memory");
        if (code != serve) return;
    }
    WgJob job;
    job.src = in + (size_t)b * in_stride;
    job.n = in_len ? in_len[b] : in_len_uniform;
    job.cend = job.n; job.c0 = 0; job.w0 = 0; job.last = true;
    job.out_len = out_len + b; job.exit_pos = nullptr; job.nbits = nullptr; job.open_info = nullptr;
    WgOut o;
    o.flushed = 0; o.head = 0;
    o.dst = out + (size_t)b * out_stride;
    o.cap = out_cap;
    o.aligned4 = ((uintptr_t)o.dst & 3u) == 0;
    o.limit = out_cap; o.ored = false;
    wg_compress_job<0, kHopEnd>(L, job, o);
}

// The same from PACKED blocks to rooms (include/lzs/lzs_batch.h "PACKED streams"; DESIGN.md 3.15): block b lies at in + in_off[b] and
// is written at out + out_off[b]; its room, out_off[b + 1] - out_off[b], is its capacity AND where its stores stop, so the
// neighbour's first byte, which lies right behind, is never touched.  An entry that is not a block gets length 0 here when the
// kernel runs alone (`serve` 0); under the variants' protocol lzs_classify_packed_kernel has written that 0 already, and 0 is no
// variant's code.  (An entry of its own beside lzs_compress_blocks_wg_kernel, not a body shared with it, and its own instance of
// wg_compress_job: either kind of sharing moved that kernel's instructions in some variants.)
#ifdef LZS_WGV_WAVES
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(LZS_WGV_WAVES, LZS_WGV_WAVES)))
#else
__global__ __launch_bounds__(kWgThreads)
#endif
void lzs_compress_packed_wg_kernel(uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_len,
                                   const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                   const uint32_t *__restrict__ in_len, uint32_t nblocks, uint32_t serve)
{
    __shared__ BlkLds L;
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    if (serve != 0u) {                                         // (as in lzs_compress_blocks_wg_kernel)
        uint32_t code;
        asm volatile("s_load_dword %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(code) : "s"(out_len + b) : "memory");
        if (code != serve) return;
    }
    uint64_t from, to;
    uint32_t n, room;
    if (!packed_entry(in_off, in_len, out_off, b, from, n, to, room)) {
        if (threadIdx.x == 0) out_len[b] = 0;
        return;
    }
    WgJob job;
    job.src = in + from;
    job.n = n;
    job.cend = job.n; job.c0 = 0; job.w0 = 0; job.last = true;
    job.out_len = out_len + b; job.exit_pos = nullptr; job.nbits = nullptr; job.open_info = nullptr;
    WgOut o;
    o.flushed = 0; o.head = 0;
    o.dst = out + to;
    o.cap = room;
    o.aligned4 = ((uintptr_t)o.dst & 3u) == 0;
    o.limit = room; o.ored = false;
    wg_compress_job<1, kHopEnd>(L, job, o);
}
#endif  // !LZS_WGV_CHANNELS

// One long stream cut into segments of `seg` bytes (a multiple of 64), one workgroup each.  The
// search is a pure function of (input, position), so a segment only needs the 2047 bytes before it
// in its chains -- but where its first token starts, and at which bit its output begins, depends
// on the segment before.  Every segment writes its bits into a slot of its own, as if it began at
// bit 0; the host (lzs_host.c) enters every segment at its own start first, re-runs the segments
// whose predecessor turned out to end its last token elsewhere (`dirty`) until all entries agree,
// takes the prefix sum of the bit counts and has lzs_stitch_segments_kernel shift the slots into
// place.
#ifdef LZS_WGV_SEGMENTS
#ifdef LZS_WGV_WAVES
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(LZS_WGV_WAVES, LZS_WGV_WAVES)))
#else
__global__ __launch_bounds__(kWgThreads)
#endif
void lzs_compress_segments_kernel(uint8_t *__restrict__ slots, size_t slot_stride,
                                  const uint8_t *__restrict__ in, uint32_t n, uint32_t seg, uint32_t nseg,
                                  const uint32_t *__restrict__ entry, const uint8_t *__restrict__ dirty,
                                  uint32_t *__restrict__ exit_pos, unsigned long long *__restrict__ nbits,
                                  uint8_t *__restrict__ out, const unsigned long long *__restrict__ bit_at,
                                  uint32_t lim, uint32_t *__restrict__ open_info)
{
    __shared__ BlkLds L;
    const uint32_t k = blockIdx.x;
    if (k >= nseg) return;
    if (dirty && !dirty[k]) return;
    const uint32_t s = k * seg;
    // The last segment ends with the input -- or, for a piece of a stream that will go on
    // (lim < n), 15 bytes before it: a token is decided once 12 bytes of look-ahead are there,
    // a length nibble once 15 are (lzs-compression.c:641-647, 750-758).
    const uint32_t e = s + seg < lim ? s + seg : lim;
    WgJob job;
    job.src = in; job.n = n; job.cend = e;
    job.c0 = entry[k];
    // chains from a window before the first token: batches of 64, and one more so that HASH sees
    // the byte before the first position that matters
    const uint32_t c64 = job.c0 & ~63u;
    job.w0 = c64 > 2176u ? c64 - 2176u : 0u;
    job.last = false;
    job.out_len = nullptr; job.exit_pos = exit_pos + k; job.nbits = nbits + k;
    job.open_info = open_info ? open_info + 2 * k : nullptr;
    if (job.c0 >= e) {                                         // the segment before ran over all of this one
        if (threadIdx.x == 0) {
            exit_pos[k] = job.c0; nbits[k] = 0;
            if (open_info) { open_info[2 * k] = 0; open_info[2 * k + 1] = 0; }
        }
        return;
    }
    WgOut o;
    o.flushed = 0; o.cap = ~0u; o.aligned4 = true;
    if (!out) {
        // the usual case: the segment's bits fit its slot (they do unless a match runs on for more
        // than ~120 KB past the segment); if not, the stores stop there and the count goes on
        o.dst = slots + (size_t)k * slot_stride;               // 16-aligned by the host
        o.head = 0; o.limit = (uint32_t)slot_stride; o.ored = false;
    } else {
        // a segment that did not fit: once more, now that its bit offset is known, ORed straight
        // into the output (into the 256-byte granule its first bit falls in)
        const unsigned long long g = bit_at[k];
        o.dst = out + 256ull * (g >> 11);
        o.head = (uint32_t)(g & 2047ull); o.limit = ~0u; o.ored = true;
    }
    wg_compress_job(L, job, o);
}

// The same for the segments of MANY streams, the blocks of a batch (lzs_batch_compress.c; DESIGN.md 3.19): segment k belongs to
// block seg_block[k], which is the blk_len[b] bytes at in + blk_at[b] (64-bit: a batch may be longer than 4 GiB), and starts
// seg_start[k] bytes into it.  The job is the BLOCK's -- src its first byte, n its length, every position relative to it -- so the
// chains never reach before the block and no load goes past its end, whatever lies beside it in memory; the slot index stays
// global.  Every block is whole (no `lim`, no open match).  The second pass ORs into the block's own output, out + b out_stride
// (4-aligned), and stops where its capacity, rounded up to a word (cap4), ends: the next block's output may begin right there.
// (Instance 2 of wg_compress_job: the bounded form of the ORed stores is its alone.)
#ifdef LZS_WGV_WAVES
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(LZS_WGV_WAVES, LZS_WGV_WAVES)))
#else
__global__ __launch_bounds__(kWgThreads)
#endif
void lzs_compress_segments_batch_kernel(uint8_t *__restrict__ slots, size_t slot_stride,
                                        const uint8_t *__restrict__ in, const unsigned long long *__restrict__ blk_at,
                                        const uint32_t *__restrict__ blk_len, const uint32_t *__restrict__ seg_block,
                                        const uint32_t *__restrict__ seg_start, uint32_t seg, uint32_t nseg,
                                        const uint32_t *__restrict__ entry, const uint8_t *__restrict__ dirty,
                                        uint32_t *__restrict__ exit_pos, unsigned long long *__restrict__ nbits,
                                        uint8_t *__restrict__ out, size_t out_stride, uint32_t cap4,
                                        const unsigned long long *__restrict__ bit_at)
{
    __shared__ BlkLds L;
    const uint32_t k = blockIdx.x;
    if (k >= nseg) return;
    if (dirty && !dirty[k]) return;
    // (one load per table and workgroup, then scalars)
    const uint32_t b = uniform(seg_block[k]), s = uniform(seg_start[k]);
    const uint32_t n = uniform(blk_len[b]);
    const unsigned long long at0 = blk_at[b];
    const unsigned long long at = ((unsigned long long)uniform((uint32_t)(at0 >> 32)) << 32) | uniform((uint32_t)at0);
    const uint32_t e = n - s > seg ? s + seg : n;              // (s <= n by the table's construction)
    WgJob job;
    job.src = in + at; job.n = n; job.cend = e;
    job.c0 = uniform(entry[k]);
    const uint32_t c64 = job.c0 & ~63u;
    job.w0 = c64 > 2176u ? c64 - 2176u : 0u;                   // block coordinates: never from before the block
    job.last = false;
    job.out_len = nullptr; job.exit_pos = exit_pos + k; job.nbits = nbits + k;
    job.open_info = nullptr;
    if (job.c0 >= e) {                                         // the segment before ran over all of this one (or the block is empty)
        if (threadIdx.x == 0) { exit_pos[k] = job.c0; nbits[k] = 0; }
        return;
    }
    WgOut o;
    o.flushed = 0; o.cap = ~0u; o.aligned4 = true;
    if (!out) {
        o.dst = slots + (size_t)k * slot_stride;               // 16-aligned by the host
        o.head = 0; o.limit = (uint32_t)slot_stride; o.ored = false;
    } else {
        const unsigned long long g0 = bit_at[k];
        const unsigned long long g = ((unsigned long long)uniform((uint32_t)(g0 >> 32)) << 32) | uniform((uint32_t)g0);
        const unsigned long long first = 256ull * (g >> 11);   // the 256-byte granule its first bit falls in
        if (first >= cap4) return;                             // all of it lies behind the capacity: nothing to store
        o.dst = out + (size_t)b * out_stride + first;
        o.head = (uint32_t)(g & 2047ull); o.limit = cap4 - (uint32_t)first; o.ored = true;
    }
    wg_compress_job<2>(L, job, o);
}

#endif  // LZS_WGV_SEGMENTS

// Many channels, one packet each (include/lzs/lzs_channels.h, DESIGN.md 3.10): packet b is compressed on channel
// c = channel[b] as lzs_compress_incremental(add_end_marker) would on that channel's parameter block -- one job over the view
// [history | packet] with w0 = 0 (the chains are built over the history too), c0 = hlen (tokens start in the packet), the
// end marker at n.  Then the channel's history becomes the last min(2047, n) bytes of the view: read by every thread into the
// LDS ring (free once the job is done) BEFORE the barrier, written to the slot after it -- the new history overlaps the old.
#ifdef LZS_WGV_CHANNELS
#ifdef LZS_WGV_WAVES
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(LZS_WGV_WAVES, LZS_WGV_WAVES)))
#else
__global__ __launch_bounds__(kWgThreads)
#endif
void lzs_compress_channels_wg_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                     uint32_t *__restrict__ out_len,
                                     const uint8_t *__restrict__ in, size_t in_stride,
                                     const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                     const uint32_t *__restrict__ channel, uint8_t *__restrict__ states,
                                     uint8_t *__restrict__ status, uint32_t npackets)
{
    __shared__ BlkLds L;
    const uint32_t b = blockIdx.x;
    if (b >= npackets) return;
    const uint32_t ch = channel ? channel[b] : b;
    uint8_t *const st = states + (size_t)ch * kChanStateBytes;
    const uint32_t h = uniform(*reinterpret_cast<const uint32_t *>(st));
    const uint32_t len = in_len ? in_len[b] : in_len_uniform;
    if (h > kWindow) {                                         // not a state: nothing is written, nothing changes
        if (threadIdx.x == 0) { out_len[b] = 0; if (status) status[b] = 0x10u; }
        return;
    }
    WgJob job;
    job.src = in + (size_t)b * in_stride;
    job.hist = st + kChanHistAt; job.hlen = h;
    job.n = h + len;
    job.cend = job.n; job.c0 = h; job.w0 = 0; job.last = true;
    job.out_len = out_len + b; job.exit_pos = nullptr; job.nbits = nullptr; job.open_info = nullptr;
    job.status = status ? status + b : nullptr;
    WgOut o;
    o.flushed = 0; o.head = 0;
    o.dst = out + (size_t)b * out_stride;
    o.cap = out_cap;
    o.aligned4 = ((uintptr_t)o.dst & 3u) == 0;
    o.limit = out_cap; o.ored = false;
    wg_compress_job(L, job, o);
    // ---- the new history: hist[0, H) = view[n - H, n), hist[H, 2048) = 0 (the decoder writes the same bytes)
    __syncthreads();                                           // every read of the ring and of the old history is done
    const uint32_t H = job.n < kWindow ? job.n : kWindow, base = job.n - H;
    static_assert(kWgRingWords >= 512u && kWgThreads * 2u >= 512u, "the 2048 bytes of history are staged in the ring");
    for (uint32_t w = threadIdx.x; w < 512u; w += kWgThreads) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t i = 4u * w + k;
            if (i < H) v |= wg_view_byte(job, base + i) << (8u * k);
        }
        L.ring[w] = v;
    }
    __syncthreads();
    uint32_t *const hist = reinterpret_cast<uint32_t *>(st + kChanHistAt);
    for (uint32_t w = threadIdx.x; w < 512u; w += kWgThreads) hist[w] = L.ring[w];
    if (threadIdx.x == 0) *reinterpret_cast<uint32_t *>(st) = H;
}
// The same from PACKED packets to rooms (include/lzs/lzs_channels.h; DESIGN.md 3.15): packet b lies at in + in_off[b], its room at
// out + out_off[b] is its capacity and where its stores stop.  An entry that is not a block gets ERROR and length 0 before
// anything of it -- its channel's slot included -- is looked at.  (An entry of its own, as lzs_compress_packed_wg_kernel is.)
#ifdef LZS_WGV_WAVES
__global__ __launch_bounds__(kWgThreads) __attribute__((amdgpu_waves_per_eu(LZS_WGV_WAVES, LZS_WGV_WAVES)))
#else
__global__ __launch_bounds__(kWgThreads)
#endif
void lzs_compress_channels_packed_wg_kernel(uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_len,
                                            const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                            const uint32_t *__restrict__ in_len, const uint32_t *__restrict__ channel,
                                            uint8_t *__restrict__ states, uint8_t *__restrict__ status, uint32_t npackets)
{
    __shared__ BlkLds L;
    const uint32_t b = blockIdx.x;
    if (b >= npackets) return;
    uint64_t from, to;
    uint32_t len, room;
    if (!packed_entry(in_off, in_len, out_off, b, from, len, to, room)) {
        if (threadIdx.x == 0) { out_len[b] = 0; if (status) status[b] = 0x10u; }
        return;
    }
    const uint32_t ch = channel ? channel[b] : b;
    uint8_t *const st = states + (size_t)ch * kChanStateBytes;
    const uint32_t h = uniform(*reinterpret_cast<const uint32_t *>(st));
    if (h > kWindow) {                                         // not a state: nothing is written, nothing changes
        if (threadIdx.x == 0) { out_len[b] = 0; if (status) status[b] = 0x10u; }
        return;
    }
    WgJob job;
    job.src = in + from;
    job.hist = st + kChanHistAt; job.hlen = h;
    job.n = h + len;
    job.cend = job.n; job.c0 = h; job.w0 = 0; job.last = true;
    job.out_len = out_len + b; job.exit_pos = nullptr; job.nbits = nullptr; job.open_info = nullptr;
    job.status = status ? status + b : nullptr;
    WgOut o;
    o.flushed = 0; o.head = 0;
    o.dst = out + to;
    o.cap = room;
    o.aligned4 = ((uintptr_t)o.dst & 3u) == 0;
    o.limit = room; o.ored = false;
    wg_compress_job<1>(L, job, o);
    // ---- the new history: hist[0, H) = view[n - H, n), hist[H, 2048) = 0 (the decoder writes the same bytes)
    __syncthreads();                                           // every read of the ring and of the old history is done
    const uint32_t H = job.n < kWindow ? job.n : kWindow, base = job.n - H;
    static_assert(kWgRingWords >= 512u && kWgThreads * 2u >= 512u, "the 2048 bytes of history are staged in the ring");
    for (uint32_t w = threadIdx.x; w < 512u; w += kWgThreads) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t i = 4u * w + k;
            if (i < H) v |= wg_view_byte(job, base + i) << (8u * k);
        }
        L.ring[w] = v;
    }
    __syncthreads();
    uint32_t *const hist = reinterpret_cast<uint32_t *>(st + kChanHistAt);
    for (uint32_t w = threadIdx.x; w < 512u; w += kWgThreads) hist[w] = L.ring[w];
    if (threadIdx.x == 0) *reinterpret_cast<uint32_t *>(st) = H;
}
#endif  // LZS_WGV_CHANNELS

#undef LZS_WGV_HEAD3
#undef LZS_WGV_HEAD2
#undef LZS_WGV_SUBSTEPS
#undef LZS_WGV_HOPS
#undef LZS_WGV_HOP_END
#undef LZS_WGV_HOPS_LAST
#undef LZS_HOPS_HERE
#undef LZS_WGV_CHAIN_SAFE
#undef LZS_WGV_SEGMENTS
#undef LZS_WGV_CHANNELS
#undef LZS_WGV_PACK_BY_CHUNK
#undef LZS_WGV_PRIO
#undef LZS_WGV_LEAN
#undef LZS_WGV_NO3
#undef LZS_WGV_WAVES
#undef LZS_WGV_WG_WAVES
#undef LZS_WGV_HASH3_MUL
#undef LZS_WGV_HASH2_MUL
#undef LZS_WGV_POOL
#undef LZS_WGV_EXIT8
