// kernels/decompress_blocks.inc -- lzs_decompress() per block on the device.
// Part of lzs_kernels.hip (included there, inside its anonymous namespace); not a translation unit of its own.
//
// One decoder, lzs_decompress_blocks_grp, behind every block and channel entry point (the kernels at the end of this file and
// kernels/decompress_packed.inc): EIGHT STREAMS PER WAVEFRONT, 8 lanes each, and no scalar control flow inside a token.
// DESIGN.md 3.3 says how it came about and what it measures (144 / 463 / 147 GB/s of output on text / low-entropy /
// high-entropy blocks).
//
// A decoder that gives a wavefront to one stream is bound by the CU's one scalar unit (rocprofv3, round 1: 2.1e10 scalar
// instructions per GiB of text output, 87 % of its issue slots): every token is a trip through wave-uniform branches while
// 63 of the 64 lanes have nothing to do.  Here a group of 8 lanes owns a stream; its state (bit buffer, counts, offset, "a
// length nibble follows") is held redundantly in the registers of its lanes, and one trip of the loop decodes one step -- a
// run of up to 7 literals, a match token, or a length nibble -- for all eight groups at once, with every flag of the step a
// MASK (reference rules: lzs-decompression.c:189, 200, 217-233, 238-342, 346-406; the stop rules are those of the
// wave-per-stream decoders, test for test).  A match step copies at most 15 bytes: lane j of the group produces bytes j and
// j + 8, overlapping copies replicate with period `off` (index mod off from a per-lane table), sources before out[0] read as
// zero (the window starts as zeros).  Each group has its own 2304-byte output window in LDS (2047 + what waits to be
// drained), drained 128 bytes at a time with 16-byte stores (the wave branches there only when some group is due); the
// compressed words come 128 bytes per group at a time, a chunk ahead, and across the group's lanes by ds_bpermute.
// Measured on 1 GiB (MI355X) when it was new: 60 / 300 / 62 GB/s of output against 27 / 165 / 32 for one wavefront per
// stream (16 lanes per stream 36, 4 lanes 56).
//
// Round 1's two wave-per-stream decoders live in tools/variants/decompress_variants.inc and are compiled only into
// liblzs_variants.so (LZS_WITH_VARIANTS; LZS_DECODER=v1|v2 selects them there), as independent implementations of the same
// rules for the cross-checks of tests/test_gpu_parity.py.  The compare-and-select form of this decoder (rounds 2-4) and the
// four-lanes-a-stream experiment are gone: commit 36cad77 is the last that has them, profiles/r05/abdec_*.txt their numbers.
// reference lzs-decompression.c:156-412
// ---------------------------------------------------------------------------------
#ifdef LZS_WITH_VARIANTS
#include "decompress_variants.inc"
#endif

constexpr uint32_t kDecLanes  = 8;               // lanes per stream: two bytes of a step per lane
constexpr uint32_t kDecGroups = 64 / kDecLanes;  // streams per wavefront
#ifndef LZS_DEC_DRAIN
#define LZS_DEC_DRAIN 128
#endif
constexpr uint32_t kDecDrain  = LZS_DEC_DRAIN;   // finished output leaves in pieces of this size (16 B per lane and store)
constexpr uint32_t kDecPiece  = 16u * kDecLanes; // what one store of a group takes out
constexpr uint32_t kDecDrainStores = kDecDrain / kDecPiece;
// bytes of output window per stream: >= 2047 + kDecDrain + 15, a multiple of kDecPiece (no piece wraps inside itself)
constexpr uint32_t kDecRing   = (kWindow + kDecDrain + 15u + kDecPiece - 1u) / kDecPiece * kDecPiece;
static_assert(kDecDrain % kDecPiece == 0, "a drain is whole pieces");

struct __attribute__((aligned(16))) DecGroupLds {
    uint32_t ring[kDecGroups][kDecRing / 4];     // output windows
    uint32_t dummy[64];                          // where a lane with nothing to write stores
};

__device__ __forceinline__ uint32_t ffbh_u32(uint32_t x)      // leading zeros; 0xFFFFFFFF for 0
{
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// ---- flags as masks (0 or all ones) for the mask form of the decoder below.  What gfx950 charges for an instruction
// (tools/probes/valu_rates, profiles/r05/valu_rates.txt; two or more wavefronts per SIMD): add, subtract, and / or / xor,
// right shifts and the 16-bit minimum and maximum issue in 2 cycles, v_bitop3_b32 in 2.5 -- and every compare, every select
// (v_cndmask), the 32-bit minimum and maximum, left shifts, multiplies and the three-operand integer forms in 4.  A step
// written as compares and selects is half compares and selects; as masks a condition is a subtract and an arithmetic shift
// (or just the shift, for a bit of the token), masks combine in one bitop3, and a select is one bitop3.
// (the shift as assembly: from (x - y) >> 31 the compiler goes back to a compare and a select wherever it can prove the ranges)
__device__ __forceinline__ uint32_t m_sign(uint32_t x) { uint32_t r; asm("v_ashrrev_i32 %0, 31, %1" : "=v"(r) : "v"(x)); return r; }   // bit 31 as a mask
__device__ __forceinline__ uint32_t m_lt(uint32_t x, uint32_t y) { return m_sign(x - y); }      // x < y (both far below 2^31)
__device__ __forceinline__ uint32_t m_nz(uint32_t x) { return m_sign(0u - x); }                 // x != 0 (x < 2^31)
__device__ __forceinline__ uint32_t m_z(uint32_t x) { return m_sign(x - 1u); }                  // x == 0 (x < 2^31)
// (the truth tables: a = 0xF0, b = 0xCC, c = 0xAA)
__device__ __forceinline__ uint32_t m_sel(uint32_t m, uint32_t a, uint32_t b) { return __builtin_amdgcn_bitop3_b32(m, a, b, 0xCA); }   // m ? a : b, bit by bit
__device__ __forceinline__ uint32_t m_andnot(uint32_t a, uint32_t b) { return __builtin_amdgcn_bitop3_b32(a, b, b, 0x30); }          // a & ~b
__device__ __forceinline__ uint32_t m_nor(uint32_t a, uint32_t b) { return __builtin_amdgcn_bitop3_b32(a, b, b, 0x03); }             // ~(a | b)
__device__ __forceinline__ uint32_t m_ornot(uint32_t a, uint32_t b) { return __builtin_amdgcn_bitop3_b32(a, b, b, 0xF3); }           // a | ~b
__device__ __forceinline__ uint32_t twice(uint32_t x) { uint32_t r; asm("v_add_u32 %0, %1, %1" : "=v"(r) : "v"(x)); return r; }   // (x + x becomes a left shift otherwise: half rate)
// the 16-bit minimum and maximum (full rate; the operands' upper halves are ignored, the result's is zero on gfx9)
__device__ __forceinline__ uint32_t min16(uint32_t a, uint32_t b) { uint32_t r; asm("v_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ uint32_t max16i(uint32_t a, uint32_t b) { uint32_t r; asm("v_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// x mod kDecRing for x < 2 * kDecRing (wrap1) or x < 3 * kDecRing (wrap2): what is too small wraps around to something huge
// (in 16 bits: kDecRing and the sums are far below 2^16)
__device__ __forceinline__ uint32_t dec_wrap1(uint32_t x) { return min16(x, x - kDecRing); }
__device__ __forceinline__ uint32_t dec_wrap2(uint32_t x) { return min16(min16(x, x - kDecRing), x - 2u * kDecRing); }

typedef __attribute__((address_space(3))) uint8_t dec_lds_u8_t;
__device__ __forceinline__ uint32_t dec_lds_at(const void *p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p; }
__device__ __forceinline__ dec_lds_u8_t *dec_lds_byte(uint32_t at) { return (dec_lds_u8_t *)(uintptr_t)at; }

// CHAN (lzs_decompress_channels_grp_kernel): stream b is a packet of channel channel[b] (b if NULL) -- the channel's history is
// put into the part of the stream's window before output byte 0 (where the plain decoder reads zeros) and the last 2047 bytes
// of history | output go back to the state slot at the end.
struct DecChan {
    uint8_t *states = nullptr;
    const uint32_t *channel = nullptr;
    uint8_t *status = nullptr;
    // RUN (lzs_decompress_runs_grp_kernel, CHAN as well): stream b is a RUN of one channel's packets, decoded one after the
    // other in the same window.  The packets sorted by channel (skey / sidx: channel id -- nchannels for one out of range --
    // and packet at each sorted position); run b starts at sorted position run_at[b] and ends before run_end[run_at[b]];
    // run_key[b] == 0: there is no run b.  rt (calls with packet flags): a channel may have several runs -- one that starts
    // from a reset has an empty history whatever the slot holds, and only the channel's last run leaves a history (run_commit_to).
    const uint32_t *run_key = nullptr, *run_at = nullptr, *run_end = nullptr, *skey = nullptr, *sidx = nullptr;
    uint32_t nchannels = 0;
    RunTables rt;
};

// (CHAN) hist[0, H) of the state slot = the H window bytes before position cpos, hist[H, 2048) = 0 -- the bytes the compressor
// writes
__device__ __forceinline__ void dec_put_history(uint8_t *cst, const uint8_t *ring8, uint32_t cpos, uint32_t H, uint32_t j)
{
    uint32_t *hist = reinterpret_cast<uint32_t *>(cst + kChanHistAt);
    for (uint32_t w = j; w < 512u; w += kDecLanes) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t i = 4u * w + k;
            uint32_t r = cpos + kDecRing - H + i;
            r = r >= kDecRing ? r - kDecRing : r;
            if (i < H) v |= (uint32_t)ring8[r] << (8u * k);
        }
        hist[w] = v;
    }
}

// (RUN) 16 window bytes from any position a < kDecRing + kDecPiece, wrapping: a packet's output starts where the one before
// it ended, so its drains are not aligned to the window
__device__ __forceinline__ uint4 dec_ring_load16(const uint8_t *ring8, uint32_t a)
{
    a = a >= kDecRing ? a - kDecRing : a;
    const uint32_t *ring = reinterpret_cast<const uint32_t *>(ring8);
    const uint32_t s = a & 3u;
    uint32_t w = a >> 2, v[5];
#pragma unroll
    for (uint32_t k = 0; k < 5u; k++) { v[k] = ring[w]; w = w + 1u == kDecRing / 4u ? 0u : w + 1u; }
    return make_uint4(__builtin_amdgcn_alignbyte(v[1], v[0], s), __builtin_amdgcn_alignbyte(v[2], v[1], s),
                      __builtin_amdgcn_alignbyte(v[3], v[2], s), __builtin_amdgcn_alignbyte(v[4], v[3], s));
}

// (RUN) window position `start` + i, for i up to kDecRing
__device__ __forceinline__ uint32_t dec_ring_at(uint32_t start, uint32_t i)
{
    const uint32_t r = start + i;
    return r >= kDecRing ? r - kDecRing : r;
}

// PACKED (kernels/decompress_packed.inc; DESIGN.md 3.14): stream b lies at in + in_off[b] -- in_len[b] bytes, or up to
// in_off[b + 1] without lengths -- and decodes to out + out_off[b] with out_off[b + 1] - out_off[b] bytes of room.
struct DecPacked {
    const uint64_t *in_off = nullptr, *out_off = nullptr;
};

// (PACKED) entry b: where it lies, how long it is, where it goes and its room (a 64-bit difference, clamped).  False: not a
// block -- offsets that decrease, a length above LZS_BLOCK_MAX -- of which nothing is read or written.
__device__ __forceinline__ bool dec_packed_entry(const DecPacked &pk, const uint32_t *in_len, uint32_t b, uint64_t &from, uint32_t &n,
                                                 uint64_t &to, uint32_t &room)
{
    from = pk.in_off[b];
    to = pk.out_off[b];
    const uint64_t to_end = pk.out_off[b + 1u];
    bool ok = to_end >= to;
    uint64_t len;
    if (in_len) {
        len = in_len[b];
    } else {
        const uint64_t next = pk.in_off[b + 1u];
        ok = ok && next >= from;
        len = next - from;
    }
    ok = ok && len <= 0xC0000000ull;                               // LZS_BLOCK_MAX
    const uint64_t space = to_end - to;
    n = ok ? (uint32_t)len : 0u;
    room = ok ? (space < 0xFFFFFFFFull ? (uint32_t)space : 0xFFFFFFFFu) : 0u;
    return ok;
}

// (PACKED) the wavefront's input extent, from every group's first lane, as text for the two places of the decoder that need it (once
// per wavefront; RUN: once per trip): pk_lo = the lowest first word of the streams that have bytes (`act`; src and n are theirs),
// pk_rel = how far behind it this lane's stream's first word lies, pk_extent = where the last of them ends from there, pk_fits = that
// is a 32-bit extent.  No stream has bytes: an empty extent at 0, nothing is read.  (A function gives the kernels of
// kernels/decompress_packed.inc other instructions in the turn-taking path: profiles/r19/README.md.)
#define LZS_DEC_PACKED_EXTENT(act_) \
        const bool act = (act_); \
        const uint64_t first = (uint64_t)(uintptr_t)src & ~(uint64_t)3; \
        uint64_t lo = ~0ull, hi = 0; \
        _Pragma("unroll") \
        for (uint32_t gg = 0; gg < kDecGroups; gg++) { \
            const int at = (int)(gg * kDecLanes); \
            const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)(act ? 1u : 0u), at); \
            const uint64_t f = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(first >> 32), at) << 32) | \
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)first, at); \
            const uint64_t e = f + (uint32_t)__builtin_amdgcn_readlane((int)(((uint32_t)(uintptr_t)src & 3u) + n), at);   /* (3 + LZS_BLOCK_MAX fits) */ \
            if (a != 0u && f < lo) lo = f; \
            if (a != 0u && e > hi) hi = e; \
        } \
        if (hi == 0) lo = 0;                                       /* (no stream has bytes: an empty extent, nothing is read) */ \
        pk_lo = lo; \
        pk_fits = hi - lo <= 0xFFFF0000ull; \
        pk_rel = act ? (uint32_t)(first - lo) : 0u; \
        pk_extent = (uint32_t)(hi - lo);

// The decoder.  Its forms, picked per wavefront by what its streams' lengths say about them (the kernels below); a wavefront never
// changes form on the way:
// TWO: a second token in the same trip where that is possible.  Text is mostly short matches (3.4 bytes a token: one token a
// trip is 3.0 bytes a trip) and gains a quarter by it; high-entropy data (runs of seven literals) and long runs (nibble after
// nibble) lose 16 - 20 % to the extra instructions.  The second token is taken when the first is a run of literals or a whole
// match without extension, the next token is a match with a real offset whose bits are all there, both fit the trip's 16
// byte slots and the room, and the second copy reads nothing the first writes (offset >= both lengths together: no
// replication inside it either).  Otherwise it is simply the next trip's first token: nothing about it can stop a stream.
// WIDE: a 96-bit bit buffer fed with up to TWO words per trip (never across a 128-byte chunk).  A run of seven literals is 63
// bits and one word a trip is 32: on high-entropy data the loop was fed, not decoding -- 3.5 literals a trip.  Costs ~25
// instructions a trip: the form for streams that are longer than nine tenths of their output.
// The feed never masks the stream's last word: what follows the stream in it lies past `have` bits, is never joined by
// another word, and every rule of the step counts bits before it believes them (`need`).  A stream that is done may still be
// fed once or twice: nothing reads its buffer any more.
// CONCAT: the file rule -- after an end marker the pad bits up to the byte boundary are dropped and the next stream follows
// (compile time: the pad bits cost the one-shot rule nothing).  CHAN, RUN, PACKED: see DecChan and DecPacked above.
template <bool TWO, bool WIDE, bool CONCAT, bool CHAN = false, bool RUN = false, bool PACKED = false>
__device__ __forceinline__ void lzs_decompress_blocks_grp(DecGroupLds &L, uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                      uint32_t *__restrict__ out_len,
                                      const uint8_t *__restrict__ in, size_t in_stride,
                                      const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                      uint32_t nblocks, uint32_t concat_arg, uint32_t per_wave, DecChan ch = DecChan(),
                                      DecPacked pk = DecPacked())
{
    static_assert(CHAN || !RUN, "a run is a channel's");
    static_assert(!PACKED || !CONCAT, "packed streams are single blocks, single packets or the packets of a run");
    const uint32_t lane = threadIdx.x;
    const uint32_t g = lane / kDecLanes, j = lane % kDecLanes;
    const uint32_t b = blockIdx.x * per_wave + g;                  // per_wave: kDecGroups, or 1 (see the launcher)
    // the windows start as zeros: a copy from before out[0] reads a part of its window nothing has been written to
    // yet (it lies at most 2047 behind and the window is longer than 2047 + a step), which is the zero the rule asks for
    for (uint32_t i = lane; i < sizeof(L.ring) / 16u; i += 64u) reinterpret_cast<uint4 *>(&L.ring[0][0])[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    uint8_t *cst = nullptr;                                        // CHAN: the stream's state slot ...
    uint32_t hlen = 0;                                             // ... and its history's length (> 2047: not a state)
    uint32_t r_at = 0, r_end = 0;                                  // RUN: the run's sorted positions
    uint8_t *r_commit = nullptr;                                   // RUN: where its final history goes (null: nowhere)
    uint64_t pk_from = 0, pk_to = 0;                               // PACKED: the entry's offsets, its length and its room
    uint32_t pk_n = 0, pk_room = 0;
    bool pk_block = false;
    if constexpr (PACKED && !RUN) {
        if (b < nblocks) pk_block = dec_packed_entry(pk, in_len, b, pk_from, pk_n, pk_to, pk_room);
    }
    if constexpr (RUN) {
        if (b < nblocks && g < per_wave && ch.run_key[b] != 0u) {
            r_at = ch.run_at[b];
            r_end = ch.run_end[r_at];
            const uint32_t c = ch.skey[r_at];
            if (c < ch.nchannels) {
                cst = ch.states + (size_t)c * kChanStateBytes;
                hlen = run_is_fresh(ch.rt, r_at) ? 0u : *reinterpret_cast<const uint32_t *>(cst);
                r_commit = run_commit_to(ch.rt, ch.skey, r_at, r_end, nblocks, c, cst);
            }
        }
    } else if constexpr (CHAN) {
        if (b < nblocks && g < per_wave && (!PACKED || pk_block)) {
            cst = ch.states + (size_t)(ch.channel ? ch.channel[b] : b) * kChanStateBytes;
            hlen = *reinterpret_cast<const uint32_t *>(cst);
        }
    }
    // (RUN: `live` is the run's here -- a channel id in range, a state -- and the current packet's in the loop below)
    bool live = RUN ? (cst != nullptr && hlen <= kWindow) : (b < nblocks && g < per_wave && (!CHAN || hlen <= kWindow) && (!PACKED || pk_block));
    const bool live_run = live;
    uint32_t bb = live ? b : 0u;
    uint8_t *ring8 = reinterpret_cast<uint8_t *>(L.ring[g]);
    uint8_t *dummy8 = reinterpret_cast<uint8_t *>(&L.dummy[lane]);
    const uint8_t *src = PACKED ? in + pk_from : in + (size_t)bb * in_stride;
    uint32_t n   = live ? (PACKED ? pk_n : (in_len ? in_len[bb] : in_len_uniform)) : 0u;
    uint8_t *dst       = PACKED ? out + pk_to : out + (size_t)bb * out_stride;
    bool dst16   = ((uintptr_t)dst & 15u) == 0;
    uint32_t cap = live ? (PACKED ? pk_room : out_cap) : 0u;
    // PACKED: an entry that is not decoded -- not a block, or (CHAN) a slot that is not a state -- has length 0 and is an
    // ERROR; that is all that is written of it.  Then the wavefront's input extent: the descriptor of the loads below starts
    // at the lowest first word of the streams that have bytes (pk_lo) and each of them lies pk_rel behind it; where the last of
    // them ends more than 32 bits from there (pk_fits false) the groups take turns, one a trip of the loop below, each with a
    // descriptor of its own stream -- slow, and right.
    uint64_t pk_lo = 0;
    uint32_t pk_rel = 0, pk_extent = 0;
    bool pk_fits = true;
    if constexpr (PACKED && !RUN) {
        if (b < nblocks && !live && j == 0u) {
            out_len[b] = 0;
            if constexpr (CHAN) { if (ch.status) ch.status[b] = 0x10u; }
        }
        LZS_DEC_PACKED_EXTENT(live && n != 0u)
    }
    const bool live_all = live;
    if constexpr (RUN) {                                           // a run that is not decoded: every packet of it is an ERROR
        if (!live_run)
            for (uint32_t at = r_at + j; at < r_end; at += kDecLanes) {
                const uint32_t p = ch.sidx[at];
                out_len[p] = 0;
                if (ch.status) ch.status[p] = 0x10u;
            }
    }
    if constexpr (CHAN) {
        // history byte i is output byte i - hlen: window position kDecRing - hlen + i, which no output reaches before that
        // byte is more than 2047 behind (the argument of the zeros above)
        if (live) {
            const uint32_t *hist = reinterpret_cast<const uint32_t *>(cst + kChanHistAt);
            for (uint32_t w = j; w < 512u; w += kDecLanes) {
                const uint32_t v = hist[w];
                for (uint32_t k = 0; k < 4u; k++)
                    if (4u * w + k < hlen) ring8[kDecRing - hlen + 4u * w + k] = (uint8_t)(v >> (8u * k));
            }
        }
        __syncthreads();
    }

    // RUN: one trip of this loop per packet of the run (the k-th of every group's run side by side); the window and its
    // position carry over from packet to packet, the bit feed and the token state start afresh.  Otherwise one trip.
    uint32_t run_pos = 0;                                          // (RUN) the window position after the packets so far
    uint32_t produced = 0;                                         // (RUN) output of the run so far
    uint32_t pb = b;                                               // the packet
    // RUN && PACKED (lzs_decompress_runs_packed_grp_kernel; DESIGN.md 3.16): the packets of a trip are entries of the offset
    // arrays, and what PACKED decides once per wavefront is decided per trip -- the entries that are not blocks (ERROR, length 0,
    // nothing read or written, the window as it was), the extent, and where that is no 32-bit extent the groups' turns: trip rk
    // is then kDecGroups passes of this loop, group `turn` alone in each.
    uint32_t rk = 0, turn = 0, tk = 0;
    bool any_block = false;                                        // (RUN && PACKED) some packet of the run was a block
    for (uint32_t k = 0;; k++) {
        if constexpr (RUN && PACKED) {
            if (turn == 0u) {
                const uint32_t at = r_at + rk;
                const bool here = live_run && at < r_end;
                if (__builtin_amdgcn_ballot_w64(here) == 0ull) break;
                pb = here ? ch.sidx[at] : 0u;
                pk_block = here && dec_packed_entry(pk, in_len, pb, pk_from, pk_n, pk_to, pk_room);
                if (here && !pk_block && j == 0u) {
                    out_len[pb] = 0;
                    if (ch.status) ch.status[pb] = 0x10u;
                }
                if (!pk_block) { pk_from = 0; pk_to = 0; pk_n = 0u; pk_room = 0u; }
                any_block = any_block || pk_block;
                src = in + pk_from;
                dst = out + pk_to;
                dst16 = ((uintptr_t)dst & 15u) == 0;
                n = pk_n;
                LZS_DEC_PACKED_EXTENT(pk_block && pk_n != 0u)
            }
            tk = turn;
            live = pk_block && (pk_fits || g == tk);
            if (pk_fits || tk + 1u == kDecGroups) { rk++; turn = 0u; } else turn = tk + 1u;
            if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;
            n = live ? pk_n : 0u;
            cap = live ? pk_room : 0u;
        }
        if constexpr (PACKED && !RUN) {
            if (k > 0u && (pk_fits || k == kDecGroups)) break;
            if (!pk_fits) {                                            // (too far apart: group k alone)
                live = live_all && g == k;
                if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;
                n = live ? pk_n : 0u;
                cap = live ? pk_room : 0u;
            }
        }
        if constexpr (RUN && !PACKED) {
            const uint32_t at = r_at + k;
            live = live_run && at < r_end;
            if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
            pb = live ? ch.sidx[at] : 0u;
            bb = pb;
            src = in + (size_t)bb * in_stride;
            n = live ? (in_len ? in_len[bb] : in_len_uniform) : 0u;
            dst = out + (size_t)bb * out_stride;
            dst16 = ((uintptr_t)dst & 15u) == 0;
            cap = live ? out_cap : 0u;
        }

        // ---- the input as aligned words: word k holds stream bytes [4k - skew, 4k - skew + 4).  A
        // group takes 16 x kDecLanes bytes at a time: lane j holds words 4j .. 4j + 3 of the current
        // chunk (one coalesced load for the group) and of the next one, requested a chunk ahead; the
        // word the group feeds next comes across the lanes (ds_bpermute), fetched a step before it is
        // used.  (Sixteen bytes at a time in every lane meant a load every other step somewhere in
        // the wavefront, and the wave waited ~1 us for each.)  The loads are BUFFER loads bounded by
        // the end of the last of the wavefront's streams: past it they return zeros instead of
        // faulting, so the end of a stream is no special case (what lies past it is never fed: `rem`
        // below), and lanes that do not move on load what they have again -- one load instruction for
        // the whole wavefront, not waited for until the chunk is needed.
        const uint32_t skew = (uint32_t)((uintptr_t)src & 3u);
        const uint32_t b0 = blockIdx.x * per_wave;
        // (RUN: the packets of a trip lie anywhere in the input -- the launcher sees to it that all of it is one 32-bit extent, or
        // gives each wavefront one run)
        const uint8_t *wave_in = PACKED ? nullptr : (RUN ? (per_wave == 1u ? src : in) : in + (size_t)b0 * in_stride);
        uintptr_t in_lo = (uintptr_t)wave_in & ~(uintptr_t)3;
        const uint32_t rel = live ? (uint32_t)(RUN ? (per_wave == 1u ? (size_t)0 : (size_t)pb * in_stride) : (size_t)(b - b0) * in_stride) : 0u;      // my stream, from wave_in
        uint32_t wave_end = 0;
        // (PACKED) where my stream's first word lies from in_lo, and the end of the last word that holds a byte of it: a lane loads
        // nothing outside its own stream's words (see bload)
        uint32_t pk_at = 0, pk_end = 0;
        if constexpr (PACKED) {
            if (pk_fits) {
                in_lo = (uintptr_t)pk_lo;
                wave_end = pk_extent;
                pk_at = pk_rel;
            } else {                                                   // group k's stream alone (RUN: group tk's)
                const int at = (int)(((RUN && PACKED) ? tk : k) * kDecLanes);
                const uintptr_t first = (uintptr_t)src & ~(uintptr_t)3;
                in_lo = (uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)first >> 32), at) << 32) |
                                    (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)first, at));
                wave_end = (uint32_t)__builtin_amdgcn_readlane((int)(skew + n), at);
            }
            pk_end = n != 0u ? (pk_at + skew + n + 3u) & ~3u : 0u;
        } else {
#pragma unroll
        for (uint32_t gg = 0; gg < kDecGroups; gg++) {
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)(rel + n), (int)(gg * kDecLanes));
            wave_end = e > wave_end ? e : wave_end;
        }
        }
        // (the descriptor is the same in every lane, and said to be: or the load sits in a loop over the distinct ones)
        const uintptr_t in_lo_u = ((uintptr_t)uniform((uint32_t)((uint64_t)in_lo >> 32)) << 32) | uniform((uint32_t)in_lo);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void *)in_lo_u, 0, (int)uniform((wave_end + (uint32_t)((uintptr_t)wave_in & 3u) + 3u) & ~3u), 0x00020000);
        const auto bload = [&](uint32_t byte_off) {
            if constexpr (PACKED) {
                // sixteen bytes that lie in the lane's own stream's words as one load; what lies past them altogether from an
                // offset past every extent (zeros, and no access); the piece the stream ends in word by word, where some lane is there
                const bool whole = byte_off + 16u <= pk_end;
                u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(whole ? byte_off : 0xFFFFFFF0u), 0, 0);
                const bool part = !whole && byte_off < pk_end;
                if (__builtin_amdgcn_ballot_w64(part) != 0ull) {
                    if (part) {
                        v.x = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)byte_off, 0, 0);
                        if (byte_off + 4u < pk_end) v.y = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)(byte_off + 4u), 0, 0);
                        if (byte_off + 8u < pk_end) v.z = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)(byte_off + 8u), 0, 0);
                    }
                }
                return make_uint4(v.x, v.y, v.z, v.w);
            } else {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0);
            return make_uint4(v.x, v.y, v.z, v.w);
            }
        };
        constexpr uint32_t kChunk = 16u * kDecLanes;                    // bytes
        uint32_t nxt_off = (PACKED ? pk_at : (uint32_t)((uintptr_t)(src - skew) - in_lo)) + 16u * j + kChunk;
        uint4 cur = bload(nxt_off - kChunk), nxt = bload(nxt_off);
        const uint32_t glane4 = (lane & ~(kDecLanes - 1u)) << 2;       // byte index of the group's lane 0 for ds_bpermute
        // A lane's four words ROTATE by one with every word its group takes, so that the word to feed next (word wi of the
        // stream) is always in cur.x of lane (wi / 4) mod 8, and the one after it in cur.y of the lane that holds that:
        // one address and one ds_bpermute a trip, no select on wi as well.  (32 words to a chunk: the next chunk moves
        // in when the rotation is back at 0.)
        const auto rotate = [&](uint32_t on) {
            const uint32_t x0 = cur.x;
            cur.x = on ? cur.y : cur.x; cur.y = on ? cur.z : cur.y; cur.z = on ? cur.w : cur.z; cur.w = on ? x0 : cur.w;
        };
        static_assert(kChunk == 16u * kDecLanes, "a lane holds four words of the chunk");
        const auto fetch = [&](uint32_t wi_) {
            return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(glane4 + (wi_ & (4u * kDecLanes - 4u))), (int)cur.x);
        };
        const auto fetch_after = [&](uint32_t wi_) {
            return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(glane4 + ((wi_ + 1u) & (4u * kDecLanes - 4u))), (int)cur.y);
        };
        uint64_t bits = 0;        // left-aligned bit buffer
        uint32_t have = 0;        // valid bits in it
        uint32_t left = n;        // bytes of the stream not fed yet
        uint32_t wi   = 0;        // next word to feed
        {
            const uint32_t first = fetch(0);
            if (n) {
                uint32_t w = __builtin_bswap32(first) << (8u * skew);
                const uint32_t avail = 4u - skew < n ? 4u - skew : n;
                if (avail < 4u) w &= ~0u << (32u - 8u * avail);
                bits = (uint64_t)w << 32;
                have = 8u * avail;
                left = n - avail;
                wi = 1;
            }
        }
        rotate(wi);
        uint32_t nextw = fetch(wi);
        uint32_t nextw2 = WIDE ? fetch_after(wi) : 0u;                 // (WIDE: the word after it; only used when in the same chunk)
        uint32_t bits_lo = 0;                                          // (WIDE: bits 64..95 of the buffer, left-aligned)
        // PACKED: a stream's output starts anywhere, fifteen times in sixteen off a 16-byte boundary, where the drain below would
        // store byte by byte.  So the drains start at the first boundary of dst, `head` bytes in: every piece is an aligned store
        // fed from the window at an unaligned position (dec_ring_load16), and the head bytes go out byte by byte with the first
        // drain, or with the tail if there is none.  (-DLZS_PACKED_BYTE_DRAIN: the strided calls' drain, for the measurement.)
#ifdef LZS_PACKED_BYTE_DRAIN
        constexpr bool kPackedHead = false;
#else
        constexpr bool kPackedHead = PACKED;
#endif
        const uint32_t head = kPackedHead ? (0u - (uint32_t)(uintptr_t)dst) & 15u : 0u;
        uint32_t head_left = head;
        uint32_t count = 0, flushed = head, off = 0;
        uint32_t m_ext = 0;                                            // "a length nibble follows", as a mask
        // (RUN: the packet's output starts at window position run_pos, its head bytes lie from there on)
        const uint32_t head_pos = (RUN && kPackedHead) ? dec_ring_at(run_pos, head) : 0u;
        uint32_t cpos = RUN ? run_pos : 0u, fpos = RUN ? (kPackedHead ? head_pos : run_pos) : head;  // count and flushed modulo kDecRing
        const uint32_t fpos0 = cpos;                                   // (where the packet's output starts in the window)
        uint32_t m_done = live ? 0u : ~0u;                             // the stream has stopped, as a mask
        uint32_t m_eos = 0u;                                           // (CHAN) ... at an end marker
        uint32_t m_cut = 0u;                                           // (CHAN) a copy lost bytes to the room: no end marker counts after it
        // overlapping copies replicate with period off: byte idx of a step comes from byte idx mod off.  Lane j's
        // bytes are j and j + 8: a 3-bit entry per off = 0 .. 8 (0 and 8 and more: j itself), a 4-bit one per off = 0 .. 15
        uint32_t mod_lo = 0; uint64_t mod_hi = 0;
        // (mod_tab: what is left of the four-lane tables, read by nothing.  Taking it out leaves every instruction as it is
        // and moves the order of this set-up's in six kernels, which then have to be measured: profiles/r12/decoder_refactor.txt)
        uint64_t mod_tab[2];
        if (kDecLanes == 8u) {
#pragma unroll
            for (uint32_t e = 0; e <= 8u; e++) mod_lo |= ((e == 0u || e == 8u) ? j : j % (e ? e : 1u)) << (3u * e);
#pragma unroll
            for (uint32_t e = 0; e < 16u; e++) mod_hi |= (uint64_t)(e == 0u ? j + 8u : (j + 8u) % (e ? e : 1u)) << (4u * e);
        }
#pragma unroll
        for (uint32_t sl = 0; sl < 2u; sl++) {
            mod_tab[sl] = 0;
#pragma unroll
            for (uint32_t e = 0; e < 16u; e++) mod_tab[sl] |= (uint64_t)(e == 0u ? j + kDecLanes * sl : (j + kDecLanes * sl) % (e ? e : 1u)) << (4u * e);
        }

        // per-lane constants of the loop
        const uint32_t lit_shift = 55u - 9u * (j < 7u ? j : 6u);      // where byte j of a run of literals sits in the bit buffer
        const uint32_t ring_at = dec_lds_at(ring8), dummy_at = dec_lds_at(dummy8);   // (LDS addresses as numbers: a select between them is one bitop3)
        for (;;) {
            if (__builtin_amdgcn_ballot_w64(m_done == 0u) == 0ull) break;
            // ---- refill (:181-187): one word per step keeps more than a token's worth in the buffer (the last word is not
            // masked and a stream that is done may still be fed: see the header)
            if (!WIDE) {
                const uint32_t nb4 = min(left, 4u);                    // (left may be anything up to LZS_BLOCK_MAX -- no m_nz of it --; this is 0 .. 4)
                const uint32_t m_rf = m_lt(have, 33u) & m_nz(nb4);
                const uint32_t nb = nb4 & m_rf;                        // bytes taken
                const uint32_t w = __builtin_bswap32(nextw) & m_rf;
                bits |= (uint64_t)w << ((32u - have) & 63u);
                have = (nb << 3) + have;
                left -= nb;
                wi   -= m_rf;                                          // (+ 1 where the mask is -1)
                const uint32_t x0 = cur.x;
                cur.x = m_sel(m_rf, cur.y, cur.x); cur.y = m_sel(m_rf, cur.z, cur.y); cur.z = m_sel(m_rf, cur.w, cur.z); cur.w = m_sel(m_rf, x0, cur.w);
                // the chunk is used up: the next one moves in, the one after is requested
                const uint32_t not_roll = m_ornot(wi & (4u * kDecLanes - 1u), m_rf);   // 0 where a word was taken and it was the chunk's last
                if (__builtin_amdgcn_ballot_w64(not_roll == 0u) != 0ull) {
                    const bool roll = not_roll == 0u;
                    cur.x = roll ? nxt.x : cur.x; cur.y = roll ? nxt.y : cur.y;
                    cur.z = roll ? nxt.z : cur.z; cur.w = roll ? nxt.w : cur.w;
                    nxt_off = roll ? nxt_off + kChunk : nxt_off;
                    nxt = bload(nxt_off);
                }
                nextw = fetch(wi);
            } else {
                // two words where 64 bits or fewer are left (the second only from the same chunk: its copy was fetched a trip ago
                // like the first's); the buffer is bits : bits_lo, 96 bits.  As masks too: a word that is not taken is a word of
                // zeros OR-ed in, so nothing of the buffer needs a select.
                uint32_t m_took = 0u;
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const uint32_t nb4 = min(left, 4u);                // (left may be anything up to LZS_BLOCK_MAX; this is 0 .. 4)
                    uint32_t m_rf = m_lt(have, 65u) & m_nz(nb4);
                    if (r == 1) m_rf &= m_took & m_nz(wi & (4u * kDecLanes - 1u));   // the second only after the first, and from the same chunk
                    m_took = m_rf;
                    const uint32_t w = __builtin_bswap32(r == 0 ? nextw : nextw2) & m_rf;     // (the stream's last word not masked)
                    const uint32_t nb = nb4 & m_rf;                    // bytes taken
                    // w at bit offset `have` (0 .. 64) of the 96: its part in the upper 64 bits and what falls below them
                    const uint64_t hi = ((uint64_t)w << 32) >> (have & 63u);           // (have = 64: all of it falls below)
                    const uint32_t keep_hi = m_lt(have, 64u);
                    const uint32_t lo = (uint32_t)((uint64_t)w << ((64u - have) & 63u)) & m_lt(32u, have);
                    bits    |= hi & (((uint64_t)keep_hi << 32) | keep_hi);
                    bits_lo |= lo;
                    have += nb << 3;
                    left -= nb;
                    wi   -= m_rf;                                      // (+ 1 where the mask is -1)
                    const uint32_t x0 = cur.x;
                    cur.x = m_sel(m_rf, cur.y, cur.x); cur.y = m_sel(m_rf, cur.z, cur.y); cur.z = m_sel(m_rf, cur.w, cur.z); cur.w = m_sel(m_rf, x0, cur.w);
                    const uint32_t not_roll = m_ornot(wi & (4u * kDecLanes - 1u), m_rf);   // 0 where a word was taken and it was the chunk's last
                    if (__builtin_amdgcn_ballot_w64(not_roll == 0u) != 0ull) {
                        const bool roll = not_roll == 0u;
                        cur.x = roll ? nxt.x : cur.x; cur.y = roll ? nxt.y : cur.y;
                        cur.z = roll ? nxt.z : cur.z; cur.w = roll ? nxt.w : cur.w;
                        nxt_off = roll ? nxt_off + kChunk : nxt_off;
                        nxt = bload(nxt_off);
                    }
                }
                nextw = fetch(wi);
                nextw2 = fetch_after(wi);
            }
            const uint32_t room = min(cap - count, 255u);              // (all that is asked of it: is it 0, is it less than a step)
            const uint32_t top = (uint32_t)(bits >> 32);

            // ---- the three kinds of step, side by side
            const uint32_t m_t31 = m_sign(top);
            const uint32_t m_lit = m_nor(m_t31, m_ext);               // a run of literals
            const uint32_t m_mat = m_andnot(m_t31, m_ext);            // a match token
            const uint32_t e = top >> 28;                              // a length nibble (:370-406)
            // a run of literals (:217-233): token i of an all-literal run starts at bit 63 - 9i
            uint32_t kv;
            if (TWO) {                                                 // four a trip at most, counted in the upper word
                kv = min16(ffbh_u32(top & 0x80402010u), 36u) >> 3;     // 0 9 18 27 36 leading zeros: 0 1 2 3 4 literals
            } else {
                const uint32_t lead_hi = ffbh_u32(top & 0x80402010u), lead_lo = ffbh_u32((uint32_t)bits & 0x08040200u) | 32u;
                kv = min16(min16(lead_hi, lead_lo), 63u) >> 3;         // 0 9 .. 54, or none (ffbh of 0 is all ones: 0xFFFF in 16 bits): 0 .. 7 literals
            }
            kv = min16(min16(kv, __umul24(have, 57u) >> 9), room);     // no more than the bits that are there (have / 9) and the room
            // a match token: 1 s ooooooo[oooo] cccc (:238-342)
            const uint32_t m_short = m_sign(twice(top));
            const uint32_t short4 = m_short & 4u;
            const uint32_t norm = (top & 0x3FFFFFFFu) >> short4;
            const uint32_t o = norm >> 19;
            const uint32_t code = (norm >> 15) & 0xFu;
            const uint32_t len = max16i(((norm >> 17) & 3u) + 2u, code - 7u);          // 2 2 2 2 3 3 3 3 4 4 4 4 5 6 7 8
            const uint32_t used = 13u - short4;
            const uint32_t width = 4u - (m_lt(code, 12u) & 2u);
            const uint32_t m_zoff = m_z(o);
            const uint32_t m_copying = m_andnot(m_mat, m_zoff);       // a match token with a real offset
            // bits the step needs; short of them it stops for good (:222, 240, 250, 274, 334, 375)
            const uint32_t need_mat = used + m_andnot(width, m_zoff);
            const uint32_t need = m_sel(m_ext, 4u, m_sel(m_lit, 9u, need_mat));
            // :189 (no bits: every step needs four at least), :200 and mid-copy :361-364 (no room), and the token's own stops
            const uint32_t m_stop = m_lt(have, need) | m_z(room);
            const uint32_t m_go = m_nor(m_done, m_stop);
            const uint32_t m_endm = m_mat & m_zoff & m_short;         // end marker (:255-260 / file rule :564-576)
            // (CHAN) the end marker is reached; it needs no room, so a full output may end at it -- also behind the closing
            // length nibble 0 of a copy that filled the output.  Not after a copy the room cut short (m_cut): its token was
            // consumed whole but not all of its bytes were written, so the output is not the packet's
            if constexpr (CHAN) {
                const uint32_t m_nib0_end = m_ext & m_z(e) & m_z(((top << 4) >> 23) ^ 0x180u) & ~m_lt(have, 13u);
                m_eos |= m_andnot((m_endm & ~m_lt(have, 9u)) | m_nib0_end, m_done | m_cut);
            }
            uint32_t consume = m_sel(m_lit, (kv << 3) + kv, need);
            // file rule: after an end marker drop the pad bits up to the byte boundary and go on
            if (CONCAT) consume += m_endm & ((have - used) & 7u);
            const uint32_t copy_len = m_sel(m_ext, e, len & m_copying);
            const uint32_t off_now = m_sel(m_copying, o, off);
            // long offset 0: no copy, and the offset register is cleared (:280); an end marker leaves it
            const uint32_t off_next = m_andnot(off_now, m_andnot(m_mat & m_zoff, m_short));
            const uint32_t m_ext_next = m_sel(m_ext, m_lt(14u, e), m_copying & m_lt(7u, len));
            const uint32_t m = min16(copy_len, room);
            if constexpr (CHAN) m_cut |= m_andnot(m_go, m_lit) & m_lt(m, copy_len);   // (a run of literals is cut unread, a copy is not)
            const uint32_t nA = m_sel(m_lit, kv, m) & m_go;           // bytes of this step's (first) token
            // ---- TWO: a second token in the same trip (the header says when; two of its conditions follow
            // from the others -- a second offset of 0 cannot be >= both lengths together, and a first copy cut by the room
            // leaves no room for a second)
            uint32_t m_okB = 0u, nB = 0u, oB = 0u, lenB = 0u, needB = 0u;
            if (TWO) {
                const uint32_t topB = (uint32_t)((bits << (consume & 63u)) >> 32);
                const uint32_t haveB = have - consume;                 // (meaningless unless go)
                const uint32_t m_shortB = m_sign(twice(topB));
                const uint32_t short4B = m_shortB & 4u;
                const uint32_t normB = (topB & 0x3FFFFFFFu) >> short4B;
                oB = normB >> 19;
                const uint32_t codeB = (normB >> 15) & 0xFu;
                lenB = max16i(((normB >> 17) & 3u) + 2u, codeB - 7u);
                needB = 17u - (m_lt(codeB, 12u) & 2u) - short4B;
                const uint32_t m_firstA = (m_lit | m_andnot(m_copying, m_ext_next)) & m_go;
                const uint32_t both = nA + lenB;
#ifndef LZS_DEC_TWO_MAX
#define LZS_DEC_TWO_MAX 16
#endif
                const uint32_t lim = min16(min16(oB, (uint32_t)LZS_DEC_TWO_MAX), room);      // both <= 16, <= room, <= oB (so oB is not 0)
                m_okB = m_firstA & m_sign(topB) & m_nor(m_lt(haveB, needB), m_lt(lim, both));
                nB = lenB & m_okB;
            }
            const uint32_t nwrite = nA + nB;

            // ---- lane j of the group produces byte j of the step, and byte j + 8; overlap replicates with period off
#pragma unroll
            for (uint32_t sl = 0; sl < 2u; sl++) {
                if (sl > 0u && __builtin_amdgcn_ballot_w64(nwrite > 8u) == 0ull) break;
                const uint32_t idx = j + 8u * sl;                      // byte of the step
                // idx mod off from the lane's table (idx itself for off 0 and for off > idx)
                uint32_t k1;
                if (sl == 0u) { const uint32_t o8 = min16(off_now, 8u); k1 = (mod_lo >> (o8 + o8 + o8)) & 7u; }
                else          k1 = off_now < 16u ? (uint32_t)(mod_hi >> (4u * (off_now & 15u))) & 15u : idx;
                uint32_t k = k1, oo = off_now, m_second = 0u;
                if (TWO) {                                             // a byte past the first token is the second's: no replication there
                    m_second = ~m_lt(idx, nA);
                    k = m_sel(m_second, idx, k1);
                    oo = m_sel(m_second, oB, off_now);
                }
                // source: position count + k - off (a part of the window nothing has been written to reads as the zero the rule asks for)
                const uint32_t sx = cpos + k + (kDecRing - oo);        // < 2 * kDecRing + 15
                const uint32_t sp = dec_wrap2(sx);
                const uint32_t copied = *dec_lds_byte(ring_at + sp);
                const uint32_t wx = cpos + idx;
                const uint32_t wp = dec_wrap1(wx);
                dec_lds_u8_t *const to = dec_lds_byte(m_sel(m_lt(idx, nwrite), ring_at + wp, dummy_at));
                uint32_t val = copied;
                if (sl == 0u) {                                        // (this slot can hold a literal of a run)
                    const uint32_t lit = (uint32_t)(bits >> lit_shift) & 0xFFu;
                    val = m_sel(m_andnot(m_lit, m_second), lit, copied);
                }
                *to = (uint8_t)val;
            }

            count = count + nwrite;
            cpos = dec_wrap1(cpos + nwrite);
            // (a stream that has stopped writes nothing any more, so what happens to its buffer, offset and flags from here on is
            // nobody's business: no selects to keep them)
            const uint32_t shift = consume + (needB & m_okB);          // (<= 36 + 17: one shift for both tokens)
            if (WIDE) {                                                // (never with TWO) 96 bits move up by `consume` < 64
                const uint32_t cs = consume & 63u;
                const uint64_t lo64 = (uint64_t)bits_lo << 32;
                const uint32_t m_cs = m_nz(cs);                        // (a shift by 64 - 0 would be a shift by 0)
                const uint64_t carry = (lo64 >> ((64u - cs) & 63u)) & (((uint64_t)m_cs << 32) | m_cs);
                bits = (bits << cs) | carry;
                bits_lo = (uint32_t)((lo64 << cs) >> 32);
            } else {
                bits <<= (shift & 63u);
            }
            have  -= shift;
            off    = TWO ? m_sel(m_okB, oB, off_next) : off_next;
            m_ext  = TWO ? m_sel(m_okB, m_lt(7u, lenB), m_ext_next) : m_ext_next;
            m_done |= m_stop | (CONCAT ? 0u : m_endm);

            // ---- drain finished output, 16 bytes per lane at a time (the wave goes there when some group is due)
            const bool due = kPackedHead ? (count - flushed >= kDecDrain && count >= flushed) : count - flushed >= kDecDrain;
            if (__builtin_amdgcn_ballot_w64(due) != 0ull) {
                if (due) {
                    if constexpr (kPackedHead) {                       // (the first drain: the window has not wrapped yet)
                        for (uint32_t i = j; i < head_left; i += kDecLanes) dst[i] = ring8[RUN ? dec_ring_at(fpos0, i) : i];
                        head_left = 0;
                    }
#pragma unroll
                    for (uint32_t piece = 0; piece < kDecDrainStores; piece++) {
                        const uint32_t p = flushed + kDecPiece * piece + 16u * j;
                        uint32_t fp = fpos + kDecPiece * piece;
                        fp = fp >= kDecRing ? fp - kDecRing : fp;
                        uint4 v;
                        if constexpr (RUN || kPackedHead) v = dec_ring_load16(ring8, fp + 16u * j);
                        else v = *reinterpret_cast<const uint4 *>(ring8 + fp + 16u * j);
                        if (kPackedHead || dst16) {
                            *reinterpret_cast<uint4 *>(dst + p) = v;
                        } else {
                            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                            for (uint32_t t = 0; t < 16; t++) dst[p + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
                        }
                    }
                    flushed += kDecDrain;
                    fpos = fpos + kDecDrain >= kDecRing ? fpos + kDecDrain - kDecRing : fpos + kDecDrain;
                }
            }
        }

        if constexpr (kPackedHead) {                                   // (no drain took them: the window has not wrapped)
            for (uint32_t i = j; i < (head_left < count ? head_left : count); i += kDecLanes) dst[i] = ring8[RUN ? dec_ring_at(fpos0, i) : i];
        }
        for (uint32_t i = flushed + j; i < count; i += kDecLanes) {
            uint32_t r = fpos + (i - flushed);
            r = r >= kDecRing ? r - kDecRing : r;
            dst[i] = ring8[r];
        }
        if (live && j == 0u) out_len[pb] = count;
        if constexpr (RUN) {
            if (live && j == 0u && ch.status) ch.status[pb] = (uint8_t)(m_eos ? 0x04u : (count >= cap ? 0x08u : 0x03u));
            produced += live ? count : 0u;
            run_pos = cpos;
        } else if constexpr (CHAN) {
            if (live) {
                // the new history: hist[0, H) = the last H bytes of history | output (output byte count - H + i is at window
                // position cpos - H + i), hist[H, 2048) = 0 -- the bytes the compressor writes
                const uint32_t H = min(hlen + count, kWindow);
                dec_put_history(cst, ring8, cpos, H, j);
                if (j == 0u) {
                    *reinterpret_cast<uint32_t *>(cst) = H;
                    if (ch.status) ch.status[b] = (uint8_t)(m_eos ? 0x04u : (count >= cap ? 0x08u : 0x03u));
                }
            } else if (!PACKED && cst && j == 0u) {                    // not a state: nothing is written, nothing changes
                out_len[b] = 0;
                if (ch.status) ch.status[b] = 0x10u;
            }
        }
        if constexpr (!RUN && !PACKED) break;
    }
    // (RUN) the run's history goes back once, at its end (PACKED: not if no packet of the run was a block -- the slot stays as it is,
    // byte for byte, as after the packed calls rank by rank, which look at no slot for such entries)
    if constexpr (RUN) {
        if (live_run && r_commit != nullptr && (!PACKED || any_block)) {
            const uint32_t H = min(hlen + produced, kWindow);
            dec_put_history(r_commit, ring8, run_pos, H, j);
            if (j == 0u) *reinterpret_cast<uint32_t *>(r_commit) = H;
        }
    }
}

template <bool CONCAT>
__global__ __launch_bounds__(64)
void lzs_decompress_blocks_grp_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                      uint32_t *__restrict__ out_len,
                                      const uint8_t *__restrict__ in, size_t in_stride,
                                      const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                      uint32_t nblocks, uint32_t concat, uint32_t per_wave)
{
    __shared__ DecGroupLds L;
    // Compressed bytes of this wavefront's streams against the output they may fill: between a
    // quarter and nine tenths is the range of short matches (text: 0.57), where a second token per
    // trip pays; above it literals dominate (high entropy: 1.11, a slot-sized stride given as the
    // length: 1.125), below it long runs (0.04).
    // (64-bit: a block may be up to LZS_BLOCK_MAX long and a slot close to 4 GiB -- ADVICE r03)
    uint64_t total = 0, blocks = 0;
    const uint32_t b0 = blockIdx.x * per_wave;
    for (uint32_t g = 0; g < per_wave && b0 + g < nblocks; g++) {
        total += in_len ? in_len[b0 + g] : in_len_uniform;
        blocks++;
    }
    const uint64_t full = blocks * (uint64_t)out_cap;
    const bool two = uniform((4ull * total > full && 10ull * total < 9ull * full) ? 1u : 0u) != 0u;
    const bool wide = uniform(10ull * total >= 9ull * full ? 1u : 0u) != 0u;      // literals dominate: the 96-bit buffer
#ifdef LZS_DEC_ONE_TOKEN
    lzs_decompress_blocks_grp<false, false, CONCAT>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, nblocks, concat, per_wave);
#else
    if (two)       lzs_decompress_blocks_grp<true, false, CONCAT>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, nblocks, concat, per_wave);
    else if (wide) lzs_decompress_blocks_grp<false, true, CONCAT>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, nblocks, concat, per_wave);
    else           lzs_decompress_blocks_grp<false, false, CONCAT>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, nblocks, concat, per_wave);
#endif
}

// Many channels, one packet each (include/lzs/lzs_channels.h, DESIGN.md 3.10): lzs_decompress_blocks_grp_kernel<false> with every
// stream's window starting with its channel's history, and the history carried back.
__global__ __launch_bounds__(64)
void lzs_decompress_channels_grp_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                        uint32_t *__restrict__ out_len,
                                        const uint8_t *__restrict__ in, size_t in_stride,
                                        const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                        const uint32_t *__restrict__ channel, uint8_t *__restrict__ states,
                                        uint8_t *__restrict__ status, uint32_t npackets, uint32_t per_wave)
{
    __shared__ DecGroupLds L;
    // (the form by the wavefront's ratio of input to room, as lzs_decompress_blocks_grp_kernel picks it)
    uint64_t total = 0, blocks = 0;
    const uint32_t b0 = blockIdx.x * per_wave;
    for (uint32_t g = 0; g < per_wave && b0 + g < npackets; g++) {
        total += in_len ? in_len[b0 + g] : in_len_uniform;
        blocks++;
    }
    const uint64_t full = blocks * (uint64_t)out_cap;
    const bool two = uniform((4ull * total > full && 10ull * total < 9ull * full) ? 1u : 0u) != 0u;
    const bool wide = uniform(10ull * total >= 9ull * full ? 1u : 0u) != 0u;
    DecChan ch;
    ch.states = states; ch.channel = channel; ch.status = status;
    if (two)       lzs_decompress_blocks_grp<true, false, false, true>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, npackets, 0u, per_wave, ch);
    else if (wide) lzs_decompress_blocks_grp<false, true, false, true>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, npackets, 0u, per_wave, ch);
    else           lzs_decompress_blocks_grp<false, false, false, true>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, npackets, 0u, per_wave, ch);
}

// Many packets per channel (include/lzs/lzs_channels.h, lzs_decompress_channels_burst_device; DESIGN.md 3.11): group g of
// wavefront w decodes run w * per_wave + g of the runs sorted longest first -- its channel's history preloaded once, its packets
// one after the other in the same window, the history written back once.  The form as lzs_decompress_channels_grp_kernel
// picks it, from the wavefront's runs.
__global__ __launch_bounds__(64)
void lzs_decompress_runs_grp_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                    uint32_t *__restrict__ out_len,
                                    const uint8_t *__restrict__ in, size_t in_stride,
                                    const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                    const uint32_t *__restrict__ run_key, const uint32_t *__restrict__ run_at,
                                    const uint32_t *__restrict__ run_end, const uint32_t *__restrict__ skey,
                                    const uint32_t *__restrict__ sidx, uint32_t nchannels, uint8_t *__restrict__ states,
                                    uint8_t *__restrict__ status, uint32_t nruns, uint32_t per_wave, RunTables rt)
{
    __shared__ DecGroupLds L;
    uint64_t total = 0, blocks = 0;
    const uint32_t b0 = blockIdx.x * per_wave;
    if (b0 >= nruns || run_key[b0] == 0u) return;                 // (runs are sorted by weight: none from here on)
    for (uint32_t g = 0; g < per_wave && b0 + g < nruns; g++) {
        const uint32_t w = run_key[b0 + g];                        // 1 + the run's compressed bytes (saturated), 0: no run
        if (w == 0u) break;
        const uint32_t at = run_at[b0 + g];
        total += w - 1u;
        blocks += run_end[at] - at;
    }
    const uint64_t full = blocks * (uint64_t)out_cap;
    const bool two = uniform((4ull * total > full && 10ull * total < 9ull * full) ? 1u : 0u) != 0u;
    const bool wide = uniform(10ull * total >= 9ull * full ? 1u : 0u) != 0u;
    DecChan ch;
    ch.states = states; ch.status = status;
    ch.run_key = run_key; ch.run_at = run_at; ch.run_end = run_end; ch.skey = skey; ch.sidx = sidx; ch.nchannels = nchannels;
    ch.rt = rt;
    if (two)       lzs_decompress_blocks_grp<true, false, false, true, true>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, nruns, 0u, per_wave, ch);
    else if (wide) lzs_decompress_blocks_grp<false, true, false, true, true>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, nruns, 0u, per_wave, ch);
    else           lzs_decompress_blocks_grp<false, false, false, true, true>(L, out, out_stride, out_cap, out_len, in, in_stride, in_len, in_len_uniform, nruns, 0u, per_wave, ch);
}
