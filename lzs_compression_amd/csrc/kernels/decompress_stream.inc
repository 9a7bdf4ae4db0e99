// kernels/decompress_stream.inc -- one stream (or a small batch) decompressed by many wavefronts: scan / decode / resolve.
// Part of lzs_kernels.hip (included there, inside its anonymous namespace); not a translation unit of its own.

// ---------------------------------------------------------------------------------
// ONE long stream decompressed by many wavefronts (the counterpart of the segment compressor).
// The compressed stream is cut into segments of `seg` bytes (kDecSeg below).  What a segment
// cannot know by itself is the decoder's state when its bit cursor first crosses into it: the bit
// where the first token starts, whether an extension is running and at which offset.  So:
//   SCAN    every segment walks its tokens without copying anything, entered at its first bit in
//           the normal state, and reports the state in which it leaves and how many bytes it
//           would produce; the host re-runs the segments whose predecessor left in another state
//           until all agree (walks entered at different bits fall in step after some tokens), and
//           takes the prefix sum of the byte counts;
//   DECODE  every segment decodes into the output at its offset.  A copy whose source lies before
//           the segment's own output cannot be done yet -- that part of the output is being
//           produced by another wave -- so every byte carries an ORIGIN: clean, or the output
//           position it is a copy of.  Origins are copied along with the bytes;
//   RESOLVE every origin lies in the 2047 bytes in front of its segment (its tail): the tails are
//           settled by workgroups that take chunks of consecutive segments in order, then by a
//           few rounds of pointer jumping on the tails in front of the chunks (a byte whose
//           origin is final takes its value, otherwise it adopts its origin's origin), and one
//           pass over everything finishes.
// Stop rules as in lzs_decompress_blocks_v2_kernel, one-shot form (the first end marker ends it).
// The first forms -- one wavefront per segment: lzs_stream_segment<>, lzs_scan_stream_kernel,
// lzs_decode_stream_kernel -- are kept for the cases noted at their launchers (long runs; A/B).
// ---------------------------------------------------------------------------------
#ifndef LZS_DEC_SEG_MAX
#define LZS_DEC_SEG_MAX 8192
#endif
constexpr uint32_t kDecSegMax = LZS_DEC_SEG_MAX;              // compressed bytes per segment of a long stream (a wave walks it in
                                                      // ~1 ms); short streams take smaller ones (the host chooses `seg`)
constexpr uint32_t kClean    = 0xFFFFFFFFu;           // origin: the byte is final
constexpr uint32_t kDoneBase = 0xFFFFFF00u;           // origin: resolved in round (value & 0xFF)
constexpr uint32_t kSegStop  = 1u << 30;              // state word: the stream ended in this segment
constexpr uint32_t kScanMarkWords = 140;              // per segment: 64 marks, 64 byte counts; [128, 129] exit state and total;
                                                      // [130, 131] the same of the walk continued past end markers; [132..134] marks
                                                      // before its 1st, 2nd, 3rd end marker, [135..137] bytes up to each; pad
// state word: bits 0..7 cursor past the segment start (bits), bit 8 extension running, 9..19 offset

// In LDS an origin is how far BEFORE the segment's output it lies (1..2047: a copy can only reach
// that far, and copies of copies inherit it), 0 = clean: 16 bits per byte of the window.
struct DecSegLds {
    uint32_t ring[kRingWords];                        // the segment's own output window
    uint16_t origin[kRingWords * 4];                  // per byte of it
};

template <bool DECODE>
__device__ __forceinline__ void lzs_stream_segment(const uint8_t *__restrict__ in, uint32_t n, uint32_t seg_byte, uint32_t entry,
                                                   uint32_t *exit_out, uint32_t *count_out,
                                                   uint8_t *out, uint32_t cap, uint32_t out_start, uint32_t out_floor,
                                                   uint32_t *origin_g, uint32_t *tainted_total,
                                                   DecSegLds *Lp, uint32_t lane, uint32_t kDecSeg, bool concat,
                                                   uint32_t *marks = nullptr, bool compare = false)
{
    const uint32_t kDecEnd = 8u * kDecSeg;                        // the segment's length in bits
    // SCAN only.  A walk that is repeated from another entry falls in step with the walk before
    // after a few dozen tokens, and from there on it IS that walk: a full walk leaves behind its
    // 64 of its token starts (state word and bytes produced so far: `marks`), and a repeated one
    // stops as soon as it stands on one of them -- it leaves as the full walk left, with that
    // walk's byte count from there on.  (Otherwise every round costs a walk over the whole
    // segment.)  The marks are the first 16 steps of the walk, then every 2nd, 4th, .. 64th, eight
    // of each: two walks in step take the same steps, so the repeated one meets the next mark
    // within that many, and the marks reach a thousand steps into the segment.
    uint32_t my_mark = ~0u, my_count = 0, nmark = 0, iter = 0, next_mark = 0, mark_step = 1;
    uint32_t old_mark = ~0u, old_count = 0, old_last = 0;
    bool checking = false, merged = false;
    if (!DECODE && compare) {
        old_mark = marks[lane]; old_count = marks[64u + lane];
        const uint64_t valid = __builtin_amdgcn_ballot_w64(old_mark != ~0u);
        if (valid) {
            checking = true;
            old_last = (uint32_t)__builtin_amdgcn_readlane((int)old_mark, 63 - (int)__builtin_clzll(valid)) & 0xFFFFu;
        }
    }
    uint8_t *ring8 = DECODE ? reinterpret_cast<uint8_t *>(Lp->ring) : nullptr;
    uint16_t *origin = DECODE ? Lp->origin : nullptr;
    const uint32_t rel0 = entry & 0xFFu;
    const uint32_t byte0 = seg_byte + (rel0 >> 3);              // (the segment starts at in[seg_byte], its stream ends at in[n])
    uint32_t count = 0, flushed = 0, tainted = 0;
    uint32_t off = (entry >> 9) & 0x7FFu;
    uint32_t extended = (entry >> 8) & 1u;
    uint32_t state = kSegStop;
    if (byte0 < n) {
        const uint8_t *src = in + byte0;
        const uint32_t nn = n - byte0;
        // the input as aligned words (as in lzs_decompress_blocks_v2_kernel)
        const uint32_t skew = (uint32_t)((uintptr_t)src & 3u);
        const uint32_t *w32 = reinterpret_cast<const uint32_t *>(src - skew);
        const uint32_t nwords = (skew + nn + 3u) >> 2;
        uint64_t bits; uint32_t have, pos, wi = 1, nextw = 0;
        {
            uint32_t w = __builtin_bswap32(w32[0]) << (8u * skew);
            const uint32_t avail = 4u - skew < nn ? 4u - skew : nn;
            if (avail < 4u) w &= ~0u << (32u - 8u * avail);
            bits = (uint64_t)w << 32; have = 8u * avail; pos = avail;
            if (nwords > 1u) nextw = w32[1];
        }
        bits <<= rel0 & 7u; have -= rel0 & 7u;                   // the first token starts inside the byte
        const uint32_t base = 8u * (rel0 >> 3);
        for (;;) {
            if (have <= 32u) {
                if (pos < nn) {
                    uint32_t w = __builtin_bswap32(nextw);
                    const uint32_t rem = nn - pos;
                    const uint32_t nb = rem < 4u ? rem : 4u;
                    if (rem < 4u) w &= ~0u << (32u - 8u * rem);
                    bits |= (uint64_t)w << (32u - have);
                    have += 8u * nb; pos += nb; wi += 1u;
                    if (wi < nwords) nextw = w32[wi];
                }
            }
            const uint32_t cur = base + 8u * pos - have;         // bits past the segment start
            if (cur >= kDecEnd) {                                // the next token belongs to the next segment
                // (the offset is part of the state only while an extension runs: otherwise two walks
                // that fell in step would still look different to the host)
                state = (cur - kDecEnd) | (extended << 8) | ((extended ? off : 0u) << 9);
                break;
            }
            if (!DECODE && marks) {
                const uint32_t word = cur | (extended << 16) | ((extended ? off : 0u) << 17);
                if (checking) {
                    const uint64_t hit = __builtin_amdgcn_ballot_w64(old_mark == word);
                    if (hit) {
                        const uint32_t j = uniform((uint32_t)__builtin_ctzll(hit));
                        state = marks[128];
                        count += marks[129] - (uint32_t)__builtin_amdgcn_readlane((int)old_count, (int)j);
                        merged = true;
                        break;
                    }
                    if (cur > old_last) checking = false;
                }
                if (nmark < 64u && iter == next_mark) {
                    my_mark = lane == nmark ? word : my_mark;
                    my_count = lane == nmark ? count : my_count;
                    if (nmark >= 15u && ((nmark - 15u) & 7u) == 0u) mark_step <<= 1;
                    next_mark += mark_step;
                    nmark++;
                }
                iter++;
            }
            if (have == 0u) break;                               // input exhausted (:189)
            if (DECODE && out_start + count >= cap) break;       // output full (:200)
            uint32_t copy_len = 0;
            const uint32_t top = (uint32_t)(bits >> 32);
            if (extended) {                                      // :370-406
                if (have < 4u) break;
                // nibbles of 15 (a long match is thousands of them) go up to four at a time: 60 bytes
                const uint32_t ones = (~bits ? (uint32_t)__builtin_clzll(~bits) : 64u) >> 2;   // leading 1111 nibbles
                uint32_t run = ones < have / 4u ? ones : have / 4u;
                const uint32_t mine = (kDecEnd - cur + 3u) / 4u;                // nibbles that start in this segment
                run = run < mine ? run : mine;
                run = run < 4u ? run : 4u;
                if (run) {
                    copy_len = kNibbleMax * run;
                    bits <<= 4u * run; have -= 4u * run;
                } else {
                    copy_len = top >> 28;                        // the closing nibble, 0..14
                    bits <<= 4; have -= 4u;
                    extended = 0;
                }
            } else if ((int32_t)top >= 0) {
                // a run of literals, but only those that start inside this segment
                if (have < 9u) break;
                const uint64_t types = bits & 0x8040201008040200ull;
                uint32_t kk = (types ? (uint32_t)__builtin_clzll(types) : 64u) / 9u;
                const uint32_t fit = have / 9u;
                const uint32_t mine = (kDecEnd - cur + 8u) / 9u;
                kk = kk < fit ? kk : fit;
                kk = kk < mine ? kk : mine;
                if (DECODE) {
                    if (lane < kk) {
                        const uint32_t at = (count + lane) & kRingMask;
                        ring8[at] = (uint8_t)(bits >> (55u - 9u * lane));
                        origin[at] = 0;
                    }
                }
                count += kk;
                bits <<= 9u * kk; have -= 9u * kk;
            } else {
                // 1 s ooooooo[oooo] cccc: fields on the vector unit (see lzs_decompress_blocks_v2_kernel)
                const uint32_t t = opaque(top) >> 11;
                const bool is_short_v = (t >> 19) & 1u;
                const uint32_t o_v = is_short_v ? (t >> 12) & 0x7Fu : (t >> 8) & 0x7FFu;
                const uint32_t used_v = is_short_v ? 9u : 13u;
                const uint32_t code_v = (is_short_v ? t >> 8 : t >> 4) & 0xFu;
                const uint32_t len_v = code_v < 0xCu ? 2u + (code_v >> 2) : code_v - 7u;
                const uint32_t width_v = code_v < 0xCu ? 2u : 4u;
                const uint32_t packed = uniform(o_v | (used_v << 11) | (len_v << 15) | (width_v << 19) | ((is_short_v ? 1u : 0u) << 22));
                const uint32_t o = packed & 0x7FFu, used = (packed >> 11) & 15u;
                const bool is_short = (packed >> 22) & 1u;
                if (o == 0u) {
                    if (have < used) break;
                    bits <<= used; have -= used;
                    if (is_short) {
                        if (!concat) break;                      // end marker: the stream ends here (:255-260)
                        const uint32_t pad = have & 7u;          // file rule (:564-576): on from the next byte
                        bits <<= pad; have -= pad;
                        continue;
                    }
                    off = 0;                                     // long offset 0: no copy (:280)
                    continue;
                }
                const uint32_t len = (packed >> 15) & 15u, width = (packed >> 19) & 7u;
                if (have < used + width) break;
                bits <<= used + width; have -= used + width;
                off = o;
                extended = len == kTokenMax ? 1u : 0u;
                copy_len = len;
            }
            if (copy_len) {
                if (DECODE) {
                    __builtin_amdgcn_wave_barrier();
                    uint32_t v = 0, og = 0;
                    if (lane < copy_len) {
                        // overlap replicates with period `off` (copy_len <= 60)
                        const uint32_t kk = off >= 60u ? lane : (off ? lane % off : 0u);
                        const uint32_t from = count + kk;        // position + off of the source
                        if (from >= off) {                       // inside this segment's own output
                            const uint32_t at = (from - off) & kRingMask;
                            v = ring8[at]; og = origin[at];
                        } else if ((unsigned long long)out_start + from >= (unsigned long long)off + out_floor) {
                            og = off - from;                     // produced by another wave: that far before my output
                        }                                        // else before the stream's out[0] (out_floor): zero (:350-357)
                    }
                    __builtin_amdgcn_wave_barrier();
                    if (lane < copy_len) {
                        const uint32_t at = (count + lane) & kRingMask;
                        ring8[at] = (uint8_t)v; origin[at] = (uint16_t)og;
                    }
                }
                count += copy_len;
            }
            if (DECODE) {
                if (count - flushed >= kTile) {                  // a finished KiB goes out
                    __builtin_amdgcn_wave_barrier();
                    for (uint32_t j = 0; j < kTile; j += 64u) {
                        const uint32_t p = flushed + j + lane;
                        const uint32_t g = out_start + p;
                        const uint32_t og = origin[p & kRingMask];
                        if (g < cap && g >= out_start) { out[g] = ring8[p & kRingMask]; origin_g[g] = og ? out_start - og : kClean; tainted += og != 0u; }
                    }
                    flushed += kTile;
                }
            }
        }
    }
    if (DECODE) {
        __builtin_amdgcn_wave_barrier();
        for (uint32_t p = flushed + lane; p < count; p += 64u) {
            const uint32_t g = out_start + p;
            const uint32_t og = origin[p & kRingMask];
            if (g < cap && g >= out_start) { out[g] = ring8[p & kRingMask]; origin_g[g] = og ? out_start - og : kClean; tainted += og != 0u; }
        }
        if (tainted) atomicAdd(tainted_total, tainted);
    } else {
        if (marks && !merged) {
            marks[lane] = my_mark; marks[64u + lane] = my_count;
            if (lane == 0) { marks[128] = state; marks[129] = count; }
        }
        if (lane == 0) {
            *exit_out = state;
            *count_out = count;
        }
    }
}

__global__ __launch_bounds__(256)
void lzs_scan_stream_kernel(const uint8_t *__restrict__ in, uint32_t n, uint32_t nseg,
                            const uint32_t *__restrict__ entry, const uint8_t *__restrict__ dirty,
                            uint32_t *__restrict__ exit_state, uint32_t *__restrict__ count,
                            uint8_t *__restrict__ all_ones, uint32_t *__restrict__ marks, uint32_t compare,
                            uint32_t kDecSeg, uint32_t concat,
                            const uint32_t *__restrict__ seg_base, const uint32_t *__restrict__ seg_end)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = blockIdx.x * 4u + uniform(threadIdx.x >> 6);
    if (k >= nseg) return;
    // one stream cut into equal segments -- or many streams in one buffer (a batch of blocks), each
    // cut into segments of its own: then the tables say where segment k starts and its stream ends
    const uint32_t sbase = seg_base ? uniform(seg_base[k]) : k * kDecSeg;
    if (seg_end) n = uniform(seg_end[k]);
    if (all_ones) {
        // A whole segment of 0xFF bytes inside a running extension is nothing but nibbles of 15:
        // it leaves in the state in which it was entered.  The host uses this to carry a long
        // match across its segments without a round each.
        bool ones = (size_t)sbase + kDecSeg <= n;
        if (ones) {
            const uint8_t *p = in + sbase;
            for (uint32_t i = lane; i < kDecSeg && ones; i += 64u) ones = p[i] == 0xFFu;
        }
        const bool all = __builtin_amdgcn_ballot_w64(!ones) == 0ull;
        // 2: and so are the first three bits after it (the last nibble that starts in the segment
        // may reach that far into the next one)
        const size_t after = (size_t)sbase + kDecSeg;
        if (lane == 0) all_ones[k] = !all ? 0 : (after < n && (in[after] & 0xE0u) == 0xE0u) ? 2 : 1;
    }
    if (dirty && !dirty[k]) return;
    lzs_stream_segment<false>(in, n, sbase, uniform(entry[k]), exit_state + k, count + k,
                              nullptr, 0, 0, 0, nullptr, nullptr, nullptr, lane, kDecSeg, concat != 0u,
                              marks ? marks + (size_t)k * kScanMarkWords : nullptr, compare != 0u);
}

// ---- SCAN, first round: EIGHT SEGMENTS PER WAVEFRONT, 8 lanes each (the block decoder's shape,
// decompress_blocks.inc: no scalar control flow inside a step; here nothing is copied, so no LDS
// either).  The first round walks every token of the stream once and was, at one wavefront per
// segment, bound by the scalar unit like the wave-per-stream block decoder; the later rounds walk
// a few thousand segments a few dozen tokens far and stay with lzs_scan_stream_kernel.  Same
// steps as lzs_stream_segment<false> (runs of <= 7 literals, <= 4 nibbles of 15 at a time, the
// same refill rule), so the marks left here are met by the repeated walks of the later rounds.
//
// LANES = 1: ONE LANE PER SEGMENT.  Nothing in a scan step is done by the lanes of a group
// together -- all eight compute the same -- so a wavefront can just as well walk 64 segments: an
// eighth of the instructions (the walk of one segment is as long as before, ~0.5 ms, but a GiB of
// text is 2300 wavefronts of them, all resident at once).  Each lane reads its own segment, 16
// bytes at a time.
// The scan's token arithmetic, in compares and selects (the walk is one lane a segment and waits for its input, not for the
// vector unit; the decoders' step, kernels/decompress_blocks.inc, has the same identities as masks).
// The fields of a match token 1 s ooooooo[oooo] cccc at the top of `top` (lzs-decompression.c:238-342), every
// decoder's way: a short token moved down four bits has its fields where a long one has them (offset 29..19, code
// 18..15).  short4: 4 for a 7-bit offset, 0 for an 11-bit one -- the token is 13 - short4 bits up to its length code,
// and that is 2 bits (lengths 2 3 4) below code 12, 4 bits (5 6 7 8) from there.
__device__ __forceinline__ void dec_match_fields(uint32_t top, uint32_t &short4, uint32_t &o, uint32_t &code, uint32_t &len)
{
    short4 = (uint32_t)((int32_t)(top << 1) >> 31) & 4u;
    const uint32_t norm = (top & 0x3FFFFFFFu) >> short4;
    o = norm >> 19;
    code = (norm >> 15) & 0xFu;
    len = (uint32_t)max((int32_t)(((norm >> 17) & 3u) + 2u), (int32_t)code - 7);      // 2 2 2 2 3 3 3 3 4 4 4 4 5 6 7 8
}

// How many of the tokens at the top of the 64 bits top : low are literals, one after the other (:217-233): token i of
// an all-literal run starts at bit 63 - 9i, so the first set type bit among those ends the run.  SHORT: counted in the
// upper word alone, four at most (where matches dominate, runs are short).  The caller clips to the bits it has.
template <bool SHORT>
__device__ __forceinline__ uint32_t dec_literal_run(uint32_t top, uint32_t low)
{
    uint32_t lead;
    if (SHORT) {
        lead = min(ffbh_u32(top & 0x80402010u), 36u);
    } else {
        const uint32_t lead_hi = ffbh_u32(top & 0x80402010u), lead_lo = ffbh_u32(low & 0x08040200u) | 32u;
        lead = min(min(lead_hi, lead_lo), 64u);                    // (ffbh of 0 is huge: all seven are literals)
    }
    return __umul24(lead, 57u) >> 9;                               // lead / 9 for lead <= 64
}

constexpr uint32_t kScanWin = 32;                     // words of input a lane of the scan keeps in LDS
template <uint32_t LANES, bool CONCAT>
__global__ __launch_bounds__(64)
void lzs_scan_stream_g8_kernel(const uint8_t *__restrict__ in, uint32_t n_all, uint32_t nseg,
                               const uint32_t *__restrict__ entry, const uint8_t *__restrict__ dirty,
                               uint32_t *__restrict__ exit_state, uint32_t *__restrict__ count_out,
                               uint32_t *__restrict__ marks_all, uint32_t compare, uint32_t kDecSeg, uint32_t concat_arg,
                               const uint32_t *__restrict__ seg_base, const uint32_t *__restrict__ seg_end, uint32_t in_extent)
{
    constexpr uint32_t concat = CONCAT ? 1u : 0u;                  // (compile time, as in the decoders)
    (void)concat_arg;
    __shared__ uint32_t win[kScanWin][64];                          // a lane's next words of input: word w of its stream in win[w % 32][lane]
    const uint32_t lane = threadIdx.x;
    const uint32_t g = lane / LANES, j = lane % LANES;
    const uint32_t k = blockIdx.x * (64u / LANES) + g;
    const bool live = k < nseg && (!dirty || dirty[k < nseg ? k : 0u]);
    const uint32_t kk = k < nseg ? k : 0u;
    const uint32_t sbase = seg_base ? seg_base[kk] : kk * kDecSeg;
    const uint32_t n = seg_end ? seg_end[kk] : n_all;
    const uint32_t e0 = entry[kk];
    uint32_t *marks = marks_all ? marks_all + (size_t)kk * kScanMarkWords : nullptr;
    const uint32_t kDecEnd = 8u * kDecSeg;
    const uint32_t rel0 = e0 & 0xFFu;
    const uint32_t byte0 = sbase + (rel0 >> 3);
    const bool any = live && byte0 < n;
    if (LANES > 1u && live && marks && !compare) for (uint32_t i = j; i < 128u; i += LANES) marks[i] = ~0u;   // (LANES = 1: the launcher clears them all)
    // A repeated walk (compare): the marks are those of the segment's FIRST walk and stay so.  The
    // lane keeps the next one that is not behind it; standing on it, it leaves as that walk left.
    // (One step may pass several marks and the lane moves on by one: it then misses a meeting
    // point, not the result -- the marks thin out and it catches up.)
    uint32_t mi = 0, mword = ~0u, checking = 0;
    if (compare && live && marks) { mword = marks[0]; checking = mword != ~0u ? 1u : 0u; }

    // The input as aligned words, every lane its own stream.  Sixty-four lanes use up their words at sixty-four
    // different times; a load per lane whenever IT runs out (rounds 2 and 3) is a load somewhere in the wavefront
    // on nearly every trip, and since loads come back in order, whoever needs his waits for the youngest: ~1.5 us
    // a trip, the whole round.  Now the words wait in LDS (32 per lane) and ALL lanes fetch on a fixed beat:
    // every eighth trip a lane stores the eight words it asked for eight trips ago (they have long arrived) and
    // asks for the next eight -- if its window has room for them; a lane takes at most one word a trip, so it
    // can never run dry.  Bounded buffer loads (`in_extent` bytes from `in`): no tail cases.
    const uint8_t *src = in + (any ? byte0 : 0u);
    const uint32_t nn = any ? n - byte0 : 0u;
    const uint32_t skew = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t nwords = nn ? (skew + nn + 3u) >> 2 : 0u;
    const uintptr_t in_lo = (uintptr_t)in & ~(uintptr_t)3;
    const uintptr_t in_lo_u = ((uintptr_t)uniform((uint32_t)((uint64_t)in_lo >> 32)) << 32) | uniform((uint32_t)in_lo);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)in_lo_u, 0, (int)uniform((in_extent + (uint32_t)((uintptr_t)in & 3u) + 3u) & ~3u), 0x00020000);
    const auto bload = [&](uint32_t byte_off) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    };
    const auto put4 = [&](uint32_t w, uint4 v) {                    // words w .. w + 3 (w a multiple of 4) into the window
        const uint32_t r = w & (kScanWin - 1u);
        win[r][lane] = v.x; win[r + 1u][lane] = v.y; win[r + 2u][lane] = v.z; win[r + 3u][lane] = v.w;
    };
    const uint32_t off0 = (uint32_t)((uintptr_t)(src - skew) - in_lo);       // my word 0, in bytes from the buffer's base
    uint32_t first_word = 0;
#pragma unroll
    for (uint32_t q = 0; q < kScanWin / 4u; q++) {
        const uint4 v = bload(off0 + 16u * q);
        put4(4u * q, v);
        if (q == 0u) first_word = v.x;
    }
    uint32_t lc = kScanWin;                                         // words asked for so far
    uint32_t pending = 0, pl = 0;                                   // eight words asked for and not stored yet: pl .. pl + 7
    uint4 pend0 = make_uint4(0, 0, 0, 0), pend1 = pend0;
    uint32_t tick = 0;                                              // trips, for the beat (wave-uniform)
    uint64_t bits = 0;
    uint32_t have = 0, left = nn, wi = 0;                           // bits in the buffer, bytes not fed yet, next word
    if (nwords) {
        uint32_t w = __builtin_bswap32(first_word) << (8u * skew);
        const uint32_t avail = 4u - skew < nn ? 4u - skew : nn;
        if (avail < 4u) w &= ~0u << (32u - 8u * avail);
        bits = (uint64_t)w << 32; have = 8u * avail; left = nn - avail; wi = 1;
        bits <<= rel0 & 7u; have -= rel0 & 7u;                     // the first token starts inside the byte
    }
    uint32_t cur = rel0;                                            // bits past the segment start: where the next token begins
    uint32_t count = 0;
    uint32_t off = (e0 >> 9) & 0x7FFu, extended = (e0 >> 8) & 1u;
    uint32_t state = kSegStop;
    // (the first walk's marks fall on the same trips for every lane that still walks: the schedule is the wavefront's)
    uint32_t nmark = 0, iter = 0, next_mark = 0, mark_step = 1;
    uint32_t nem = 0, emn0 = 0, emn1 = 0, emn2 = 0, emc0 = 0, emc1 = 0, emc2 = 0;   // end markers walked past (marks before each: >= 1; 0 = none): see the end of the step
    uint32_t done = any ? 0u : 1u;
    uint32_t nextw = win[wi & (kScanWin - 1u)][lane];              // the word to feed next, fetched a trip before it is used

    for (;;) {
        if (__builtin_amdgcn_ballot_w64(done == 0u) == 0ull) break;
        if ((uniform(tick++) & 7u) == 0u) {                        // the beat: store what was asked for eight trips ago, ask for more
            // (stored only once the eight words it overwrites have been used: the window is 32 words)
            const bool store = pending && wi + kScanWin >= pl + 8u;
            if (store) { put4(pl, pend0); put4(pl + 4u, pend1); }
            pending = store ? 0u : pending;
            if (!pending) {
                pend0 = bload(off0 + 4u * lc); pend1 = bload(off0 + 4u * lc + 16u);
                pl = lc; lc += 8u; pending = 1u;
            }
        }
        {   // refill: one word when 32 bits or fewer are left (the stream's last word not masked: what follows the
            // stream in it lies past `have` bits and is never believed -- lzs_decompress_blocks_grp)
            const uint32_t rf = (done == 0u) & (have <= 32u) & (left != 0u);
            const uint32_t w = rf ? __builtin_bswap32(nextw) : 0u;
            const uint32_t nb = rf ? min(left, 4u) : 0u;           // bytes taken
            bits |= (uint64_t)w << ((32u - have) & 63u);
            have = (nb << 3) + have;
            left -= nb;
            wi   = rf ? wi + 1u : wi;
            nextw = win[wi & (kScanWin - 1u)][lane];
        }
        // the next token belongs to the next segment: leave, in this state
        const uint32_t past = (done == 0u) & (cur >= kDecEnd ? 1u : 0u);
        state = past ? (cur - kDecEnd) | (extended << 8) | ((extended ? off : 0u) << 9) : state;
        done |= past;
        // marks: the first 16 steps, then every 2nd, 4th, .. 64th, eight of each (see lzs_stream_segment)
        if (marks && compare) {
            const uint32_t word = cur | (extended << 16) | ((extended ? off : 0u) << 17);
            const uint32_t act = (done == 0u) & checking;
            const uint32_t meet = act & (mword == word ? 1u : 0u);
            if (__builtin_amdgcn_ballot_w64(meet != 0u) != 0ull) {
                if (meet) {
                    // from here on this walk is the first walk: it leaves as that left -- or, if that
                    // walked on past end markers (below), ends at the first of them that lies ahead
                    uint32_t st = marks[130], cn = marks[131];
                    if (mi < marks[134]) { st = kSegStop; cn = marks[137]; }
                    if (mi < marks[133]) { st = kSegStop; cn = marks[136]; }
                    if (mi < marks[132]) { st = kSegStop; cn = marks[135]; }
                    state = st; count += cn - marks[64u + mi]; done = 1u;
                }
            }
            const uint32_t adv = act & (meet ^ 1u) & ((mword & 0xFFFFu) < cur ? 1u : 0u);
            if (__builtin_amdgcn_ballot_w64(adv != 0u) != 0ull) {
                if (adv) { mi++; mword = mi < 64u ? marks[mi] : ~0u; checking = mword != ~0u ? 1u : 0u; }
            }
        } else if (marks) {
            if (uniform(nmark) < 64u && uniform(iter) == uniform(next_mark)) {
                if (done == 0u && j == 0u) {
                    marks[nmark] = cur | (extended << 16) | ((extended ? off : 0u) << 17);
                    marks[64u + nmark] = count;
                }
                if (nmark >= 15u && ((nmark - 15u) & 7u) == 0u) mark_step <<= 1;
                next_mark += mark_step;
                nmark++;
            }
            iter++;
        }
        // (input exhausted, :189: every step needs four bits at least -- `stop` below)
        const uint32_t top = (uint32_t)(bits >> 32), low = (uint32_t)bits;
        const uint32_t is_ext = extended;
        const uint32_t is_lit = (is_ext ^ 1u) & ((top >> 31) ^ 1u);
        const uint32_t is_mat = (is_ext ^ 1u) & (top >> 31);
        // length nibbles (:370-406): up to four 1111 at a time, only those that start in this segment
        const uint32_t inv_hi = ffbh_u32(~top);                    // leading ones of the top word (0xFFFFFFFF if all)
        const uint32_t ones = (inv_hi < 32u ? inv_hi : 32u) >> 2;
        uint32_t run = ones < (have >> 2) ? ones : (have >> 2);
        const uint32_t mine4 = (kDecEnd - cur + 3u) >> 2;
        run = run < mine4 ? run : mine4;
        run = run < 4u ? run : 4u;
        const uint32_t e = top >> 28;
        // a run of literals that start inside this segment
        uint32_t kv = dec_literal_run<false>(top, low);
        const uint32_t fit = __umul24(have, 57u) >> 9;             // have / 9
        kv = kv < fit ? kv : fit;
        const uint32_t mine_lit = __umul24(min(kDecEnd - cur + 8u, 72u), 57u) >> 9;     // (bits left + 8) / 9, eight and more as eight (a run is <= 7)
        kv = kv < mine_lit ? kv : mine_lit;
        // a match token
        uint32_t short4, o, code, len;
        dec_match_fields(top, short4, o, code, len);
        const uint32_t is_short = short4 >> 2;
        const uint32_t used = 13u - short4;
        const uint32_t width = code < 0xCu ? 2u : 4u;
        const uint32_t zero_off = o == 0u ? 1u : 0u;
        const uint32_t copying = is_mat & (zero_off ^ 1u);
        const uint32_t need = is_ext ? 4u : (is_lit ? 9u : (zero_off ? used : used + width));
        const uint32_t stop = have < need ? 1u : 0u;
        const uint32_t go = (done | stop) ^ 1u;
        const uint32_t endm = is_mat & zero_off & is_short;
        uint32_t consume = is_ext ? (run ? 4u * run : 4u) : (is_lit ? 9u * kv : need);
        consume += (endm & concat) ? ((have - used) & 7u) : 0u;
        const uint32_t produced = is_ext ? (run ? kNibbleMax * run : e) : (is_lit ? kv : (copying ? len : 0u));
        const uint32_t off_now = copying ? o : off;
        const uint32_t off_next = (is_mat & zero_off & (is_short ^ 1u)) ? 0u : off_now;
        const uint32_t ext_next = is_ext ? (run ? 1u : 0u) : (copying & (len == kTokenMax ? 1u : 0u));
        // (a walk that has stopped leaves with its count and, if it ran out of its segment, its state: both are frozen
        // by `go` / taken while it still went; its buffer, position, offset and flags need no selects to stay as they are)
        count    = go ? count + produced : count;
        bits     = bits << (consume & 63u);
        have     = have - consume;
        cur      = cur + consume;
        off      = off_next;
        extended = ext_next;
        // An end marker ends the stream -- but the first walk of a segment, entered at a guessed
        // bit, reads one into the data now and then before it has fallen in step (one token in
        // 512: 1.5-4 % of the segments), and a walk that stops leaves no marks for the repeated
        // one to meet, which then has to go over the whole segment -- and the round is as long
        // as its slowest lane.  So the first walk notes what it has at an end marker (at the first
        // one: that is its result) and walks on for the marks' sake, past up to three of them; a
        // repeated walk that meets one of its marks ends at the first of those end markers that
        // still lies ahead, or leaves as the continued walk left.
        const uint32_t endstop = go & endm & (concat ? 0u : 1u);
        const uint32_t noted = endstop & ((marks && !compare) ? 1u : 0u) & (nem < 3u ? 1u : 0u);
        if (__builtin_amdgcn_ballot_w64(noted != 0u) != 0ull) {
            emn0 = (noted & (nem == 0u)) ? nmark : emn0; emc0 = (noted & (nem == 0u)) ? count : emc0;
            emn1 = (noted & (nem == 1u)) ? nmark : emn1; emc1 = (noted & (nem == 1u)) ? count : emc1;
            emn2 = (noted & (nem == 2u)) ? nmark : emn2; emc2 = (noted & (nem == 2u)) ? count : emc2;
            nem += noted;
        }
        done |= stop | (endstop & (noted ^ 1u));
    }
    if (live && j == 0u) {
        const uint32_t state1 = nem ? kSegStop : state, count1 = nem ? emc0 : count;
        exit_state[k] = state1;
        count_out[k] = count1;
        if (marks && !compare) {
            marks[128] = state1; marks[129] = count1; marks[130] = state; marks[131] = count;
            marks[132] = emn0; marks[133] = emn1; marks[134] = emn2;
            marks[135] = emc0; marks[136] = emc1; marks[137] = emc2;
        }
    }
}

// ---- DECODE: EIGHT SEGMENTS PER WAVEFRONT as well.  Every byte of a group's output window is an
// entry in LDS: the value, or a flag | how far before the segment's output its origin lies
// (1..2047: a copy can only reach that far, and copies of copies inherit it).  Every step stores what it produced straight to HBM --
// the value to `out`, the origin as an absolute position (or kClean) to `origin_g` -- because the
// eight groups of a wavefront would reach a drain point at eight different times, and the wave
// would pay for a drain pass eight times as often as a wave with one stream (measured: 165 ms
// per GiB of text with 128-byte drains against 57 for one wavefront per segment; 35 this way).
// Steps as in lzs_scan_stream_g8_kernel, one length nibble (<= 15 bytes) per step: lane j of the
// group produces bytes j and j + 8.  Unlike the block decoder nothing is clipped to the capacity
// inside a step (the window takes the whole step, only what lies below `cap` is stored), which is
// what lzs_stream_segment<true> does.  Long runs are the one case where one wavefront per segment
// is faster (it takes four nibbles, 60 bytes, per step): the launcher keeps it for streams that
// expand more than sixfold.
// The ring is 2048 entries (as 16-bit words, rounds 2 and 3: exactly 32 KiB a wavefront, FIVE wavefronts per
// CU; 2064 entries and a dummy word per lane were four).  That is enough: a step reads positions [cpos - 2047, cpos) and
// writes [cpos, cpos + 15]; the second half-step (bytes 8..15) reads no further back than
// cpos + 8 - 2047, and what the first half wrote lies on the slots of cpos - 2048 .. cpos - 2041.
// Lanes with nothing to read read any slot; lanes with nothing to write sit out the store.
// Round 4: the entry is 12 bits (a flag, and 11 bits of distance or 8 of value), kept as TWO PLANES -- the low
// eight bits of entry i in byte i of `lo`, the upper four in byte i mod 1024 of `hi`, nibble i / 1024 -- 3 KiB a
// segment, 24 KiB a wavefront: SIX wavefronts per CU, and the kernel, which waits more than it issues at
// 1.25 wavefronts per SIMD, is a fifth faster for 15 more instructions a trip (1 GiB of text: 16.3 -> 13.3 ms;
// -DLZS_SEG_PLANES=0 is the 16-bit ring).  A store into `hi` is a read-modify-write of a byte shared with
// the entry 1024 positions away: no two lanes of a step meet there (a step writes 16 consecutive entries),
// and a lane that reads the other nibble meanwhile reads what was there before and after.
#ifndef LZS_SEG_PLANES
#define LZS_SEG_PLANES 1
#endif
constexpr uint32_t kSegRing  = 2048;
constexpr uint32_t kSegOpen  = LZS_SEG_PLANES ? 0x800u : 0x8000u;     // the flag of an entry that is a distance
struct __attribute__((aligned(16))) DecSegG8Lds {
#if LZS_SEG_PLANES
    uint8_t lo[8][kSegRing];
    uint8_t hi[8][kSegRing / 2];
#else
    uint16_t ring[8][kSegRing];
#endif
};

// TWO: a second token in the same trip where that is possible, as in lzs_decompress_blocks_grp (text
// gains a quarter by it, the other classes lose to the extra instructions: the launcher picks the
// form by the stream's ratio).
// WIDE: the 96-bit bit buffer fed with up to two words per trip (lzs_decompress_blocks_grp), for streams
// that are mostly literals.
template <bool TWO, bool WIDE, bool CONCAT>
__global__ __launch_bounds__(64)
void lzs_decode_stream_g8_kernel(uint8_t *__restrict__ out, uint32_t cap_all, uint32_t *__restrict__ origin_g,
                                 uint32_t *__restrict__ tainted_total,
                                 const uint8_t *__restrict__ in, uint32_t n_all, uint32_t in_extent, uint32_t nseg,
                                 const uint32_t *__restrict__ entry, const uint32_t *__restrict__ out_start_all,
                                 uint32_t kDecSeg, uint32_t concat_arg,
                                 const uint32_t *__restrict__ seg_base, const uint32_t *__restrict__ seg_end,
                                 const uint32_t *__restrict__ out_floor_all, const uint32_t *__restrict__ out_limit)
{
    __shared__ DecSegG8Lds L;
    constexpr uint32_t concat = CONCAT ? 1u : 0u;                  // (compile time, as in lzs_decompress_blocks_grp)
    (void)concat_arg;
    const uint32_t lane = threadIdx.x;
    const uint32_t g = lane >> 3, j = lane & 7u;
    const uint32_t k = blockIdx.x * 8u + g;
    const uint32_t kk = k < nseg ? k : 0u;
    const uint32_t e0 = entry[kk];
    const bool live = k < nseg && !(e0 & kSegStop);
    const uint32_t sbase = seg_base ? seg_base[kk] : kk * kDecSeg;
    const uint32_t n = seg_end ? seg_end[kk] : n_all;
    const uint32_t cap = out_limit ? out_limit[kk] : cap_all;
    const uint32_t out_start = out_start_all[kk];
    const uint32_t out_floor = out_floor_all ? out_floor_all[kk] : 0u;
    const uint32_t room = cap > out_start ? cap - out_start : 0u;  // bytes of my output that are stored
    // how far before my output the stream's out[0] lies, as far as a copy can tell (it reaches 2047 back)
    const uint32_t headroom = min(out_start - out_floor, 4096u);
#if LZS_SEG_PLANES
    uint8_t *ring_lo = L.lo[g], *ring_hi = L.hi[g];
#else
    uint16_t *ring = L.ring[g];
#endif
    const uint32_t kDecEnd = 8u * kDecSeg;
    const uint32_t rel0 = e0 & 0xFFu;
    const uint32_t byte0 = sbase + (rel0 >> 3);
    const bool any = live && byte0 < n;

    const uint8_t *src = in + (any ? byte0 : 0u);
    const uint32_t nn = any ? n - byte0 : 0u;
    const uint32_t skew = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(src - skew);
    const uint32_t nwords = nn ? (skew + nn + 3u) >> 2 : 0u;
    // The input of a group, 128 bytes at a time: lane j of the group holds words 4j .. 4j + 3 of the
    // current 32 (one coalesced load for the eight of them) and of the next 32, requested a chunk
    // ahead; the word the group needs next comes across the lanes (ds_bpermute), fetched a step
    // before it is used.  (Sixteen bytes at a time in every lane, as before, meant a load every
    // other step somewhere in the wavefront, and the wave waited for each: ~1 us a step.)  They
    // are BUFFER loads, bounded by the whole input (`in_extent` bytes from `in`): past the end
    // they return zeros instead of faulting, so there is no tail case -- what lies past the end of
    // a segment's own stream is never used (`rem` below) -- and lanes that do not move on simply
    // load what they have again, so the load is one instruction for the whole wavefront, not
    // waited for until the chunk is needed.
    const uintptr_t in_lo = (uintptr_t)in & ~(uintptr_t)3;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)in_lo, 0, (int)((in_extent + (uint32_t)((uintptr_t)in & 3u) + 3u) & ~3u), 0x00020000);
    const auto bload = [&](uint32_t byte_off) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    };
    uint32_t nxt_off = (uint32_t)((uintptr_t)w32 - in_lo) + 16u * j + 128u;
    uint4 cur4 = bload(nxt_off - 128u), nxt4 = bload(nxt_off);
    const uint32_t glane4 = (lane & 56u) << 2;        // byte index of the group's lane 0 for ds_bpermute
    // (a lane's four words rotate by one with every word its group takes: lzs_decompress_blocks_grp)
    const auto rotate = [&](uint32_t on) {
        const uint32_t x0 = cur4.x;
        cur4.x = on ? cur4.y : cur4.x; cur4.y = on ? cur4.z : cur4.y; cur4.z = on ? cur4.w : cur4.z; cur4.w = on ? x0 : cur4.w;
    };
    const auto fetch = [&](uint32_t wi_) {            // word wi_ of the input (inside the current 32)
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(glane4 + (wi_ & 28u)), (int)cur4.x);
    };
    const auto fetch_after = [&](uint32_t wi_) {      // word wi_ + 1
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(glane4 + ((wi_ + 1u) & 28u)), (int)cur4.y);
    };
    uint64_t bits = 0;
    uint32_t have = 0, left = nn, wi = 0;             // bits in the buffer, bytes not fed yet, next word
    if (nwords) {
        uint32_t w = __builtin_bswap32(w32[0]) << (8u * skew);
        const uint32_t avail = 4u - skew < nn ? 4u - skew : nn;
        if (avail < 4u) w &= ~0u << (32u - 8u * avail);
        bits = (uint64_t)w << 32; have = 8u * avail; left = nn - avail; wi = 1;
        bits <<= rel0 & 7u; have -= rel0 & 7u;
    }
    rotate(wi);
    uint32_t nextw = fetch(wi);
    uint32_t nextw2 = WIDE ? fetch_after(wi) : 0u;
    uint32_t bits_lo = 0;                                          // (WIDE: bits 64..95 of the buffer)
    uint32_t cur = rel0;                               // bits past the segment start: where the next token begins
    uint32_t count = 0, cpos = 0, tainted = 0;
    uint32_t off = (e0 >> 9) & 0x7FFu, extended = (e0 >> 8) & 1u;
    uint32_t done = any ? 0u : 1u;
    // idx mod off for my two bytes of a step, idx = j and j + 8 (lzs_decompress_blocks_grp)
    uint32_t mod_lo = 0; uint64_t mod_hi = 0;
#pragma unroll
    for (uint32_t e = 0; e <= 8u; e++) mod_lo |= ((e == 0u || e == 8u) ? j : j % (e ? e : 1u)) << (3u * e);
#pragma unroll
    for (uint32_t e = 0; e < 16u; e++) mod_hi |= (uint64_t)(e == 0u ? j + 8u : (j + 8u) % (e ? e : 1u)) << (4u * e);

    for (;;) {
        if (__builtin_amdgcn_ballot_w64(done == 0u) == 0ull) break;
        if (!WIDE) {   // refill: one word when 32 bits or fewer are left (the last word not masked: lzs_decompress_blocks_grp)
            const uint32_t rf = (have <= 32u) & (left != 0u);
            const uint32_t w = rf ? __builtin_bswap32(nextw) : 0u;
            const uint32_t nb = rf ? min(left, 4u) : 0u;           // bytes taken
            bits |= (uint64_t)w << ((32u - have) & 63u);
            have = (nb << 3) + have;
            left -= nb;
            wi   = rf ? wi + 1u : wi;
            rotate(rf);
            const bool roll = rf && (wi & 31u) == 0u;               // into the next 32 words
            if (__builtin_amdgcn_ballot_w64(roll) != 0ull) {
                cur4.x = roll ? nxt4.x : cur4.x; cur4.y = roll ? nxt4.y : cur4.y;
                cur4.z = roll ? nxt4.z : cur4.z; cur4.w = roll ? nxt4.w : cur4.w;
                nxt_off = roll ? nxt_off + 128u : nxt_off;
                nxt4 = bload(nxt_off);
            }
            nextw = fetch(wi);
        } else {       // two words where 64 bits or fewer are left, the second only from the same chunk: bits : bits_lo, 96 bits
            // (as masks, like lzs_decompress_blocks_grp's: a word that is not taken is a word of zeros OR-ed in)
            uint32_t m_took = 0u;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const uint32_t nb4 = min(left, 4u);                // (0 .. 4)
                uint32_t m_rf = m_lt(have, 65u) & m_nz(nb4);
                if (r == 1) m_rf &= m_took & m_nz(wi & 31u);       // the second only after the first, and from the same chunk
                m_took = m_rf;
                const uint32_t w = __builtin_bswap32(r == 0 ? nextw : nextw2) & m_rf;
                const uint32_t nb = nb4 & m_rf;                    // bytes taken
                const uint64_t hi = ((uint64_t)w << 32) >> (have & 63u);           // (have = 64: all of it falls below)
                const uint32_t keep_hi = m_lt(have, 64u);
                const uint32_t lo = (uint32_t)((uint64_t)w << ((64u - have) & 63u)) & m_lt(32u, have);
                bits    |= hi & (((uint64_t)keep_hi << 32) | keep_hi);
                bits_lo |= lo;
                have += nb << 3;
                left -= nb;
                wi   -= m_rf;
                const uint32_t x0 = cur4.x;
                cur4.x = m_sel(m_rf, cur4.y, cur4.x); cur4.y = m_sel(m_rf, cur4.z, cur4.y); cur4.z = m_sel(m_rf, cur4.w, cur4.z); cur4.w = m_sel(m_rf, x0, cur4.w);
                const uint32_t not_roll = m_ornot(wi & 31u, m_rf);
                if (__builtin_amdgcn_ballot_w64(not_roll == 0u) != 0ull) {
                    const bool roll = not_roll == 0u;
                    cur4.x = roll ? nxt4.x : cur4.x; cur4.y = roll ? nxt4.y : cur4.y;
                    cur4.z = roll ? nxt4.z : cur4.z; cur4.w = roll ? nxt4.w : cur4.w;
                    nxt_off = roll ? nxt_off + 128u : nxt_off;
                    nxt4 = bload(nxt_off);
                }
            }
            nextw = fetch(wi);
            nextw2 = fetch_after(wi);
        }
        const uint32_t top = (uint32_t)(bits >> 32), low = (uint32_t)bits;
        // ---- the step with its flags as masks (lzs_decompress_blocks_grp, kernels/decompress_blocks.inc: a compare or a select
        // costs the SIMD twice what an add or a v_bitop3 does); the 0 / 1 words the slots below read are made of them at the end
        const uint32_t m_ext = 0u - extended;
        const uint32_t m_t31 = m_sign(top);
        const uint32_t m_lit = m_nor(m_t31, m_ext);
        const uint32_t m_mat = m_andnot(m_t31, m_ext);
        const uint32_t e = top >> 28;                              // a length nibble (:370-406)
        // a run of literals that start inside this segment
        uint32_t kv;
        if (TWO) {                                                 // four a trip at most, counted in the upper word
            kv = min16(ffbh_u32(top & 0x80402010u), 36u) >> 3;     // 0 9 18 27 36 leading zeros: 0 1 2 3 4 literals
        } else {
            const uint32_t lead_hi = ffbh_u32(top & 0x80402010u), lead_lo = ffbh_u32(low & 0x08040200u) | 32u;
            kv = min16(min16(lead_hi, lead_lo), 63u) >> 3;         // (ffbh of 0 is all ones: 0xFFFF in 16 bits)
        }
        const uint32_t mine_lit = __umul24(min(kDecEnd - cur + 8u, 72u), 57u) >> 9;     // those that start in this segment: (bits left + 8) / 9, eight and more as eight
        kv = min16(min16(kv, __umul24(have, 57u) >> 9), mine_lit);
        // a match token
        const uint32_t m_short = m_sign(twice(top));
        const uint32_t short4 = m_short & 4u;
        const uint32_t norm = (top & 0x3FFFFFFFu) >> short4;
        const uint32_t o = norm >> 19;
        const uint32_t code = (norm >> 15) & 0xFu;
        const uint32_t len = max16i(((norm >> 17) & 3u) + 2u, code - 7u);
        const uint32_t used = 13u - short4;
        const uint32_t width = 4u - (m_lt(code, 12u) & 2u);
        const uint32_t m_zoff = m_z(o);
        const uint32_t m_copying = m_andnot(m_mat, m_zoff);
        const uint32_t need = m_sel(m_ext, 4u, m_sel(m_lit, 9u, used + m_andnot(width, m_zoff)));
        // the token's own stops and :189 (no bits: every step needs four at least); the next token belongs to the next
        // segment; output full (:200)  (compares: room and the counts may be anything up to 4 GiB)
        const uint32_t stop = ((have < need) | (cur >= kDecEnd) | (count >= room)) ? 1u : 0u;
        const uint32_t go = (done | stop) ^ 1u;
        const uint32_t m_go = 0u - go;
        const uint32_t m_endm = m_mat & m_zoff & m_short;
        uint32_t consume = m_sel(m_lit, (kv << 3) + kv, need);
        if (CONCAT) consume += m_endm & ((have - used) & 7u);
        const uint32_t copy_len = m_sel(m_ext, e, len & m_copying);
        const uint32_t off_now = m_sel(m_copying, o, off);
        const uint32_t off_next = m_andnot(off_now, m_andnot(m_mat & m_zoff, m_short));
        const uint32_t m_ext_next = m_sel(m_ext, m_lt(14u, e), m_copying & m_lt(7u, len));
        const uint32_t nA = m_sel(m_lit, kv, copy_len) & m_go;    // bytes of this step's (first) token
        // ---- TWO: the next token too, if it is a match with a real offset that starts inside this
        // segment, its bits are all there, both fit the trip's 16 byte slots, and its copy reads
        // nothing the first token writes (offset >= both lengths together: so it is not 0); else it is the next
        // trip's first token.  (The output's capacity is checked byte by byte below, as before.)
        uint32_t okB = 0u, nB = 0u, oB = 0u, lenB = 0u, needB = 0u;
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
            const uint32_t m_okB = m_firstA & m_sign(topB) & m_nor(m_lt(haveB, needB), m_lt(min16(oB, 16u), both));
            okB = (m_okB & 1u) & (cur + consume < kDecEnd ? 1u : 0u) & (count + nA < room ? 1u : 0u);
            nB = okB ? lenB : 0u;
        }
        const uint32_t is_lit = m_lit & 1u;
        const uint32_t ext_next = m_ext_next & 1u;
        const uint32_t endm = m_endm & 1u;
        const uint32_t nwrite = nA + nB;

#pragma unroll
        for (uint32_t sl = 0; sl < 2u; sl++) {
            if (sl > 0u && __builtin_amdgcn_ballot_w64(nwrite > 8u) == 0ull) break;   // bytes 8..15: rare in text with one token a trip
            const uint32_t idx = j + 8u * sl;
            const uint32_t second = TWO ? (idx >= nA ? 1u : 0u) : 0u;      // a byte past the first token: the second's (no replication there), or not written
            // idx mod off from the lane's table (idx itself for off 0 and for off > idx)
            const uint32_t k1 = sl == 0u ? (mod_lo >> (3u * (off_now < 8u ? off_now : 8u))) & 7u
                                         : (off_now < 16u ? (uint32_t)(mod_hi >> (4u * (off_now & 15u))) & 15u : idx);
            const uint32_t kx = second ? idx : k1;
            const uint32_t oo = second ? oB : off_now;
            const uint32_t from = count + kx;                      // position + off of the source
            const uint32_t sp = (cpos + kx - oo) & (kSegRing - 1u);
            const uint32_t inside = from >= oo ? 1u : 0u;          // inside this segment's own output
#if LZS_SEG_PLANES
            const uint32_t wp = (cpos + idx) & (kSegRing - 1u);
            const uint32_t hi_mine = ring_hi[wp & (kSegRing / 2u - 1u)];           // (the byte my entry's upper four bits go into: read early)
            const uint32_t got = ring_lo[sp] | (((ring_hi[sp & (kSegRing / 2u - 1u)] >> ((sp >> 10) << 2)) & 15u) << 8);
#else
            const uint32_t got = ring[sp];
#endif
            // produced by another wave: that far before my output -- unless it lies before the stream's out[0]: zero
            const uint32_t back = oo - from;
            const uint32_t outside = headroom + from >= oo ? (kSegOpen | back) : 0u;
            uint32_t val = inside ? got : outside;
            if (8u * sl < 7u) {
                const uint32_t lit = (uint32_t)(bits >> ((55u - 9u * (idx < 7u ? idx : 6u)) & 63u)) & 0xFFu;
                val = (is_lit & (second ^ 1u)) ? lit : val;
            }
#if !LZS_SEG_PLANES
            const uint32_t wp = (cpos + idx) & (kSegRing - 1u);
#endif
            const bool mine = idx < nwrite;
            // ... and out it goes (what lies past the capacity is the last step's, and nobody reads it)
            const uint32_t gpos = out_start + count + idx;
            if (mine && count + idx < room) {
#if LZS_SEG_PLANES
                const uint32_t nib = (wp >> 10) << 2;
                ring_lo[wp] = (uint8_t)val;
                ring_hi[wp & (kSegRing / 2u - 1u)] = (uint8_t)((hi_mine & ~(15u << nib)) | ((val >> 8) << nib));
#else
                ring[wp] = (uint16_t)val;
#endif
                const uint32_t og = val & kSegOpen ? val & (kSegOpen - 1u) : 0u;
                out[gpos] = (uint8_t)val;
                origin_g[gpos] = og ? out_start - og : kClean;
                tainted += og != 0u;
            }
        }
        count    = count + nwrite;
        cpos     = (cpos + nwrite) & (kSegRing - 1u);
        if (WIDE) {                                                // (never with TWO) 96 bits move up by `consume` < 64
            const uint32_t cs = consume & 63u;
            const uint64_t lo64 = (uint64_t)bits_lo << 32;
            const uint64_t carry = cs ? lo64 >> ((64u - cs) & 63u) : 0ull;
            bits = (bits << cs) | carry;
            bits_lo = (uint32_t)((lo64 << cs) >> 32);
        } else {
            bits <<= ((consume + (okB ? needB : 0u)) & 63u);                         // (at most 36 + 17: one shift for both tokens)
        }
        // (a segment that has stopped writes nothing any more -- nA and okB hang on `go`, `done` is for good -- so its
        // buffer, position, offset and flags need no selects to stay as they are)
        const uint32_t taken = consume + (okB ? needB : 0u);
        have     = have - taken;
        cur      = cur + taken;
        off      = okB ? oB : off_next;
        extended = okB ? (lenB == kTokenMax ? 1u : 0u) : ext_next;
        done    |= stop | (endm & (concat ? 0u : 1u));
    }
    // one add per wavefront
    for (int m = 32; m >= 1; m >>= 1) tainted += (uint32_t)__shfl_xor((int)tainted, m, 64);
    if (lane == 0 && tainted) atomicAdd(tainted_total, tainted);
}

// A whole segment of 0xFF bytes inside a running extension is nothing but nibbles of 15: it leaves
// in the state in which it was entered, and the host carries a long match across such segments
// without a round each.  2: and so are the first three bits after it (the last nibble that starts
// in the segment may reach that far into the next one).  One wavefront per segment, 16 bytes a lane.
__global__ __launch_bounds__(256)
void lzs_all_ones_kernel(const uint8_t *__restrict__ in, uint32_t n_all, uint32_t nseg, uint8_t *__restrict__ all_ones,
                         uint32_t kDecSeg, const uint32_t *__restrict__ seg_base, const uint32_t *__restrict__ seg_end)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = blockIdx.x * 4u + uniform(threadIdx.x >> 6);
    if (k >= nseg) return;
    const uint32_t sbase = seg_base ? uniform(seg_base[k]) : k * kDecSeg;
    const uint32_t n = seg_end ? uniform(seg_end[k]) : n_all;
    bool ones = (size_t)sbase + kDecSeg <= n;
    if (ones) {
        const uint8_t *p = in + sbase;
        if ((((uintptr_t)p) & 15u) == 0 && (kDecSeg & 15u) == 0) {
            for (uint32_t i = 16u * lane; i < kDecSeg && ones; i += 1024u) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p + i);
                ones = (v.x & v.y & v.z & v.w) == 0xFFFFFFFFu;
            }
        } else {
            for (uint32_t i = lane; i < kDecSeg && ones; i += 64u) ones = p[i] == 0xFFu;
        }
    }
    const bool all = __builtin_amdgcn_ballot_w64(!ones) == 0ull;
    const size_t after = (size_t)sbase + kDecSeg;
    if (lane == 0) all_ones[k] = !all ? 0 : (after < n && (in[after] & 0xE0u) == 0xE0u) ? 2 : 1;
}

__global__ __launch_bounds__(256)
void lzs_decode_stream_kernel(uint8_t *__restrict__ out, uint32_t cap, uint32_t *__restrict__ origin_g,
                              uint32_t *__restrict__ tainted_total,
                              const uint8_t *__restrict__ in, uint32_t n, uint32_t nseg,
                              const uint32_t *__restrict__ entry, const uint32_t *__restrict__ out_start,
                              uint32_t kDecSeg, uint32_t concat,
                              const uint32_t *__restrict__ seg_base, const uint32_t *__restrict__ seg_end,
                              const uint32_t *__restrict__ out_floor, const uint32_t *__restrict__ out_limit)
{
    __shared__ DecSegLds lds[4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = uniform(threadIdx.x >> 6);
    const uint32_t k = blockIdx.x * 4u + wv;
    if (k >= nseg) return;
    const uint32_t e = uniform(entry[k]);
    if (e & kSegStop) return;                                 // the stream ended before this segment
    const uint32_t sbase = seg_base ? uniform(seg_base[k]) : k * kDecSeg;
    if (seg_end) n = uniform(seg_end[k]);
    if (out_limit) cap = uniform(out_limit[k]);                // where this segment's stream must stop writing
    lzs_stream_segment<true>(in, n, sbase, e, nullptr, nullptr, out, cap, uniform(out_start[k]),
                             out_floor ? uniform(out_floor[k]) : 0u,
                             origin_g, tainted_total, &lds[wv], lane, kDecSeg, concat != 0u);
}

// One round of pointer jumping over the origins (each launch only trusts what earlier launches
// finished: a byte resolved in this round is marked with the round number and becomes a source in
// the next one).  `left` counts the bytes still open after the round.  A thread takes four
// consecutive bytes: one 16-byte load of their origins, up to four jumps per byte (the farthest
// origin that is still open is adopted), one 4-byte store of the values, one 16-byte store of
// the origins -- byte-wide stores and one jump per launch cost 6 rounds of 4-6 ms per GiB of
// text, this form 3 of ~3.
__device__ __forceinline__ uint32_t resolve_one(uint8_t *__restrict__ out, const uint32_t *__restrict__ origin_g,
                                                uint32_t o, uint32_t round, uint32_t &value, uint32_t &open)
{
    // o < kDoneBase: the position this byte is a copy of.  Follow it while it leads to open bytes.
#pragma unroll
    for (int jump = 0; jump < 4; jump++) {
        const uint32_t oo = origin_g[o];
        if (oo == kClean || (oo >= kDoneBase && (oo & 0xFFu) < round)) {   // final before this round: take its value
            value = out[o];
            return kDoneBase | round;
        }
        if (oo >= kDoneBase) break;                                        // resolved in this very round: next time
        o = oo;                                                            // open itself: look further back
    }
    open++;
    return o;
}

// One group of four bytes (words of `out`, uint4s of `origin_g`).  The four chains are followed in
// lock step -- four independent loads per jump, not sixteen dependent ones: a round is bound by
// the latency of these loads (~2 us each under load), not by their bytes.
template <bool LAST = false>
__device__ __forceinline__ void resolve_group(uint8_t *__restrict__ out, uint32_t *__restrict__ origin_g, uint32_t q,
                                              uint32_t round, uint32_t &open)
{
    const uint4 og = reinterpret_cast<const uint4 *>(origin_g)[q];
    if (og.x >= kDoneBase && og.y >= kDoneBase && og.z >= kDoneBase && og.w >= kDoneBase) return;
    uint32_t word = reinterpret_cast<const uint32_t *>(out)[q];
    uint32_t o[4] = {og.x, og.y, og.z, og.w};
    bool was_open[4], walking[4], take[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { was_open[i] = walking[i] = o[i] < kDoneBase; take[i] = false; }
#pragma unroll
    for (int jump = 0; jump < 4; jump++) {
        uint32_t oo[4];
#pragma unroll
        for (int i = 0; i < 4; i++) oo[i] = walking[i] ? origin_g[o[i]] : 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // final before this round: take its value; resolved in this very round: next time;
            // open itself: look further back
            const bool fin = oo[i] == kClean || (oo[i] >= kDoneBase && (oo[i] & 0xFFu) < round);
            take[i] = take[i] || (walking[i] && fin);
            walking[i] = walking[i] && oo[i] < kDoneBase;
            o[i] = walking[i] ? oo[i] : o[i];
        }
        if (!(walking[0] || walking[1] || walking[2] || walking[3])) break;
    }
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = take[i] ? out[o[i]] : 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (take[i]) { word = (word & ~(0xFFu << (8 * i))) | (v[i] << (8 * i)); o[i] = kDoneBase | round; }
        else if (was_open[i]) open++;
    }
    reinterpret_cast<uint32_t *>(out)[q] = word;
    // LAST: the pass that is expected to finish.  Nobody will ask for the marks of a group that is
    // done (4 GiB of stores per GiB of output), and without them the origins it keeps stay true
    // should another pass be needed after all.
    if (LAST && (take[0] || !was_open[0]) && (take[1] || !was_open[1]) && (take[2] || !was_open[2]) && (take[3] || !was_open[3])) return;
    reinterpret_cast<uint4 *>(origin_g)[q] = make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256)
void lzs_resolve_stream_kernel(uint8_t *__restrict__ out, uint32_t *__restrict__ origin_g, uint32_t total,
                               uint32_t round, uint32_t *__restrict__ left, uint32_t last)
{
    uint32_t open = 0;
    const bool words = (((uintptr_t)out) & 3u) == 0 && (((uintptr_t)origin_g) & 15u) == 0;
    const uint32_t groups = total >> 2;
    if (words && last)
        for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u)
            resolve_group<true>(out, origin_g, q, round, open);
    else if (words)
        for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u)
            resolve_group(out, origin_g, q, round, open);
    // the last 0..3 bytes -- or all of them when the buffers are not aligned for the wide form
    for (uint32_t p = (words ? groups * 4u : 0u) + blockIdx.x * 256u + threadIdx.x; p < total; p += gridDim.x * 256u) {
        const uint32_t o = origin_g[p];
        if (o >= kDoneBase) continue;
        uint32_t v = out[p];
        const uint32_t r = resolve_one(out, origin_g, o, round, v, open);
        if (r >= kDoneBase) out[p] = (uint8_t)v;
        origin_g[p] = r;
    }
    // one atomic per wavefront: one per thread is 19 M on one address, 3.4 ms a round
    open = wave_inclusive_sum(open);
    if ((threadIdx.x & 63u) == 63u && open) atomicAdd(left, open);
}

// The same, for the TAILS only.  Every origin DECODE records for a byte of segment s lies in the
// 2047 bytes in front of that segment (a copy reaches no further, and a chain of copies inside the
// segment ends where it leaves it), so all jumps land in the union of those tails -- a seventh of
// the output with 8 KiB segments of text.  The rounds of pointer jumping run on the tails alone
// (this kernel: one workgroup per segment, the groups of four bytes that reach into
// [start[s] - 2048, start[s]) and belong to no earlier segment's tail, so that each group has ONE
// owner); once they are final, every other byte is one jump from its value and a single pass of
// lzs_resolve_stream_kernel finishes the job.  Needs the word-aligned buffers (the host checks).
__global__ __launch_bounds__(256)
void lzs_resolve_tails_kernel(uint8_t *__restrict__ out, uint32_t *__restrict__ origin_g, uint32_t total,
                              const uint32_t *__restrict__ seg_start, uint32_t stride, uint32_t round,
                              uint32_t *__restrict__ left)
{
    const uint32_t s = blockIdx.x * stride;           // every stride-th segment's tail (see the chunks kernel)
    const uint32_t at = seg_start[s];
    const uint32_t groups = total >> 2;
    uint32_t hi = at ? ((at - 1u) >> 2) + 1u : 0u;                       // one past the group of byte at-1
    hi = hi < groups ? hi : groups;
    uint32_t lo = at > 2048u ? (at - 2048u) >> 2 : 0u;
    if (s) {
        const uint32_t prev = seg_start[s - stride];
        const uint32_t prev_hi = prev ? ((prev - 1u) >> 2) + 1u : 0u;   // the tail before owns up to here
        lo = lo > prev_hi ? lo : prev_hi;
    }
    uint32_t open = 0;
    for (uint32_t q = lo + threadIdx.x; q < hi; q += 256u)
        resolve_group(out, origin_g, q, round, open);
    // one atomic per wavefront: one per thread is 19 M on one address, 3.4 ms a round
    open = wave_inclusive_sum(open);
    if ((threadIdx.x & 63u) == 63u && open) atomicAdd(left, open);
}

// Pointer jumping pays a round (a pass over all tails, bound by the scattered loads) for every
// factor of five in chain length, and chains of copies of copies are as long as the stream.  But a
// chain only ever steps from a segment into the tail in front of it, so a workgroup that takes
// `per_chunk` consecutive segments IN ORDER needs no rounds: it keeps the state of the last 2047
// tail positions in an LDS ring (like a decoder's window: final value, or "open, copy of position e
// in front of the chunk"), and the tail bytes inside segment s (its last <= 2047 bytes: the tail of
// s + 1) look their origins up there.  Afterwards every tail byte is final or a copy of a byte in
// the 2047 bytes in front of its CHUNK; lzs_resolve_tails_kernel with stride = per_chunk settles
// those few (one in per_chunk of the tails: they stay in L2), and lzs_resolve_stream_kernel
// finishes everything in one pass of at most two jumps per byte.
// No workgroup reads what another writes: bytes in front of the chunk are named, never looked at.
__global__ __launch_bounds__(256)
void lzs_resolve_chunks_kernel(uint8_t *__restrict__ out, uint32_t *__restrict__ origin_g, uint32_t total,
                               const uint32_t *__restrict__ seg_start, uint32_t nseg, uint32_t per_chunk, uint32_t round)
{
    __shared__ uint16_t ring[2048];                   // by position & 2047: value, or 0x8000 | (position - ebase)
    const uint32_t s0 = blockIdx.x * per_chunk;
    uint32_t s1 = s0 + per_chunk;
    s1 = s1 < nseg - 1u ? s1 : nseg - 1u;             // the last segment's end is nobody's tail
    if (s0 >= s1) return;
    const uint32_t first = seg_start[s0];
    const uint32_t ebase = first - 2047u;             // (may wrap: only differences are used)
    for (uint32_t s = s0; s < s1; s++) {
        const uint32_t a = seg_start[s];
        uint32_t b = seg_start[s + 1];
        b = b < total ? b : total;
        const uint32_t u0 = b > a + 2047u ? b - 2047u : a;
        uint32_t ent[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t p = u0 + threadIdx.x + 256u * k;
            ent[k] = 0;
            if (p < b) {
                const uint32_t o = origin_g[p];
                if (o >= kDoneBase) ent[k] = out[p];                              // final already
                else if (o < first || s == s0) ent[k] = 0x8000u | ((o - ebase) & 0x7FFu);
                else {
                    const uint32_t r = ring[o & 2047u];                           // o in [a - 2047, a): kept below
                    ent[k] = r;
                    if (r & 0x8000u) origin_g[p] = ebase + (r & 0x7FFu);          // a copy of that byte, then
                    else { out[p] = (uint8_t)r; origin_g[p] = kDoneBase | round; }
                }
            }
        }
        __syncthreads();                                                          // all look-ups before the ring moves on
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t p = u0 + threadIdx.x + 256u * k;
            if (p < b) ring[p & 2047u] = (uint16_t)ent[k];
        }
        __syncthreads();
    }
}

// The same for a batch of blocks (lzs_decompress_batch of a small batch: every block cut into
// segments): origins never leave their block, so one workgroup per block jumps pointers until its
// block is done, with barriers instead of launches between the rounds.  In place: a byte whose
// origin is clean takes its value and becomes clean itself (value first, then the mark: release /
// acquire at workgroup scope), any other adopts its origin's origin -- whichever of the two a
// neighbour reads meanwhile is a valid origin of that byte.
__global__ __launch_bounds__(1024)
void lzs_resolve_blocks_kernel(uint8_t *__restrict__ out, uint32_t *__restrict__ origin_g, size_t out_stride,
                               const uint32_t *__restrict__ len)
{
    const uint32_t b = blockIdx.x;
    const uint32_t n = len[b];
    const uint32_t base = (uint32_t)(b * out_stride);
    for (;;) {
        int pending = 0;
        for (uint32_t p = base + threadIdx.x; p < base + n; p += 1024u) {
            const uint32_t o = origin_g[p];
            if (o == kClean) continue;
            const uint32_t oo = __hip_atomic_load(&origin_g[o], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (oo == kClean) {
                out[p] = out[o];
                __hip_atomic_store(&origin_g[p], kClean, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                origin_g[p] = oo;
                pending = 1;
            }
        }
        if (!__syncthreads_or(pending)) break;
    }
}
