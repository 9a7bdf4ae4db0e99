// kernels/compress_aux.inc -- what goes with the compress kernel and does not depend on its variant: the choice of a variant
// per block, the bit-level stitch of a stream's segments, the resume of a long match, the LDS ordering check.
// Part of lzs_kernels.hip (included there once, inside its anonymous namespace); not a translation unit of its own.

// Which variant of the compress kernel a block gets (round 5).  The variants differ in what they are tuned for, never in
// what they produce: small bucket tables and six workgroups per CU for blocks of few distinct grams (long matches: the
// kernel waits there, and a sixth workgroup is 13 % -- 344 -> 388 GB/s on the low-entropy class), one full step per pass of
// the SEARCH loop for blocks that are nearly all literals (91 -> 95 on the high-entropy class), the default for the rest.
// One wavefront per block counts the distinct 2-grams among the block's first 2048 positions in a 4096-bit hashed set
// (text ~430, the low-entropy class <= 53, random bytes ~1610 of the seeded workloads' blocks) and leaves the variant's
// code in out_len[b] -- free until the block's kernel writes the length there, and no length: lengths are below
// kClassCode.  No memory of its own, no host round trip: the launches are graph-capturable like the single one was.
constexpr uint32_t kClassCode = 0xFFFFFFF0u;         // | 1 default, | 2 few distinct grams, | 3 nearly all literals
constexpr uint32_t kClassFewMax = 160, kClassManyMin = 1200;
constexpr uint32_t kClassifyMinBlocks = 64;            // smaller launches take the default variant alone (three empty grids cost more than they gain)
// WHICH variants a launch runs is the host's guess, and never more than a guess: an empty grid of 16 384 workgroups costs
// ~50 us (measured: 0.11 ms for two of them beside 14.7 ms of text, 5 % of a low-entropy launch), so a launch only runs the
// variants that recent launches had blocks for -- `allow`, bit c for class c -- and this kernel gives a block whose own
// class is not among them to `catch_all` (any variant produces the same bytes).  What recent launches had: one workgroup in
// 64 stores the launch's id into h_seen[c] (pinned host memory) for the classes of its four blocks -- plain stores, a
// sample, no counting (counters that 4096 workgroups add to cost 0.2 ms in same-address atomics: measured, round 5) -- and the
// next launch reads the three words without waiting for anything.
__global__ __launch_bounds__(256)
void lzs_classify_blocks_kernel(uint32_t *__restrict__ out_len, const uint8_t *__restrict__ in, size_t in_stride,
                                const uint32_t *__restrict__ in_len, uint32_t in_len_uniform, uint32_t nblocks,
                                uint32_t allow, uint32_t catch_all, uint32_t *__restrict__ h_seen, uint32_t id)
{
    __shared__ uint32_t seen[4][128];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * 4u + wv;
    if (b >= nblocks) return;
    const uint8_t *src = in + (size_t)b * in_stride;
    const uint32_t n = in_len ? in_len[b] : in_len_uniform;
    uint32_t cls = 1u;
    if (n >= 2049u) {                                  // (a shorter block is over before the choice could matter)
        seen[wv][lane] = 0; seen[wv][64u + lane] = 0;
        __builtin_amdgcn_wave_barrier();
        // positions 32 lane .. 32 lane + 31 and the byte after them: two 16-byte loads a lane (byte loads at a stride of 32
        // were 33 requests of 64 sectors each for 2 KiB: the classifier took 0.1 ms of a 14.7 ms launch), the byte after from
        // the next lane's first word (the last lane's from memory: n >= 2049)
        const bool src16 = ((uintptr_t)src & 15u) == 0, src4 = ((uintptr_t)src & 3u) == 0;
        const uint4 lo = load16(src, 32u * lane, n, src16, src4), hi = load16(src, 32u * lane + 16u, n, src16, src4);
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t after = (uint32_t)__shfl_down((int)lo.x, 1, 64) & 0xFFu;
        if (lane == 63u) after = src[2048];
        uint32_t prev = w[0] & 0xFFu;
#pragma unroll
        for (uint32_t i = 1; i <= 32u; i++) {
            const uint32_t cur = i < 32u ? (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu : after;
            const uint32_t h = (((prev | (cur << 8)) * 40503u) >> 4) & 4095u;
            // (looked at first: on a block of runs all sixty-four lanes want the same bit thirty-two times over, and
            // same-address atomics of one instruction take their turns -- 0.1 ms of a 2.7 ms launch on the low-entropy class)
            if (!((seen[wv][h >> 5] >> (h & 31u)) & 1u)) atomicOr(&seen[wv][h >> 5], 1u << (h & 31u));
            prev = cur;
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t c2 = (uint32_t)__builtin_popcount(seen[wv][lane]) + (uint32_t)__builtin_popcount(seen[wv][64u + lane]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c2 += (uint32_t)__shfl_xor((int)c2, m, 64);
        cls = c2 <= kClassFewMax ? 2u : (c2 >= kClassManyMin ? 3u : 1u);
    }
    if (lane == 0) {
        out_len[b] = kClassCode | (((allow >> cls) & 1u) ? cls : catch_all);
        if (h_seen && (blockIdx.x & 63u) == 0u) __hip_atomic_store(&h_seen[cls], id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The same for a packed launch (lzs_compress_packed_wg_kernel; DESIGN.md 3.15): block b lies at in + in_off[b]; the counting and the
// thresholds are those above, line for line (a copy: a body shared with lzs_classify_blocks_kernel moved that kernel's
// instructions).  An entry that is not a block gets its length, 0, HERE: that is no variant's code, so none of them serves it.
__global__ __launch_bounds__(256)
void lzs_classify_packed_kernel(uint32_t *__restrict__ out_len, const uint64_t *__restrict__ out_off, const uint8_t *__restrict__ in,
                                const uint64_t *__restrict__ in_off, const uint32_t *__restrict__ in_len, uint32_t nblocks,
                                uint32_t allow, uint32_t catch_all, uint32_t *__restrict__ h_seen, uint32_t id)
{
    __shared__ uint32_t seen[4][128];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * 4u + wv;
    if (b >= nblocks) return;
    uint64_t from, to;
    uint32_t n, room;
    if (!packed_entry(in_off, in_len, out_off, b, from, n, to, room)) {
        if (lane == 0) out_len[b] = 0;
        return;
    }
    const uint8_t *src = in + from;
    uint32_t cls = 1u;
    if (n >= 2049u) {                                  // (a shorter block is over before the choice could matter)
        seen[wv][lane] = 0; seen[wv][64u + lane] = 0;
        __builtin_amdgcn_wave_barrier();
        // positions 32 lane .. 32 lane + 31 and the byte after them: two 16-byte loads a lane (byte loads at a stride of 32
        // were 33 requests of 64 sectors each for 2 KiB: the classifier took 0.1 ms of a 14.7 ms launch), the byte after from
        // the next lane's first word (the last lane's from memory: n >= 2049)
        const bool src16 = ((uintptr_t)src & 15u) == 0, src4 = ((uintptr_t)src & 3u) == 0;
        const uint4 lo = load16(src, 32u * lane, n, src16, src4), hi = load16(src, 32u * lane + 16u, n, src16, src4);
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t after = (uint32_t)__shfl_down((int)lo.x, 1, 64) & 0xFFu;
        if (lane == 63u) after = src[2048];
        uint32_t prev = w[0] & 0xFFu;
#pragma unroll
        for (uint32_t i = 1; i <= 32u; i++) {
            const uint32_t cur = i < 32u ? (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu : after;
            const uint32_t h = (((prev | (cur << 8)) * 40503u) >> 4) & 4095u;
            // (looked at first: on a block of runs all sixty-four lanes want the same bit thirty-two times over, and
            // same-address atomics of one instruction take their turns -- 0.1 ms of a 2.7 ms launch on the low-entropy class)
            if (!((seen[wv][h >> 5] >> (h & 31u)) & 1u)) atomicOr(&seen[wv][h >> 5], 1u << (h & 31u));
            prev = cur;
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t c2 = (uint32_t)__builtin_popcount(seen[wv][lane]) + (uint32_t)__builtin_popcount(seen[wv][64u + lane]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c2 += (uint32_t)__shfl_xor((int)c2, m, 64);
        cls = c2 <= kClassFewMax ? 2u : (c2 >= kClassManyMin ? 3u : 1u);
    }
    if (lane == 0) {
        out_len[b] = kClassCode | (((allow >> cls) & 1u) ? cls : catch_all);
        if (h_seen && (blockIdx.x & 63u) == 0u) __hip_atomic_store(&h_seen[cls], id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// d_bound[b] = LZS_COMPRESSED_MAX(length of packed block b), 0 for an entry that is not a block: the rooms' sizes before
// compression (lzs_compressed_bound_packed_device).  At most 0xC0000000 + 0x18000000 + 3: it fits 32 bits.
__global__ __launch_bounds__(256)
void lzs_compressed_bound_packed_kernel(uint32_t *__restrict__ bound, const uint64_t *__restrict__ in_off,
                                        const uint32_t *__restrict__ in_len, uint32_t nblocks)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nblocks) return;
    uint64_t len;
    bool ok = true;
    if (in_len) {
        len = in_len[b];
    } else {
        const uint64_t from = in_off[b], next = in_off[b + 1u];
        ok = next >= from;
        len = next - from;
    }
    ok = ok && len <= 0xC0000000ull;                               // LZS_BLOCK_MAX
    bound[b] = ok ? (uint32_t)(len + (len + 7u) / 8u + 3u) : 0u;
}

// Segment k's bits (nbits[k] of them, MSB first from bit 0 of its slot) go to bit bit_at[k] of the
// stream; the last segment is followed by the end marker 1 1 0000000.  `out` is 4-aligned and
// zeroed.  A destination word is assembled from the two source words it spans (round 6: rounds 1-5 ORed every source
// word into its two destination words, two atomics a word): the words that hold this segment's bits alone -- all but
// the first, which the segment before may share, and those from the word of the segment's last bit on, which the next
// one may -- are plain stores; the boundary words are ORed in.
__global__ __launch_bounds__(256)
void lzs_stitch_segments_kernel(uint8_t *__restrict__ out, const uint8_t *__restrict__ slots, size_t slot_stride,
                                const unsigned long long *__restrict__ bit_at,
                                const unsigned long long *__restrict__ nbits, uint32_t nseg, uint32_t end_marker)
{
    const uint32_t k = blockIdx.x;
    if (k >= nseg) return;
    const unsigned long long at = bit_at[k];
    const bool fits = nbits[k] <= 8ull * slot_stride;              // else its bits are ORed in directly
    const uint32_t nb = fits ? (uint32_t)nbits[k] : 0u;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(slots + (size_t)k * slot_stride);
    unsigned int *dst = reinterpret_cast<unsigned int *>(out) + (at >> 5);
    const uint32_t sh = (uint32_t)(at & 31ull);
    const uint32_t words = (nb + 31u) >> 5;
    const uint32_t tail = (nb & 31u) ? ~0u << (32u - (nb & 31u)) : ~0u;   // the bits of the last source word that count
    const uint32_t shared = (sh + nb) >> 5;                        // destination word of the first bit after mine (words - 1 or words)
    for (uint32_t j = threadIdx.x; j <= words; j += blockDim.x) {  // destination word j of the segment
        uint32_t cur = 0, prev = 0;                                // big-endian: stream bit 32j is the MSB of source word j
        if (j < words) cur = __builtin_bswap32(src[j]) & (j == words - 1u ? tail : ~0u);
        if (j > 0u && sh) prev = __builtin_bswap32(src[j - 1u]) & (j == words ? tail : ~0u);
        const uint32_t v = (cur >> sh) | (sh ? prev << (32u - sh) : 0u);
        if (j > 0u && j < shared) dst[j] = __builtin_bswap32(v);
        else if (v) atomicOr(dst + j, __builtin_bswap32(v));
    }
    if (end_marker && k == nseg - 1u && threadIdx.x == 0) {        // end marker after the last bit
        const unsigned long long end = at + nbits[k];
        const uint32_t s2 = (uint32_t)(end & 31ull);
        const unsigned long long m = (unsigned long long)0x180u << (64u - 9u - s2);   // 9 bits, left-aligned after s2
        unsigned int *d2 = reinterpret_cast<unsigned int *>(out) + (end >> 5);
        atomicOr(d2, __builtin_bswap32((uint32_t)(m >> 32)));
        if ((uint32_t)m) atomicOr(d2 + 1, __builtin_bswap32((uint32_t)m));
    }
}

// The same for the segments of the blocks of a batch (lzs_compress_segments_batch_kernel's tables; DESIGN.md 3.19): segment k's
// bits go to bit bit_at[k] of ITS BLOCK's output, out + b out_stride (4-aligned, zeroed as far as it is written), and the end
// marker follows the last segment of every block -- the one that reaches blk_len[b]; a block without a byte has one segment
// without a bit and is nothing but the marker.  No store, plain or ORed, leaves the block's capw words (its capacity rounded up
// to a word, within its out_stride bytes by the caller's check): a destination word at or past them is dropped.
__global__ __launch_bounds__(256)
void lzs_stitch_segments_batch_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t capw,
                                      const uint8_t *__restrict__ slots, size_t slot_stride,
                                      const unsigned long long *__restrict__ bit_at, const unsigned long long *__restrict__ nbits,
                                      const uint32_t *__restrict__ seg_block, const uint32_t *__restrict__ seg_start,
                                      const uint32_t *__restrict__ blk_len, uint32_t seg, uint32_t nseg)
{
    const uint32_t k = blockIdx.x;
    if (k >= nseg) return;
    const uint32_t b = uniform(seg_block[k]), s = uniform(seg_start[k]), n = uniform(blk_len[b]);
    const unsigned long long at = bit_at[k], mine = nbits[k];
    const bool fits = mine <= 8ull * slot_stride;                  // else its bits are ORed in directly
    const uint32_t nb = fits ? (uint32_t)mine : 0u;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(slots + (size_t)k * slot_stride);
    unsigned int *blk = reinterpret_cast<unsigned int *>(out + (size_t)b * out_stride);
    const unsigned long long w0 = at >> 5;                         // destination word of the segment's first bit
    const uint32_t sh = (uint32_t)(at & 31ull);
    const uint32_t words = (nb + 31u) >> 5;
    const uint32_t tail = (nb & 31u) ? ~0u << (32u - (nb & 31u)) : ~0u;
    const uint32_t shared = (sh + nb) >> 5;
    for (uint32_t j = threadIdx.x; j <= words; j += blockDim.x) {
        if (w0 + j >= capw) break;                                 // (ascending in j: the rest lies behind the capacity too)
        uint32_t cur = 0, prev = 0;
        if (j < words) cur = __builtin_bswap32(src[j]) & (j == words - 1u ? tail : ~0u);
        if (j > 0u && sh) prev = __builtin_bswap32(src[j - 1u]) & (j == words ? tail : ~0u);
        const uint32_t v = (cur >> sh) | (sh ? prev << (32u - sh) : 0u);
        if (j > 0u && j < shared) blk[w0 + j] = __builtin_bswap32(v);
        else if (v) atomicOr(blk + w0 + j, __builtin_bswap32(v));
    }
    if (n - s <= seg && threadIdx.x == 0) {                        // the block's last segment: the end marker after its last bit
        const unsigned long long end = at + mine;
        const uint32_t s2 = (uint32_t)(end & 31ull);
        const unsigned long long m = (unsigned long long)0x180u << (64u - 9u - s2);
        const unsigned long long w2 = end >> 5;
        if (w2 < capw) atomicOr(blk + w2, __builtin_bswap32((uint32_t)(m >> 32)));
        if ((uint32_t)m && w2 + 1u < capw) atomicOr(blk + w2 + 1u, __builtin_bswap32((uint32_t)m));
    }
}

// A piece of a stream that begins inside a long match (lzs_compress_incremental: the call before
// ended with the match still running, state COMPRESS_EXTENDED of lzs-compression.c:750-776).  One
// wavefront measures how far in[c0..n) goes on repeating what lies `off` before it and writes the
// length nibbles at bit `bit0` of the zeroed, 4-aligned `out`: 1111 for every 15 bytes, then the
// closing nibble -- unless the run reaches the end of the data and more may follow (!last): then
// only the full 15s are written and the match stays open.  result: {next position, still open,
// bits written (low, high)}.
__global__ __launch_bounds__(64)
void lzs_extend_resume_kernel(uint8_t *__restrict__ out, uint32_t bit0, const uint8_t *__restrict__ in,
                              uint32_t n, uint32_t c0, uint32_t off, uint32_t last, uint32_t *__restrict__ result)
{
    const uint32_t lane = threadIdx.x;
    uint32_t c = c0;
    for (;;) {                                                     // 256 bytes a round, 4 per lane
        const uint32_t q = c + 4u * lane;
        uint32_t eq = 0;
        while (eq < 4u && q + eq < n && in[q + eq] == in[q + eq - off]) eq++;
        const uint64_t stops = __builtin_amdgcn_ballot_w64(eq < 4u);
        if (stops) {
            const uint32_t l = uniform((uint32_t)__builtin_ctzll(stops));
            c += 4u * l + (uint32_t)__builtin_amdgcn_readlane((int)eq, (int)l);
            break;
        }
        c += 256u;
    }
    const uint32_t run = c - c0;
    const bool open = c == n && !last;
    const uint32_t full = run / kNibbleMax;
    const unsigned long long ones_end = (unsigned long long)bit0 + 4ull * full;
    unsigned int *dst = reinterpret_cast<unsigned int *>(out);
    for (unsigned long long w = (bit0 >> 5) + lane; w <= (ones_end >> 5) && 4ull * full; w += 64) {
        const unsigned long long lo = w * 32ull > bit0 ? w * 32ull : bit0;
        const unsigned long long hi = (w + 1ull) * 32ull < ones_end ? (w + 1ull) * 32ull : ones_end;
        if (hi > lo) {
            const uint32_t a = (uint32_t)(lo - w * 32ull), b = (uint32_t)(hi - w * 32ull);    // bits [a, b) of the word, MSB first
            const uint32_t m = (~0u >> a) & (b == 32u ? ~0u : ~(~0u >> b));
            atomicOr(dst + w, __builtin_bswap32(m));
        }
    }
    if (!open && lane == 0) {
        const uint32_t s2 = (uint32_t)(ones_end & 31ull);
        const unsigned long long m = (unsigned long long)(run - kNibbleMax * full) << (64u - 4u - s2);
        unsigned int *d2 = dst + (ones_end >> 5);
        if ((uint32_t)(m >> 32)) atomicOr(d2, __builtin_bswap32((uint32_t)(m >> 32)));
        if ((uint32_t)m) atomicOr(d2 + 1, __builtin_bswap32((uint32_t)m));
    }
    if (lane == 0) {
        const unsigned long long bits = 4ull * full + (open ? 0ull : 4ull);
        result[0] = open ? c0 + kNibbleMax * full : c;
        result[1] = open ? 1u : 0u;
        result[2] = (uint32_t)bits; result[3] = (uint32_t)(bits >> 32);
    }
}

// Does this device apply the lanes of ONE returning LDS exchange that hit the same address in
// ascending lane order (each lane receives what its nearest lower neighbour stored)?  CHAIN's
// fast form rests on it and it is a measured property of gfx950, not an ISA promise -- so the
// library asks the device itself, once per device, before the first compress launch
// (lzs_hip_chain_mode): `npat` wave-sized conflict patterns drawn from a counter PRNG -- 1 to 64
// distinct addresses, same-bank strides, runs, and every other pattern with some lanes redirected
// to a word of their own the way CHAIN redirects lanes that do not insert.  *bad counts lanes
// that received anything else.
__global__ __launch_bounds__(256)
void lzs_lds_order_check_kernel(uint32_t *__restrict__ bad, uint32_t npat)
{
    __shared__ uint32_t tab[4][2048 + 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t *t = tab[wv];
    uint32_t wrong = 0;
    for (uint32_t pat = blockIdx.x * 4u + wv; pat < npat; pat += gridDim.x * 4u) {
        uint64_t x = ((uint64_t)pat << 8 | lane) * 0x9E3779B97F4A7C15ull + 0xD1342543DE82EF95ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; x ^= x >> 31;
        uint32_t v = (uint32_t)(x >> 20);
        const uint32_t mode = pat & 7u;
        if (mode < 4u) v &= (1u << (mode + 1u)) - 1u;
        else if (mode == 4u) v = (v & 7u) * 32u;
        else if (mode == 5u) v = (v & 15u) * 64u + ((v >> 8) & 1u);
        else if (mode == 6u) v &= 2047u;
        else v = (lane / 5u) * 33u;
        const uint32_t a = v & 2047u;
        const bool active = ((pat >> 3) & 1u) == 0u || ((x >> 13) & 3u) != 0u;
        uint32_t expect = 0;                                       // nearest lower ACTIVE lane with my address (+1), else 0
        for (uint32_t l = 0; l < 64u; l++) {
            const uint32_t al = (uint32_t)__shfl((int)a, (int)l, 64);
            const int act = __shfl((int)active, (int)l, 64);
            if (l < lane && al == a && act) expect = l + 1u;
        }
        t[a] = 0;
        __builtin_amdgcn_wave_barrier();
        uint32_t *const where = active ? &t[a] : &t[2048u + lane];
        const uint32_t got = __hip_atomic_exchange(where, lane + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_wave_barrier();
        wrong += (active && got != expect) ? 1u : 0u;
    }
    if (wrong) atomicAdd(bad, wrong);
}
