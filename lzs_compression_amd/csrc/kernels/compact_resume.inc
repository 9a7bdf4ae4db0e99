// kernels/compact_resume.inc -- slot compaction; the resumable one-wavefront decoder of lzs_decompress_incremental().
// Part of lzs_kernels.hip (included there, inside its anonymous namespace); not a translation unit of its own.

// ---------------------------------------------------------------------------------
// Compaction of fixed-stride slots into one dense string.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(1024)
void lzs_scan_lengths_kernel(uint64_t *__restrict__ offsets, const uint32_t *__restrict__ len,
                             uint32_t nblocks)
{
    // single workgroup: each thread sums a contiguous chunk, then a block-wide scan of the sums
    __shared__ uint64_t partial[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nblocks + 1023u) / 1024u;
    const uint32_t lo = t * per < nblocks ? t * per : nblocks;
    const uint32_t hi = lo + per < nblocks ? lo + per : nblocks;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += len[i];
    partial[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t add = t >= d ? partial[t - d] : 0;
        __syncthreads();
        partial[t] += add;
        __syncthreads();
    }
    uint64_t run = partial[t] - sum;     // exclusive prefix of this chunk
    for (uint32_t i = lo; i < hi; i++) { offsets[i] = run; run += len[i]; }
    if (t == 1023) offsets[nblocks] = partial[1023];
}

__global__ __launch_bounds__(256)
void lzs_gather_slots_kernel(uint8_t *__restrict__ dense, const uint64_t *__restrict__ offsets,
                             const uint8_t *__restrict__ slots, size_t slot_stride,
                             const uint32_t *__restrict__ len, uint32_t nblocks)
{
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    const uint8_t *s = slots + (size_t)b * slot_stride;
    uint8_t *d = dense + offsets[b];
    const uint32_t n = len[b];
    // head bytes until d is 4-aligned, then dst-aligned words assembled from two aligned
    // source words, then tail bytes
    const uint32_t head = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
    const uint32_t h = head < n ? head : n;
    if (threadIdx.x < h) d[threadIdx.x] = s[threadIdx.x];
    const uint32_t words = (n - h) >> 2;
    const uint8_t *sb = s + h;
    const uint32_t shift = (uint32_t)((uintptr_t)sb & 3u);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(sb - shift);
    uint32_t *dw = reinterpret_cast<uint32_t *>(d + h);
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) {
        const uint32_t lo = sw[i];
        const uint32_t hi = shift ? sw[i + 1] : 0u;
        dw[i] = __builtin_amdgcn_alignbyte(hi, lo, shift);
    }
    const uint32_t done = h + 4 * words;
    if (threadIdx.x < n - done) d[done + threadIdx.x] = s[done + threadIdx.x];
}

// The same with slot b at src + src_off[b] -- the rooms of a packed compress launch (lzs_compact_packed_device; DESIGN.md 3.15).
__global__ __launch_bounds__(256)
void lzs_gather_packed_kernel(uint8_t *__restrict__ dense, const uint64_t *__restrict__ offsets,
                              const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                              const uint32_t *__restrict__ len, uint32_t nblocks)
{
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    const uint8_t *s = src + src_off[b];
    uint8_t *d = dense + offsets[b];
    const uint32_t n = len[b];
    // head bytes until d is 4-aligned, then dst-aligned words assembled from two aligned
    // source words, then tail bytes
    const uint32_t head = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
    const uint32_t h = head < n ? head : n;
    if (threadIdx.x < h) d[threadIdx.x] = s[threadIdx.x];
    const uint32_t words = (n - h) >> 2;
    const uint8_t *sb = s + h;
    const uint32_t shift = (uint32_t)((uintptr_t)sb & 3u);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(sb - shift);
    uint32_t *dw = reinterpret_cast<uint32_t *>(d + h);
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) {
        const uint32_t lo = sw[i];
        const uint32_t hi = shift ? sw[i + 1] : 0u;
        dw[i] = __builtin_amdgcn_alignbyte(hi, lo, shift);
    }
    const uint32_t done = h + 4 * words;
    if (threadIdx.x < n - done) d[done + threadIdx.x] = s[done + threadIdx.x];
}

// ---------------------------------------------------------------------------------
// lzs_decompress_incremental(): one call's worth of decoding, resumable.
// reference lzs-decompression.c:459-743 (a 9-state machine over a 32-bit queue; here the same
// stop rules at token granularity).  One wavefront.  `st` carries what the reference keeps in
// LzsDecompressParameters_t between calls: the bits of an unfinished token, the copy in progress
// (offset, bytes left, extended), and the last <= 2047 bytes of output as history.  The call
// stops when the input runs out (INPUT_STARVED, with INPUT_FINISHED if no bit is left), when the
// next byte has no room in `out` (NO_OUTPUT_BUFFER_SPACE, also in the middle of a copy), or after
// an end marker (END_MARKER: the pad bits up to the byte boundary are dropped, :564-576, and
// history is kept for what follows).  Whole unread input bytes are handed back (in_used).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64)
void lzs_decode_resume_kernel(lzs_dec_resume_t *__restrict__ st, const uint8_t *__restrict__ in, uint32_t n,
                              uint8_t *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t ring[kRingWords];
    uint8_t *ring8 = reinterpret_cast<uint8_t *>(ring);
    const uint32_t lane = threadIdx.x;
    const uint32_t base = uniform(st->hist_len);                  // ring position of out[0]
    // (history and output move as words: the small calls of the incremental interface run this
    // kernel on pinned HOST memory, where every byte access is a transaction of its own on the bus)
    const uint32_t *hist32 = reinterpret_cast<const uint32_t *>(st->hist);          // 4-aligned (offset 40 of the state)
    for (uint32_t i = lane; 4u * i < base; i += 64) ring[i] = hist32[i];
    __builtin_amdgcn_wave_barrier();
    // bytes [from, to) of the ring's positions to dst[0..), dst 4-aligned; whole words, then the last bytes
    const auto ring_to = [&](uint8_t *dst, uint32_t from, uint32_t to) {
        const uint32_t nbytes = to - from, nw = nbytes >> 2;
        uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst);
        for (uint32_t i = lane; i < nw; i += 64) {
            const uint32_t q = from + 4u * i, a = (q & kRingMask) >> 2;
            dst32[i] = __builtin_amdgcn_alignbyte(ring[(a + 1u) & (kRingWords - 1u)], ring[a], q);
        }
        for (uint32_t i = 4u * nw + lane; i < nbytes; i += 64) dst[i] = ring8[(from + i) & kRingMask];
    };

    uint64_t bits = (uint64_t)uniform(st->bitq) << 32;            // left-aligned
    uint32_t have = uniform(st->qlen);
    const uint32_t carried = have;                                // bits that are not from `in`
    uint32_t off = uniform(st->off), rem = uniform(st->rem);
    bool extended = uniform(st->extended) != 0;
    uint32_t ipos = 0;                                            // next input byte to feed (multiple of 4)
    uint32_t count = base, flushed = base;
    const uint32_t limit = base + cap;
    uint32_t status = 0;
    // The compressed input, 256 bytes (a word per lane) at a time and one batch ahead of use: a
    // dependent global load per word would cost its full latency every 4 bytes.
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(in);   // staged 4-aligned by the host
    const uint32_t nwords = (n + 3u) >> 2;
    uint32_t batch = 0;
    uint32_t cur = lane < nwords ? in32[lane] : 0u;
    uint32_t nxt = 64u + lane < nwords ? in32[64u + lane] : 0u;

    for (;;) {
        while (have <= 32 && ipos < n) {
            const uint32_t wi = ipos >> 2;
            if ((wi >> 6) != batch) {
                batch = wi >> 6;
                cur = nxt;
                const uint32_t at = 64u * (batch + 1u) + lane;
                nxt = at < nwords ? in32[at] : 0u;
            }
            uint32_t w = __builtin_bswap32((uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(wi & 63u)));
            const uint32_t nb = n - ipos < 4 ? n - ipos : 4;
            if (nb < 4) w &= ~0u << (8 * (4 - nb));
            bits |= (uint64_t)w << (32 - have);
            have += 8 * nb;
            ipos += 4;
        }
        // No bit left: the reference stops here whatever it was doing (:475-478, :492-496) -- also
        // with a copy pending, which then waits for the next call that brings input.
        if (have == 0) { status |= LZS_INC_INPUT_FINISHED | LZS_INC_INPUT_STARVED; break; }
        if (rem) {                                                 // :640-704
            const uint32_t room = limit - count;
            if (room == 0) { status |= LZS_INC_NO_OUTPUT_SPACE; break; }
            const uint32_t m = rem < room ? rem : room;
            __builtin_amdgcn_wave_barrier();
            uint32_t v = 0;
            if (lane < m) {
                const uint32_t k = off > 15u ? lane : lane % off;
                const uint32_t from = count + k;
                v = from >= off ? ring8[(from - off) & kRingMask] : 0u;   // before the history's start -> 0 (:676-683)
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < m) ring8[(count + lane) & kRingMask] = (uint8_t)v;
            count += m;
            rem -= m;
        } else {
            bool starved = false;
            if (extended) {                                        // :706-723
                if (have < 4) starved = true;
                else {
                    const uint32_t e = (uint32_t)(bits >> 60);
                    bits <<= 4; have -= 4;
                    rem = e;
                    if (e != kNibbleMax) extended = false;
                }
            } else if ((bits >> 63) == 0) {                        // literals :516-541, up to 7 at once
                if (have < 9) starved = true;
                else if (count >= limit) { status |= LZS_INC_NO_OUTPUT_SPACE; break; }
                else {
                    const uint64_t types = bits & 0x8040201008040200ull;
                    uint32_t k = (types ? (uint32_t)__builtin_clzll(types) : 64u) / 9u;
                    k = k < have / 9u ? k : have / 9u;
                    k = k < limit - count ? k : limit - count;
                    if (lane < k) ring8[(count + lane) & kRingMask] = (uint8_t)(bits >> (55u - 9u * lane));
                    count += k;
                    bits <<= 9u * k; have -= 9u * k;
                }
            } else {                                               // offset, then length or end marker
                const bool is_short = ((bits >> 62) & 1u) != 0;
                const uint32_t used = is_short ? 9u : 13u;
                if (have < used) starved = true;
                else {
                    const uint32_t o = is_short ? (uint32_t)(bits >> 55) & 0x7Fu : (uint32_t)(bits >> 51) & 0x7FFu;
                    if (o == 0) {
                        bits <<= used; have -= used;
                        if (is_short) {                            // end marker :564-576
                            const uint32_t pad = have & 7u;
                            bits <<= pad; have -= pad;
                            status |= LZS_INC_END_MARKER;
                            break;
                        }
                        off = 0;                                   // long offset 0: no copy (one-shot rule, :280)
                    } else {
                        const uint32_t code = (uint32_t)((bits << used) >> 60);
                        const uint32_t width = code < 0xCu ? 2u : 4u;
                        if (have < used + width) starved = true;
                        else {
                            const uint32_t len = code < 0xCu ? 2u + (code >> 2) : 5u + (code - 0xCu);
                            bits <<= used + width; have -= used + width;
                            off = o;
                            rem = len;
                            extended = len == kTokenMax;
                        }
                    }
                }
            }
            if (starved) { status |= LZS_INC_INPUT_STARVED; break; }     // the token's bits stay queued
        }
        if (count - flushed >= kTile) {                            // whole words go out; up to 3 bytes stay for the next time
            __builtin_amdgcn_wave_barrier();
            const uint32_t upto = flushed + ((count - flushed) & ~3u);
            if (((uintptr_t)out & 3u) == 0 && ((flushed - base) & 3u) == 0) ring_to(out + (flushed - base), flushed, upto);
            else for (uint32_t i = flushed + lane; i < upto; i += 64) out[i - base] = ring8[i & kRingMask];
            flushed = upto;
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (((uintptr_t)out & 3u) == 0 && ((flushed - base) & 3u) == 0) ring_to(out + (flushed - base), flushed, count);
    else for (uint32_t i = flushed + lane; i < count; i += 64) out[i - base] = ring8[i & kRingMask];

    // whole bytes of this call's input that were not needed go back to the caller
    const uint32_t fed = ipos < n ? ipos : n;
    const uint32_t consumed = carried + 8u * fed - have;          // bits used up in this call
    const uint32_t fed_left = consumed >= carried ? have : 8u * fed;
    // (a starved call keeps the unfinished token's bits, < 17, and takes all the input, as the
    // reference does: its callers read more only when inLength is 0)
    const uint32_t back = (status & LZS_INC_INPUT_STARVED) ? 0u : fed_left >> 3;
    have -= 8u * back;
    const uint32_t hist_len = count < kWindow ? count : kWindow;
    ring_to(st->hist, count - hist_len, count);
    if (lane == 0) {
        st->bitq = (uint32_t)(bits >> 32) & (have ? ~0u << (32u - have) : 0u);
        st->qlen = have;
        st->off = off; st->rem = rem; st->extended = extended ? 1u : 0u;
        st->hist_len = hist_len;
        st->in_used = fed - back;
        st->out_made = count - base;
        st->status = status;
    }
}

// LZS_VERIFY=N (lzs_hip_launch_compress): every N-th launch is run once more with CHAIN in its
// order-independent form into scratch slots, and this kernel compares the two results block by block --
// length and every byte; *bad counts the blocks that differ.  One workgroup per block.
__global__ __launch_bounds__(256)
void lzs_verify_slots_kernel(const uint8_t *__restrict__ a, const uint32_t *__restrict__ len_a,
                             const uint8_t *__restrict__ b, const uint32_t *__restrict__ len_b,
                             size_t stride_a, size_t stride_b, uint32_t nblocks, uint32_t *__restrict__ bad)
{
    const uint32_t k = blockIdx.x;
    if (k >= nblocks) return;
    const uint32_t n = len_a[k];
    uint32_t differs = len_b[k] != n ? 1u : 0u;
    const uint8_t *pa = a + (size_t)k * stride_a, *pb = b + (size_t)k * stride_b;
    for (uint32_t i = threadIdx.x; i < n && !differs; i += blockDim.x) differs = pa[i] != pb[i] ? 1u : 0u;
    if (__syncthreads_or((int)differs) && threadIdx.x == 0) atomicAdd(bad, 1u);
}

