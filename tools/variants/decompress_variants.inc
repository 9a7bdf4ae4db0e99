struct __attribute__((aligned(16))) DecLds {
    uint32_t ring[kRingWords];     // output window
    uint32_t inbuf[kTile / 4];     // compressed input tile
};

__global__ __launch_bounds__(kWavesPerWG * 64)
void lzs_decompress_blocks_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                  uint32_t *__restrict__ out_len,
                                  const uint8_t *__restrict__ in, size_t in_stride,
                                  const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                  uint32_t nblocks, uint32_t concat)
{
    __shared__ DecLds lds[kWavesPerWG];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv   = uniform(threadIdx.x >> 6);   // wave-uniform, and the compiler knows it
    const uint32_t b    = blockIdx.x * kWavesPerWG + wv;
    if (b >= nblocks) return;

    DecLds &L = lds[wv];
    uint8_t *ring8 = reinterpret_cast<uint8_t *>(L.ring);
    const uint8_t *src = in + (size_t)b * in_stride;
    const uint32_t n   = in_len ? in_len[b] : in_len_uniform;
    const bool src16   = ((uintptr_t)src & 15u) == 0;
    uint8_t *dst       = out + (size_t)b * out_stride;
    const bool dst16   = ((uintptr_t)dst & 15u) == 0;
    const uint32_t cap = out_cap;

    uint64_t bits = 0;        // left-aligned bit buffer
    uint32_t have = 0;        // valid bits in `bits`
    uint32_t ipos = 0;        // next input byte to feed (multiple of 4)
    uint32_t itile = 0;       // inbuf holds input [itile-1024, itile)
    uint32_t count = 0;       // bytes produced
    uint32_t flushed = 0;     // bytes stored to HBM (multiple of kTile)
    uint32_t off = 0;
    bool extended = false;

    for (;;) {
        // ---- refill (lzs-decompression.c:181-187): top up to > 32 bits while input lasts
        while (have <= 32 && ipos < n) {
            if (ipos >= itile) {
                const uint32_t p = itile + 16 * lane;
                *reinterpret_cast<uint4 *>(&L.inbuf[(p & (kTile - 1)) >> 2]) = load16(src, p, n, src16);
                itile += kTile;
                __builtin_amdgcn_wave_barrier();
            }
            uint32_t w = uniform(__builtin_bswap32(L.inbuf[(ipos & (kTile - 1)) >> 2]));
            const uint32_t nb = n - ipos < 4 ? n - ipos : 4;     // bytes that really exist
            if (nb < 4) w &= ~0u << (8 * (4 - nb));
            bits |= (uint64_t)w << (32 - have);
            have += 8 * nb;
            ipos += 4;
        }
        if (have == 0 || count >= cap) break;                      // :189, :200

        uint32_t copy_len = 0;
        if (extended) {                                            // :370-406
            if (have < 4) break;
            const uint32_t e = (uint32_t)(bits >> 60);
            bits <<= 4; have -= 4;
            copy_len = e;
            if (e != kNibbleMax) extended = false;
        } else if ((bits >> 63) == 0 && have >= 9) {
            // a run of literals (:217-233), up to 7 at once: token i of an all-literal run starts
            // at bit 63 - 9i, so the first set type bit among those tells how long the run is
            const uint64_t types = bits & 0x8040201008040200ull;
            uint32_t k = (types ? (uint32_t)__builtin_clzll(types) : 64u) / 9u;
            k = k < have / 9u ? k : have / 9u;
            k = k < cap - count ? k : cap - count;
            if (lane < k) ring8[(count + lane) & kRingMask] = (uint8_t)(bits >> (55u - 9u * lane));
            count += k;
            bits <<= 9u * k; have -= 9u * k;
        } else if (have > 32 && (bits >> 63) != 0) {
            // a match token whose bits are all certainly there (at most 17 + 4 of more than 32):
            // same decoding as below without the per-field "enough bits left?" tests
            const uint32_t top = (uint32_t)(bits >> 43);           // 1 s ooooooo[oooo] cccc ...
            const bool is_short = (top >> 19) & 1u;
            const uint32_t o = is_short ? (top >> 12) & 0x7Fu : (top >> 8) & 0x7FFu;
            const uint32_t used = is_short ? 9u : 13u;
            if (o == 0) {
                bits <<= used; have -= used;
                if (is_short) {                                    // end marker (:255-260 / :564-576)
                    if (!concat) break;
                    const uint32_t pad = have & 7u;
                    bits <<= pad; have -= pad;
                } else {
                    off = 0;                                       // long offset 0: no copy (:280)
                }
                continue;
            }
            const uint32_t code = (is_short ? top >> 8 : top >> 4) & 0xFu;
            const uint32_t len = code < 0xC ? 2 + (code >> 2) : 5 + (code - 0xC);
            const uint32_t width = code < 0xC ? 2u : 4u;
            bits <<= used + width; have -= used + width;
            off = o;
            if (len == kTokenMax) extended = true;
            copy_len = len;
        } else {
            const uint32_t is_match = (uint32_t)(bits >> 63);
            bits <<= 1; have -= 1;
            if (!is_match) {                                       // literal :217-233
                if (have < 8) break;
                const uint32_t byte = (uint32_t)(bits >> 56);
                bits <<= 8; have -= 8;
                if (lane == 0) ring8[count & kRingMask] = (uint8_t)byte;
                count += 1;
            } else {
                if (have < 1) break;                               // :238-241
                const uint32_t is_short = (uint32_t)(bits >> 63);
                bits <<= 1; have -= 1;
                if (is_short) {                                    // :248-260
                    if (have < 7) break;
                    off = (uint32_t)(bits >> 57);
                    bits <<= 7; have -= 7;
                    if (off == 0) {                                // end marker
                        if (!concat) break;                        // one-shot rule: stop (:255-260)
                        // file rule (the incremental decoder, :564-576): drop the pad bits up
                        // to the byte boundary and go on with the next stream
                        const uint32_t pad = have & 7u;
                        bits <<= pad; have -= pad;
                        continue;
                    }
                } else {                                           // :272-279
                    if (have < 11) break;
                    off = (uint32_t)(bits >> 53);
                    bits <<= 11; have -= 11;
                }
                if (off != 0) {                                    // :280
                    const uint32_t code = (uint32_t)(bits >> 60);  // :103-120, :325-342
                    uint32_t len, width;
                    if (code < 0xC) { len = 2 + (code >> 2); width = 2; }
                    else            { len = 5 + (code - 0xC); width = 4; }
                    if (have < width) break;
                    bits <<= width; have -= width;
                    if (len == kTokenMax) extended = true;
                    copy_len = len;
                }
            }
        }

        if (copy_len) {                                            // :346-365, :381-400
            const uint32_t room = cap - count;
            const uint32_t m = copy_len < room ? copy_len : room;
            __builtin_amdgcn_wave_barrier();
            uint32_t v = 0;
            if (lane < m) {
                // overlap replicates with period `off`; m <= 15, so only short offsets wrap
                // (`off` is wave-uniform: the division is skipped for the common long offsets)
                const uint32_t k = off > 15u ? lane : lane % off;
                const uint32_t from = count + k;                   // position + off of the source
                v = from >= off ? ring8[(from - off) & kRingMask] : 0u;   // before out[0] -> 0
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < m) ring8[(count + lane) & kRingMask] = (uint8_t)v;
            count += m;
        }

        // ---- drain whole tiles of finished output
        while (count - flushed >= kTile) {
            __builtin_amdgcn_wave_barrier();
            const uint32_t p = flushed + 16 * lane;
            const uint4 v = *reinterpret_cast<const uint4 *>(&L.ring[(p & kRingMask) >> 2]);
            if (dst16) {
                *reinterpret_cast<uint4 *>(dst + p) = v;
            } else {
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                for (uint32_t k = 0; k < 16; k++) dst[p + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
            flushed += kTile;
        }
        if (count >= cap) break;                                   // mid-copy stop :361-364
    }

    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = flushed + lane; i < count; i += 64) dst[i] = ring8[i & kRingMask];
    if (lane == 0) out_len[b] = count;
}

// ---------------------------------------------------------------------------------
// lzs_decompress() per block, second version (round 1's default).  Same rules, same wave-per-stream
// shape; what changed is where the instructions go.  The first version spent 29 scalar
// instructions per output byte and saturated the CU's one scalar unit (rocprofv3: 3.1e10 SALU per
// GiB = 93 % of its issue slots) -- its compressed input went HBM -> LDS tile -> ds_read ->
// v_readfirstlane, and its conditions were combined as lane masks.  Here the compressed stream is
// read by plain word loads one word ahead of use (no LDS tile), the token decode is nested single
// compares, and the fields of a match token are extracted on the (idle) vector unit and come back
// packed through one v_readfirstlane.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kWavesPerWG * 64)
void lzs_decompress_blocks_v2_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                     uint32_t *__restrict__ out_len,
                                     const uint8_t *__restrict__ in, size_t in_stride,
                                     const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                     uint32_t nblocks, uint32_t concat)
{
    __shared__ uint32_t rings[kWavesPerWG][kRingWords];           // the OUTPUT's sliding window
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv   = uniform(threadIdx.x >> 6);
    const uint32_t b    = blockIdx.x * kWavesPerWG + wv;
    if (b >= nblocks) return;

    uint32_t *ring = rings[wv];
    uint8_t *ring8 = reinterpret_cast<uint8_t *>(ring);
    const uint8_t *src = in + (size_t)b * in_stride;
    const uint32_t n   = uniform(in_len ? in_len[b] : in_len_uniform);
    uint8_t *dst       = out + (size_t)b * out_stride;
    const bool dst16   = ((uintptr_t)dst & 15u) == 0;
    const uint32_t cap = out_cap;

    // ---- the input as aligned words: word j holds stream bytes [4j - skew, 4j - skew + 4)
    const uint32_t skew = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(src - skew);
    const uint32_t nwords = n ? (skew + n + 3u) >> 2 : 0u;         // words that hold stream bytes
    uint64_t bits = 0;        // left-aligned bit buffer
    uint32_t have = 0;        // valid bits in `bits`
    uint32_t pos  = 0;        // stream bytes fed so far
    uint32_t wi   = 0;        // next word to feed
    uint32_t nextw = 0;       // that word, loaded ahead of use
    if (nwords) {
        uint32_t w = __builtin_bswap32(w32[0]) << (8u * skew);
        const uint32_t avail = 4u - skew < n ? 4u - skew : n;
        if (avail < 4u) w &= ~0u << (32u - 8u * avail);
        bits = (uint64_t)w << 32;
        have = 8u * avail;
        pos = avail;
        wi = 1;
        if (nwords > 1u) nextw = w32[1];
    }
    uint32_t count = 0;       // bytes produced
    uint32_t flushed = 0;     // bytes stored to HBM (multiple of kTile)
    uint32_t off = 0;
    uint32_t extended = 0;

    for (;;) {
        // ---- refill (lzs-decompression.c:181-187).  One word per token is enough: no token path
        // below takes more than 32 bits except a run of literals, which takes what is there.
        if (have <= 32u) {
            if (pos < n) {
                uint32_t w = __builtin_bswap32(nextw);
                const uint32_t rem = n - pos;
                const uint32_t nb = rem < 4u ? rem : 4u;           // bytes that really exist
                if (rem < 4u) w &= ~0u << (32u - 8u * rem);
                bits |= (uint64_t)w << (32u - have);
                have += 8u * nb;
                pos += nb;
                wi += 1u;
                if (wi < nwords) nextw = w32[wi];
            }
        }
        if (have == 0u) break;                                     // :189
        if (count >= cap) break;                                   // :200, and mid-copy :361-364
        const uint32_t room = cap - count;

        uint32_t copy_len = 0;
        const uint32_t top = (uint32_t)(bits >> 32);
        if (extended) {                                            // :370-406
            if (have < 4u) break;
            const uint32_t e = top >> 28;
            bits <<= 4; have -= 4u;
            copy_len = e;
            extended = e == kNibbleMax ? 1u : 0u;
        } else if ((int32_t)top >= 0) {
            // a run of literals (:217-233), up to 7 at once: token i of an all-literal run starts
            // at bit 63 - 9i, so the first set type bit among those tells how long the run is
            if (have < 9u) break;                                  // type bit, then 8 more or stop (:220-223)
            // (counted on the vector unit, like the match fields below)
            const uint32_t th = opaque(top) & 0x80402010u, tl = opaque((uint32_t)bits) & 0x08040200u;
            const uint32_t lead = th ? (uint32_t)__builtin_clz(th) : (tl ? 32u + (uint32_t)__builtin_clz(tl) : 64u);
            uint32_t kv = (lead * 57u) >> 9;                       // lead / 9 for lead <= 64
            const uint32_t fitv = (opaque(have) * 57u) >> 9;       // have / 9 for have <= 64
            kv = kv < fitv ? kv : fitv;
            kv = kv < room ? kv : room;
            const uint32_t k = uniform(kv);
            if (lane < kv) ring8[(count + lane) & kRingMask] = (uint8_t)(bits >> (55u - 9u * lane));
            count += k;
            bits <<= 9u * k; have -= 9u * k;
        } else {
            // a match token: 1 s ooooooo[oooo] cccc (:238-342).  Every field is decoded from the
            // zero-padded buffer without asking whether its bits exist; the ONE test on `need`
            // covers all the "not enough bits: stop" exits of the reference (:240,250,274,334),
            // because a token produces nothing before its last field is read, and bits can only
            // be missing when the input is exhausted (the refill above keeps more than a token's
            // worth otherwise).
            // field extraction on the vector unit (the scalar unit is the bottleneck): the values
            // are the same in every lane and come back through v_readfirstlane
            const uint32_t t = opaque(top) >> 11;
            const bool is_short_v = (t >> 19) & 1u;
            const uint32_t o_v = is_short_v ? (t >> 12) & 0x7Fu : (t >> 8) & 0x7FFu;
            const uint32_t used_v = is_short_v ? 9u : 13u;
            const uint32_t code_v = (is_short_v ? t >> 8 : t >> 4) & 0xFu;
            const uint32_t len_v = code_v < 0xCu ? 2u + (code_v >> 2) : code_v - 7u;
            const uint32_t width_v = code_v < 0xCu ? 2u : 4u;
            // packed: o (11) | used (4) << 11 | len (4) << 15 | width (3) << 19 | is_short << 22
            const uint32_t packed = uniform(o_v | (used_v << 11) | (len_v << 15) | (width_v << 19) | ((is_short_v ? 1u : 0u) << 22));
            const uint32_t o = packed & 0x7FFu, used = (packed >> 11) & 15u;
            const bool is_short = (packed >> 22) & 1u;
            if (o == 0u) {
                if (have < used) break;
                bits <<= used; have -= used;
                if (is_short) {                                    // end marker (:255-260 / :564-576)
                    if (!concat) break;                            // one-shot rule: stop
                    // file rule (the incremental decoder): drop the pad bits up to the byte
                    // boundary and go on with the next stream
                    const uint32_t pad = have & 7u;
                    bits <<= pad; have -= pad;
                } else {
                    off = 0;                                       // long offset 0: no copy (:280)
                }
                continue;
            }
            const uint32_t len = (packed >> 15) & 15u, width = (packed >> 19) & 7u;
            if (have < used + width) break;
            bits <<= used + width; have -= used + width;
            off = o;
            extended = len == kTokenMax ? 1u : 0u;
            copy_len = len;
        }

        if (copy_len) {                                            // :346-365, :381-400
            const uint32_t m = copy_len < room ? copy_len : room;
            __builtin_amdgcn_wave_barrier();
            uint32_t v = 0;
            if (lane < m) {
                // overlap replicates with period `off`; m <= 15, so only short offsets wrap
                // (`off` is wave-uniform: the division is skipped for the common long offsets)
                const uint32_t k = off > 15u ? lane : lane % off;
                const uint32_t from = count + k;                   // position + off of the source
                v = from >= off ? ring8[(from - off) & kRingMask] : 0u;   // before out[0] -> 0
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < m) ring8[(count + lane) & kRingMask] = (uint8_t)v;
            count += m;
        }

        // ---- drain whole tiles of finished output
        if (count - flushed >= kTile) {
            __builtin_amdgcn_wave_barrier();
            const uint32_t p = flushed + 16 * lane;
            const uint4 v = *reinterpret_cast<const uint4 *>(&ring[(p & kRingMask) >> 2]);
            if (dst16) {
                *reinterpret_cast<uint4 *>(dst + p) = v;
            } else {
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                for (uint32_t k = 0; k < 16; k++) dst[p + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
            flushed += kTile;
        }
    }

    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = flushed + lane; i < count; i += 64) dst[i] = ring8[i & kRingMask];
    if (lane == 0) out_len[b] = count;
}
