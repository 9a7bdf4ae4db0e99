// kernels/burst_parse.inc -- the body of lzs_burst_parse_kernel and lzs_burst_parse_packed_kernel (lzs_channels_burst.hip), included
// inside each (as text, as kernels/size_walk.inc is: the strided kernel keeps its code as it was).  It expects, in scope: out_len,
// skey, sidx, ends, run_end, states, nchannels, status, origins, rec, nheavy, split_min, rt (the runs: kernels/common.inc), out_cap after BURST_PACKET(p) -- the
// packet's room --, and the macros BURST_PACKET(p) -- statements that look packet p up and answer an entry that is not a block --,
// BURST_LEN(p), BURST_SRC(p), BURST_DST(p) -- its length and where it lies and goes -- and BURST_ORIGIN_AT(i) -- where the origins of
// the packet at sorted position i begin.
    __shared__ uint8_t val[kParseRing];
    __shared__ uint16_t org[kParseRing];
    if (*nheavy == 0u) return;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint32_t key = skey[i];
    const uint32_t start = run_first(rt.rkey, i, rt.rkey[i]);
    const uint32_t end = run_end[start];
    const uint64_t bytes = ends[end - 1u] - (start ? ends[start - 1u] : 0u);
    if (!run_is_heavy((uint32_t)(bytes < 0xFFFFFFFEull ? bytes : 0xFFFFFFFEull) + 1u, split_min)) return;
    const uint32_t p = sidx[i];
    const uint32_t hl = key < nchannels ? (run_is_fresh(rt, start) ? 0u : *reinterpret_cast<const uint32_t *>(states + (size_t)key * kStateBytes)) : ~0u;
    if (hl > kWindow) {                                                    // not a channel, not a state
        if (lane == 0) {
            out_len[p] = 0;
            if (status) status[p] = 0x10u;
            rec[i] = make_uint2(0u, 0u);
        }
        return;
    }
    BURST_PACKET(p)
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)BURST_LEN(p));
    const uint8_t *const src = BURST_SRC(p);
    uint8_t *const dst = BURST_DST(p);
    uint16_t *const og = origins + BURST_ORIGIN_AT(i);
    const auto piece = [&](uint32_t k) { const uint32_t x = 64u * k + lane; return x < n ? (uint32_t)src[x] : 0u; };
    uint32_t cur = piece(0), nxt = piece(1);
    uint64_t acc = 0;                                                      // the bit buffer, left-aligned
    uint32_t have = 0, fed = 0;                                            // bits in it; bytes of the packet fed
    uint32_t count = 0, off = 0, opens = 0;
    bool ext = false, cut = false, eos = false;
    for (;;) {
        while (have <= 56u && fed < n) {
            const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(fed & 63u));
            acc |= (uint64_t)b << (56u - have);
            have += 8u;
            fed++;
            if ((fed & 63u) == 0u) { cur = nxt; nxt = piece((fed >> 6) + 1u); }
        }
        // (with fewer than 57 bits in the buffer the packet has no more: `have` is all that is left of it)
        const uint32_t top = (uint32_t)(acc >> 32);
        const uint32_t room = out_cap - count;
        uint32_t need, ncopy;
        if (ext) {                                                         // a length nibble
            const uint32_t e = top >> 28;
            if (!cut && e == 0u && have >= 13u && ((top >> 19) & 0x1FFu) == 0x180u) eos = true;
            if (have < 4u || room == 0u) break;
            need = 4u; ncopy = e; ext = e == 15u;
        } else if ((top >> 31) == 0u) {                                    // a literal
            if (have < 9u || room == 0u) break;
            const uint32_t b = (top >> 23) & 0xFFu;
            if (lane == 0) {
                val[count & (kParseRing - 1u)] = (uint8_t)b;
                org[count & (kParseRing - 1u)] = 0;
                dst[count] = (uint8_t)b;
                og[count] = 0;
            }
            count++;
            acc <<= 9u; have -= 9u;
            continue;
        } else {
            const bool shrt = ((top >> 30) & 1u) != 0u;
            const uint32_t used = shrt ? 9u : 13u;
            const uint32_t o = shrt ? (top >> 23) & 0x7Fu : (top >> 19) & 0x7FFu;
            if (o == 0u) {
                if (shrt) {                                                // the end marker
                    if (have >= 9u && !cut) eos = true;
                    break;
                }
                if (have < 13u || room == 0u) break;                       // long offset 0
                off = 0u;
                acc <<= 13u; have -= 13u;
                continue;
            }
            const uint32_t code = (top << used) >> 28;
            const uint32_t len = code < 12u ? (code >> 2) + 2u : code - 7u;
            need = used + (code < 12u ? 2u : 4u);
            if (have < need || room == 0u) break;
            off = o; ncopy = len; ext = len == 8u;
        }
        acc <<= need; have -= need;
        const uint32_t m = ncopy < room ? ncopy : room;                    // at most 15
        if (m < ncopy) cut = true;
        if (m != 0u) {
            // byte x of the copy is byte x mod off of it (x < 16: the quotient by a float, half a unit from any doubt)
            const uint32_t x = lane & 15u;
            const uint32_t k = x - off * (uint32_t)(((float)x + 0.5f) * __frcp_rn((float)off));
            const int64_t s = (int64_t)count + k - off;                    // its source in the packet; < 0: in front of it
            uint32_t v = 0, g = 0;
            if (lane < m) {
                if (s >= 0) { v = val[(uint32_t)s & (kParseRing - 1u)]; g = org[(uint32_t)s & (kParseRing - 1u)]; }
                else g = kOpen | (uint32_t)(-s);
                const uint32_t w = count + lane;
                val[w & (kParseRing - 1u)] = (uint8_t)v;
                org[w & (kParseRing - 1u)] = (uint16_t)g;
                dst[w] = (uint8_t)v;
                og[w] = (uint16_t)g;
            }
            opens += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(g != 0u));
            count += m;
        }
    }
    if (lane == 0) {
        out_len[p] = count;
        if (status) status[p] = (uint8_t)(eos ? 0x04u : (count >= out_cap ? 0x08u : 0x03u));
        rec[i] = make_uint2(count, opens);
    }
