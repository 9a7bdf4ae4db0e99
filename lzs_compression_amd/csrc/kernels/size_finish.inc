// kernels/size_finish.inc -- the token walk of kernels/size_walk.inc entered in the MIDDLE of a stream: the body of
// lzs_size_finish_kernel (lzs_size_stream.hip; DESIGN.md 3.17), included inside it.  It expects, in scope: in, from (the byte at
// which the finishing segment starts), end (the byte at which its stream ends), entry (the state word SCAN settled for that
// segment: bits 0..7 the cursor in bits past `from`, bit 8 a length extension is running), limit (the room that is left
// there), and counted, status, b (where the answers go).  From its first token on it is size_walk.inc, line for line: the same
// trips, the same rules for the end marker, for a copy the room cuts and for a token short of its bits -- so the status is the
// one the walk from bit 0 with the whole capacity gives, provided no copy was cut in front of `from` (the host picks the
// segment so: the room there is above 0, or the stream begins there).
// Input: aligned dwords from the one that holds the walk's first byte to the one that holds the stream's last, nothing else;
// what the first holds in front of that byte and the last behind the stream is masked off.  A walk entered at or behind the
// stream's end reads nothing.
    const uint32_t rel0 = entry & 0xFFu;
    const uint64_t first = (uint64_t)from + (rel0 >> 3);                   // the byte that holds the walk's first bit
    const uint32_t n = first < end ? end - (uint32_t)first : 0u;           // bytes from there to the stream's end
    const uint32_t skip = rel0 & 7u;                                       // bits of that byte in front of the first token
    const uint8_t *const src = in + first;
    const uint32_t a0 = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u); // bytes in front of it in its dword
    const uint32_t *const wp = reinterpret_cast<const uint32_t *>(src - a0);
    const uint32_t total = a0 + n;                                         // bytes from wp to the stream's end
    const uint32_t nwords = n ? (total >> 2) + ((total & 3u) != 0u) : 0u;  // (nothing left of the stream: not read at all)
    FinishQuad q0 = finish_quad(wp, 0u, nwords), q1 = finish_quad(wp, 1u, nwords), q2 = finish_quad(wp, 2u, nwords);
    uint64_t acc = 0;                                                      // the bit buffer, left-aligned
    uint32_t have = 0, fed = 0;                                            // bits in it; dwords of the stream fed
    uint32_t count = 0;
    bool ext = ((entry >> 8) & 1u) != 0u, cut = false, eos = false;
    for (;;) {
        while (have <= 32u && fed < nwords) {
            uint32_t bits = __builtin_bswap32(q0.x);                       // the stream's bit order: first byte on top
            q0.x = q0.y; q0.y = q0.z; q0.z = q0.w;
            const uint32_t left = total - 4u * fed;                        // bytes from this dword to the stream's end
            uint32_t nb = 32u;
            if (left < 4u) { nb = 8u * left; bits &= ~0u << (32u - nb); }
            // (the first dword holds a byte of the walk's at least: 8 a0 + skip is below the bits it gives, and below 32)
            if (fed == 0u) { bits <<= 8u * a0 + skip; nb -= 8u * a0 + skip; }
            acc |= (uint64_t)bits << (32u - have);
            have += nb;
            fed++;
            if ((fed & 3u) == 0u) { q0 = q1; q1 = q2; q2 = finish_quad(wp, (fed >> 2) + 2u, nwords); }
        }
        // (with fewer than 33 bits in the buffer the stream has no more: `have` is all that is left of it)
        // One trip, one token (or a few of one kind), every kind by the same instructions: size_walk.inc's trip.
        const uint32_t top = (uint32_t)(acc >> 32);
        const uint32_t room = limit - count;
        const bool lit = !ext && (top >> 31) == 0u;
        const bool shrt = (top & 0x40000000u) != 0u;
        const uint32_t used = ext ? 0u : (shrt ? 9u : 13u);                 // an offset's bits (a length nibble has none in front)
        const uint32_t o = shrt ? (top >> 23) & 0x7Fu : (top >> 19) & 0x7FFu;
        const uint32_t code = (top << used) >> 28;                          // the length code behind them, or the nibble itself
        const bool zero = !ext && !lit && o == 0u;                          // the end marker, or a long offset of 0
        if (ext && !cut && code == 0u && have >= 13u && ((top >> 19) & 0x1FFu) == 0x180u) eos = true;
        if (zero && shrt && have >= 9u && !cut) eos = true;
        // up to three literals, or up to seven nibbles of 15, in one trip where each alone would have had its bits and its room
        const bool two = lit && (top & 0x00400000u) == 0u && have >= 18u && room >= 2u;
        const bool three = two && (top & 0x00002000u) == 0u && have >= 27u && room >= 3u;
        const uint32_t kl = 1u + (two ? 1u : 0u) + (three ? 1u : 0u);
        uint32_t kf = (uint32_t)__clz((int)~top) >> 2;
        kf = kf < 7u ? kf : 7u;
        const bool run = ext && kf >= 2u && have >= 4u * kf && room >= 15u * kf;
        const uint32_t need = lit ? 9u * kl : zero ? 13u : run ? 4u * kf : used + (ext || code >= 12u ? 4u : 2u);
        const uint32_t ncopy = lit ? kl : zero ? 0u : run ? 15u * kf : (ext ? code : (code < 12u ? (code >> 2) + 2u : code - 7u));
        if ((zero && shrt) || have < need || room == 0u) break;
        ext = !lit && !zero && code == 15u;
        acc <<= need; have -= need;
        const uint32_t m = ncopy < room ? ncopy : room;
        if (m < ncopy) cut = true;
        count += m;
    }
    counted[b] = count;
    status[b] = (uint8_t)(eos ? 0x04u : (count >= limit ? 0x08u : 0x03u));
