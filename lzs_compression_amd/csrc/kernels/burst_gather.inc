// kernels/burst_gather.inc -- the body of lzs_burst_gather_kernel and lzs_burst_gather_packed_kernel (lzs_channels_burst.hip), included
// inside each (as text, as kernels/size_walk.inc is: the strided kernel keeps its code as it was).  It expects, in scope: skey, sidx,
// ends, states, nchannels, work_slots, rt, and the macros BURST_LEN(p) -- packet p's length, 0 for an entry that is not a block -- and
// BURST_SRC(p) -- where its bytes lie.
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const uint32_t key = skey[i], p = sidx[i];
    uint32_t *const slot = reinterpret_cast<uint32_t *>(work_slots + (size_t)p * kStateBytes);
    const uint8_t *const st = states + (size_t)(key < nchannels ? key : 0u) * kStateBytes;
    const uint32_t start = run_first(rt.rkey, i, rt.rkey[i]);
    const uint32_t hl = key < nchannels ? (run_is_fresh(rt, start) ? 0u : *reinterpret_cast<const uint32_t *>(st)) : ~0u;
    if (hl > kWindow) {
        if (t == 0) slot[0] = ~0u;
        return;
    }
    const uint64_t e = i ? ends[i - 1u] : 0u, s = start ? ends[start - 1u] : 0u;
    const uint32_t hp = (uint32_t)(e - s < kWindow ? e - s : kWindow);     // from the run's earlier packets ...
    const uint32_t hs = hl < kWindow - hp ? hl : kWindow - hp;              // ... and from the slot, in front of them
    const uint32_t H = hs + hp;
    uint32_t w[2] = {0u, 0u};
    uint32_t q = start;                                                     // the packet that holds the byte, once found
    bool found = false;
    for (uint32_t k = 0; k < 8u; k++) {
        const uint32_t x = 8u * t + k;
        if (x >= H) break;
        uint32_t v;
        if (x < hs) {
            v = st[kHistAt + hl - hs + x];
        } else {
            const uint64_t at = e - hp + (x - hs);                          // its place in the channel's string
            if (!found) {
                uint32_t lo = start, hi = i;                                // the first q in [start, i) with ends[q] > at
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2u;
                    if (ends[mid] <= at) lo = mid + 1u; else hi = mid;
                }
                q = lo;
                found = true;
            }
            while (ends[q] <= at) q++;
            const uint32_t pq = sidx[q];
            const uint64_t begin = ends[q] - BURST_LEN(pq);
            v = BURST_SRC(pq)[(size_t)(at - begin)];
        }
        w[k >> 2] |= v << (8u * (k & 3u));
    }
    uint32_t *const hist = slot + kHistAt / 4u;
    hist[2u * t] = w[0];
    hist[2u * t + 1u] = w[1];
    if (t > 0 && t < kHistAt / 4u) slot[t] = 0u;
    if (t == 0) slot[0] = H;
