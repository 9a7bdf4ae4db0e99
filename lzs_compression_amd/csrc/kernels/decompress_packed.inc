// kernels/decompress_packed.inc -- the offset-addressed ("packed") decoders and the scan that makes their offsets
// (include/lzs/lzs_batch.h, lzs_channels.h; DESIGN.md 3.14).
// Part of lzs_kernels.hip (included there, inside its anonymous namespace); not a translation unit of its own.

// Packed streams to packed outputs: lzs_decompress_blocks_grp_kernel<false> (CHAN false) and lzs_decompress_channels_grp_kernel
// (CHAN true) with every stream's place, length and room taken from offset arrays on the device -- the PACKED mode of
// lzs_decompress_blocks_grp.  Eight entries to a wavefront always: whether their input fits one 32-bit extent is only known
// here, and the decoder deals with it.
template <bool CHAN>
__global__ __launch_bounds__(64)
void lzs_decompress_packed_grp_kernel(uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                                      uint32_t *__restrict__ out_len,
                                      const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                      const uint32_t *__restrict__ in_len,
                                      const uint32_t *__restrict__ channel, uint8_t *__restrict__ states,
                                      uint8_t *__restrict__ status, uint32_t nblocks)
{
    __shared__ DecGroupLds L;
    DecPacked pk;
    pk.in_off = in_off; pk.out_off = out_off;
    // (the form by the wavefront's ratio of input to room, as lzs_decompress_blocks_grp_kernel picks it: the room is the sum
    // of the rooms here)
    uint64_t total = 0, full = 0;
    const uint32_t b0 = blockIdx.x * kDecGroups;
    for (uint32_t g = 0; g < kDecGroups && b0 + g < nblocks; g++) {
        uint64_t from, to;
        uint32_t n, room;
        if (dec_packed_entry(pk, in_len, b0 + g, from, n, to, room)) {
            total += n;
            full += room;
        }
    }
    const bool two = uniform((4ull * total > full && 10ull * total < 9ull * full) ? 1u : 0u) != 0u;
    const bool wide = uniform(10ull * total >= 9ull * full ? 1u : 0u) != 0u;
    DecChan ch;
    if constexpr (CHAN) { ch.states = states; ch.channel = channel; ch.status = status; }
    if (two)       lzs_decompress_blocks_grp<true, false, false, CHAN, false, true>(L, out, 0, 0u, out_len, in, 0, in_len, 0u, nblocks, 0u, kDecGroups, ch, pk);
    else if (wide) lzs_decompress_blocks_grp<false, true, false, CHAN, false, true>(L, out, 0, 0u, out_len, in, 0, in_len, 0u, nblocks, 0u, kDecGroups, ch, pk);
    else           lzs_decompress_blocks_grp<false, false, false, CHAN, false, true>(L, out, 0, 0u, out_len, in, 0, in_len, 0u, nblocks, 0u, kDecGroups, ch, pk);
}

// Packed bursts (include/lzs/lzs_channels.h, lzs_decompress_channels_burst_packed_device; DESIGN.md 3.16): lzs_decompress_runs_grp_kernel
// with every packet's place, length and room taken from the offset arrays -- RUN and PACKED together.  Eight runs to a wavefront
// always: where the packets of one trip lie is only known to the decoder, trip by trip.  room_ends[i] = the sum of the rooms of the
// packets at sorted positions 0 .. i (an entry that is not a block has none): a run's rooms are a difference of two of them, which
// gives the form as lzs_decompress_packed_grp_kernel picks it.
__global__ __launch_bounds__(64)
void lzs_decompress_runs_packed_grp_kernel(uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                                           uint32_t *__restrict__ out_len,
                                           const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                           const uint32_t *__restrict__ in_len, const uint64_t *__restrict__ room_ends,
                                           const uint32_t *__restrict__ run_key, const uint32_t *__restrict__ run_at,
                                           const uint32_t *__restrict__ run_end, const uint32_t *__restrict__ skey,
                                           const uint32_t *__restrict__ sidx, uint32_t nchannels, uint8_t *__restrict__ states,
                                           uint8_t *__restrict__ status, uint32_t nruns, RunTables rt)
{
    __shared__ DecGroupLds L;
    uint64_t total = 0, full = 0;
    const uint32_t b0 = blockIdx.x * kDecGroups;
    if (b0 >= nruns || run_key[b0] == 0u) return;                 // (runs are sorted by weight: none from here on)
    for (uint32_t g = 0; g < kDecGroups && b0 + g < nruns; g++) {
        const uint32_t w = run_key[b0 + g];                        // 1 + the run's compressed bytes (saturated), 0: no run
        if (w == 0u) break;
        const uint32_t at = run_at[b0 + g];
        total += w - 1u;
        full += room_ends[run_end[at] - 1u] - (at ? room_ends[at - 1u] : 0u);
    }
    const bool two = uniform((4ull * total > full && 10ull * total < 9ull * full) ? 1u : 0u) != 0u;
    const bool wide = uniform(10ull * total >= 9ull * full ? 1u : 0u) != 0u;
    DecPacked pk;
    pk.in_off = in_off; pk.out_off = out_off;
    DecChan ch;
    ch.states = states; ch.status = status;
    ch.run_key = run_key; ch.run_at = run_at; ch.run_end = run_end; ch.skey = skey; ch.sidx = sidx; ch.nchannels = nchannels;
    ch.rt = rt;
    if (two)       lzs_decompress_blocks_grp<true, false, false, true, true, true>(L, out, 0, 0u, out_len, in, 0, in_len, 0u, nruns, 0u, kDecGroups, ch, pk);
    else if (wide) lzs_decompress_blocks_grp<false, true, false, true, true, true>(L, out, 0, 0u, out_len, in, 0, in_len, 0u, nruns, 0u, kDecGroups, ch, pk);
    else           lzs_decompress_blocks_grp<false, false, false, true, true, true>(L, out, 0, 0u, out_len, in, 0, in_len, 0u, nruns, 0u, kDecGroups, ch, pk);
}

// offsets[0] = 0, offsets[b + 1] = offsets[b] + size[b] rounded up to a multiple of pad + 1 (a power of two): lzs_scan_lengths_kernel
// with the rounding, for lzs_offsets_from_sizes_device.
__global__ __launch_bounds__(1024)
void lzs_scan_sizes_kernel(uint64_t *__restrict__ offsets, const uint32_t *__restrict__ size, uint32_t pad, uint32_t nblocks)
{
    // single workgroup: each thread sums a contiguous chunk, then a block-wide scan of the sums
    __shared__ uint64_t partial[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nblocks + 1023u) / 1024u;
    const uint32_t lo = t * per < nblocks ? t * per : nblocks;
    const uint32_t hi = lo + per < nblocks ? lo + per : nblocks;
    const auto padded = [&](uint32_t i) { return ((uint64_t)size[i] + pad) & ~(uint64_t)pad; };
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += padded(i);
    partial[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t add = t >= d ? partial[t - d] : 0;
        __syncthreads();
        partial[t] += add;
        __syncthreads();
    }
    uint64_t run = partial[t] - sum;     // exclusive prefix of this chunk
    for (uint32_t i = lo; i < hi; i++) { offsets[i] = run; run += padded(i); }
    if (t == 1023) offsets[nblocks] = partial[1023];
}
