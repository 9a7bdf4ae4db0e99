// lzs_channels_burst.hip -- many packets per channel in one call (include/lzs/lzs_channels.h, lzs_*_channels_burst_device;
// DESIGN.md 3.11).  The packets are grouped by channel with a stable sort; a channel's packets form a RUN, taken in ascending
// packet order.
//
// Compression: every packet ends with an end marker and restarts at bit 0, so its bytes depend only on its RAW history -- the
// last <= 2047 bytes of (the channel's slot | the run's packets before it), all of it input.  lzs_burst_gather_kernel writes
// that history into a slot of the work area for every packet, the unchanged channel kernel (lzs_hip_launch_compress_channels,
// packet b on slot b) compresses all packets at once, and lzs_burst_commit_kernel copies each run's last slot to its channel.
//
// Decompression: a packet's history is the output of the one before it, so a run is decoded in order by one stream of the
// block decoder that keeps its window between the packets (lzs_decompress_runs_grp_kernel), the runs longest first.
//
// (<cstring> and the HIP runtime before rocPRIM: its texture cache iterator uses memset in host code.)
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "lzs_hip_shim.h"

namespace {

constexpr uint32_t kStateBytes = 2112u, kHistAt = 64u, kWindow = 2047u;   // a channel slot (lzs_channels.h)
constexpr size_t kAlign = 256;
constexpr size_t kSortSpareBytes = 65536;      // rocPRIM's temporary storage: this + 8 bytes a packet (checked at every call)

__device__ __forceinline__ uint32_t burst_len(const uint32_t *in_len, uint32_t in_len_uniform, uint32_t p)
{
    return in_len ? in_len[p] : in_len_uniform;
}

// the first sorted position in [0, hi) whose channel is not below `key`
__device__ __forceinline__ uint32_t run_first(const uint32_t *skey, uint32_t hi, uint32_t key)
{
    uint32_t lo = 0;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (skey[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// one past the last sorted position in [lo, n) whose channel is `key`
__device__ __forceinline__ uint32_t run_last_end(const uint32_t *skey, uint32_t lo, uint32_t n, uint32_t key)
{
    while (lo < n) {
        const uint32_t mid = lo + (n - lo) / 2u;
        if (skey[mid] <= key) lo = mid + 1u; else n = mid;
    }
    return lo;
}

// key[b] = the packet's channel, nchannels for an id out of range (sorted behind every channel); val[b] = b
__global__ __launch_bounds__(256) void lzs_burst_keys_kernel(const uint32_t *__restrict__ channel, uint32_t nchannels,
                                                             uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = channel[i];
    key[i] = c < nchannels ? c : nchannels;
    val[i] = i;
}

// lens[i] = the length of the packet at sorted position i (its inclusive scan: where each packet ends in its channel's bytes)
__global__ __launch_bounds__(256) void lzs_burst_lens_kernel(const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ in_len,
                                                             uint32_t in_len_uniform, uint64_t *__restrict__ lens, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) lens[i] = burst_len(in_len, in_len_uniform, sidx[i]);
}

// One workgroup per sorted position i: the history packet p = sidx[i] is compressed with, into work slot p -- the last
// H <= 2047 bytes of (the channel's slot | the packets at sorted positions [start, i)), where `start` begins the run.  With
// ends[] the inclusive scan of the lengths, the run's earlier packets are the bytes [ends[start - 1], ends[i - 1]) of one
// string; a history byte there is found by binary search over ends[start, i) (a run of 40-byte packets needs 50 of them, a
// packet of 0 bytes none).  A channel id out of range or a slot that is not a state: hist_len = ~0, which the channel kernel
// answers with ERROR, and the slot is not committed.
__global__ __launch_bounds__(256) void lzs_burst_gather_kernel(const uint8_t *__restrict__ in, size_t in_stride,
                                                               const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                                               const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                               const uint64_t *__restrict__ ends, const uint8_t *__restrict__ states,
                                                               uint32_t nchannels, uint8_t *__restrict__ work_slots)
{
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const uint32_t key = skey[i], p = sidx[i];
    uint32_t *const slot = reinterpret_cast<uint32_t *>(work_slots + (size_t)p * kStateBytes);
    const uint8_t *const st = states + (size_t)(key < nchannels ? key : 0u) * kStateBytes;
    const uint32_t hl = key < nchannels ? *reinterpret_cast<const uint32_t *>(st) : ~0u;
    if (hl > kWindow) {
        if (t == 0) slot[0] = ~0u;
        return;
    }
    const uint32_t start = run_first(skey, i, key);
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
            const uint64_t begin = ends[q] - burst_len(in_len, in_len_uniform, pq);
            v = in[(size_t)pq * in_stride + (size_t)(at - begin)];
        }
        w[k >> 2] |= v << (8u * (k & 3u));
    }
    uint32_t *const hist = slot + kHistAt / 4u;
    hist[2u * t] = w[0];
    hist[2u * t + 1u] = w[1];
    if (t > 0 && t < kHistAt / 4u) slot[t] = 0u;
    if (t == 0) slot[0] = H;
}

// One workgroup per sorted position: the last packet of a run in range copies its work slot (the history after it, written by
// the channel kernel, a packet cut at the capacity included) to its channel.  A slot marked ~0 (not a state) is not copied.
__global__ __launch_bounds__(128) void lzs_burst_commit_kernel(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                               const uint8_t *__restrict__ work_slots, uint32_t nchannels,
                                                               uint8_t *__restrict__ states, uint32_t n)
{
    const uint32_t i = blockIdx.x;
    const uint32_t key = skey[i];
    if (key >= nchannels || (i + 1u < n && skey[i + 1u] == key)) return;
    const uint32_t *const from = reinterpret_cast<const uint32_t *>(work_slots + (size_t)sidx[i] * kStateBytes);
    if (from[0] > kWindow) return;
    uint32_t *const to = reinterpret_cast<uint32_t *>(states + (size_t)key * kStateBytes);
    for (uint32_t w = threadIdx.x; w < 512u; w += 128u) to[kHistAt / 4u + w] = from[kHistAt / 4u + w];
    if (threadIdx.x == 0) to[0] = from[0];
}

// For the decoder: at the first sorted position of each run, its weight (1 + its compressed bytes, saturated) and its end;
// 0 elsewhere.  Sorted by weight, descending, these give the runs longest first.
__global__ __launch_bounds__(256) void lzs_burst_runs_kernel(const uint32_t *__restrict__ skey, const uint64_t *__restrict__ ends,
                                                             uint32_t *__restrict__ weight, uint32_t *__restrict__ at,
                                                             uint32_t *__restrict__ run_end, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = skey[i];
    at[i] = i;
    if (i > 0 && skey[i - 1u] == key) { weight[i] = 0u; return; }
    const uint32_t end = run_last_end(skey, i, n, key);
    const uint64_t bytes = ends[end - 1u] - (i ? ends[i - 1u] : 0u);
    weight[i] = (uint32_t)(bytes < 0xFFFFFFFEull ? bytes : 0xFFFFFFFEull) + 1u;
    run_end[i] = end;
}

// The work area, in this order, each part 256-byte aligned: npackets channel slots (compression), sort keys and values twice
// each (the sort's double buffers), the lengths and their scan (64 bit), the runs' weights and positions twice each and their
// ends (decompression), rocPRIM's temporary storage.
struct BurstLayout {
    size_t slots, key[2], val[2], lens, ends, weight[2], at[2], run_end, temp, temp_bytes, total;
};

size_t up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

BurstLayout burst_layout(size_t n)
{
    BurstLayout L;
    size_t o = 0;
    const auto take = [&](size_t bytes) { const size_t at = o; o += up(bytes); return at; };
    L.slots = take(n * kStateBytes);
    for (int k = 0; k < 2; k++) L.key[k] = take(4 * n);
    for (int k = 0; k < 2; k++) L.val[k] = take(4 * n);
    L.lens = take(8 * n);
    L.ends = take(8 * n);
    for (int k = 0; k < 2; k++) L.weight[k] = take(4 * n);
    for (int k = 0; k < 2; k++) L.at[k] = take(4 * n);
    L.run_end = take(4 * n);
    L.temp_bytes = up(kSortSpareBytes + 8 * n);
    L.temp = take(L.temp_bytes);
    L.total = o;
    return L;
}

}  // namespace

extern "C" size_t lzs_hip_burst_work_bytes(size_t npackets)
{
    return burst_layout(npackets).total;
}

#define BURST_TRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

extern "C" int lzs_hip_burst(int decompress, void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                             const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                             const uint32_t *d_channel, void *d_states, uint32_t nchannels, uint8_t *d_status,
                             void *d_work, uint32_t npackets, void *stream_)
{
    if (npackets == 0) return 0;
    const hipStream_t stream = (hipStream_t)stream_;
    const BurstLayout L = burst_layout(npackets);
    uint8_t *const W = static_cast<uint8_t *>(d_work);
    const auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t *>(W + at); };
    uint64_t *const lens = reinterpret_cast<uint64_t *>(W + L.lens), *const ends = reinterpret_cast<uint64_t *>(W + L.ends);
    void *const temp = W + L.temp;
    const uint32_t grid = (npackets + 255u) / 256u;

    // ---- the runs: a stable sort by channel over the bits a channel id in range (or nchannels) can have
    hipLaunchKernelGGL(lzs_burst_keys_kernel, dim3(grid), dim3(256), 0, stream, d_channel, nchannels, u32(L.key[0]), u32(L.val[0]),
                       npackets);
    unsigned bits = 1;
    while (bits < 32u && (nchannels >> bits) != 0u) bits++;
    size_t need = 0;
    {
        rocprim::double_buffer<uint32_t> keys(u32(L.key[0]), u32(L.key[1])), vals(u32(L.val[0]), u32(L.val[1]));
        BURST_TRY(rocprim::radix_sort_pairs(nullptr, need, keys, vals, npackets, 0u, bits, stream));
    }
    if (need > L.temp_bytes) return (int)hipErrorInvalidValue;
    rocprim::double_buffer<uint32_t> keys(u32(L.key[0]), u32(L.key[1])), vals(u32(L.val[0]), u32(L.val[1]));
    BURST_TRY(rocprim::radix_sort_pairs(temp, need, keys, vals, npackets, 0u, bits, stream));
    const uint32_t *const skey = keys.current(), *const sidx = vals.current();
    // ---- where each packet ends in its channel's string of packets (a scan over all runs: the differences are what counts)
    hipLaunchKernelGGL(lzs_burst_lens_kernel, dim3(grid), dim3(256), 0, stream, sidx, d_in_len, in_len, lens, npackets);
    BURST_TRY(rocprim::inclusive_scan(nullptr, need, lens, ends, (size_t)npackets, rocprim::plus<uint64_t>(), stream));
    if (need > L.temp_bytes) return (int)hipErrorInvalidValue;
    BURST_TRY(rocprim::inclusive_scan(temp, need, lens, ends, (size_t)npackets, rocprim::plus<uint64_t>(), stream));

    if (!decompress) {
        uint8_t *const slots = W + L.slots;
        hipLaunchKernelGGL(lzs_burst_gather_kernel, dim3(npackets), dim3(256), 0, stream, (const uint8_t *)d_in, in_stride, d_in_len,
                           in_len, skey, sidx, (const uint64_t *)ends, (const uint8_t *)d_states, nchannels, slots);
        BURST_TRY(hipGetLastError());
        const int e = lzs_hip_launch_compress_channels(d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len,
                                                       nullptr, slots, d_status, npackets, stream_);
        if (e) return e;
        hipLaunchKernelGGL(lzs_burst_commit_kernel, dim3(npackets), dim3(128), 0, stream, skey, sidx, (const uint8_t *)slots,
                           nchannels, (uint8_t *)d_states, npackets);
        return (int)hipGetLastError();
    }
    // ---- decompression: the runs by weight, heaviest first, one decoder stream each
    hipLaunchKernelGGL(lzs_burst_runs_kernel, dim3(grid), dim3(256), 0, stream, skey, (const uint64_t *)ends, u32(L.weight[0]),
                       u32(L.at[0]), u32(L.run_end), npackets);
    {
        rocprim::double_buffer<uint32_t> w(u32(L.weight[0]), u32(L.weight[1])), a(u32(L.at[0]), u32(L.at[1]));
        BURST_TRY(rocprim::radix_sort_pairs_desc(nullptr, need, w, a, npackets, 0u, 32u, stream));
    }
    if (need > L.temp_bytes) return (int)hipErrorInvalidValue;
    rocprim::double_buffer<uint32_t> w(u32(L.weight[0]), u32(L.weight[1])), a(u32(L.at[0]), u32(L.at[1]));
    BURST_TRY(rocprim::radix_sort_pairs_desc(temp, need, w, a, npackets, 0u, 32u, stream));
    return lzs_hip_launch_decompress_runs(d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len, w.current(),
                                          a.current(), u32(L.run_end), skey, sidx, nchannels, d_states, d_status, npackets, stream_);
}
