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
// block decoder that keeps its window between the packets (lzs_decompress_runs_grp_kernel), the runs longest first.  With a
// work area that has room for an origin per output byte the long runs are split instead: all their packets parsed at once,
// what they copy from each other resolved per run afterwards (lzs_burst_parse_kernel, lzs_burst_resolve_kernel).
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

// ---- Long runs split over the device.  Every channel packet starts at bit 0 and ends at its own end marker,
// so all packets of all long runs are parsed at once (PARSE); what a packet copies from in front of its own out[0] is not
// known then and is left as an ORIGIN, settled per run afterwards (RESOLVE).  A packet's length and status depend on its tokens
// and out_cap alone, never on the history's bytes, so PARSE writes both in final form.
constexpr uint32_t kOpen = 0x8000u;            // an origin: kOpen | how far before the packet's out[0] the byte's value lies, 1 .. 2047
constexpr uint32_t kParseRing = 2048u;         // PARSE: the packet's last bytes and their origins (a copy reaches 2047 back)
constexpr uint32_t kResolveRing = 4096u;       // RESOLVE: the run's last 2047 final bytes, and room to append 2048 beside them
constexpr uint32_t kResolveFast = 2048u;       // packets up to this length go from registers, requested kResolveAhead packets ahead
constexpr uint32_t kResolveAhead = 4u;
constexpr uint32_t kResolveMeta = 256u;        // packets whose (packet, length, open bytes) a workgroup reads at a time

// a run's weight is 1 + its compressed bytes (saturated), 0: no run; heavy runs are split
__device__ __forceinline__ bool run_is_heavy(uint32_t weight, uint32_t split_min) { return weight != 0u && weight - 1u >= split_min; }

// The runs sorted by weight, heaviest first: the heavy ones are a prefix.  *nheavy = its length; light_w / light_at = the
// tables without it -- the first light run at index 0, zeros behind the last -- for the run decoder, which takes a first
// weight of 0 in a wavefront for "none from here on".
__global__ __launch_bounds__(256) void lzs_burst_split_plan_kernel(const uint32_t *__restrict__ weight, const uint32_t *__restrict__ at,
                                                                   uint32_t split_min, uint32_t *__restrict__ light_w,
                                                                   uint32_t *__restrict__ light_at, uint32_t *__restrict__ nheavy,
                                                                   uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t lo = 0, hi = n;                                               // the first run that is not heavy
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (run_is_heavy(weight[mid], split_min)) lo = mid + 1u; else hi = mid;
    }
    if (i == 0) *nheavy = lo;
    if (i >= n) return;
    const bool in = i < n - lo;
    light_w[i] = in ? weight[i + lo] : 0u;
    light_at[i] = in ? at[i + lo] : 0u;
}

// PARSE: one wavefront per sorted position i whose run is heavy.  The tokens are parsed once for the wavefront (all of it
// wave-uniform: the bit buffer is filled from a 64-byte piece of the packet held a byte a lane, the next piece requested a
// piece ahead, and bounded by the packet's length), the bytes of a copy are produced a lane each.  The ring keeps the last
// 2048 bytes and their origins: a copied byte takes both along, so every origin that is left points in front of the packet.
// Written: out[0, len) (open bytes as 0), origins[i * out_cap + (0 .. len)), out_len, status, rec[i] = {len, open bytes}.
// The rules are those of lzs_decompress_channels_grp_kernel: an end marker needs no room and counts unless a copy was cut
// at out_cap before it -- also behind the closing length nibble 0 of a copy that filled the output --, a token short of its
// bits or of any room stops the packet, a long offset of 0 copies nothing and clears the offset.
__global__ __launch_bounds__(64) void lzs_burst_parse_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                                             uint32_t *__restrict__ out_len, const uint8_t *__restrict__ in,
                                                             size_t in_stride, const uint32_t *__restrict__ in_len,
                                                             uint32_t in_len_uniform, const uint32_t *__restrict__ skey,
                                                             const uint32_t *__restrict__ sidx, const uint64_t *__restrict__ ends,
                                                             const uint32_t *__restrict__ run_end, const uint8_t *__restrict__ states,
                                                             uint32_t nchannels, uint8_t *__restrict__ status,
                                                             uint16_t *__restrict__ origins, uint2 *__restrict__ rec,
                                                             const uint32_t *__restrict__ nheavy, uint32_t split_min)
{
    __shared__ uint8_t val[kParseRing];
    __shared__ uint16_t org[kParseRing];
    if (*nheavy == 0u) return;
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint32_t key = skey[i];
    const uint32_t start = run_first(skey, i, key);
    const uint32_t end = run_end[start];
    const uint64_t bytes = ends[end - 1u] - (start ? ends[start - 1u] : 0u);
    if (!run_is_heavy((uint32_t)(bytes < 0xFFFFFFFEull ? bytes : 0xFFFFFFFEull) + 1u, split_min)) return;
    const uint32_t p = sidx[i];
    const uint32_t hl = key < nchannels ? *reinterpret_cast<const uint32_t *>(states + (size_t)key * kStateBytes) : ~0u;
    if (hl > kWindow) {                                                    // not a channel, not a state
        if (lane == 0) {
            out_len[p] = 0;
            if (status) status[p] = 0x10u;
            rec[i] = make_uint2(0u, 0u);
        }
        return;
    }
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)burst_len(in_len, in_len_uniform, p));
    const uint8_t *const src = in + (size_t)p * in_stride;
    uint8_t *const dst = out + (size_t)p * out_stride;
    uint16_t *const og = origins + (size_t)i * out_cap;
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
}

// RESOLVE: one workgroup per heavy run walks its packets in order with the run's last 2047 final bytes in an LDS ring --
// zeros, the slot's history, then what the packets before gave.  All open bytes of a packet point in front of it, so a packet
// is one gather: a thread reads its byte's origin, takes the value from the ring, writes it to out and appends the packet to
// the ring (bytes, not words: neighbours of one copy read neighbouring bytes, four to a bank word, which the LDS broadcasts).
// A packet of up to 2048 bytes is appended while it is gathered (what it reads and what it writes are 4096 apart at most:
// the ring's size); its bytes and origins are requested kResolveAhead packets ahead, a set of registers each, and the
// (packet, length, open bytes) of 256 packets at a time go through LDS half a table ahead.  A longer packet is gathered
// first, its last 2048 bytes kept aside, and appended after a barrier.  At the end the ring's last min(2047, history +
// produced) bytes are the channel's new history (COMMIT).  Runs that are not a state's were answered by PARSE: not touched.
__global__ __launch_bounds__(256) void lzs_burst_resolve_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                                                const uint32_t *__restrict__ run_at, const uint32_t *__restrict__ run_end,
                                                                const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                                uint8_t *__restrict__ states, uint32_t nchannels,
                                                                const uint16_t *__restrict__ origins, const uint2 *__restrict__ rec,
                                                                const uint32_t *__restrict__ nheavy)
{
    __shared__ __attribute__((aligned(16))) uint8_t ring[kResolveRing];
    __shared__ uint8_t aside[kResolveFast];
    __shared__ uint32_t meta_p[2u * kResolveMeta], meta_len[2u * kResolveMeta], meta_open[2u * kResolveMeta];
    const uint32_t r = blockIdx.x, t = threadIdx.x;
    if (r >= *nheavy) return;
    const uint32_t at = run_at[r], end = run_end[at], key = skey[at];
    if (key >= nchannels) return;
    uint8_t *const st = states + (size_t)key * kStateBytes;
    const uint32_t hl = *reinterpret_cast<const uint32_t *>(st);
    if (hl > kWindow) return;
    const uint32_t npk = end - at;
    // the table of packet k of the run: entry k mod 512
    const auto meta_load = [&](uint32_t k0, uint32_t &mp, uint2 &mr) {
        mp = 0u; mr = make_uint2(0u, 0u);
        if (k0 + t < npk) { mp = sidx[at + k0 + t]; mr = rec[at + k0 + t]; }
    };
    const auto meta_store = [&](uint32_t k0, uint32_t mp, uint2 mr) {
        const uint32_t e = (k0 + t) & (2u * kResolveMeta - 1u);
        meta_p[e] = mp; meta_len[e] = mr.x; meta_open[e] = mr.y;
    };
    uint32_t mp; uint2 mr;
    meta_load(0u, mp, mr);
    for (uint32_t x = t; x < kResolveRing / 4u; x += 256u) reinterpret_cast<uint32_t *>(ring)[x] = 0u;
    meta_store(0u, mp, mr);
    meta_load(kResolveMeta, mp, mr);
    __syncthreads();
    uint32_t P = kResolveFast;                                             // where the next packet begins in the ring
    for (uint32_t x = t; x < hl; x += 256u) ring[P - hl + x] = st[kHistAt + x];
    meta_store(kResolveMeta, mp, mr);
    meta_load(2u * kResolveMeta, mp, mr);                                  // (stored when packet 256 + 128 is reached)
    __syncthreads();

    uint32_t v[kResolveAhead][8], g[kResolveAhead][8];
    // packet k's bytes and origins, eight of each a thread (not for a packet that is longer than that, or past the run's end)
    const auto request = [&](uint32_t k, uint32_t (&vv)[8], uint32_t (&gg)[8]) {
        const uint32_t e = k & (2u * kResolveMeta - 1u);
        const uint32_t len = k < npk ? meta_len[e] : 0u;
        const bool open = meta_open[e] != 0u;
        const uint8_t *const d = out + (size_t)meta_p[e] * out_stride;
        const uint16_t *const o = origins + (size_t)(at + k) * out_cap;
#pragma unroll
        for (uint32_t s = 0; s < 8u; s++) {
            const uint32_t j = t + 256u * s;
            vv[s] = 0u; gg[s] = 0u;
            if (len <= kResolveFast && j < len) {
                vv[s] = d[j];
                if (open) gg[s] = o[j];
            }
        }
    };
#pragma unroll
    for (uint32_t a = 0; a < kResolveAhead; a++) request(a, v[a], g[a]);
    uint32_t produced = 0;                                                 // of the run, saturated at the window
    for (uint32_t k0 = 0; k0 < npk; k0 += kResolveAhead) {
#pragma unroll
        for (uint32_t a = 0; a < kResolveAhead; a++) {
            const uint32_t k = k0 + a;
            if (k >= npk) break;
            const uint32_t e = k & (2u * kResolveMeta - 1u);
            const uint32_t len = meta_len[e];
            uint8_t *const d = out + (size_t)meta_p[e] * out_stride;
            if (len <= kResolveFast) {
#pragma unroll
                for (uint32_t s = 0; s < 8u; s++) {
                    const uint32_t j = t + 256u * s;
                    if (j < len) {
                        uint32_t b = v[a][s];
                        if (g[a][s] & kOpen) {
                            b = ring[(P - (g[a][s] & kWindow)) & (kResolveRing - 1u)];
                            d[j] = (uint8_t)b;
                        }
                        ring[(P + j) & (kResolveRing - 1u)] = (uint8_t)b;
                    }
                }
            } else {
                const bool open = meta_open[e] != 0u;
                const uint16_t *const o = origins + (size_t)(at + k) * out_cap;
                for (uint32_t j = t; j < len; j += 256u) {
                    uint32_t b = d[j];
                    const uint32_t gg = open ? o[j] : 0u;
                    if (gg & kOpen) {
                        b = ring[(P - (gg & kWindow)) & (kResolveRing - 1u)];
                        d[j] = (uint8_t)b;
                    }
                    if (len - j <= kResolveFast) aside[j & (kResolveFast - 1u)] = (uint8_t)b;
                }
                __syncthreads();
                for (uint32_t j = len - kResolveFast + t; j < len; j += 256u)
                    ring[(P + j) & (kResolveRing - 1u)] = aside[j & (kResolveFast - 1u)];
            }
            P = (P + len) & (kResolveRing - 1u);
            produced = len < kWindow - produced ? produced + len : kWindow;
            // the next half of the table moves in while this one is in use; its entries were asked for half a table ago
            if ((k & (kResolveMeta - 1u)) == kResolveMeta / 2u && k >= kResolveMeta) {
                meta_store(k - kResolveMeta / 2u + kResolveMeta, mp, mr);
            }
            __syncthreads();
            if ((k & (kResolveMeta - 1u)) == kResolveMeta / 2u && k >= kResolveMeta)
                meta_load(k - kResolveMeta / 2u + 2u * kResolveMeta, mp, mr);
            request(k + kResolveAhead, v[a], g[a]);
        }
    }
    // COMMIT: hist[0, H) = the last H bytes of the run's string, zeros behind them, the length in front
    const uint32_t H = hl + produced < kWindow ? hl + produced : kWindow;
    uint32_t *const hist = reinterpret_cast<uint32_t *>(st + kHistAt);
    for (uint32_t w = t; w < 512u; w += 256u) {
        uint32_t word = 0;
        for (uint32_t b = 0; b < 4u; b++) {
            const uint32_t x = 4u * w + b;
            if (x < H) word |= (uint32_t)ring[(P - H + x) & (kResolveRing - 1u)] << (8u * b);
        }
        hist[w] = word;
    }
    if (t == 0) *reinterpret_cast<uint32_t *>(st) = H;
}

// The work area, in this order, each part 256-byte aligned: npackets channel slots (compression), sort keys and values twice
// each (the sort's double buffers), the lengths and their scan (64 bit), the runs' weights and positions twice each and their
// ends (decompression), rocPRIM's temporary storage.
// A split decode keeps its tables where compression has its slots -- the light runs' weights and positions, {length, open
// bytes} of every packet by sorted position, the number of heavy runs: 16 bytes a packet -- and npackets * out_cap 16-bit
// origins, packet by packet in sorted order, behind everything else (`total` is where): the larger work area's extra part.
struct BurstLayout {
    size_t slots, key[2], val[2], lens, ends, weight[2], at[2], run_end, temp, temp_bytes, total;
    size_t light_w, light_at, rec, nheavy, origins;
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
    o = L.slots;
    L.nheavy = take(4);
    L.light_w = take(4 * n);
    L.light_at = take(4 * n);
    L.rec = take(8 * n);
    static_assert(kStateBytes >= 4 * kAlign + 16 + kAlign, "the split decode's tables fit the slots of one packet and more");
    L.origins = L.total;
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
                             void *d_work, uint32_t npackets, int split, uint32_t split_min, void *stream_)
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
    if (split) {
        // ---- the heavy runs (a prefix of that order, found on the device) by PARSE and RESOLVE, the others by the run decoder
        // from tables of their own
        uint16_t *const origins = reinterpret_cast<uint16_t *>(W + L.origins);
        uint2 *const rec = reinterpret_cast<uint2 *>(W + L.rec);
        hipLaunchKernelGGL(lzs_burst_split_plan_kernel, dim3(grid), dim3(256), 0, stream, (const uint32_t *)w.current(),
                           (const uint32_t *)a.current(), split_min, u32(L.light_w), u32(L.light_at), u32(L.nheavy), npackets);
        hipLaunchKernelGGL(lzs_burst_parse_kernel, dim3(npackets), dim3(64), 0, stream, (uint8_t *)d_out, out_stride, out_cap, d_out_len,
                           (const uint8_t *)d_in, in_stride, d_in_len, in_len, skey, sidx, (const uint64_t *)ends,
                           (const uint32_t *)u32(L.run_end), (const uint8_t *)d_states, nchannels, d_status, origins, rec,
                           (const uint32_t *)u32(L.nheavy), split_min);
        const uint32_t most_runs = npackets <= nchannels ? npackets : nchannels + 1u;     // (the ids out of range are one more)
        hipLaunchKernelGGL(lzs_burst_resolve_kernel, dim3(most_runs), dim3(256), 0, stream, (uint8_t *)d_out, out_stride, out_cap,
                           (const uint32_t *)a.current(), (const uint32_t *)u32(L.run_end), skey, sidx, (uint8_t *)d_states,
                           nchannels, (const uint16_t *)origins, (const uint2 *)rec, (const uint32_t *)u32(L.nheavy));
        BURST_TRY(hipGetLastError());
        return lzs_hip_launch_decompress_runs(d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len,
                                              u32(L.light_w), u32(L.light_at), u32(L.run_end), skey, sidx, nchannels, d_states,
                                              d_status, npackets, stream_);
    }
    return lzs_hip_launch_decompress_runs(d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len, w.current(),
                                          a.current(), u32(L.run_end), skey, sidx, nchannels, d_states, d_status, npackets, stream_);
}
