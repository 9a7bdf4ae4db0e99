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
// Packed bursts (lzs_*_channels_burst_packed_device): the same with every packet and its room addressed by offset
// arrays on the device.  The kernels that look at a packet's bytes exist in both forms from one body each (BurstIo, PACKED); the
// compressor is lzs_hip_launch_compress_channels_packed, the run decoder lzs_hip_launch_decompress_runs_packed.
//
// (<cstring> and the HIP runtime before rocPRIM: its texture cache iterator uses memset in host code.)
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "lzs_hip_shim.h"

namespace {

#include "kernels/common.inc"                  // kWindow, packed_entry

constexpr uint32_t kStateBytes = 2112u, kHistAt = 64u;                    // a channel slot (lzs_channels.h)
constexpr size_t kAlign = 256;
constexpr size_t kSortSpareBytes = 65536;      // rocPRIM's temporary storage: this + 8 bytes a packet (checked at every call)

__device__ __forceinline__ uint32_t burst_len(const uint32_t *in_len, uint32_t in_len_uniform, uint32_t p)
{
    return in_len ? in_len[p] : in_len_uniform;
}

// Where the packets lie and where their output goes: slots a stride apart with one capacity (lzs_*_channels_burst_device), or --
// PACKED -- entries of offset arrays, the rule of packed_entry (lzs_*_channels_burst_packed_device).  An entry that is not a block
// has length 0 and room 0.  room_ends (PACKED, decompression): the inclusive scan of the rooms by sorted position -- where each
// packet's origins end in the work area (split route), and a run's rooms as a difference.
struct BurstIo {
    const uint8_t *in;
    uint8_t *out;
    size_t in_stride, out_stride;
    uint32_t out_cap;
    const uint32_t *in_len;
    uint32_t in_len_uniform;
    const uint64_t *in_off, *out_off, *room_ends;
};

struct BurstPacket {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t n, cap;
    bool block;
};

template <bool PACKED>
__device__ __forceinline__ BurstPacket burst_packet(const BurstIo &io, uint32_t p)
{
    BurstPacket k;
    if constexpr (PACKED) {
        uint64_t from, to;
        k.block = packed_entry(io.in_off, io.in_len, io.out_off, p, from, k.n, to, k.cap);
        k.src = io.in + (k.block ? from : 0u);
        k.dst = io.out + (k.block ? to : 0u);
    } else {
        k.block = true;
        k.n = burst_len(io.in_len, io.in_len_uniform, p);
        k.cap = io.out_cap;
        k.src = io.in + (size_t)p * io.in_stride;
        k.dst = io.out + (size_t)p * io.out_stride;
    }
    return k;
}

// where the origins of the packet at sorted position i begin (split route)
template <bool PACKED>
__device__ __forceinline__ size_t burst_origin_at(const BurstIo &io, uint32_t i)
{
    if constexpr (PACKED) return i ? (size_t)io.room_ends[i - 1u] : (size_t)0;
    else return (size_t)i * io.out_cap;
}

__device__ __forceinline__ BurstIo burst_strided(const uint8_t *in, size_t in_stride, const uint32_t *in_len, uint32_t in_len_uniform,
                                                 uint8_t *out = nullptr, size_t out_stride = 0, uint32_t out_cap = 0)
{
    return BurstIo{in, out, in_stride, out_stride, out_cap, in_len, in_len_uniform, nullptr, nullptr, nullptr};
}

__device__ __forceinline__ BurstIo burst_packed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                                                const uint64_t *out_off, const uint64_t *room_ends = nullptr)
{
    return BurstIo{in, out, 0, 0, 0u, in_len, 0u, in_off, out_off, room_ends};
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

// (PACKED) the same from the entries -- 0 for one that is not a block --, and rooms[i] (if given) = the packet's room, for room_ends
__global__ __launch_bounds__(256) void lzs_burst_lens_packed_kernel(const uint32_t *__restrict__ sidx, const uint64_t *__restrict__ in_off,
                                                                    const uint32_t *__restrict__ in_len, const uint64_t *__restrict__ out_off,
                                                                    uint64_t *__restrict__ lens, uint64_t *__restrict__ rooms, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const BurstPacket k = burst_packet<true>(burst_packed(nullptr, in_off, in_len, nullptr, out_off), sidx[i]);
    lens[i] = k.n;
    if (rooms) rooms[i] = k.cap;
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
#define BURST_LEN(p) burst_len(in_len, in_len_uniform, (p))
#define BURST_SRC(p) (in + (size_t)(p) * in_stride)
#include "kernels/burst_gather.inc"
#undef BURST_LEN
#undef BURST_SRC
}

__global__ __launch_bounds__(256) void lzs_burst_gather_packed_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
                                                                      const uint32_t *__restrict__ in_len, const uint64_t *__restrict__ out_off,
                                                                      const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                                      const uint64_t *__restrict__ ends, const uint8_t *__restrict__ states,
                                                                      uint32_t nchannels, uint8_t *__restrict__ work_slots)
{
    const BurstIo io = burst_packed(in, in_off, in_len, nullptr, out_off);
#define BURST_LEN(p) burst_packet<true>(io, (p)).n
#define BURST_SRC(p) burst_packet<true>(io, (p)).src
#include "kernels/burst_gather.inc"
#undef BURST_LEN
#undef BURST_SRC
}

// One workgroup per sorted position: the last packet of a run in range copies its work slot (the history after it, written by
// the channel kernel, a packet cut at the capacity included) to its channel.  A slot marked ~0 (not a state) is not copied.
// PACKED: an entry that is not a block leaves its work slot as the gather wrote it -- the history behind the blocks before it --,
// so the last slot is the run's whatever its last entry is; but a run with no block at all is not committed: its channel's slot
// stays as it is byte for byte (the packed call looks at no slot for such an entry), not rewritten in canonical form.
template <bool PACKED>
__device__ __forceinline__ void burst_commit(const BurstIo &io, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                             const uint8_t *__restrict__ work_slots, uint32_t nchannels,
                                             uint8_t *__restrict__ states, uint32_t n)
{
    const uint32_t i = blockIdx.x;
    const uint32_t key = skey[i];
    if (key >= nchannels || (i + 1u < n && skey[i + 1u] == key)) return;
    if constexpr (PACKED) {
        for (uint32_t q = i; !burst_packet<true>(io, sidx[q]).block; q--)
            if (q == 0u || skey[q - 1u] != key) return;
    }
    const uint32_t *const from = reinterpret_cast<const uint32_t *>(work_slots + (size_t)sidx[i] * kStateBytes);
    if (from[0] > kWindow) return;
    uint32_t *const to = reinterpret_cast<uint32_t *>(states + (size_t)key * kStateBytes);
    for (uint32_t w = threadIdx.x; w < 512u; w += 128u) to[kHistAt / 4u + w] = from[kHistAt / 4u + w];
    if (threadIdx.x == 0) to[0] = from[0];
}

__global__ __launch_bounds__(128) void lzs_burst_commit_kernel(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                               const uint8_t *__restrict__ work_slots, uint32_t nchannels,
                                                               uint8_t *__restrict__ states, uint32_t n)
{
    burst_commit<false>(BurstIo{}, skey, sidx, work_slots, nchannels, states, n);
}

__global__ __launch_bounds__(128) void lzs_burst_commit_packed_kernel(const uint64_t *__restrict__ in_off, const uint32_t *__restrict__ in_len,
                                                                      const uint64_t *__restrict__ out_off, const uint32_t *__restrict__ skey,
                                                                      const uint32_t *__restrict__ sidx, const uint8_t *__restrict__ work_slots,
                                                                      uint32_t nchannels, uint8_t *__restrict__ states, uint32_t n)
{
    burst_commit<true>(burst_packed(nullptr, in_off, in_len, nullptr, out_off), skey, sidx, work_slots, nchannels, states, n);
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
__device__ __forceinline__ void burst_split_plan(const uint32_t *__restrict__ weight, const uint32_t *__restrict__ at,
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

__global__ __launch_bounds__(256) void lzs_burst_split_plan_kernel(const uint32_t *__restrict__ weight, const uint32_t *__restrict__ at,
                                                                   uint32_t split_min, uint32_t *__restrict__ light_w,
                                                                   uint32_t *__restrict__ light_at, uint32_t *__restrict__ nheavy,
                                                                   uint32_t n)
{
    burst_split_plan(weight, at, split_min, light_w, light_at, nheavy, n);
}

// PACKED: the host does not know the rooms, so whether their origins fit the work area is seen here -- origin_cap 16-bit origins
// behind the burst part against the sum of the rooms.  If they do not fit no run is heavy (no weight reaches a threshold of ~0):
// PARSE and RESOLVE return at once and write nothing, the run decoder takes every run.
__global__ __launch_bounds__(256) void lzs_burst_split_plan_packed_kernel(const uint32_t *__restrict__ weight, const uint32_t *__restrict__ at,
                                                                          uint32_t split_min, const uint64_t *__restrict__ room_ends,
                                                                          uint64_t origin_cap, uint32_t *__restrict__ light_w,
                                                                          uint32_t *__restrict__ light_at, uint32_t *__restrict__ nheavy,
                                                                          uint32_t n)
{
    burst_split_plan(weight, at, room_ends[n - 1u] <= origin_cap ? split_min : ~0u, light_w, light_at, nheavy, n);
}

// PARSE: one wavefront per sorted position i whose run is heavy.  The tokens are parsed once for the wavefront (all of it
// wave-uniform: the bit buffer is filled from a 64-byte piece of the packet held a byte a lane, the next piece requested a
// piece ahead, and bounded by the packet's length), the bytes of a copy are produced a lane each.  The ring keeps the last
// 2048 bytes and their origins: a copied byte takes both along, so every origin that is left points in front of the packet.
// Written: out[0, len) (open bytes as 0), origins[i * out_cap + (0 .. len)), out_len, status, rec[i] = {len, open bytes}.
// The rules are those of lzs_decompress_channels_grp_kernel: an end marker needs no room and counts unless a copy was cut
// at out_cap before it -- also behind the closing length nibble 0 of a copy that filled the output --, a token short of its
// bits or of any room stops the packet, a long offset of 0 copies nothing and clears the offset.
// PACKED: the packet, its room (out_cap) and where its origins lie come from the entries; one that is not a block is answered like
// a slot that is no state, with rec[i] = {0, 1} -- no packet has more open bytes than bytes -- so that RESOLVE knows it from a
// packet of no bytes.
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
#define BURST_PACKET(p)
#define BURST_LEN(p) burst_len(in_len, in_len_uniform, (p))
#define BURST_SRC(p) (in + (size_t)(p) * in_stride)
#define BURST_DST(p) (out + (size_t)(p) * out_stride)
#define BURST_ORIGIN_AT(i) ((size_t)(i) * out_cap)
#include "kernels/burst_parse.inc"
#undef BURST_PACKET
#undef BURST_LEN
#undef BURST_SRC
#undef BURST_DST
#undef BURST_ORIGIN_AT
}

__global__ __launch_bounds__(64) void lzs_burst_parse_packed_kernel(uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                                                                    uint32_t *__restrict__ out_len, const uint8_t *__restrict__ in,
                                                                    const uint64_t *__restrict__ in_off, const uint32_t *__restrict__ in_len,
                                                                    const uint64_t *__restrict__ room_ends, const uint32_t *__restrict__ skey,
                                                                    const uint32_t *__restrict__ sidx, const uint64_t *__restrict__ ends,
                                                                    const uint32_t *__restrict__ run_end, const uint8_t *__restrict__ states,
                                                                    uint32_t nchannels, uint8_t *__restrict__ status,
                                                                    uint16_t *__restrict__ origins, uint2 *__restrict__ rec,
                                                                    const uint32_t *__restrict__ nheavy, uint32_t split_min)
{
    const BurstIo io = burst_packed(in, in_off, in_len, out, out_off, room_ends);
    // (one that is not a block: nothing of it is read or written)
#define BURST_PACKET(p) \
    const BurstPacket pkt = burst_packet<true>(io, (p)); \
    if (!pkt.block) { \
        if (lane == 0) { \
            out_len[p] = 0; \
            if (status) status[p] = 0x10u; \
            rec[i] = make_uint2(0u, 1u); \
        } \
        return; \
    } \
    const uint32_t out_cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)pkt.cap);
#define BURST_LEN(p) pkt.n
#define BURST_SRC(p) pkt.src
#define BURST_DST(p) pkt.dst
#define BURST_ORIGIN_AT(i) burst_origin_at<true>(io, (i))
#include "kernels/burst_parse.inc"
#undef BURST_PACKET
#undef BURST_LEN
#undef BURST_SRC
#undef BURST_DST
#undef BURST_ORIGIN_AT
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
// PACKED: a packet's output and its origins are found through the entries, and a run none of whose entries is a block (rec = {0, 1}
// throughout) is not committed: its slot stays as it is byte for byte.
template <bool PACKED>
__device__ __forceinline__ void burst_resolve(const BurstIo &io, const uint32_t *__restrict__ run_at, const uint32_t *__restrict__ run_end,
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
    bool any_block = false;                                                // (PACKED) of the entries this thread has loaded
    const auto meta_load = [&](uint32_t k0, uint32_t &mp, uint2 &mr) {
        mp = 0u; mr = make_uint2(0u, 0u);
        if (k0 + t < npk) {
            mp = sidx[at + k0 + t]; mr = rec[at + k0 + t];
            if constexpr (PACKED) any_block = any_block || mr.x != 0u || mr.y == 0u;
        }
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
        const uint8_t *const d = burst_packet<PACKED>(io, meta_p[e]).dst;
        const uint16_t *const o = origins + burst_origin_at<PACKED>(io, PACKED && k >= npk ? at : at + k);   // (room_ends has no entry past the run)
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
            uint8_t *const d = burst_packet<PACKED>(io, meta_p[e]).dst;
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
                const uint16_t *const o = origins + burst_origin_at<PACKED>(io, at + k);
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
    if constexpr (PACKED) {
        if (__syncthreads_or(any_block ? 1 : 0) == 0) return;
    }
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

__global__ __launch_bounds__(256) void lzs_burst_resolve_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                                                const uint32_t *__restrict__ run_at, const uint32_t *__restrict__ run_end,
                                                                const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                                uint8_t *__restrict__ states, uint32_t nchannels,
                                                                const uint16_t *__restrict__ origins, const uint2 *__restrict__ rec,
                                                                const uint32_t *__restrict__ nheavy)
{
    burst_resolve<false>(burst_strided(nullptr, 0, nullptr, 0u, out, out_stride, out_cap), run_at, run_end, skey, sidx, states, nchannels,
                         origins, rec, nheavy);
}

__global__ __launch_bounds__(256) void lzs_burst_resolve_packed_kernel(uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                                                                       const uint64_t *__restrict__ in_off, const uint32_t *__restrict__ in_len,
                                                                       const uint64_t *__restrict__ room_ends,
                                                                       const uint32_t *__restrict__ run_at, const uint32_t *__restrict__ run_end,
                                                                       const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                                       uint8_t *__restrict__ states, uint32_t nchannels,
                                                                       const uint16_t *__restrict__ origins, const uint2 *__restrict__ rec,
                                                                       const uint32_t *__restrict__ nheavy)
{
    burst_resolve<true>(burst_packed(nullptr, in_off, in_len, out, out_off, room_ends), run_at, run_end, skey, sidx, states, nchannels,
                        origins, rec, nheavy);
}

// The work area, in this order, each part 256-byte aligned: npackets channel slots (compression), sort keys and values twice
// each (the sort's double buffers), the lengths and their scan (64 bit), the runs' weights and positions twice each and their
// ends (decompression), rocPRIM's temporary storage.
// A split decode keeps its tables where compression has its slots -- the light runs' weights and positions, {length, open
// bytes} of every packet by sorted position, the number of heavy runs: 16 bytes a packet -- and npackets * out_cap 16-bit
// origins, packet by packet in sorted order, behind everything else (`total` is where): the larger work area's extra part.
// A packed decode has the rooms by sorted position and their scan there as well (16 bytes a packet more), and its origins lie
// room by room: origin_bytes / 2 of them, as many as the caller's work area holds behind `total`.
struct BurstLayout {
    size_t slots, key[2], val[2], lens, ends, weight[2], at[2], run_end, temp, temp_bytes, total;
    size_t light_w, light_at, rec, nheavy, rooms, room_ends, origins;
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
    L.rooms = take(8 * n);
    L.room_ends = take(8 * n);
    static_assert(kStateBytes >= 6 * kAlign + 32 + kAlign, "the decoders' tables fit the slots of one packet and more");
    L.origins = L.total;
    return L;
}

#define BURST_TRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// What a call gives: the packets strided (off: nullptr) or packed.
struct BurstCall {
    void *d_out;
    const void *d_in;
    size_t out_stride, in_stride;
    uint32_t out_cap, in_len;
    const uint32_t *d_in_len;
    const uint64_t *d_in_off, *d_out_off;
    bool packed() const { return d_in_off != nullptr; }
};

// One burst: the grouping, then the kernels of the direction.  split (decompression): the long runs by PARSE and RESOLVE, with
// origin_cap 16-bit origins behind the burst part of the work area (PACKED; the strided call's host code knows that they fit).
int burst(int decompress, const BurstCall &c, uint32_t *d_out_len, const uint32_t *d_channel, void *d_states, uint32_t nchannels,
          uint8_t *d_status, void *d_work, uint32_t npackets, int split, uint64_t origin_cap, uint32_t split_min, void *stream_)
{
    if (npackets == 0) return 0;
    const hipStream_t stream = (hipStream_t)stream_;
    const BurstLayout L = burst_layout(npackets);
    uint8_t *const W = static_cast<uint8_t *>(d_work);
    const auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t *>(W + at); };
    const auto u64 = [&](size_t at) { return reinterpret_cast<uint64_t *>(W + at); };
    uint64_t *const lens = u64(L.lens), *const ends = u64(L.ends);
    uint64_t *const rooms = u64(L.rooms), *const room_ends = u64(L.room_ends);     // (packed decompression)
    void *const temp = W + L.temp;
    const uint32_t grid = (npackets + 255u) / 256u;
    const uint8_t *const in = (const uint8_t *)c.d_in;
    uint8_t *const out = (uint8_t *)c.d_out;

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
    // ---- where each packet ends in its channel's string of packets (a scan over all runs: the differences are what counts);
    // packed decompression: the same of the rooms
    if (c.packed())
        hipLaunchKernelGGL(lzs_burst_lens_packed_kernel, dim3(grid), dim3(256), 0, stream, sidx, c.d_in_off, c.d_in_len, c.d_out_off, lens,
                           decompress ? rooms : (uint64_t *)nullptr, npackets);
    else
        hipLaunchKernelGGL(lzs_burst_lens_kernel, dim3(grid), dim3(256), 0, stream, sidx, c.d_in_len, c.in_len, lens, npackets);
    BURST_TRY(rocprim::inclusive_scan(nullptr, need, lens, ends, (size_t)npackets, rocprim::plus<uint64_t>(), stream));
    if (need > L.temp_bytes) return (int)hipErrorInvalidValue;
    BURST_TRY(rocprim::inclusive_scan(temp, need, lens, ends, (size_t)npackets, rocprim::plus<uint64_t>(), stream));
    if (c.packed() && decompress)
        BURST_TRY(rocprim::inclusive_scan(temp, need, rooms, room_ends, (size_t)npackets, rocprim::plus<uint64_t>(), stream));

    if (!decompress) {
        uint8_t *const slots = W + L.slots;
        if (c.packed())
            hipLaunchKernelGGL(lzs_burst_gather_packed_kernel, dim3(npackets), dim3(256), 0, stream, in, c.d_in_off, c.d_in_len, c.d_out_off,
                               skey, sidx, (const uint64_t *)ends, (const uint8_t *)d_states, nchannels, slots);
        else
            hipLaunchKernelGGL(lzs_burst_gather_kernel, dim3(npackets), dim3(256), 0, stream, in, c.in_stride, c.d_in_len,
                               c.in_len, skey, sidx, (const uint64_t *)ends, (const uint8_t *)d_states, nchannels, slots);
        BURST_TRY(hipGetLastError());
        const int e = c.packed() ? lzs_hip_launch_compress_channels_packed(c.d_out, c.d_out_off, d_out_len, c.d_in, c.d_in_off, c.d_in_len,
                                                                           nullptr, slots, d_status, npackets, stream_)
                                 : lzs_hip_launch_compress_channels(c.d_out, c.out_stride, c.out_cap, d_out_len, c.d_in, c.in_stride,
                                                                    c.d_in_len, c.in_len, nullptr, slots, d_status, npackets, stream_);
        if (e) return e;
        if (c.packed())
            hipLaunchKernelGGL(lzs_burst_commit_packed_kernel, dim3(npackets), dim3(128), 0, stream, c.d_in_off, c.d_in_len, c.d_out_off,
                               skey, sidx, (const uint8_t *)slots, nchannels, (uint8_t *)d_states, npackets);
        else
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
    const auto runs = [&](const uint32_t *run_key, const uint32_t *run_at) {
        if (c.packed())
            return lzs_hip_launch_decompress_runs_packed(c.d_out, c.d_out_off, d_out_len, c.d_in, c.d_in_off, c.d_in_len, room_ends, run_key,
                                                         run_at, u32(L.run_end), skey, sidx, nchannels, d_states, d_status, npackets, stream_);
        return lzs_hip_launch_decompress_runs(c.d_out, c.out_stride, c.out_cap, d_out_len, c.d_in, c.in_stride, c.d_in_len, c.in_len,
                                              run_key, run_at, u32(L.run_end), skey, sidx, nchannels, d_states, d_status, npackets, stream_);
    };
    if (split) {
        // ---- the heavy runs (a prefix of that order, found on the device) by PARSE and RESOLVE, the others by the run decoder
        // from tables of their own
        uint16_t *const origins = reinterpret_cast<uint16_t *>(W + L.origins);
        uint2 *const rec = reinterpret_cast<uint2 *>(W + L.rec);
        const uint32_t most_runs = npackets <= nchannels ? npackets : nchannels + 1u;     // (the ids out of range are one more)
        if (c.packed()) {
            hipLaunchKernelGGL(lzs_burst_split_plan_packed_kernel, dim3(grid), dim3(256), 0, stream, (const uint32_t *)w.current(),
                               (const uint32_t *)a.current(), split_min, (const uint64_t *)room_ends, origin_cap, u32(L.light_w),
                               u32(L.light_at), u32(L.nheavy), npackets);
            hipLaunchKernelGGL(lzs_burst_parse_packed_kernel, dim3(npackets), dim3(64), 0, stream, out, c.d_out_off, d_out_len, in,
                               c.d_in_off, c.d_in_len, (const uint64_t *)room_ends, skey, sidx, (const uint64_t *)ends,
                               (const uint32_t *)u32(L.run_end), (const uint8_t *)d_states, nchannels, d_status, origins, rec,
                               (const uint32_t *)u32(L.nheavy), split_min);
            hipLaunchKernelGGL(lzs_burst_resolve_packed_kernel, dim3(most_runs), dim3(256), 0, stream, out, c.d_out_off, c.d_in_off,
                               c.d_in_len, (const uint64_t *)room_ends, (const uint32_t *)a.current(), (const uint32_t *)u32(L.run_end),
                               skey, sidx, (uint8_t *)d_states, nchannels, (const uint16_t *)origins, (const uint2 *)rec,
                               (const uint32_t *)u32(L.nheavy));
        } else {
            hipLaunchKernelGGL(lzs_burst_split_plan_kernel, dim3(grid), dim3(256), 0, stream, (const uint32_t *)w.current(),
                               (const uint32_t *)a.current(), split_min, u32(L.light_w), u32(L.light_at), u32(L.nheavy), npackets);
            hipLaunchKernelGGL(lzs_burst_parse_kernel, dim3(npackets), dim3(64), 0, stream, out, c.out_stride, c.out_cap, d_out_len,
                               in, c.in_stride, c.d_in_len, c.in_len, skey, sidx, (const uint64_t *)ends,
                               (const uint32_t *)u32(L.run_end), (const uint8_t *)d_states, nchannels, d_status, origins, rec,
                               (const uint32_t *)u32(L.nheavy), split_min);
            hipLaunchKernelGGL(lzs_burst_resolve_kernel, dim3(most_runs), dim3(256), 0, stream, out, c.out_stride, c.out_cap,
                               (const uint32_t *)a.current(), (const uint32_t *)u32(L.run_end), skey, sidx, (uint8_t *)d_states,
                               nchannels, (const uint16_t *)origins, (const uint2 *)rec, (const uint32_t *)u32(L.nheavy));
        }
        BURST_TRY(hipGetLastError());
        return runs(u32(L.light_w), u32(L.light_at));
    }
    return runs(w.current(), a.current());
}

}  // namespace

extern "C" size_t lzs_hip_burst_work_bytes(size_t npackets)
{
    return burst_layout(npackets).total;
}

extern "C" int lzs_hip_burst(int decompress, void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                             const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                             const uint32_t *d_channel, void *d_states, uint32_t nchannels, uint8_t *d_status,
                             void *d_work, uint32_t npackets, int split, uint32_t split_min, void *stream_)
{
    const BurstCall c = {d_out, d_in, out_stride, in_stride, out_cap, in_len, d_in_len, nullptr, nullptr};
    return burst(decompress, c, d_out_len, d_channel, d_states, nchannels, d_status, d_work, npackets, split, 0, split_min, stream_);
}

extern "C" int lzs_hip_burst_packed(int decompress, void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                    const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel, void *d_states,
                                    uint32_t nchannels, uint8_t *d_status, void *d_work, uint32_t npackets, size_t origin_bytes,
                                    uint32_t split_min, void *stream_)
{
    const BurstCall c = {d_out, d_in, 0, 0, 0u, 0u, d_in_len, d_in_off, d_out_off};
    const uint64_t origin_cap = origin_bytes / 2u;
    return burst(decompress, c, d_out_len, d_channel, d_states, nchannels, d_status, d_work, npackets,
                 decompress && origin_cap != 0, origin_cap, split_min, stream_);
}
