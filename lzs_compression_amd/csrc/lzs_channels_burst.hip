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
// Packet flags (lzs_*_channels_burst*_flags_device): a packet flagged LZS_PACKET_RESET starts from an empty history,
// so it depends on nothing before it and STARTS A NEW RUN.  The start marks -- a channel's first position, or a flagged block of a
// channel in range -- are scanned into run ids (rkey[], ascending by sorted position like skey[]), and every place that looks for a
// run's borders searches rkey[] where it searched skey[]; without flags rkey is skey and rmark null, and every kernel does what it
// did.  A run that a reset started reads no slot; only a channel's last run leaves a history, and where that is not also its first
// run it goes to a staging slot that a kernel behind all the others copies to the channel (run_commit_to, kernels/common.inc).
//
// (<cstring> and the HIP runtime before rocPRIM: its texture cache iterator uses memset in host code.)
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "lzs_burst_plan.h"                    // the work area's layout and a call's host decisions: plain functions, held to a table on the CPU
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

// (packet flags) start[i] = 1 where a run starts at sorted position i -- the first of its channel, or a flagged packet of a channel
// in range that is a block --, 0 elsewhere: their inclusive scan is the run id of every position.  rmark[i]: kRunStart, kRunFresh.
template <bool PACKED>
__device__ __forceinline__ void burst_marks(const BurstIo &io, const uint8_t *__restrict__ flags, const uint32_t *__restrict__ skey,
                                            const uint32_t *__restrict__ sidx, uint32_t nchannels, uint32_t *__restrict__ start,
                                            uint32_t *__restrict__ rmark, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = skey[i], p = sidx[i];
    const bool first = i == 0u || skey[i - 1u] != key;
    const bool reset = (flags[p] & 1u) != 0u && key < nchannels && burst_packet<PACKED>(io, p).block;
    start[i] = first || reset ? 1u : 0u;
    rmark[i] = (first || reset ? kRunStart : 0u) | (reset ? kRunFresh : 0u);
}

__global__ __launch_bounds__(256) void lzs_burst_marks_kernel(const uint8_t *__restrict__ flags, const uint32_t *__restrict__ skey,
                                                              const uint32_t *__restrict__ sidx, uint32_t nchannels,
                                                              uint32_t *__restrict__ start, uint32_t *__restrict__ rmark, uint32_t n)
{
    burst_marks<false>(BurstIo{}, flags, skey, sidx, nchannels, start, rmark, n);
}

__global__ __launch_bounds__(256) void lzs_burst_marks_packed_kernel(const uint64_t *__restrict__ in_off, const uint32_t *__restrict__ in_len,
                                                                     const uint64_t *__restrict__ out_off, const uint8_t *__restrict__ flags,
                                                                     const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                                     uint32_t nchannels, uint32_t *__restrict__ start,
                                                                     uint32_t *__restrict__ rmark, uint32_t n)
{
    burst_marks<true>(burst_packed(nullptr, in_off, in_len, nullptr, out_off), flags, skey, sidx, nchannels, start, rmark, n);
}

// (packet flags, decompression) One workgroup per sorted position: where the last run of a channel that has several starts, its
// staging slot goes to the channel -- after every kernel that may read that channel's slot has ended (run_commit_to).  Such a run
// was started by a reset, so it is of a channel in range, holds a block and was decoded: its staging slot was written.
__global__ __launch_bounds__(128) void lzs_burst_stage_commit_kernel(const uint32_t *__restrict__ skey, RunTables rt,
                                                                     uint8_t *__restrict__ states, uint32_t n)
{
    const uint32_t i = blockIdx.x;
    if ((rt.rmark[i] & kRunStart) == 0u) return;
    const uint32_t key = skey[i];
    if (i == 0u || skey[i - 1u] != key) return;                            // the channel's first run: it wrote the slot itself, if it is the last
    const uint32_t end = run_last_end(rt.rkey, i, n, rt.rkey[i]);
    if (end < n && skey[end] == key) return;
    const uint32_t *const from = reinterpret_cast<const uint32_t *>(run_commit_to(rt, skey, i, end, n, key, nullptr));
    uint32_t *const to = reinterpret_cast<uint32_t *>(states + (size_t)key * kStateBytes);
    for (uint32_t w = threadIdx.x; w < 512u; w += 128u) to[kHistAt / 4u + w] = from[kHistAt / 4u + w];
    if (threadIdx.x == 0) to[0] = from[0];
}

// One workgroup per sorted position i: the history packet p = sidx[i] is compressed with, into work slot p -- the last
// H <= 2047 bytes of (the channel's slot | the packets at sorted positions [start, i)), where `start` begins the run.  With
// ends[] the inclusive scan of the lengths, the run's earlier packets are the bytes [ends[start - 1], ends[i - 1]) of one
// string; a history byte there is found by binary search over ends[start, i) (a run of 40-byte packets needs 50 of them, a
// packet of 0 bytes none).  A channel id out of range or a slot that is not a state: hist_len = ~0, which the channel kernel
// answers with ERROR, and the slot is not committed.  rt (packet flags): the run is the one of rkey[], and one that a reset
// started has no slot in front of it -- the slot is not read, whatever it holds.
__global__ __launch_bounds__(256) void lzs_burst_gather_kernel(const uint8_t *__restrict__ in, size_t in_stride,
                                                               const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                                               const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                               const uint64_t *__restrict__ ends, const uint8_t *__restrict__ states,
                                                               uint32_t nchannels, uint8_t *__restrict__ work_slots, RunTables rt)
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
                                                                      uint32_t nchannels, uint8_t *__restrict__ work_slots, RunTables rt)
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
// Packet flags change nothing here: the last position of a channel is the last of its last run, whose work slot holds that run's
// history alone; and a run that a reset started begins with a block, so the walk back finds one inside it.
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
                                                             const uint32_t *__restrict__ nheavy, uint32_t split_min, RunTables rt)
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
                                                                    const uint32_t *__restrict__ nheavy, uint32_t split_min, RunTables rt)
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
// rt (packet flags): a run that a reset started begins with the ring all zero and reads no slot, and the run's history goes where
// run_commit_to says -- nowhere, the slot, or a staging slot.
template <bool PACKED>
__device__ __forceinline__ void burst_resolve(const BurstIo &io, const uint32_t *__restrict__ run_at, const uint32_t *__restrict__ run_end,
                                              const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                              uint8_t *__restrict__ states, uint32_t nchannels,
                                              const uint16_t *__restrict__ origins, const uint2 *__restrict__ rec,
                                              const uint32_t *__restrict__ nheavy, const RunTables &rt, uint32_t n)
{
    __shared__ __attribute__((aligned(16))) uint8_t ring[kResolveRing];
    __shared__ uint8_t aside[kResolveFast];
    __shared__ uint32_t meta_p[2u * kResolveMeta], meta_len[2u * kResolveMeta], meta_open[2u * kResolveMeta];
    const uint32_t r = blockIdx.x, t = threadIdx.x;
    if (r >= *nheavy) return;
    const uint32_t at = run_at[r], end = run_end[at], key = skey[at];
    if (key >= nchannels) return;
    uint8_t *const st = states + (size_t)key * kStateBytes;
    const uint32_t hl = run_is_fresh(rt, at) ? 0u : *reinterpret_cast<const uint32_t *>(st);
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
    uint8_t *const to = run_commit_to(rt, skey, at, end, n, key, st);
    if (to == nullptr) return;
    const uint32_t H = hl + produced < kWindow ? hl + produced : kWindow;
    uint32_t *const hist = reinterpret_cast<uint32_t *>(to + kHistAt);
    for (uint32_t w = t; w < 512u; w += 256u) {
        uint32_t word = 0;
        for (uint32_t b = 0; b < 4u; b++) {
            const uint32_t x = 4u * w + b;
            if (x < H) word |= (uint32_t)ring[(P - H + x) & (kResolveRing - 1u)] << (8u * b);
        }
        hist[w] = word;
    }
    if (t == 0) *reinterpret_cast<uint32_t *>(to) = H;
}

__global__ __launch_bounds__(256) void lzs_burst_resolve_kernel(uint8_t *__restrict__ out, size_t out_stride, uint32_t out_cap,
                                                                const uint32_t *__restrict__ run_at, const uint32_t *__restrict__ run_end,
                                                                const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                                uint8_t *__restrict__ states, uint32_t nchannels,
                                                                const uint16_t *__restrict__ origins, const uint2 *__restrict__ rec,
                                                                const uint32_t *__restrict__ nheavy, RunTables rt, uint32_t n)
{
    burst_resolve<false>(burst_strided(nullptr, 0, nullptr, 0u, out, out_stride, out_cap), run_at, run_end, skey, sidx, states, nchannels,
                         origins, rec, nheavy, rt, n);
}

__global__ __launch_bounds__(256) void lzs_burst_resolve_packed_kernel(uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
                                                                       const uint64_t *__restrict__ in_off, const uint32_t *__restrict__ in_len,
                                                                       const uint64_t *__restrict__ room_ends,
                                                                       const uint32_t *__restrict__ run_at, const uint32_t *__restrict__ run_end,
                                                                       const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                                       uint8_t *__restrict__ states, uint32_t nchannels,
                                                                       const uint16_t *__restrict__ origins, const uint2 *__restrict__ rec,
                                                                       const uint32_t *__restrict__ nheavy, RunTables rt, uint32_t n)
{
    burst_resolve<true>(burst_packed(nullptr, in_off, in_len, out, out_off, room_ends), run_at, run_end, skey, sidx, states, nchannels,
                        origins, rec, nheavy, rt, n);
}

// ---- The host side: a call's stages, in order.  Where the parts of the work area lie, and what a call decides before it launches,
// is lzs_burst_plan.h's (tests/cpu_shim/burst_plan_check.c).
static_assert(kStateBytes == LZS_BURST_SLOT_BYTES && kAlign == LZS_BURST_ALIGN && kSortSpareBytes == LZS_BURST_SORT_SPARE,
              "lzs_burst_plan.h lays the work area out with these");

#define BURST_TRY(x) do { const int e_ = (int)(x); if (e_ != 0) return e_; } while (0)

// One burst on its way through the stages: what the call gives -- the packets strided (in_off: nullptr) or packed --, what the host
// decided for it (lzs_burst_plan.h), the parts of the work area, and what a stage leaves for those behind it.
struct Burst {
    uint8_t *out;
    const uint8_t *in;
    size_t out_stride, in_stride;
    uint32_t out_cap, in_len_uniform;
    const uint32_t *in_len;
    const uint64_t *in_off, *out_off;
    bool packed() const { return in_off != nullptr; }
    int decompress;
    uint32_t *out_len;
    const uint32_t *channel;
    const uint8_t *flags;                          // a byte a packet, bit 0: a reset in front of it; or nullptr
    uint8_t *states, *status;
    uint32_t nchannels, npackets, grid;            // grid: workgroups of 256 threads, a thread a packet
    uint64_t origin_cap;                           // (split, PACKED) 16-bit origins behind the burst part; the strided call's host code knows that they fit
    uint32_t split_min;
    hipStream_t stream;
    // the work area (rooms, room_ends: packed decompression)
    uint8_t *slots;
    uint32_t *key[2], *val[2], *weight[2], *at[2], *run_end, *light_w, *light_at, *nheavy;
    uint64_t *lens, *ends, *rooms, *room_ends;
    uint2 *rec;
    uint16_t *origins;
    void *temp;                                    // rocPRIM's
    size_t temp_bytes;
    const uint32_t *skey, *sidx;                   // group: channel (nchannels if out of range) and packet at each sorted position
    uint32_t *key_free, *val_free;                 // group: the halves of key[] and val[] the sort left unused
    uint8_t *stage;                                // (flags, decompression) staging slots of the channels with several runs
    RunTables rt;                                  // runs: without flags a run a channel (rkey = skey, no marks), else the scanned marks
    const uint32_t *run_w, *run_at;                // runs by weight, then split: the runs the run decoder takes, heaviest first
};

void burst_lay_out(Burst &b, void *d_work)
{
    const lzs_burst_layout_t L = lzs_burst_layout(b.npackets);
    uint8_t *const W = static_cast<uint8_t *>(d_work);
    const auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t *>(W + at); };
    const auto u64 = [&](size_t at) { return reinterpret_cast<uint64_t *>(W + at); };
    b.slots = W + L.slots;
    for (int k = 0; k < 2; k++) { b.key[k] = u32(L.key[k]); b.val[k] = u32(L.val[k]); b.weight[k] = u32(L.weight[k]); b.at[k] = u32(L.at[k]); }
    b.run_end = u32(L.run_end); b.light_w = u32(L.light_w); b.light_at = u32(L.light_at); b.nheavy = u32(L.nheavy);
    b.lens = u64(L.lens); b.ends = u64(L.ends); b.rooms = u64(L.rooms); b.room_ends = u64(L.room_ends);
    b.rec = reinterpret_cast<uint2 *>(W + L.rec); b.origins = reinterpret_cast<uint16_t *>(W + L.origins);
    b.temp = W + L.temp; b.temp_bytes = L.temp_bytes;
    b.stage = W + L.stage;
}

// rocPRIM's way, once: call(nullptr, need) asks for the temporary storage's size, which the layout's has to cover; then it runs.
template <class Call>
int burst_prim(const Burst &b, Call call)
{
    size_t need = 0;
    BURST_TRY(call(nullptr, need));
    if (need > b.temp_bytes) return (int)hipErrorInvalidValue;
    return (int)call(b.temp, need);
}

int burst_scan(const Burst &b, uint64_t *from, uint64_t *to)
{
    return burst_prim(b, [&](void *temp, size_t &need) {
        return rocprim::inclusive_scan(temp, need, from, to, (size_t)b.npackets, rocprim::plus<uint64_t>(), b.stream); });
}

// ---- the runs: a stable sort by channel
int burst_group(Burst &b)
{
    hipLaunchKernelGGL(lzs_burst_keys_kernel, dim3(b.grid), dim3(256), 0, b.stream, b.channel, b.nchannels, b.key[0], b.val[0], b.npackets);
    const unsigned bits = lzs_burst_plan_sort_bits(b.nchannels);
    rocprim::double_buffer<uint32_t> keys(b.key[0], b.key[1]), vals(b.val[0], b.val[1]);
    const int e = burst_prim(b, [&](void *temp, size_t &need) {
        return rocprim::radix_sort_pairs(temp, need, keys, vals, b.npackets, 0u, bits, b.stream); });
    b.skey = keys.current(); b.sidx = vals.current();
    b.key_free = keys.alternate(); b.val_free = vals.alternate();
    return e;
}

// ---- the runs inside the channels: without flags one each; with flags a reset starts another (marks in weight[0], which no direction
// has written yet, scanned into ids)
int burst_runs(Burst &b)
{
    b.rt = RunTables{b.skey, nullptr, nullptr};
    if (!b.flags) return 0;
    uint32_t *const start = b.weight[0];
    if (b.packed())
        hipLaunchKernelGGL(lzs_burst_marks_packed_kernel, dim3(b.grid), dim3(256), 0, b.stream, b.in_off, b.in_len, b.out_off, b.flags, b.skey,
                           b.sidx, b.nchannels, start, b.val_free, b.npackets);
    else
        hipLaunchKernelGGL(lzs_burst_marks_kernel, dim3(b.grid), dim3(256), 0, b.stream, b.flags, b.skey, b.sidx, b.nchannels, start, b.val_free,
                           b.npackets);
    BURST_TRY(hipGetLastError());
    uint32_t *const rkey = b.key_free;
    BURST_TRY(burst_prim(b, [&](void *temp, size_t &need) {
        return rocprim::inclusive_scan(temp, need, start, rkey, (size_t)b.npackets, rocprim::plus<uint32_t>(), b.stream); }));
    b.rt = RunTables{rkey, b.val_free, b.decompress ? b.stage : nullptr};
    return 0;
}

// ---- where each packet ends in its channel's string of packets (a scan over all runs: the differences are what counts); packed
// decompression: the same of the rooms
int burst_lengths(const Burst &b)
{
    const bool rooms = b.packed() && b.decompress;
    if (b.packed())
        hipLaunchKernelGGL(lzs_burst_lens_packed_kernel, dim3(b.grid), dim3(256), 0, b.stream, b.sidx, b.in_off, b.in_len, b.out_off, b.lens,
                           rooms ? b.rooms : nullptr, b.npackets);
    else
        hipLaunchKernelGGL(lzs_burst_lens_kernel, dim3(b.grid), dim3(256), 0, b.stream, b.sidx, b.in_len, b.in_len_uniform, b.lens, b.npackets);
    BURST_TRY(burst_scan(b, b.lens, b.ends));
    return rooms ? burst_scan(b, b.rooms, b.room_ends) : 0;
}

// ---- compression: every packet's history into its work slot, the channel kernel on all packets, each run's last slot to its channel
int burst_compress(const Burst &b)
{
    const dim3 grid(b.npackets);
    if (b.packed()) {
        hipLaunchKernelGGL(lzs_burst_gather_packed_kernel, grid, dim3(256), 0, b.stream, b.in, b.in_off, b.in_len, b.out_off, b.skey, b.sidx,
                           b.ends, b.states, b.nchannels, b.slots, b.rt);
        BURST_TRY(hipGetLastError());
        BURST_TRY(lzs_hip_launch_compress_channels_packed(b.out, b.out_off, b.out_len, b.in, b.in_off, b.in_len, nullptr, b.slots, b.status,
                                                          b.npackets, b.stream));
        hipLaunchKernelGGL(lzs_burst_commit_packed_kernel, grid, dim3(128), 0, b.stream, b.in_off, b.in_len, b.out_off, b.skey, b.sidx, b.slots,
                           b.nchannels, b.states, b.npackets);
    } else {
        hipLaunchKernelGGL(lzs_burst_gather_kernel, grid, dim3(256), 0, b.stream, b.in, b.in_stride, b.in_len, b.in_len_uniform, b.skey, b.sidx,
                           b.ends, b.states, b.nchannels, b.slots, b.rt);
        BURST_TRY(hipGetLastError());
        BURST_TRY(lzs_hip_launch_compress_channels(b.out, b.out_stride, b.out_cap, b.out_len, b.in, b.in_stride, b.in_len, b.in_len_uniform,
                                                   nullptr, b.slots, b.status, b.npackets, b.stream));
        hipLaunchKernelGGL(lzs_burst_commit_kernel, grid, dim3(128), 0, b.stream, b.skey, b.sidx, b.slots, b.nchannels, b.states, b.npackets);
    }
    return (int)hipGetLastError();
}

// ---- decompression: the runs by weight, heaviest first
int burst_runs_by_weight(Burst &b)
{
    hipLaunchKernelGGL(lzs_burst_runs_kernel, dim3(b.grid), dim3(256), 0, b.stream, b.rt.rkey, b.ends, b.weight[0], b.at[0], b.run_end, b.npackets);
    rocprim::double_buffer<uint32_t> w(b.weight[0], b.weight[1]), a(b.at[0], b.at[1]);
    const int e = burst_prim(b, [&](void *temp, size_t &need) {
        return rocprim::radix_sort_pairs_desc(temp, need, w, a, b.npackets, 0u, 32u, b.stream); });
    b.run_w = w.current(); b.run_at = a.current();
    return e;
}

// ---- the heavy runs (a prefix of that order, found on the device) by PARSE and RESOLVE; the others are left in tables of their own
int burst_split(Burst &b)
{
    const dim3 grid(b.grid), packets(b.npackets), runs(lzs_burst_plan_resolve_grid_flags(b.npackets, b.nchannels, b.flags != nullptr));
    if (b.packed()) {
        hipLaunchKernelGGL(lzs_burst_split_plan_packed_kernel, grid, dim3(256), 0, b.stream, b.run_w, b.run_at, b.split_min, b.room_ends,
                           b.origin_cap, b.light_w, b.light_at, b.nheavy, b.npackets);
        hipLaunchKernelGGL(lzs_burst_parse_packed_kernel, packets, dim3(64), 0, b.stream, b.out, b.out_off, b.out_len, b.in, b.in_off, b.in_len,
                           b.room_ends, b.skey, b.sidx, b.ends, b.run_end, b.states, b.nchannels, b.status, b.origins, b.rec, b.nheavy,
                           b.split_min, b.rt);
        hipLaunchKernelGGL(lzs_burst_resolve_packed_kernel, runs, dim3(256), 0, b.stream, b.out, b.out_off, b.in_off, b.in_len, b.room_ends,
                           b.run_at, b.run_end, b.skey, b.sidx, b.states, b.nchannels, b.origins, b.rec, b.nheavy, b.rt, b.npackets);
    } else {
        hipLaunchKernelGGL(lzs_burst_split_plan_kernel, grid, dim3(256), 0, b.stream, b.run_w, b.run_at, b.split_min, b.light_w, b.light_at,
                           b.nheavy, b.npackets);
        hipLaunchKernelGGL(lzs_burst_parse_kernel, packets, dim3(64), 0, b.stream, b.out, b.out_stride, b.out_cap, b.out_len, b.in, b.in_stride,
                           b.in_len, b.in_len_uniform, b.skey, b.sidx, b.ends, b.run_end, b.states, b.nchannels, b.status, b.origins, b.rec,
                           b.nheavy, b.split_min, b.rt);
        hipLaunchKernelGGL(lzs_burst_resolve_kernel, runs, dim3(256), 0, b.stream, b.out, b.out_stride, b.out_cap, b.run_at, b.run_end, b.skey,
                           b.sidx, b.states, b.nchannels, b.origins, b.rec, b.nheavy, b.rt, b.npackets);
    }
    BURST_TRY(hipGetLastError());
    b.run_w = b.light_w; b.run_at = b.light_at;
    return 0;
}

// ---- one decoder stream a run
int burst_decode_runs(const Burst &b)
{
    if (b.packed())
        return lzs_hip_launch_decompress_runs_packed(b.out, b.out_off, b.out_len, b.in, b.in_off, b.in_len, b.room_ends, b.run_w, b.run_at,
                                                     b.run_end, b.skey, b.sidx, b.nchannels, b.states, b.status, b.npackets, b.rt.rkey, b.rt.rmark,
                                                     b.rt.stage, b.stream);
    return lzs_hip_launch_decompress_runs(b.out, b.out_stride, b.out_cap, b.out_len, b.in, b.in_stride, b.in_len, b.in_len_uniform, b.run_w,
                                          b.run_at, b.run_end, b.skey, b.sidx, b.nchannels, b.states, b.status, b.npackets, b.rt.rkey, b.rt.rmark, b.rt.stage,
                                          b.stream);
}

// ---- (flags) the staged final slots to their channels, behind every kernel that read a slot
int burst_commit_staged(const Burst &b)
{
    hipLaunchKernelGGL(lzs_burst_stage_commit_kernel, dim3(b.npackets), dim3(128), 0, b.stream, b.skey, b.rt, b.states, b.npackets);
    return (int)hipGetLastError();
}

// One burst: the grouping, then the kernels of the direction.  b: where the packets lie.  split (decompression): the long runs by PARSE and RESOLVE.
int burst(Burst &b, int decompress, uint32_t *d_out_len, const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, uint32_t nchannels, uint8_t *d_status,
          void *d_work, uint32_t npackets, int split, uint64_t origin_cap, uint32_t split_min, void *stream)
{
    if (npackets == 0) return 0;
    b.decompress = decompress; b.out_len = d_out_len; b.channel = d_channel; b.flags = d_flags; b.states = static_cast<uint8_t *>(d_states); b.status = d_status;
    b.nchannels = nchannels; b.npackets = npackets; b.grid = (npackets + 255u) / 256u;
    b.origin_cap = origin_cap; b.split_min = split_min; b.stream = static_cast<hipStream_t>(stream);
    burst_lay_out(b, d_work);
    BURST_TRY(burst_group(b));
    BURST_TRY(burst_runs(b));
    BURST_TRY(burst_lengths(b));
    if (!decompress) return burst_compress(b);
    BURST_TRY(burst_runs_by_weight(b));
    if (split) BURST_TRY(burst_split(b));
    BURST_TRY(burst_decode_runs(b));
    return b.flags ? burst_commit_staged(b) : 0;
}

}  // namespace

extern "C" int lzs_hip_burst(int decompress, void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                             const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                             const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, uint32_t nchannels, uint8_t *d_status,
                             void *d_work, uint32_t npackets, int split, uint32_t split_min, void *stream)
{
    Burst b = {(uint8_t *)d_out, (const uint8_t *)d_in, out_stride, in_stride, out_cap, in_len, d_in_len, nullptr, nullptr};
    return burst(b, decompress, d_out_len, d_channel, d_flags, d_states, nchannels, d_status, d_work, npackets, split, 0, split_min, stream);
}

extern "C" int lzs_hip_burst_packed(int decompress, void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                    const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                    const uint8_t *d_flags, void *d_states, uint32_t nchannels, uint8_t *d_status, void *d_work, uint32_t npackets, int split,
                                    uint64_t origin_cap, uint32_t split_min, void *stream)
{
    Burst b = {(uint8_t *)d_out, (const uint8_t *)d_in, 0, 0, 0u, 0u, d_in_len, d_in_off, d_out_off};
    return burst(b, decompress, d_out_len, d_channel, d_flags, d_states, nchannels, d_status, d_work, npackets, split, origin_cap, split_min, stream);
}
