// kernels/common.inc -- constants, LDS ring helpers, the wave-level output bit sink.
// Part of lzs_kernels.hip (included there, inside its anonymous namespace); not a translation unit of its own.

constexpr uint32_t kWindow     = 2047;   // farthest offset (11 bits)      lzs.h:60
constexpr uint32_t kSearchCap  = 12;     // search stops improving here    lzs-compression.c:62
constexpr uint32_t kTokenMax   = 8;      // first length code carries <=8  lzs-common.h:52
constexpr uint32_t kNibbleMax  = 15;     // extension nibble "continue"    lzs-common.h:53
constexpr uint32_t kShortMax   = 127;    // 7-bit offsets                  lzs-common.h:43

constexpr uint32_t kRing       = 4096;   // bytes, power of two >= window + tile + look-ahead
constexpr uint32_t kRingMask   = kRing - 1;
constexpr uint32_t kRingWords  = kRing / 4;
constexpr uint32_t kTile       = 1024;   // 64 lanes x 16 B per refill
constexpr uint32_t kLookAhead  = 64;     // bytes past c guaranteed resident (>= 15)
constexpr uint32_t kStage      = 256;    // output staging bytes per wave
constexpr uint32_t kWavesPerWG = 4;

struct __attribute__((aligned(16))) WaveLds {
    uint32_t ring[kRingWords];
    uint32_t stage[kStage / 4];
};

// A channel's state slot (include/lzs/lzs_channels.h): uint32 hist_len, reserved to byte 64, then 2048 bytes of history.
constexpr uint32_t kChanStateBytes = 2112u, kChanHistAt = 64u;

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// Entry b of a packed compress call (include/lzs/lzs_batch.h "PACKED streams"; DESIGN.md 3.15): its input at `from`, n bytes (in_len[b],
// or up to in_off[b + 1] without in_len), its output at `to` with `room` bytes (up to out_off[b + 1], clamped to 0xFFFFFFFF).  false:
// not a block -- offsets that decrease, or more than LZS_BLOCK_MAX bytes -- and n = room = 0: nothing of it is read or written.
__device__ __forceinline__ bool packed_entry(const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, uint32_t b,
                                             uint64_t &from, uint32_t &n, uint64_t &to, uint32_t &room)
{
    from = in_off[b];
    to = out_off[b];
    const uint64_t to_end = out_off[b + 1u];
    bool ok = to_end >= to;
    uint64_t len;
    if (in_len) {
        len = in_len[b];
    } else {
        const uint64_t next = in_off[b + 1u];
        ok = ok && next >= from;
        len = next - from;
    }
    ok = ok && len <= 0xC0000000ull;                               // LZS_BLOCK_MAX
    const uint64_t space = to_end - to;
    n = ok ? (uint32_t)len : 0u;
    room = ok ? (space < 0xFFFFFFFFull ? (uint32_t)space : 0xFFFFFFFFu) : 0u;
    return ok;
}

// Bursts with packet flags (include/lzs/lzs_channels.h LZS_PACKET_RESET; DESIGN.md 3.18): a reset starts a new run, so a channel may
// have several.  The decoders' tables by sorted position: rkey[i] = the run's id (1-based, ascending), rmark[i] = kRunStart at a run's
// first position, | kRunFresh where the run starts from an empty history and reads no slot; skey[i] = the channel.  Without flags
// rmark is null: a run per channel, from its slot, back to its slot.
constexpr uint32_t kRunStart = 1u, kRunFresh = 2u;

struct RunTables {
    const uint32_t *rkey = nullptr, *rmark = nullptr;
    uint8_t *stage = nullptr;                                      // staging slots, lzs_burst_plan_stage_slot() of the run
};

__device__ __forceinline__ bool run_is_fresh(const RunTables &rt, uint32_t at) { return rt.rmark != nullptr && (rt.rmark[at] & kRunFresh) != 0u; }

// Where the run at sorted positions [at, end) of n, of channel `key` in range whose slot is `st`, leaves its final history: nowhere
// (null) unless it is its channel's last; in the slot if it is also the first -- the workgroup that read the slot is the one that
// writes it --; otherwise in a staging slot, which lzs_burst_stage_commit_kernel copies to the channel after every decode kernel
// of the call has ended: no workgroup writes a slot that another may still read.
__device__ __forceinline__ uint8_t *run_commit_to(const RunTables &rt, const uint32_t *skey, uint32_t at, uint32_t end, uint32_t n,
                                                  uint32_t key, uint8_t *st)
{
    if (rt.rmark == nullptr) return st;
    if (end < n && skey[end] == key) return nullptr;
    if (at == 0u || skey[at - 1u] != key) return st;
    return rt.stage + (size_t)((rt.rkey[at] - 2u) / 2u) * kChanStateBytes;
}

// A value the optimiser may not look through (keeps a select a select, a compare a compare).
template <class T> __device__ __forceinline__ T opaque(T x) { asm volatile("" : "+v"(x)); return x; }

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = v > o ? v : o;
    }
    return v;
}

// 16 input bytes at block position p (multiple of 16), zero past n.
__device__ __forceinline__ uint4 load16(const uint8_t *src, uint32_t p, uint32_t n, bool aligned16, bool aligned4 = false)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p + 16 <= n && aligned16) {
        v = *reinterpret_cast<const uint4 *>(src + p);
    } else if (p + 16 <= n && aligned4) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(src + p);
        v = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (p < n) {
        uint32_t w[4] = {0, 0, 0, 0};
        uint32_t m = n - p < 16 ? n - p : 16;
        for (uint32_t k = 0; k < m; k++)
            w[k >> 2] |= (uint32_t)src[p + k] << (8 * (k & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

// 12 bytes of the ring starting at block position q (any alignment), little-endian words.
__device__ __forceinline__ void ring_read12(const uint32_t *ring, uint32_t q,
                                            uint32_t &w0, uint32_t &w1, uint32_t &w2)
{
    const uint32_t a = (q & kRingMask) >> 2;
    const uint32_t s = q & 3;
    const uint32_t d0 = ring[a];
    const uint32_t d1 = ring[(a + 1) & (kRingWords - 1)];
    const uint32_t d2 = ring[(a + 2) & (kRingWords - 1)];
    const uint32_t d3 = ring[(a + 3) & (kRingWords - 1)];
    w0 = __builtin_amdgcn_alignbyte(d1, d0, s);
    w1 = __builtin_amdgcn_alignbyte(d2, d1, s);
    w2 = __builtin_amdgcn_alignbyte(d3, d2, s);
}

__device__ __forceinline__ uint32_t ring_byte(const uint32_t *ring, uint32_t q)
{
    return reinterpret_cast<const uint8_t *>(ring)[q & kRingMask];
}

// Equal leading bytes (0..4) given the XOR of two little-endian words.
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x)
{
    const uint32_t t = ((uint32_t)__builtin_ffs((int)x) - 1u) >> 3;   // x==0 -> huge
    return t < 4u ? t : 4u;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // what a 128-bit buffer load returns

// 12 bytes of a ring with a 16-byte mirror (ring[kRingWords..+3] repeats ring[0..3]): no wrap handling.
__device__ __forceinline__ void ringm_read12(const uint32_t *ring, uint32_t q,
                                             uint32_t &w0, uint32_t &w1, uint32_t &w2)
{
    const uint32_t a = (q & kRingMask) >> 2;     // words a..a+3 exist thanks to the mirror
    const uint32_t d0 = ring[a], d1 = ring[a + 1], d2 = ring[a + 2], d3 = ring[a + 3];
    w0 = __builtin_amdgcn_alignbyte(d1, d0, q);  // v_alignbyte_b32 shifts by the low two bits of q
    w1 = __builtin_amdgcn_alignbyte(d2, d1, q);
    w2 = __builtin_amdgcn_alignbyte(d3, d2, q);
}

// Inclusive prefix sum across the wave with DPP adds only (no LDS round trips):
// row_shr 1/2/4/8 scan each row of 16, row_bcast 15/31 carry the row totals upward.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

constexpr uint32_t kNoLink    = 0xFFFFu;
#ifndef LZS_REFILL_MIN
#define LZS_REFILL_MIN 32
#endif
constexpr uint32_t kRefillMin = LZS_REFILL_MIN;  // idle lanes that justify a refill pass

// in-kernel profiling hooks (tools/probes/prof_compress.hip builds with LZS_PROFILE; empty otherwise)
#ifdef LZS_PROFILE
// Diagnostic build only (tools/probes/prof_compress): per-phase cycle sums of every wave, by the wave's role in
// CHAIN (role 0 chains the 3-byte buckets, role 1 the 2-byte buckets, roles 2 and 3 wait there); entries 32.. are the
// cycles spent inside each workgroup barrier of the round (PROF_SYNC).
constexpr int kProfN = 48;
__device__ unsigned long long lzs_prof[4][kProfN];
#ifdef LZS_PROFILE_COUNTS     // the counts alone (trips for tools/ledger.py): no cycle stamps, plain barriers -- the kernel's own timing
#define PROF_DECL uint32_t prof_acc[kProfN] = {0}               /* (32 bits: fewer registers; a block's counts fit) */
#define PROF_MARK(i)
#define PROF_COUNT(i, v) do { prof_acc[i] += (v); } while (0)
#define PROF_T0
#define PROF_T1(i)
#define PROF_T0B
#define PROF_T1B(i)
#define PROF_T0C
#define PROF_T1C(i)
#define PROF_STAMP0
#define PROF_STAMP(i)
#define PROF_SYNC(i) __syncthreads()
#else
#define PROF_DECL unsigned long long prof_t = __builtin_readcyclecounter(), prof_acc[kProfN] = {0}
#define PROF_MARK(i) do { unsigned long long t_ = __builtin_readcyclecounter(); prof_acc[i] += t_ - prof_t; prof_t = t_; } while (0)
#define PROF_COUNT(i, v) do { prof_acc[i] += (v); } while (0)
#define PROF_T0 unsigned long long prof_u = __builtin_readcyclecounter()
#define PROF_T1(i) do { prof_acc[i] += __builtin_readcyclecounter() - prof_u; } while (0)
#define PROF_T0B unsigned long long prof_v = __builtin_readcyclecounter()
#define PROF_T1B(i) do { prof_acc[i] += __builtin_readcyclecounter() - prof_v; } while (0)
#define PROF_T0C unsigned long long prof_w = __builtin_readcyclecounter()
#define PROF_T1C(i) do { prof_acc[i] += __builtin_readcyclecounter() - prof_w; } while (0)
#define PROF_STAMP0 unsigned long long prof_s = __builtin_readcyclecounter()
#define PROF_STAMP(i) do { unsigned long long t_ = __builtin_readcyclecounter(); prof_acc[i] += t_ - prof_s; prof_s = t_; } while (0)
#define PROF_SYNC(i) do { unsigned long long t_ = __builtin_readcyclecounter(); __syncthreads(); prof_acc[i] += __builtin_readcyclecounter() - t_; } while (0)
#endif
// (trips of a loop that only some lanes run: the longest lane's count)
#define PROF_ITER_DECL uint32_t prof_it = 0
#define PROF_ITER prof_it++
#define PROF_ITER_DONE(i) do { prof_acc[i] += wave_max(prof_it); prof_it = 0; } while (0)
#define PROF_DONE do { if (lane == 0) for (int i_ = 0; i_ < kProfN; i_++) atomicAdd(&lzs_prof[(wave + blockIdx.x) & 3u][i_], (unsigned long long)prof_acc[i_]); } while (0)
#else
#define PROF_DECL
#define PROF_MARK(i)
#define PROF_COUNT(i, v)
#define PROF_T0
#define PROF_T1(i)
#define PROF_T0B
#define PROF_T1B(i)
#define PROF_T0C
#define PROF_T1C(i)
#define PROF_STAMP0
#define PROF_STAMP(i)
#define PROF_SYNC(i) __syncthreads()
#define PROF_ITER_DECL
#define PROF_ITER
#define PROF_ITER_DONE(i)
#define PROF_DONE
#endif
