// lzs_kernels.hip -- hand-written CDNA4 (gfx950) kernels for the LZS one-shot path,
// plus the extern-"C" shim the C host library calls.
//
// Path and contract (what must come out, bit for bit):
//   reference c/src/liblzs/lzs-compression.c:249-467   lzs_compress()
//   reference c/src/liblzs/lzs-decompression.c:156-412 lzs_decompress()
// The encoder decision rule is SURVEY.md Appendix A.2: at each token start c, take the
// NEAREST offset in 1..min(c,2047) that maximises min(common_prefix, min(remaining,12));
// a match whose first length code is 8 is then extended at that same offset in nibbles
// of up to 15 bytes.  The search is a pure function of (input, c), which is what makes
// the lane-parallel scan below legal.
//
// The kernels are in kernels/*.inc, included below into one translation unit (one hipcc run,
// one anonymous namespace):
//   common.inc             constants, LDS ring helpers, the wave-level bit sink
//   compress_wg.inc        the default compressor: one 256-thread workgroup per block, pools of
//                          512 positions pipelined through HASH/CHAIN, SEARCH, EXTEND, PARSE, PACK
//                          (DESIGN.md 3.1); the same loop from the middle of a stream for segments
//                          of one long stream, their bit-level stitch, and the resume of a long
//                          match for the incremental interface (3.5, 3.7)
//   (tools/variants/compress_variants.inc: "scan" and "chain", the earlier compressors -- LZS_KERNEL=, A/B builds only)
//   decompress_blocks.inc  eight streams per wavefront (3.3); the earlier one-wavefront-per-stream
//                          decoders for A/B builds
//   decompress_stream.inc  one stream or a small batch on many wavefronts: scan (a lane per
//                          segment), decode with per-byte origins (eight segments per wavefront),
//                          origins resolved on the segments' tails by chunks, then everywhere (3.6)
//   compact_resume.inc     slot compaction (3.4); the resumable decoder of the incremental
//                          interface (3.7)
// No MFMA anywhere: this is byte search and bit packing, not a contraction.
//
// The library compiles this file TWICE (csrc/Makefile): -DLZS_TU_COMPRESS at -Os -fno-unroll-loops -- the compress kernel's
// 15 KB of code are run by five workgroups per CU at five different places, and smaller is faster there -- and
// -DLZS_TU_DECOMPRESS at -O3 -fno-unroll-loops, which the decoders' one loop prefers by 2-4 % (profiles/r05/
// abdec_s27_optimisation_levels.txt).  Each half leaves the other's kernels and launchers out; with neither macro (the probes
// of tools/probes/, which include this file) everything is in.
//
// gfx950 only.  No CUDA compatibility layer, no alternate code paths.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <pthread.h>
#include <stdlib.h>

#include "lzs_hip_shim.h"
#include "lzs_launch_plan.h"       // which kernels a launcher runs: plain functions, held to a table on the CPU (tests/cpu_shim/plan_check.c)

namespace {

#include "kernels/common.inc"
#ifndef LZS_TU_DECOMPRESS
#ifdef LZS_WITH_VARIANTS   // the earlier compressors ("chain", "scan") and the v1 decoder: A/B builds only
#include "compress_variants.inc"                 // tools/variants/ (the Makefile adds the path for liblzs_variants.so only)
#endif
// The compress kernel, once per variant (kernels/compress_wg.inc says what the LZS_WGV_* mean): the default, the
// order-independent CHAIN for a device that fails the LDS ordering check, and the two a block's class may ask for.
namespace wgv_text {
#define LZS_WGV_SEGMENTS 1
#define LZS_WGV_HOP_END 1        // (round 7: hops may end a walk, 2 + 3 hops a pass -- the block and packed entries; profiles/r07/README.md)
#define LZS_WGV_HOPS_LAST 3
#include "kernels/wgv_text_shape.inc"
#include "kernels/compress_wg.inc"
}
namespace wgv_safe {
#define LZS_WGV_CHAIN_SAFE 1
#define LZS_WGV_SEGMENTS 1
#define LZS_WGV_PRIO 1
#include "kernels/compress_wg.inc"
}
// The channel kernel (lzs_compress_channels_wg_kernel: [history | packet] as one view) in the default shape and in the
// order-independent CHAIN form; nothing else is compiled into these two.
namespace wgv_text_ch {
#define LZS_WGV_CHANNELS 1
#include "kernels/wgv_text_shape.inc"
#include "kernels/compress_wg.inc"
}
namespace wgv_safe_ch {
#define LZS_WGV_CHANNELS 1
#define LZS_WGV_CHAIN_SAFE 1
#define LZS_WGV_PRIO 1
#include "kernels/compress_wg.inc"
}
#ifdef LZS_WITH_VARIANTS      // liblzs_variants.so only (LZS_KERNEL=wg8 | p256): round 6's two other shapes of the default kernel, kept
namespace wgv_text8 {         // under test as parameters of kernels/compress_wg.inc -- eight waves per workgroup (pools of 1024) ...
#define LZS_WGV_PRIO 1
#define LZS_WGV_WG_WAVES 8
#define LZS_WGV_WAVES 6
#define LZS_WGV_EXIT8 1
#include "kernels/compress_wg.inc"
}
namespace wgv_pool256 {       // ... and pools of 256 positions (one chunk per wave)
#define LZS_WGV_PRIO 1
#define LZS_WGV_POOL 256
#include "kernels/compress_wg.inc"
}
#endif
#ifndef LZS_ONE_VARIANT      // (tools/probes/ab.sh -DLZS_ONE_VARIANT: the default alone, for the probes that launch it directly)
// Round 6: NEITHER of the two keeps a 3-byte chain (LZS_WGV_NO3: every position walks the 2-byte chain with the full rule, which is
// exact for any block -- that chain is complete for every match of 2 and more).  Where grams do not repeat the 3-byte chain holds
// collisions only, where few grams repeat endlessly it holds what the 2-byte chain holds; without head3[] / link3[] HASH and CHAIN do
// half the work, a step has no restart on another chain, and 18.5 KB of LDS with the registers held to 64 (LZS_WGV_WAVES: no vector
// spills) are EIGHT workgroups per CU -- all a SIMD takes.  profiles/r06/ab_s10 ... ab_s15, GB/s through the library's launch:
//   high entropy 107.4 (both chains, six workgroups) -> 115 (no 3-byte chain, 1024 buckets, seven) -> 119-122 (2048 buckets; hops 0 / 1 / 2 /
//   3 / 4 / 5: 120.2 / 122.4 / 121.5 / 119.1 / 116.0 / 112.8; 4096 buckets -- five workgroups -- 110; two sub-steps 112-116) -> 125.4 (eight
//   workgroups with 1024 buckets, two hops; one 124.3, none 116.7)
//   low entropy 416 -> 433 / 436 / 437 (512 / 1024 / 2048 buckets, seven workgroups; one hop 419) -> 493 (eight workgroups, 1024 buckets; 512:
//   484; run mode's pool 64 / 256: 470 / 460, its rounds 1 / 3: 491 / 491)
// Forced on text they are 58-68 GB/s: the default keeps both chains.
namespace wgv_few {           // blocks of few distinct grams: long matches, the kernel waits -- eight workgroups per CU; no priorities (+0.2 %: noise)
#define LZS_WGV_NO3 1
#define LZS_WGV_HEAD2 1024
#define LZS_WGV_WAVES 8
#define LZS_WGV_PACK_BY_CHUNK 1   // (these blocks have few tokens to format)
#define LZS_WGV_LEAN 1
#define LZS_WGV_HOPS 0        // (few candidates, long matches: the quick-reject test itself is the cost)
#include "kernels/compress_wg.inc"
}
namespace wgv_lit {           // blocks that are nearly all literals: one full step per pass of the SEARCH loop with two hops in front, PACK chunk by chunk
#define LZS_WGV_NO3 1
#define LZS_WGV_HEAD2 1024
#define LZS_WGV_WAVES 8
#define LZS_WGV_SUBSTEPS 1
#define LZS_WGV_HOPS 2
#define LZS_WGV_PACK_BY_CHUNK 1
#define LZS_WGV_PRIO 1
#define LZS_WGV_LEAN 1
#include "kernels/compress_wg.inc"
}
#endif
using wgv_text::lzs_compress_blocks_wg_kernel;        // (what tools/probes/ launch by name)
using wgv_text::kWgThreads;
#include "kernels/compress_aux.inc"
#endif  // !LZS_TU_DECOMPRESS
#ifndef LZS_TU_COMPRESS
#include "kernels/decompress_blocks.inc"
#include "kernels/decompress_stream.inc"
#include "kernels/decompress_packed.inc"
#endif
#ifndef LZS_TU_DECOMPRESS
#include "kernels/compact_resume.inc"
#endif

}  // namespace

// =====================================================================================
// extern "C" shim (see lzs_hip_shim.h)
// =====================================================================================
extern "C" {
#ifndef LZS_TU_DECOMPRESS

int lzs_hip_device_count(int *count) { return (int)hipGetDeviceCount(count); }

const char *lzs_hip_strerror(int e) { return hipGetErrorString((hipError_t)e); }

int lzs_hip_chain_mode(void *stream, int *mode);

int lzs_hip_describe(char *buf, size_t cap)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return (int)e;
    int mode = -1;
    (void)lzs_hip_chain_mode(nullptr, &mode);
    snprintf(buf, cap, "hip device %d: %s (%s), %d CUs, %.0f GiB, LDS/CU %zu KiB; kernels: workgroup-per-block LZS compress "
                       "(chain build: %s), eight-streams-per-wavefront decompress (gfx950)",
             dev, p.name, p.gcnArchName, p.multiProcessorCount,
             (double)p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0),
             (size_t)p.maxSharedMemoryPerMultiProcessor / 1024,
             mode == 0 ? "ordered LDS exchange, verified on this device" : (mode == 1 ? "order-independent fallback" : "not checked"));
    return 0;
}

int lzs_hip_total_memory(size_t *bytes)
{
    size_t free_b = 0, total = 0;
    const hipError_t e = hipMemGetInfo(&free_b, &total);
    if (e == hipSuccess) *bytes = total;
    return (int)e;
}
int lzs_hip_malloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes ? bytes : 1); }
int lzs_hip_free(void *p) { return (int)hipFree(p); }
int lzs_hip_host_malloc(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault); }
int lzs_hip_host_malloc_staging(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocNonCoherent); }
int lzs_hip_host_free(void *p) { return (int)hipHostFree(p); }
void lzs_hip_clear_error(void) { (void)hipGetLastError(); }

namespace {
__global__ __launch_bounds__(256) void lzs_words_to_host_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
    __threadfence_system();                         // dst is host memory that the host reads at an event
}
}  // namespace
int lzs_hip_words_to_host(uint32_t *h_dst, const uint32_t *d_src, size_t nwords, void *stream)
{
    if (nwords == 0) return 0;
    const size_t grid = (nwords + 255) / 256;
    hipLaunchKernelGGL(lzs_words_to_host_kernel, dim3((unsigned)(grid < 64 ? grid : 64)), dim3(256), 0, (hipStream_t)stream, h_dst, d_src, nwords);
    return (int)hipGetLastError();
}
int lzs_hip_stream_create(void **s) { return (int)hipStreamCreateWithFlags((hipStream_t *)s, hipStreamNonBlocking); }
int lzs_hip_stream_destroy(void *s) { return (int)hipStreamDestroy((hipStream_t)s); }
int lzs_hip_stream_sync(void *s) { return (int)hipStreamSynchronize((hipStream_t)s); }
int lzs_hip_event_create(void **e) { return (int)hipEventCreateWithFlags((hipEvent_t *)e, hipEventDisableTiming); }
int lzs_hip_event_destroy(void *e) { return (int)hipEventDestroy((hipEvent_t)e); }
int lzs_hip_event_record(void *e, void *s) { return (int)hipEventRecord((hipEvent_t)e, (hipStream_t)s); }
int lzs_hip_event_sync(void *e) { return (int)hipEventSynchronize((hipEvent_t)e); }
int lzs_hip_event_done(void *e)
{
    const hipError_t r = hipEventQuery((hipEvent_t)e);
    return r == hipSuccess ? 1 : (r == hipErrorNotReady ? 0 : -(int)r);
}
int lzs_hip_stream_wait_event(void *s, void *e) { return (int)hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)e, 0); }
int lzs_hip_h2d(void *d, const void *s, size_t n, void *st)
{
    return n ? (int)hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, (hipStream_t)st) : 0;
}
int lzs_hip_d2h(void *d, const void *s, size_t n, void *st)
{
    return n ? (int)hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)st) : 0;
}
int lzs_hip_d2d(void *d, const void *s, size_t n, void *st)
{
    return n ? (int)hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, (hipStream_t)st) : 0;
}
int lzs_hip_memset(void *d, int v, size_t n, void *st)
{
    return n ? (int)hipMemsetAsync(d, v, n, (hipStream_t)st) : 0;
}

// 0: CHAIN by ordered LDS exchange (verified on this device), 1: the order-independent form.
// Asked once per device: lzs_lds_order_check_kernel over 16384 conflict patterns (~0.1 ms); a device
// that fails it -- or LZS_CHAIN_FALLBACK=1 -- gets the slower form, with a note on stderr.
static int g_chain_mode[64];            // 0 = not asked yet, else mode + 1
// What the classifiers of recent launches found (compress_aux.inc): four words of pinned host memory per device, h_seen[c] =
// the id of the last launch a sampled workgroup of which met a block of class c.  Made with the LDS ordering check, once per
// device; without them (the allocation failed) every launch runs all three variants.
static uint32_t *g_hint_seen[64];
static unsigned g_hint_launch;
int lzs_hip_chain_mode(void *stream, int *mode)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 0 || dev >= 64) { *mode = 1; return 0; }
    int m = __atomic_load_n(&g_chain_mode[dev], __ATOMIC_ACQUIRE);
    if (m == 0) {
        const char *force = getenv("LZS_CHAIN_FALLBACK");
        if (force && force[0] && force[0] != '0') {
            m = 2;
        } else {
            // On a stream of its own: the caller's stream is neither waited for nor
            // made to wait, whichever call is the first to ask -- normally require_device(), i.e.
            // the first entry into the library on this device, not the first "asynchronous" launch.
            (void)stream;
            hipStream_t own = nullptr;
            uint32_t *d_bad = nullptr, bad = 0;
            e = hipStreamCreateWithFlags(&own, hipStreamNonBlocking);
            if (e != hipSuccess) return (int)e;
            e = hipMalloc((void **)&d_bad, sizeof(uint32_t));
            if (e != hipSuccess) { (void)hipStreamDestroy(own); return (int)e; }
            e = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), own);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(lzs_lds_order_check_kernel, dim3(512), dim3(256), 0, own, d_bad, 16384u);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, own);
            if (e == hipSuccess) e = hipStreamSynchronize(own);
            (void)hipFree(d_bad);
            (void)hipStreamDestroy(own);
            if (e != hipSuccess) return (int)e;
            m = bad ? 2 : 1;
            if (!bad && !g_hint_seen[dev]) {
                uint32_t *h_seen = nullptr;
                if (hipHostMalloc((void **)&h_seen, 4 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess) {
                    h_seen[0] = h_seen[1] = h_seen[2] = h_seen[3] = 0;
                    uint32_t *none = nullptr;         // (two threads asking at once: one set of words stays)
                    if (!__atomic_compare_exchange_n(&g_hint_seen[dev], &none, h_seen, false, __ATOMIC_RELEASE, __ATOMIC_RELAXED)) (void)hipHostFree(h_seen);
                } else {
                    (void)hipGetLastError();
                }
            }
            if (bad)
                fprintf(stderr, "liblzs: device %d does not apply same-address LDS exchanges of one instruction in lane order "
                                "(%u lanes off in 16384 patterns): using the order-independent chain build (slower, same output)\n", dev, bad);
        }
        __atomic_store_n(&g_chain_mode[dev], m, __ATOMIC_RELEASE);
    }
    *mode = m - 1;
    return 0;
}

// ---- the ordering property once more, UNDER LOAD: lzs_hip_chain_mode() asks an idle device.  Beside the
// first compress launch of a process on a device the same check runs again on a stream of its own -- 65536 patterns
// this time, so that it overlaps the launch -- and whichever later launch finds it finished reads the verdict: a device
// that fails it gets the order-independent CHAIN from then on, with a loud note (the launches before may be
// off in their candidates' order: same format, possibly not the reference's bytes).
struct LoadCheck { int state; hipStream_t own; hipEvent_t done; uint32_t *d_bad; uint32_t *h_bad; };   // state: 0 not started, 1 in flight, 2 read
static LoadCheck g_load_check[64];
static pthread_mutex_t g_load_lock = PTHREAD_MUTEX_INITIALIZER;

static void load_check_step(int dev, bool start)
{
    if (dev < 0 || dev >= 64 || __atomic_load_n(&g_load_check[dev].state, __ATOMIC_ACQUIRE) == 2) return;
    pthread_mutex_lock(&g_load_lock);
    LoadCheck &c = g_load_check[dev];
    if (c.state == 0 && start) {
        c.state = 2;                                             // whatever fails below: do not try again
        if (hipStreamCreateWithFlags(&c.own, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&c.done, hipEventDisableTiming) == hipSuccess &&
            hipMalloc((void **)&c.d_bad, sizeof(uint32_t)) == hipSuccess &&
            hipHostMalloc((void **)&c.h_bad, sizeof(uint32_t), hipHostMallocDefault) == hipSuccess) {
            *c.h_bad = 0;
            (void)hipMemsetAsync(c.d_bad, 0, sizeof(uint32_t), c.own);
            hipLaunchKernelGGL(lzs_lds_order_check_kernel, dim3(512), dim3(256), 0, c.own, c.d_bad, 65536u);
            if (hipGetLastError() == hipSuccess &&
                hipMemcpyAsync(c.h_bad, c.d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, c.own) == hipSuccess &&
                hipEventRecord(c.done, c.own) == hipSuccess)
                c.state = 1;
        }
    } else if (c.state == 1 && hipEventQuery(c.done) == hipSuccess) {
        if (*c.h_bad) {
            fprintf(stderr, "liblzs: device %d applied same-address LDS exchanges out of lane order UNDER LOAD (%u lanes off in 65536 "
                            "patterns beside a compress launch) although it passed the check when idle: switching to the "
                            "order-independent chain build; the launches so far may differ from the reference's bytes\n", dev, *c.h_bad);
            __atomic_store_n(&g_chain_mode[dev], 2, __ATOMIC_RELEASE);
        }
        // (the four bytes, the event and the stream stay for the life of the process: releasing device memory waits for
        // the device, and this runs inside a launch that promised to be asynchronous)
        __atomic_store_n(&c.state, 2, __ATOMIC_RELEASE);
    }
    pthread_mutex_unlock(&g_load_lock);
}

// 0: never asked / finished clean; for tests: has the check beside a launch run to its end, and what did it say
int lzs_hip_load_check_state(int dev) { return dev >= 0 && dev < 64 ? __atomic_load_n(&g_load_check[dev].state, __ATOMIC_ACQUIRE) : -1; }

// LZS_VERIFY=N: every N-th compress launch of the process is run again with CHAIN in its order-independent form
// into scratch slots and compared on the device, length and bytes of every block; a difference is an error of the
// launch (and a line on stderr).  That launch waits for its result: an audit mode, not the asynchronous contract.
static int verify_every(void)
{
    static const int n = [] { const char *v = getenv("LZS_VERIFY"); const long k = v ? strtol(v, nullptr, 10) : 0; return k > 0 ? (int)k : 0; }();
    return n;
}
static unsigned g_launch_count;

static int verify_launch(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                         const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len, uint32_t nblocks, hipStream_t stream)
{
    const size_t stride = ((size_t)out_cap + 15u) & ~(size_t)15u;
    uint8_t *d_scratch = nullptr; uint32_t *d_len2 = nullptr, bad = 0;
    hipError_t e = hipMalloc((void **)&d_scratch, stride * nblocks + 16);
    if (e == hipSuccess) e = hipMalloc((void **)&d_len2, sizeof(uint32_t) * ((size_t)nblocks + 1));
    if (e == hipSuccess) e = hipMemsetAsync(d_len2 + nblocks, 0, sizeof(uint32_t), stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(wgv_safe::lzs_compress_blocks_wg_kernel, dim3(nblocks), dim3(wgv_safe::kWgThreads), 0, stream, d_scratch, stride, out_cap, d_len2,
                           (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, 0u);
        hipLaunchKernelGGL(lzs_verify_slots_kernel, dim3(nblocks), dim3(256), 0, stream, (const uint8_t *)d_out, (const uint32_t *)d_out_len,
                           (const uint8_t *)d_scratch, (const uint32_t *)d_len2, out_stride, stride, nblocks, d_len2 + nblocks);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_len2 + nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_scratch); (void)hipFree(d_len2);
    if (e != hipSuccess) return (int)e;
    if (bad) {
        fprintf(stderr, "liblzs: LZS_VERIFY: %u of %u blocks of this launch differ between the ordered-exchange chain build and the "
                        "order-independent one\n", bad, nblocks);
        return (int)hipErrorAssert;
    }
    return 0;
}

// LZS_VARIANT=text|few|lit (development, read once) gives every block that variant: 1, 2, 3; 0: the blocks' classes decide.
static int forced_variant(void)
{
    static const int forced = [] {
        const char *v = getenv("LZS_VARIANT");
        return !v ? 0 : (v[0] == 't' ? 1 : (v[0] == 'f' ? 2 : (v[0] == 'l' ? 3 : 0)));
    }();
    return forced;
}
// (for tests: what LZS_VARIANT forces in this process -- 0 none, 1 text, 2 few, 3 lit)
int lzs_hip_forced_variant(void) { return forced_variant(); }

static_assert(kClassifyMinBlocks == 64u && (kClassCode & 0xFu) == 0u, "lzs_launch_plan.h and tests/cpu_shim/plan_check.c are written for these");

// What lzs_plan_variants() decides from: the ids the last classifiers left per class, and whether the stream is being captured into
// a graph (the guess would be frozen with it: every variant is launched, so that a replay on another class of data keeps its
// variant -- ADVICE r05).  h_seen: where this launch's classifier leaves what it met, under `id`.
static lzs_plan_variants_t variant_hint(void *stream, uint32_t *&h_seen, uint32_t &id)
{
    int dev = 0, capturing = 0;
    uint32_t seen[4] = { 0, 0, 0, 0 };
    h_seen = nullptr;
    id = (uint32_t)__atomic_add_fetch(&g_hint_launch, 1u, __ATOMIC_RELAXED) | 0x80000000u;      // (never 0)
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && (h_seen = __atomic_load_n(&g_hint_seen[dev], __ATOMIC_ACQUIRE)) != nullptr) {
        for (int c = 1; c <= 3; c++) seen[c] = __atomic_load_n(&h_seen[c], __ATOMIC_RELAXED);
        hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
        if (stream && hipStreamIsCapturing((hipStream_t)stream, &status) != hipSuccess) { status = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
        capturing = status != hipStreamCaptureStatusNone;
    }
    return lzs_plan_variants(seen, h_seen != nullptr, capturing);
}

// A variant's namespace as a type, for the launchers' entry functors: its block entry, its packed entry, its workgroup.
#define LZS_VARIANT_TAG(ns) \
    struct ns##_tag { static constexpr auto blocks = ns::lzs_compress_blocks_wg_kernel; static constexpr auto packed = ns::lzs_compress_packed_wg_kernel; \
                      static constexpr unsigned threads = ns::kWgThreads; }
LZS_VARIANT_TAG(wgv_safe);
LZS_VARIANT_TAG(wgv_text);
#ifndef LZS_ONE_VARIANT
LZS_VARIANT_TAG(wgv_few);
LZS_VARIANT_TAG(wgv_lit);
#endif
#undef LZS_VARIANT_TAG

// Which variant compresses a block, for the strided and the packed call alike (lzs_plan_compress): the order-independent CHAIN for
// all of them on a device that needs it; otherwise the block's class decides, on the device (the classifier leaves a code in
// out_len[b]; every allowed variant is launched over the whole grid and a workgroup whose block is another's returns at once: ~10 us
// per empty grid of 16 384).  LZS_VARIANT=text|few|lit (development, read once) gives every block that one; small launches take the
// default alone.
//   earlier(&e)        true: the call was served by another kernel (LZS_KERNEL= of the A/B builds), e its result
//   variant(tag, serve)  launches that variant's entry over the whole grid
//   classify(v, h_seen, id)  launches the entry's classifier
// *ordered: the ordered-exchange form was launched (what LZS_VERIFY samples).
extern "C++" {
template <class Earlier, class Variant, class Classify>
static int compress_dispatch(uint32_t nblocks, void *stream, bool *ordered, const Earlier &earlier, const Variant &variant, const Classify &classify)
{
    *ordered = false;
    if (nblocks == 0) return 0;
    int chain_mode = 0;
    { const int e = lzs_hip_chain_mode(stream, &chain_mode); if (e) return e; }
    { int e = 0; if (earlier(&e)) return e; }
#ifdef LZS_ONE_VARIANT
    const lzs_plan_compress_t plan = lzs_plan_compress(chain_mode, 0, nblocks, kClassifyMinBlocks, 1);
#else
    const lzs_plan_compress_t plan = lzs_plan_compress(chain_mode, forced_variant(), nblocks, kClassifyMinBlocks, 0);
#endif
    switch (plan.run) {
    case LZS_RUN_SAFE: variant(wgv_safe_tag{}, 0u); break;
#ifndef LZS_ONE_VARIANT
    case LZS_RUN_FEW: variant(wgv_few_tag{}, 0u); break;
    case LZS_RUN_LIT: variant(wgv_lit_tag{}, 0u); break;
    case LZS_RUN_CLASSIFY: {
        uint32_t *h_seen, id;
        const lzs_plan_variants_t v = variant_hint(stream, h_seen, id);
        classify(v, h_seen, id);
        if (v.allow & 2u) variant(wgv_text_tag{}, kClassCode | 1u);
        if (v.allow & 4u) variant(wgv_few_tag{}, kClassCode | 2u);
        if (v.allow & 8u) variant(wgv_lit_tag{}, kClassCode | 3u);
        break;
    }
#endif
    default: variant(wgv_text_tag{}, 0u); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (plan.load_check) {
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess) load_check_step(dev, plan.load_check_start != 0);     // (beside a launch that fills the device)
        *ordered = true;
    }
    return 0;
}
}  // extern "C++"

#ifdef LZS_WITH_VARIANTS
// A/B builds only: LZS_KERNEL=chain (one wave per block) | scan (brute force) select the earlier kernels, wg8 | p256 the default
// kernel in its two other shapes (round 6).  True: one of them served the call.
static bool launch_earlier_kernel(int *result, void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                  const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len, uint32_t nblocks, hipStream_t stream)
{
    static const int variant = [] {
        const char *v = getenv("LZS_KERNEL");
        return !v ? 0 : (v[0] == 's' ? 2 : (v[0] == 'c' ? 1 : (v[0] == 'w' ? 3 : (v[0] == 'p' ? 4 : 0))));
    }();
    const uint32_t grid = (nblocks + kWavesPerWG - 1) / kWavesPerWG;
    if (variant == 3)
        hipLaunchKernelGGL(wgv_text8::lzs_compress_blocks_wg_kernel, dim3(nblocks), dim3(wgv_text8::kWgThreads), 0, stream, (uint8_t *)d_out,
                           out_stride, out_cap, d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, 0u);
    else if (variant == 4)
        hipLaunchKernelGGL(wgv_pool256::lzs_compress_blocks_wg_kernel, dim3(nblocks), dim3(wgv_pool256::kWgThreads), 0, stream, (uint8_t *)d_out,
                           out_stride, out_cap, d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, 0u);
    else if (variant == 2)
        hipLaunchKernelGGL(lzs_compress_blocks_scan_kernel, dim3(grid), dim3(kWavesPerWG * 64), 0, stream, (uint8_t *)d_out, out_stride, out_cap,
                           d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks);
    else if (variant == 1)
        hipLaunchKernelGGL(lzs_compress_blocks_kernel, dim3(nblocks), dim3(64), 0, stream, (uint8_t *)d_out, out_stride, out_cap,
                           d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks);
    else
        return false;
    *result = (int)hipGetLastError();
    return true;
}
#endif

int lzs_hip_launch_compress(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                            const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                            uint32_t in_len, uint32_t nblocks, void *stream)
{
    bool ordered = false;
    const int e = compress_dispatch(nblocks, stream, &ordered,
        [&](int *result) {
#ifdef LZS_WITH_VARIANTS
            return launch_earlier_kernel(result, d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len, nblocks, (hipStream_t)stream);
#else
            (void)result;
            return false;
#endif
        },
        [&](auto v, uint32_t serve) {
            hipLaunchKernelGGL(decltype(v)::blocks, dim3(nblocks), dim3(decltype(v)::threads), 0, (hipStream_t)stream, (uint8_t *)d_out, out_stride,
                               out_cap, d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, serve);
        },
        [&](const lzs_plan_variants_t &v, uint32_t *h_seen, uint32_t id) {
            hipLaunchKernelGGL(lzs_classify_blocks_kernel, dim3((nblocks + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_out_len,
                               (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, v.allow, v.catch_all, h_seen, id);
        });
    if (e || !ordered) return e;
    const int every = verify_every();
    if (every && (__atomic_add_fetch(&g_launch_count, 1u, __ATOMIC_RELAXED) % (unsigned)every) == 0u)
        return verify_launch(d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len, nblocks, (hipStream_t)stream);
    return 0;
}

// The classifier alone (tests, bench.py's class mix): d_codes[b] = 1 the default variant, 2 few distinct grams, 3 nearly all literals.
int lzs_hip_classify_blocks(uint32_t *d_codes, const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                            uint32_t nblocks, void *stream)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(lzs_classify_blocks_kernel, dim3((nblocks + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_codes,
                       (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, 0xEu, 1u, (uint32_t *)nullptr, 0u);
    return (int)hipGetLastError();
}

// Packed compression (lzs_packed.c checks the arguments): compress_dispatch() with every block's place, length and
// room read from the offset arrays by the kernels; the A/B kernels of LZS_KERNEL= have no packed entry.  NOT covered by the sampled
// self-check: LZS_VERIFY (verify_every) compares strided slots, and a packed launch neither counts towards its sample nor is run again.
int lzs_hip_launch_compress_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                   const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t nblocks, void *stream)
{
    bool ordered = false;
    return compress_dispatch(nblocks, stream, &ordered,
        [](int *) { return false; },
        [&](auto v, uint32_t serve) {
            hipLaunchKernelGGL(decltype(v)::packed, dim3(nblocks), dim3(decltype(v)::threads), 0, (hipStream_t)stream, (uint8_t *)d_out, d_out_off,
                               d_out_len, (const uint8_t *)d_in, d_in_off, d_in_len, nblocks, serve);
        },
        [&](const lzs_plan_variants_t &v, uint32_t *h_seen, uint32_t id) {
            hipLaunchKernelGGL(lzs_classify_packed_kernel, dim3((nblocks + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_out_len, d_out_off,
                               (const uint8_t *)d_in, d_in_off, d_in_len, nblocks, v.allow, v.catch_all, h_seen, id);
        });
}

int lzs_hip_launch_compressed_bound_packed(uint32_t *d_bound, const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t nblocks, void *stream)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(lzs_compressed_bound_packed_kernel, dim3((nblocks + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, d_bound, d_in_off,
                       d_in_len, nblocks);
    return (int)hipGetLastError();
}

#endif  // !LZS_TU_DECOMPRESS
#ifndef LZS_TU_COMPRESS
static_assert(kDecGroups == LZS_PLAN_DEC_GROUPS, "lzs_launch_plan.h: streams per wavefront of the grouped decoders");

static int launch_decompress(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                             const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                             uint32_t in_len, uint32_t nblocks, void *stream, uint32_t concat)
{
    if (nblocks == 0) return 0;
#ifdef LZS_WITH_VARIANTS
    // A/B builds only: LZS_DECODER=v1|v2 select the wave-per-stream decoders of round 1
    static const int older = [] { const char *v = getenv("LZS_DECODER"); return (v && v[0] == 'v') ? (v[1] == '1' ? 1 : (v[1] == '2' ? 2 : 0)) : 0; }();
    if (older) {
        const uint32_t grid = (nblocks + kWavesPerWG - 1) / kWavesPerWG;
        if (older == 1)
            hipLaunchKernelGGL(lzs_decompress_blocks_kernel, dim3(grid), dim3(kWavesPerWG * 64), 0,
                               (hipStream_t)stream, (uint8_t *)d_out, out_stride, out_cap, d_out_len,
                               (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, concat);
        else
            hipLaunchKernelGGL(lzs_decompress_blocks_v2_kernel, dim3(grid), dim3(kWavesPerWG * 64), 0,
                               (hipStream_t)stream, (uint8_t *)d_out, out_stride, out_cap, d_out_len,
                               (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, concat);
        return (int)hipGetLastError();
    }
#endif
    // The kernel bounds a wavefront's input loads by one 32-bit extent over its streams.  Streams so
    // far apart that eight of them do not fit (strides of hundreds of MB) go one to a wavefront.
    const uint32_t per_wave = lzs_plan_dec_per_wave_blocks(in_stride, d_in_len != nullptr, in_len);
    hipLaunchKernelGGL(concat ? lzs_decompress_blocks_grp_kernel<true> : lzs_decompress_blocks_grp_kernel<false>,
                       dim3((nblocks + per_wave - 1) / per_wave), dim3(64), 0,
                       (hipStream_t)stream, (uint8_t *)d_out, out_stride, out_cap, d_out_len,
                       (const uint8_t *)d_in, in_stride, d_in_len, in_len, nblocks, concat, per_wave);
    return (int)hipGetLastError();
}

int lzs_hip_launch_decompress(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                              const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                              uint32_t in_len, uint32_t nblocks, void *stream)
{
    return launch_decompress(d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len, nblocks, stream, 0);
}

int lzs_hip_launch_decompress_concat(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                     const void *d_in, size_t in_stride, const uint32_t *d_in_len,
                                     uint32_t in_len, uint32_t nblocks, void *stream)
{
    return launch_decompress(d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len, in_len, nblocks, stream, 1);
}

int lzs_hip_launch_decompress_channels(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                       const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                                       const uint32_t *d_channel, void *d_states, uint8_t *d_status, uint32_t npackets, void *stream)
{
    if (npackets == 0) return 0;
    // (eight streams to a wavefront unless their input is too far apart for one 32-bit extent: launch_decompress's rule)
    const uint32_t per_wave = lzs_plan_dec_per_wave_blocks(in_stride, d_in_len != nullptr, in_len);
    hipLaunchKernelGGL(lzs_decompress_channels_grp_kernel, dim3((npackets + per_wave - 1) / per_wave), dim3(64), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, out_stride, out_cap, d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len,
                       d_channel, (uint8_t *)d_states, d_status, npackets, per_wave);
    return (int)hipGetLastError();
}

int lzs_hip_launch_decompress_runs(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                   const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                                   const uint32_t *d_run_key, const uint32_t *d_run_at, const uint32_t *d_run_end,
                                   const uint32_t *d_skey, const uint32_t *d_sidx, uint32_t nchannels, void *d_states,
                                   uint8_t *d_status, uint32_t npackets, const uint32_t *d_rkey, const uint32_t *d_rmark, void *d_stage,
                                   void *stream)
{
    if (npackets == 0) return 0;
    // (a wavefront's runs take packets from anywhere in the input: eight runs to a wavefront if all of it is one 32-bit extent)
    const uint32_t per_wave = lzs_plan_dec_per_wave_runs(in_stride, npackets, d_in_len != nullptr, in_len);
    hipLaunchKernelGGL(lzs_decompress_runs_grp_kernel, dim3((npackets + per_wave - 1) / per_wave), dim3(64), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, out_stride, out_cap, d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len,
                       d_run_key, d_run_at, d_run_end, d_skey, d_sidx, nchannels, (uint8_t *)d_states, d_status, npackets, per_wave,
                       RunTables{d_rkey, d_rmark, (uint8_t *)d_stage});
    return (int)hipGetLastError();
}

#endif  // !LZS_TU_COMPRESS
#ifndef LZS_TU_DECOMPRESS
// A kernel that exists in the default shape and in the order-independent CHAIN form only (segments, channel packets): the form
// the device needs, over `grid` workgroups.  LZS_SAFE_OR_TEXT names the two instances of `kernel` in wgv_safe<suffix>, wgv_text<suffix>.
extern "C++" {
template <class Kernel, class... Args>
static int launch_safe_or_text(Kernel safe, unsigned safe_threads, Kernel text, unsigned text_threads, uint32_t grid, void *stream, Args... args)
{
    int chain_mode = 0;
    { const int e = lzs_hip_chain_mode(stream, &chain_mode); if (e) return e; }
    if (chain_mode != 0) hipLaunchKernelGGL(safe, dim3(grid), dim3(safe_threads), 0, (hipStream_t)stream, args...);
    else hipLaunchKernelGGL(text, dim3(grid), dim3(text_threads), 0, (hipStream_t)stream, args...);
    return (int)hipGetLastError();
}
}  // extern "C++"
#define LZS_SAFE_OR_TEXT(suffix, kernel) wgv_safe##suffix::kernel, wgv_safe##suffix::kWgThreads, wgv_text##suffix::kernel, wgv_text##suffix::kWgThreads

int lzs_hip_launch_compress_segments(void *d_slots, size_t slot_stride, const void *d_in, uint32_t n,
                                     uint32_t seg, uint32_t nseg, const uint32_t *d_entry,
                                     const uint8_t *d_dirty, uint32_t *d_exit, uint64_t *d_nbits,
                                     void *d_out, const uint64_t *d_bit_at, uint32_t lim, uint32_t *d_open,
                                     void *stream)
{
    if (nseg == 0) return 0;
    return launch_safe_or_text(LZS_SAFE_OR_TEXT(, lzs_compress_segments_kernel), nseg, stream,
                               (uint8_t *)d_slots, slot_stride, (const uint8_t *)d_in, n, seg, nseg,
                               d_entry, d_dirty, d_exit, (unsigned long long *)d_nbits,
                               (uint8_t *)d_out, (const unsigned long long *)d_bit_at, lim, d_open);
}

// The segments of the blocks of a batch (lzs_batch_compress.c).
int lzs_hip_launch_compress_segments_batch(void *d_slots, size_t slot_stride, const void *d_in, const uint64_t *d_blk_at,
                                           const uint32_t *d_blk_len, const uint32_t *d_seg_block, const uint32_t *d_seg_start,
                                           uint32_t seg, uint32_t nseg, const uint32_t *d_entry, const uint8_t *d_dirty,
                                           uint32_t *d_exit, uint64_t *d_nbits, void *d_out, size_t out_stride, uint32_t out_cap,
                                           const uint64_t *d_bit_at, void *stream)
{
    if (nseg == 0) return 0;
    const uint32_t cap4 = out_cap > 0xFFFFFFFCu ? 0xFFFFFFFCu : (out_cap + 3u) & ~3u;
    return launch_safe_or_text(LZS_SAFE_OR_TEXT(, lzs_compress_segments_batch_kernel), nseg, stream,
                               (uint8_t *)d_slots, slot_stride, (const uint8_t *)d_in, (const unsigned long long *)d_blk_at, d_blk_len,
                               d_seg_block, d_seg_start, seg, nseg, d_entry, d_dirty, d_exit, (unsigned long long *)d_nbits,
                               (uint8_t *)d_out, out_stride, cap4, (const unsigned long long *)d_bit_at);
}

// Many channels, one packet each.
int lzs_hip_launch_compress_channels(void *d_out, size_t out_stride, uint32_t out_cap, uint32_t *d_out_len,
                                     const void *d_in, size_t in_stride, const uint32_t *d_in_len, uint32_t in_len,
                                     const uint32_t *d_channel, void *d_states, uint8_t *d_status, uint32_t npackets, void *stream)
{
    if (npackets == 0) return 0;
    return launch_safe_or_text(LZS_SAFE_OR_TEXT(_ch, lzs_compress_channels_wg_kernel), npackets, stream,
                               (uint8_t *)d_out, out_stride, out_cap, d_out_len, (const uint8_t *)d_in, in_stride, d_in_len, in_len,
                               d_channel, (uint8_t *)d_states, d_status, npackets);
}

// The same from packed packets to rooms (lzs_packed.c checks the arguments).
int lzs_hip_launch_compress_channels_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                            const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                            void *d_states, uint8_t *d_status, uint32_t npackets, void *stream)
{
    if (npackets == 0) return 0;
    return launch_safe_or_text(LZS_SAFE_OR_TEXT(_ch, lzs_compress_channels_packed_wg_kernel), npackets, stream,
                               (uint8_t *)d_out, d_out_off, d_out_len, (const uint8_t *)d_in, d_in_off, d_in_len, d_channel, (uint8_t *)d_states,
                               d_status, npackets);
}
#undef LZS_SAFE_OR_TEXT

int lzs_hip_launch_extend_resume(void *d_out, uint32_t bit0, const void *d_in, uint32_t n, uint32_t c0,
                                 uint32_t off, int last, uint32_t *d_result, void *stream)
{
    hipLaunchKernelGGL(lzs_extend_resume_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, bit0, (const uint8_t *)d_in, n, c0, off, last ? 1u : 0u, d_result);
    return (int)hipGetLastError();
}

int lzs_hip_launch_stitch_segments(void *d_out, const void *d_slots, size_t slot_stride,
                                   const uint64_t *d_bit_at, const uint64_t *d_nbits, uint32_t nseg,
                                   int end_marker, void *stream)
{
    if (nseg == 0) return 0;
    hipLaunchKernelGGL(lzs_stitch_segments_kernel, dim3(nseg), dim3(256), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, (const uint8_t *)d_slots, slot_stride,
                       (const unsigned long long *)d_bit_at, (const unsigned long long *)d_nbits, nseg,
                       end_marker ? 1u : 0u);
    return (int)hipGetLastError();
}

int lzs_hip_launch_stitch_segments_batch(void *d_out, size_t out_stride, uint32_t out_cap, const void *d_slots, size_t slot_stride,
                                         const uint64_t *d_bit_at, const uint64_t *d_nbits, const uint32_t *d_seg_block,
                                         const uint32_t *d_seg_start, const uint32_t *d_blk_len, uint32_t seg, uint32_t nseg, void *stream)
{
    if (nseg == 0) return 0;
    const uint32_t capw = out_cap / 4u + (out_cap % 4u != 0u);
    hipLaunchKernelGGL(lzs_stitch_segments_batch_kernel, dim3(nseg), dim3(256), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, out_stride, capw, (const uint8_t *)d_slots, slot_stride,
                       (const unsigned long long *)d_bit_at, (const unsigned long long *)d_nbits, d_seg_block, d_seg_start, d_blk_len,
                       seg, nseg);
    return (int)hipGetLastError();
}

// `rows` rows of `width` bytes, `pitch` apart, set to `value` (the outputs of a batch cleared as far as they are written)
int lzs_hip_memset_rows(void *d, size_t pitch, int value, size_t width, size_t rows, void *stream)
{
    if (width == 0 || rows == 0) return 0;
    if (rows == 1 || width == pitch) return (int)hipMemsetAsync(d, value, (rows - 1) * pitch + width, (hipStream_t)stream);
    return (int)hipMemset2DAsync(d, pitch, value, width, rows, (hipStream_t)stream);
}

#endif  // !LZS_TU_DECOMPRESS
#ifndef LZS_TU_COMPRESS
int lzs_hip_launch_scan_stream(const void *d_in, uint32_t n, uint32_t nseg, const uint32_t *d_entry,
                               const uint8_t *d_dirty, uint32_t *d_exit, uint32_t *d_count,
                               uint8_t *d_all_ones, uint32_t *d_marks, int compare, uint32_t seg, int concat,
                               const uint32_t *d_seg_base, const uint32_t *d_seg_end, uint32_t in_extent, void *stream)
{
    if (nseg == 0) return 0;
    static const int scan_env = [] { const char *v = getenv("LZS_SCAN"); return !v ? 0 : (v[0] == 'w' ? 1 : (v[0] == 'g' ? 2 : 0)); }();   // LZS_SCAN=wave|g8: A/B
    const lzs_plan_scan_t plan = lzs_plan_scan(d_all_ones != nullptr, compare, d_marks != nullptr, concat, scan_env);
    if (plan.lanes == 0) {
        hipLaunchKernelGGL(lzs_scan_stream_kernel, dim3((nseg + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                           (const uint8_t *)d_in, n, nseg, d_entry, d_dirty, d_exit, d_count, d_all_ones,
                           d_marks, compare ? 1u : 0u, seg, concat ? 1u : 0u, d_seg_base, d_seg_end);
        return (int)hipGetLastError();
    }
    // a lane per segment; the first round with the all-0xFF flags, the later ones against its marks
    if (plan.all_ones_first)
        hipLaunchKernelGGL(lzs_all_ones_kernel, dim3((nseg + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                           (const uint8_t *)d_in, n, nseg, d_all_ones, seg, d_seg_base, d_seg_end);
    if (plan.clear_marks)            // no marks yet (one store per lane and mark otherwise: 128 scattered words a segment)
        (void)hipMemsetAsync(d_marks, 0xFF, (size_t)nseg * kScanMarkWords * sizeof(uint32_t), (hipStream_t)stream);
#define LZS_SCAN_KERNEL(L) (plan.concat ? lzs_scan_stream_g8_kernel<L, true> : lzs_scan_stream_g8_kernel<L, false>)
    hipLaunchKernelGGL(plan.lanes == 8 ? LZS_SCAN_KERNEL(8) : LZS_SCAN_KERNEL(1), dim3(plan.lanes == 8 ? (nseg + 7) / 8 : (nseg + 63) / 64), dim3(64), 0,
                       (hipStream_t)stream, (const uint8_t *)d_in, n, nseg, d_entry, d_dirty, d_exit, d_count, d_marks, compare ? 1u : 0u, seg,
                       concat ? 1u : 0u, d_seg_base, d_seg_end, in_extent);
#undef LZS_SCAN_KERNEL
    return (int)hipGetLastError();
}

int lzs_hip_launch_decode_stream(void *d_out, uint32_t cap, uint32_t *d_origin, uint32_t *d_tainted,
                                 const void *d_in, uint32_t n, uint32_t in_extent, uint32_t nseg, const uint32_t *d_entry,
                                 const uint32_t *d_out_start, uint32_t seg, int concat,
                                 const uint32_t *d_seg_base, const uint32_t *d_seg_end,
                                 const uint32_t *d_out_floor, const uint32_t *d_out_limit, void *stream)
{
    if (nseg == 0) return 0;
    static const int old_decode = [] { const char *v = getenv("LZS_SEG_DECODE"); return v && v[0] == 'w'; }();   // LZS_SEG_DECODE=wave: A/B
    static const int one_token = [] { return getenv("LZS_DEC_ONE_TOKEN") != nullptr; }();
    const int form = lzs_plan_decode_stream(n, cap, old_decode, one_token);
    if (form == LZS_DECODE_WAVE) {
        hipLaunchKernelGGL(lzs_decode_stream_kernel, dim3((nseg + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                           (uint8_t *)d_out, cap, d_origin, d_tainted, (const uint8_t *)d_in, n, nseg, d_entry, d_out_start, seg, concat ? 1u : 0u,
                           d_seg_base, d_seg_end, d_out_floor, d_out_limit);
        return (int)hipGetLastError();
    }
    // eight segments per wavefront: a second token per trip, or the 96-bit buffer (lzs_decompress_blocks_grp has the numbers)
#define LZS_G8_KERNEL(T, W) (concat ? lzs_decode_stream_g8_kernel<T, W, true> : lzs_decode_stream_g8_kernel<T, W, false>)
    hipLaunchKernelGGL(form == LZS_DECODE_G8_TWO ? LZS_G8_KERNEL(true, false) : (form == LZS_DECODE_G8_WIDE ? LZS_G8_KERNEL(false, true) : LZS_G8_KERNEL(false, false)),
                       dim3((nseg + 7) / 8), dim3(64), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, cap, d_origin, d_tainted, (const uint8_t *)d_in, n, in_extent, nseg, d_entry, d_out_start, seg, concat ? 1u : 0u,
                       d_seg_base, d_seg_end, d_out_floor, d_out_limit);
#undef LZS_G8_KERNEL
    return (int)hipGetLastError();
}

int lzs_hip_launch_resolve_blocks(void *d_out, uint32_t *d_origin, size_t out_stride, const uint32_t *d_len,
                                  uint32_t nblocks, void *stream)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(lzs_resolve_blocks_kernel, dim3(nblocks), dim3(1024), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, d_origin, out_stride, d_len);
    return (int)hipGetLastError();
}

int lzs_hip_launch_resolve_stream(void *d_out, uint32_t *d_origin, uint32_t total, uint32_t round,
                                  uint32_t *d_left, int last, void *stream)
{
    if (total == 0) return 0;
    hipLaunchKernelGGL(lzs_resolve_stream_kernel, dim3(lzs_plan_resolve_grid(total)), dim3(256), 0, (hipStream_t)stream,     // four bytes a thread
                       (uint8_t *)d_out, d_origin, total, round, d_left, last ? 1u : 0u);
    return (int)hipGetLastError();
}

int lzs_hip_launch_resolve_tails(void *d_out, uint32_t *d_origin, uint32_t total, const uint32_t *d_seg_start,
                                 uint32_t nseg, uint32_t stride, uint32_t round, uint32_t *d_left, void *stream)
{
    if (total == 0 || nseg == 0 || stride == 0) return 0;
    hipLaunchKernelGGL(lzs_resolve_tails_kernel, dim3((nseg + stride - 1u) / stride), dim3(256), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, d_origin, total, d_seg_start, stride, round, d_left);
    return (int)hipGetLastError();
}

int lzs_hip_launch_resolve_chunks(void *d_out, uint32_t *d_origin, uint32_t total, const uint32_t *d_seg_start,
                                  uint32_t nseg, uint32_t per_chunk, uint32_t round, void *stream)
{
    if (total == 0 || nseg < 2 || per_chunk == 0) return 0;
    hipLaunchKernelGGL(lzs_resolve_chunks_kernel, dim3((nseg + per_chunk - 1u) / per_chunk), dim3(256), 0, (hipStream_t)stream,
                       (uint8_t *)d_out, d_origin, total, d_seg_start, nseg, per_chunk, round);
    return (int)hipGetLastError();
}

unsigned lzs_hip_dec_segment_bytes(void) { return kDecSegMax; }

// The packed calls (lzs_packed.c checks the arguments): offsets and lengths are on the device, so there is nothing to decide here.
int lzs_hip_launch_decompress_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                     const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t nblocks, void *stream)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(lzs_decompress_packed_grp_kernel<false>, dim3((nblocks + kDecGroups - 1) / kDecGroups), dim3(64), 0,
                       (hipStream_t)stream, (uint8_t *)d_out, d_out_off, d_out_len, (const uint8_t *)d_in, d_in_off, d_in_len,
                       (const uint32_t *)nullptr, (uint8_t *)nullptr, (uint8_t *)nullptr, nblocks);
    return (int)hipGetLastError();
}

int lzs_hip_launch_decompress_channels_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                              const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                              void *d_states, uint8_t *d_status, uint32_t npackets, void *stream)
{
    if (npackets == 0) return 0;
    hipLaunchKernelGGL(lzs_decompress_packed_grp_kernel<true>, dim3((npackets + kDecGroups - 1) / kDecGroups), dim3(64), 0,
                       (hipStream_t)stream, (uint8_t *)d_out, d_out_off, d_out_len, (const uint8_t *)d_in, d_in_off, d_in_len,
                       d_channel, (uint8_t *)d_states, d_status, npackets);
    return (int)hipGetLastError();
}

// The runs of a packed burst (lzs_channels_burst.hip): eight to a wavefront always -- the extents are the kernel's to find.
int lzs_hip_launch_decompress_runs_packed(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                          const uint64_t *d_in_off, const uint32_t *d_in_len, const uint64_t *d_room_ends,
                                          const uint32_t *d_run_key, const uint32_t *d_run_at, const uint32_t *d_run_end,
                                          const uint32_t *d_skey, const uint32_t *d_sidx, uint32_t nchannels, void *d_states,
                                          uint8_t *d_status, uint32_t npackets, const uint32_t *d_rkey, const uint32_t *d_rmark,
                                          void *d_stage, void *stream)
{
    if (npackets == 0) return 0;
    hipLaunchKernelGGL(lzs_decompress_runs_packed_grp_kernel, dim3((npackets + kDecGroups - 1) / kDecGroups), dim3(64), 0,
                       (hipStream_t)stream, (uint8_t *)d_out, d_out_off, d_out_len, (const uint8_t *)d_in, d_in_off, d_in_len,
                       d_room_ends, d_run_key, d_run_at, d_run_end, d_skey, d_sidx, nchannels, (uint8_t *)d_states, d_status, npackets,
                       RunTables{d_rkey, d_rmark, (uint8_t *)d_stage});
    return (int)hipGetLastError();
}

int lzs_hip_launch_scan_sizes(uint64_t *d_offsets, const uint32_t *d_size, uint32_t align, uint32_t nblocks, void *stream)
{
    hipLaunchKernelGGL(lzs_scan_sizes_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_offsets, d_size, align - 1u, nblocks);
    return (int)hipGetLastError();
}

#endif  // !LZS_TU_COMPRESS
#ifndef LZS_TU_DECOMPRESS
// The scan of the lengths, then the gather: from slots slot_stride apart, or (d_src_off) from slot b at d_src + d_src_off[b].
static int launch_compact(void *d_dense, uint64_t *d_offsets, const void *d_src, size_t slot_stride, const uint64_t *d_src_off,
                          const uint32_t *d_len, uint32_t nblocks, void *stream)
{
    hipLaunchKernelGGL(lzs_scan_lengths_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_offsets, d_len, nblocks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nblocks == 0) return (int)e;
    if (d_src_off)
        hipLaunchKernelGGL(lzs_gather_packed_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (uint8_t *)d_dense, d_offsets,
                           (const uint8_t *)d_src, d_src_off, d_len, nblocks);
    else
        hipLaunchKernelGGL(lzs_gather_slots_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (uint8_t *)d_dense, d_offsets,
                           (const uint8_t *)d_src, slot_stride, d_len, nblocks);
    return (int)hipGetLastError();
}

int lzs_hip_launch_compact(void *d_dense, uint64_t *d_offsets, const void *d_slots,
                           size_t slot_stride, const uint32_t *d_len, uint32_t nblocks, void *stream)
{
    return launch_compact(d_dense, d_offsets, d_slots, slot_stride, nullptr, d_len, nblocks, stream);
}

int lzs_hip_launch_compact_packed(void *d_dense, uint64_t *d_offsets, const void *d_src, const uint64_t *d_src_off,
                                  const uint32_t *d_len, uint32_t nblocks, void *stream)
{
    return launch_compact(d_dense, d_offsets, d_src, 0, d_src_off, d_len, nblocks, stream);
}

int lzs_hip_launch_decode_resume(lzs_dec_resume_t *d_state, const void *d_in, uint32_t n,
                                 void *d_out, uint32_t cap, void *stream)
{
    hipLaunchKernelGGL(lzs_decode_resume_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       d_state, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap);
    return (int)hipGetLastError();
}

#endif  // !LZS_TU_DECOMPRESS
}  // extern "C"
