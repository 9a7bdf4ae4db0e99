// lzs_decoded_size.hip -- how long a batch of LZS streams decodes to, and with which status, without decoding them
// (include/lzs/lzs_batch.h, lzs_decompressed_size_batch_device and lzs_decompressed_size_packed_device).
//
// A stream's decoded length and final status depend on its tokens and on the capacity alone, never on the bytes a copy moves
// (lzs_burst_parse_kernel writes both in final form before any history is known).  So the query is the token
// walk of that kernel without its window, its origins and its output: one LANE a stream, a 64-bit bit buffer and a byte
// counter per lane, nothing shared between lanes, no LDS.  The rules are those of lzs_decompress_channels_grp_kernel as
// lzs_burst_parse_kernel states them: an end marker needs no room and counts unless a copy was cut at the limit before it --
// also behind the closing length nibble 0 of a copy that filled the output --, a token short of its bits or of any room stops
// the stream, a long offset of 0 has no length field and copies nothing.
//
// Input: a lane reads aligned dwords of its own stream and nothing else -- from the dword that holds the stream's first byte to
// the one that holds its last, four at a time (one 16-byte load at a dword-aligned address) while four of them are left, two
// such loads ahead of the one in use: 32 to 48 bytes, two dozen tokens and more, which is what hides a miss (the lanes of a
// wavefront stream from 64 different places and meet their misses at different times: every one of them stops the wavefront).
// What the first dword holds in front of the stream and the last behind it is masked off before it reaches the bit buffer.
#include <hip/hip_runtime.h>

#include "lzs_hip_shim.h"

namespace {

// four consecutive dwords at a dword-aligned address
struct __attribute__((packed, aligned(4))) SizeQuad { uint32_t x, y, z, w; };

// dwords [4 i, 4 i + 4) of the `nwords` a stream spans from `wp`; what lies behind the stream's last dword is not read (0)
__device__ __forceinline__ SizeQuad size_quad(const uint32_t *wp, uint32_t i, uint32_t nwords)
{
    SizeQuad q = {0u, 0u, 0u, 0u};
    const uint32_t d = 4u * i;
    if (d + 4u <= nwords) {
        q = *reinterpret_cast<const SizeQuad *>(wp + d);
    } else if (d < nwords) {
        q.x = wp[d];
        if (d + 1u < nwords) q.y = wp[d + 1u];
        if (d + 2u < nwords) q.z = wp[d + 2u];
    }
    return q;
}

// One wavefront per workgroup, one stream a lane (fewer streams a wavefront were measured: DESIGN.md 3.13).
__global__ __launch_bounds__(64) void lzs_decoded_size_kernel(uint32_t *__restrict__ size, uint8_t *__restrict__ status,
                                                              const uint8_t *__restrict__ in, size_t in_stride,
                                                              const uint32_t *__restrict__ in_len, uint32_t in_len_uniform,
                                                              uint32_t limit, uint32_t nblocks)
{
    const uint64_t at = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (at >= nblocks) return;
    const uint32_t b = (uint32_t)at;
    const uint32_t n = in_len ? in_len[b] : in_len_uniform;
    const uint8_t *const src = in + (size_t)b * in_stride;
#include "kernels/size_walk.inc"
}

// The same for packed streams (lzs_decompressed_size_packed_device): stream b starts at in + in_off[b] and is
// in_len[b] bytes long, or in_off[b + 1] - in_off[b] without lengths.  An entry that is not a block -- offsets that decrease, a
// length above LZS_BLOCK_MAX (3 GiB) -- has size 0 and status ERROR, and nothing of it is read.
__global__ __launch_bounds__(64) void lzs_decoded_size_packed_kernel(uint32_t *__restrict__ size, uint8_t *__restrict__ status,
                                                                     const uint8_t *__restrict__ in,
                                                                     const uint64_t *__restrict__ in_off,
                                                                     const uint32_t *__restrict__ in_len, uint32_t limit,
                                                                     uint32_t nblocks)
{
    const uint64_t at = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (at >= nblocks) return;
    const uint32_t b = (uint32_t)at;
    const uint64_t from = in_off[b];
    uint64_t n64 = 0;
    bool block = true;
    if (in_len) {
        n64 = in_len[b];
    } else {
        const uint64_t next = in_off[b + 1u];
        block = next >= from;
        n64 = next - from;
    }
    if (!block || n64 > (3ull << 30)) {
        size[b] = 0;
        if (status) status[b] = 0x10u;
        return;
    }
    const uint8_t *const src = in + from;
    const uint32_t n = (uint32_t)n64;
#include "kernels/size_walk.inc"
}

}  // namespace

extern "C" int lzs_hip_launch_decoded_size(uint32_t *d_size, uint8_t *d_status, const void *d_in, size_t in_stride,
                                           const uint32_t *d_in_len, uint32_t in_len, uint32_t limit, uint32_t nblocks,
                                           void *stream)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(lzs_decoded_size_kernel, dim3((nblocks + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, d_size, d_status,
                       (const uint8_t *)d_in, in_stride, d_in_len, in_len, limit, nblocks);
    return (int)hipGetLastError();
}

extern "C" int lzs_hip_launch_decoded_size_packed(uint32_t *d_size, uint8_t *d_status, const void *d_in, const uint64_t *d_in_off,
                                                  const uint32_t *d_in_len, uint32_t limit, uint32_t nblocks, void *stream)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(lzs_decoded_size_packed_kernel, dim3((nblocks + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, d_size,
                       d_status, (const uint8_t *)d_in, d_in_off, d_in_len, limit, nblocks);
    return (int)hipGetLastError();
}
