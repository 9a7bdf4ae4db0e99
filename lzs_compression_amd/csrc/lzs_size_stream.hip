// lzs_size_stream.hip -- the finishing walk of the size query for long streams (include/lzs/lzs_batch.h,
// lzs_decompressed_size_stream_device and its siblings; lzs_size_stream.c has the route).
//
// SCAN (kernels/decompress_stream.inc) has walked every segment of the stream, agreed on the decoder's state at every border
// and counted the bytes every segment produces; the host has summed them.  What is left is the status byte and the place where
// the room runs out, and both depend on a few tokens only: those around that place, or around the stream's end.  So one lane
// a stream walks from the start of ONE segment -- the one in which the room runs out, or the last one the stream reaches --
// in the state SCAN settled for it, by the rules of lzs_decoded_size_kernel (lzs_decoded_size.hip): the same trips, so the
// same answer as that kernel's walk from bit 0.  Nothing is shared between lanes; no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "lzs_hip_shim.h"

namespace {

// four consecutive dwords at a dword-aligned address
struct __attribute__((packed, aligned(4))) FinishQuad { uint32_t x, y, z, w; };

// dwords [4 i, 4 i + 4) of the `nwords` the walk spans from `wp`; what lies behind the stream's last dword is not read (0)
__device__ __forceinline__ FinishQuad finish_quad(const uint32_t *wp, uint32_t i, uint32_t nwords)
{
    FinishQuad q = {0u, 0u, 0u, 0u};
    const uint32_t d = 4u * i;
    if (d + 4u <= nwords) {
        q = *reinterpret_cast<const FinishQuad *>(wp + d);
    } else if (d < nwords) {
        q.x = wp[d];
        if (d + 1u < nwords) q.y = wp[d + 1u];
        if (d + 2u < nwords) q.z = wp[d + 2u];
    }
    return q;
}

// One wavefront per workgroup, one stream a lane, as lzs_decoded_size_kernel.
__global__ __launch_bounds__(64) void lzs_size_finish_kernel(uint32_t *__restrict__ counted, uint8_t *__restrict__ status,
                                                             const uint8_t *__restrict__ in, const uint32_t *__restrict__ from_each,
                                                             const uint32_t *__restrict__ end_each,
                                                             const uint32_t *__restrict__ entry_each,
                                                             const uint32_t *__restrict__ room_each, uint32_t nstreams)
{
    const uint64_t at = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (at >= nstreams) return;
    const uint32_t b = (uint32_t)at;
    const uint32_t from = from_each[b], end = end_each[b], entry = entry_each[b], limit = room_each[b];
#include "kernels/size_finish.inc"
}

}  // namespace

extern "C" int lzs_hip_launch_size_finish(uint32_t *d_counted, uint8_t *d_status, const void *d_in, const uint32_t *d_from,
                                          const uint32_t *d_end, const uint32_t *d_entry, const uint32_t *d_room, uint32_t nstreams,
                                          void *stream)
{
    if (nstreams == 0) return 0;
    hipLaunchKernelGGL(lzs_size_finish_kernel, dim3((nstreams + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, d_counted, d_status,
                       (const uint8_t *)d_in, d_from, d_end, d_entry, d_room, nstreams);
    return (int)hipGetLastError();
}
