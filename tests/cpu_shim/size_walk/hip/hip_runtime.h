/* tests/cpu_shim/size_walk/hip/hip_runtime.h -- just enough of the HIP runtime's names for csrc/lzs_decoded_size.hip to compile
 * as host C++ (tests/test_decoded_size_host.py): a "launch" runs the kernel function once per lane of every workgroup, in
 * order, on the calling thread.  The kernel shares nothing between lanes, so this is the whole of its behaviour. */
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 threadIdx(0, 0, 0), blockIdx(0, 0, 0);
static inline int __clz(int v) { return v == 0 ? 32 : __builtin_clz((unsigned)v); }
typedef int hipError_t;
typedef void *hipStream_t;
enum { hipSuccess = 0 };
static inline hipError_t hipGetLastError() { return 0; }
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    do { for (unsigned bx_ = 0; bx_ < (grid).x; bx_++) for (unsigned tx_ = 0; tx_ < (block).x; tx_++) { \
        blockIdx.x = bx_; threadIdx.x = tx_; kernel(__VA_ARGS__); } } while (0)
