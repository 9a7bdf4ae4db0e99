// tests/cpu_shim/size_stream/kernels_host.cc -- lzs_hip_launch_size_finish on the CPU: csrc/lzs_size_stream.hip, and with it
// csrc/kernels/size_finish.inc, compiled as host C++ against the stub of the HIP names in tests/cpu_shim/size_walk/hip (a
// "launch" runs the kernel function once per lane, in order; the kernel shares nothing between lanes, so that is the whole of
// its behaviour).  The route by lanes needs lzs_hip_launch_decoded_size, which tests/cpu_shim/lzs_cpu_shim.c does not have:
// csrc/lzs_decoded_size.hip the same way.  Test infrastructure only (tests/test_size_stream_host.py).
#include "lzs_size_stream.hip"
#include "lzs_decoded_size.hip"
