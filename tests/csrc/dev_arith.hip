// Device twin of host_arith.cpp: the case bodies of arith_cases.hpp compiled by the product's hipcc flags into one small
// kernel per family.  Lane i runs case i of the input array and writes record i of the output array, 64 lanes per block,
// cases in the order tests/arith_vectors.py produces them (edge values beside random ones in the same wave, so divergent
// paths run divergently).  d_case_<family> copies in, launches, copies out and frees; it returns 0 or the first failing
// HIP code (-1: the byte counts do not match n records).  Test code only.
#include <hip/hip_runtime.h>
#include "arith_cases.hpp"

namespace {

constexpr int LANES = 64;

// the first failure wins; later steps are skipped, the buffers are still released
template <class In, class Out, class Launch>
int run_family(const void* in, size_t in_bytes, void* out, size_t out_bytes, int n, Launch launch) {
  if (n < 0 || in_bytes != (size_t)n * sizeof(In) || out_bytes != (size_t)n * sizeof(Out)) return -1;
  if (n == 0) return 0;
  In* din = nullptr;
  Out* dout = nullptr;
  hipError_t rc = hipMalloc((void**)&din, in_bytes);
  if (rc == hipSuccess) rc = hipMalloc((void**)&dout, out_bytes);
  if (rc == hipSuccess) rc = hipMemset(dout, 0xA5, out_bytes);   // a record no lane wrote cannot look like a result
  if (rc == hipSuccess) rc = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice);
  if (rc == hipSuccess) {
    launch(din, dout, n);
    rc = hipGetLastError();
  }
  if (rc == hipSuccess) rc = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost);   // synchronises with the kernel
  const hipError_t f_in = din ? hipFree(din) : hipSuccess;
  const hipError_t f_out = dout ? hipFree(dout) : hipSuccess;
  if (rc == hipSuccess) rc = f_in;
  if (rc == hipSuccess) rc = f_out;
  return (int)rc;
}

}  // namespace

#define DEV_FAMILY(name, In, Out)                                                                              \
  __global__ void __launch_bounds__(LANES) k_##name(const arith::In* in, arith::Out* out, int n) {             \
    const int i = (int)(blockIdx.x * LANES + threadIdx.x);                                                     \
    if (i < n) arith::case_##name(in[i], out[i]);                                                              \
  }                                                                                                            \
  extern "C" int d_case_##name(const void* in, size_t in_bytes, void* out, size_t out_bytes, int n) {          \
    return run_family<arith::In, arith::Out>(in, in_bytes, out, out_bytes, n,                                  \
                                             [](const arith::In* a, arith::Out* b, int m) {                    \
                                               hipLaunchKernelGGL(k_##name, dim3((m + LANES - 1) / LANES), dim3(LANES), 0, 0, a, b, m); \
                                             });                                                               \
  }                                                                                                            \
  extern "C" int d_record_size_##name(int which) { return (int)(which ? sizeof(arith::Out) : sizeof(arith::In)); }
#ifndef ARITH_GROUP
#define ARITH_GROUP ARITH_FAMILIES
#endif
ARITH_GROUP(DEV_FAMILY)
