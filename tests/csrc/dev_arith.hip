// Device twin of host_arith.cpp: the case bodies of arith_cases.hpp compiled by the product's hipcc flags into one small
// kernel per family.  Lane i runs case i of the input array and writes record i of the output array, 64 lanes per block,
// cases in the order tests/arith_vectors.py produces them (edge values beside random ones in the same wave, so divergent
// paths run divergently).  d_case_<family> copies in, launches, copies out and frees; it returns 0 or the first failing
// HIP code (-1: the byte counts do not match n records).  Test code only.
#include <hip/hip_runtime.h>
#include <cstring>
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

#ifdef ARITH_HAS_PAIRING
// The shared buffer of the families that read PairingTables28 (their kernels are in this object, and so is the pointer
// they read it through): blob = the compressed x_h || h, prepared and converted on the host by the product's
// pairing_tables_fill, uploaded once and kept for the life of the process.  0, a HIP code, or a negative code for a bad blob.
extern "C" int d_shared_tables(const void* blob, size_t bytes) {
  using namespace plonk;
  static PairingTables28 T;
  static PairingTables28* dT = nullptr;
  static uint8_t have[192];
  if (bytes != sizeof have) return -1;
  if (dT && memcmp(have, blob, sizeof have) == 0) return 0;
  const uint8_t* b = (const uint8_t*)blob;
  if (!g2_compressed_valid(b) || !g2_compressed_valid(b + 96)) return -3;
  if (!pairing_tables_fill(g2_prepare(g2_decode_valid(b)), g2_prepare(g2_decode_valid(b + 96)), &T)) return -4;
  PairingTables28* fresh = nullptr;
  hipError_t rc = hipMalloc((void**)&fresh, sizeof T);
  if (rc == hipSuccess) rc = hipMemcpy(fresh, &T, sizeof T, hipMemcpyHostToDevice);
  const PairingTables28* ptr = fresh;
  if (rc == hipSuccess) rc = hipMemcpyToSymbol(HIP_SYMBOL(arith::d_pairing_tables), &ptr, sizeof ptr);
  if (rc != hipSuccess) {
    if (fresh) (void)hipFree(fresh);
    return (int)rc;
  }
  if (dT) (void)hipFree(dT);
  dT = fresh;
  memcpy(have, blob, sizeof have);
  return 0;
}
#endif
