// extern "C" doors to the launchers of plonk_amd/csrc/kzg_domain.hip (kzg_domain.hpp) — the batched group transform, the
// pointwise kernel, the extraction and the finishing kernel — for tests/test_gpu_group_fft.py.  No kernels here: the code that
// runs is libplonk_hip.so's own.  Every door takes the plonk_ctx* the Python binding holds (Context.handle), device pointers
// and plain host arguments, queues on the context's stream, waits for that stream and returns the product's code (PLONK_ERR_*,
// negative) or, when the product was content, the HIP error of the wait (positive).  Test code only.
#include <string.h>

#include "kzg_domain.hpp"

using namespace plonk;

namespace {

int finish(Ctx& c, int rc) {
  const hipError_t e = hipStreamSynchronize(c.stream);
  if (rc) return rc;
  return (int)e;
}

}  // namespace

#define DOOR(H) \
  Ctx& c = (H)->c; \
  std::lock_guard<std::mutex> lk(c.mu)

extern "C" {

// the twiddle table of a size-2^tw_log transform (2^(tw_log - 1) entries of 32 bytes); dkd_free releases it
int dkd_twiddles(plonk_ctx* h, uint32_t tw_log, void** out) {
  DOOR(h);
  if (tw_log < 1 || tw_log > 21) return PLONK_ERR_ARG;
  GlvScalar* t = nullptr;
  const int rc = kzd_twiddles_create(&c, tw_log, &t);
  *out = t;
  return finish(c, rc);
}

int dkd_free(plonk_ctx* h, void* p) {
  DOOR(h);
  const int rc = finish(c, PLONK_OK);
  (void)hipFree(p);
  return rc;
}

// forward (inverse = 0): natural order in, bit-reversed out; inverse: bit-reversed in, natural out, without the 1 / size.
// counts (may be null): [0] += stage launches, [1] += scalar multiplications issued
int dkd_transform(plonk_ctx* h, void* slots, uint64_t stride, uint32_t size_log, uint32_t batch, int inverse, const void* tw,
                  uint32_t tw_log, uint64_t* counts) {
  DOOR(h);
  return finish(c, kzd_transform(&c, slots, stride, size_log, batch, inverse != 0, (const GlvScalar*)tw, tw_log,
                                 counts ? counts : nullptr, counts ? counts + 1 : nullptr));
}

// out[b][p] = [G[b][rev(p)] * scale] A[p]; scale: 4 Montgomery limbs
int dkd_pointwise(plonk_ctx* h, const void* A, const void* G, uint64_t g_stride, void* out_slots, uint64_t stride,
                  uint32_t size_log, uint32_t batch, const uint64_t scale[4]) {
  DOOR(h);
  Fr s;
  memcpy(s.l, scale, 32);
  return finish(c, kzd_pointwise(&c, A, (const Fr*)G, g_stride, out_slots, stride, size_log, batch, s));
}

int dkd_extract(plonk_ctx* h, void* slots, uint64_t stride, uint32_t log_n, uint32_t batch) {
  DOOR(h);
  return finish(c, kzd_extract(&c, slots, stride, log_n, batch));
}

int dkd_finish(plonk_ctx* h, const void* slots, uint64_t stride, uint64_t offset, uint32_t log_n, uint32_t batch, int bitrev,
               void* out48) {
  DOOR(h);
  return finish(c, kzd_finish(&c, slots, stride, offset, log_n, batch, bitrev != 0, (uint8_t*)out48));
}

// slots[i] = the affine point xy96[i] (device memory; 96 zero bytes = the identity)
int dkd_load_raw(plonk_ctx* h, const void* xy96, uint64_t count, void* slots) {
  DOOR(h);
  return finish(c, kzd_load_raw(&c, (const G1Affine*)xy96, count, slots));
}

}  // extern "C"
