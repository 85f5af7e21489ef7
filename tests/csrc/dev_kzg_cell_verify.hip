// extern "C" doors to the launchers of plonk_amd/csrc/kzg_cell_verify.hip (kzg_cell_verify.hpp) — the twist, the column sums,
// the weights and the per-item sums — for tests/test_gpu_kzg_cell_verify.py.  No kernels here: the code that runs is
// libplonk_hip.so's own.  Every door takes the plonk_ctx* the Python binding holds (Context.handle), device pointers and plain
// host arguments, queues on the context's stream, waits for that stream and returns the product's code (PLONK_ERR_*,
// negative) or, when the product was content, the HIP error of the wait (positive).  dkv_decode fills a point table through
// the verifier's own decoder.  Test code only.
#include <string.h>

#include <vector>

#include "kzg_cell_verify.hpp"

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

int dkv_key_copy(plonk_ctx* h, uint64_t count, void* out) {
  DOOR(h);
  return finish(c, kzv_key_copy(&c, count, (G1Affine*)out));
}

// weights may be NULL
int dkv_twist(plonk_ctx* h, const void* values, const void* cell_index, const void* weights, uint64_t count, uint32_t log_cell,
              const void* winv, const void* itw, void* out, void* flags) {
  DOOR(h);
  return finish(c, kzv_twist(&c, (const Fr*)values, (const uint32_t*)cell_index, (const Fr*)weights, count, log_cell, (const Fr*)winv,
                             (const Fr*)itw, (Fr*)out, (uint32_t*)flags));
}

int dkv_colsum(plonk_ctx* h, const void* rows, uint64_t count, uint32_t log_cell, void* part0, void* part1, void* sc, void* ids) {
  DOOR(h);
  return finish(c, kzv_colsum(&c, (const Fr*)rows, count, log_cell, (Fr*)part0, (Fr*)part1, (uint32_t*)sc, (uint32_t*)ids));
}

int dkv_weights(plonk_ctx* h, const void* pw, const void* cell_index, const void* xk, const void* perm, const void* off, uint64_t K,
                uint64_t M, uint32_t log_cell, void* sc, void* ids) {
  DOOR(h);
  return finish(c, kzv_weights(&c, (const Fr*)pw, (const uint32_t*)cell_index, (const Fr*)xk, (const uint32_t*)perm,
                               (const uint32_t*)off, K, M, log_cell, (uint32_t*)sc, (uint32_t*)ids));
}

// n compressed points (host) decoded into pts[first ..] / kind[first ..]; comp_dev: 48 n bytes of device scratch
int dkv_decode(plonk_ctx* h, const uint8_t* comp_host, uint32_t n, void* comp_dev, void* pts, void* kind, uint64_t first) {
  DOOR(h);
  std::vector<int32_t> st;
  return finish(c, decode_points(&c, comp_host, n, (uint8_t*)comp_dev, (G1Affine*)pts + first, (int32_t*)kind + first, &st));
}

int dkv_cell_sums(plonk_ctx* h, const void* coeffs, const void* commitment_index, const void* cell_index, const void* xk,
                  const void* flags, const void* pts, const void* kind, uint64_t K, uint64_t M, uint32_t log_cell, void* pairs,
                  void* pre) {
  DOOR(h);
  return finish(c, kzv_cell_sums(&c, (const Fr*)coeffs, (const uint32_t*)commitment_index, (const uint32_t*)cell_index, (const Fr*)xk,
                                 (const uint32_t*)flags, (const G1Affine*)pts, (const int32_t*)kind, K, M, log_cell, (G1*)pairs,
                                 (int32_t*)pre));
}

}  // extern "C"
