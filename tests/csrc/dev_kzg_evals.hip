// extern "C" doors to the launchers of plonk_amd/csrc/kzg_evals.hip (kzg_evals.hpp) — the scalar stage of KZG10 in evaluation
// form and the Lagrange-point build — for tests/test_gpu_kzg_evals.py.  No kernels here: the code that runs is
// libplonk_hip.so's own.  Every door takes the plonk_ctx* the Python binding holds (Context.handle), device pointers and plain
// host arguments, queues on the context's stream, waits for that stream and returns the product's code (PLONK_ERR_*, negative)
// or, when the product was content, the HIP error of the wait (positive).  Test code only.
#include <string.h>

#include "kzg_domain.hpp"
#include "kzg_evals.hpp"
#include "poly.hpp"

using namespace plonk;

namespace {

int finish(Ctx& c, int rc) {
  const hipError_t e = hipStreamSynchronize(c.stream);
  if (rc) return rc;
  return (int)e;
}
Fr fr_of(const uint64_t limbs[4]) {
  Fr r;
  memcpy(r.l, limbs, 32);
  return r;
}

}  // namespace

#define DOOR(H) \
  Ctx& c = (H)->c; \
  std::lock_guard<std::mutex> lk(c.mu)

extern "C" {

// inv[i] = 1 / (w^i - z) (0 where w^i == z), meta = {m, bad}; meta is preset here.  vecs (may be null): a device table of
// `count` vectors, scanned for non-canonical values
int dke_inverses(plonk_ctx* h, uint32_t log_n, const uint64_t z[4], void* inv, void* meta, const void* vecs, uint32_t count) {
  DOOR(h);
  if (log_n < 1 || log_n > 20) return PLONK_ERR_ARG;
  const KzeMeta preset = {KZE_NONE, 0};
  if (hipMemcpyAsync(meta, &preset, sizeof preset, hipMemcpyHostToDevice, c.stream) != hipSuccess) return PLONK_ERR_HIP;
  int rc = vecs ? kze_scan(&c, (const Fr* const*)vecs, 0, count, 1ull << log_n, (KzeMeta*)meta) : PLONK_OK;
  if (rc == PLONK_OK) rc = kze_denominators(&c, log_n, fr_of(z), (Fr*)inv, (KzeMeta*)meta);
  if (rc == PLONK_OK) rc = poly_batch_inverse(&c, (Fr*)inv, 1ull << log_n);
  return finish(c, rc);
}

// fold and evaluate `count` vectors (any count: groups of KZE_GROUP, as the handle launches them); vpow: scratch of 48 count bytes
int dke_fold_eval(plonk_ctx* h, uint32_t log_n, const void* vecs, uint32_t count, const uint64_t z[4], const uint64_t v[4],
                  const void* inv, uint64_t m, void* vpow, void* fold, void* partial, void* evals) {
  DOOR(h);
  if (log_n < 1 || log_n > 20 || !count) return PLONK_ERR_ARG;
  int rc = poly_kzg_powers(&c, vpow, count, fr_of(v));
  KzeFoldArgs a;
  a.vecs = (const Fr* const*)vecs;
  a.vpow = vpow;
  a.n = 1ull << log_n;
  a.inv = (const Fr*)inv;
  a.m = m;
  a.fold = (Fr*)fold;
  a.partial = (Fr*)partial;
  a.z = fr_of(z);
  a.scale = kze_eval_scale(a.z, log_n);
  for (uint32_t first = 0; first < count && rc == PLONK_OK; first += KZE_GROUP) {
    a.first = first;
    a.count = count - first < KZE_GROUP ? count - first : KZE_GROUP;
    a.accumulate = first ? 1 : 0;
    rc = kze_fold_eval(&c, a, (Fr*)evals + first);
  }
  return finish(c, rc);
}

int dke_quotient(plonk_ctx* h, uint32_t log_n, const void* fold, const void* inv, const uint64_t Y[4], uint64_t m, void* q, void* qpart) {
  DOOR(h);
  if (log_n < 1 || log_n > 20) return PLONK_ERR_ARG;
  return finish(c, kze_quotient(&c, log_n, (const Fr*)fold, (const Fr*)inv, fr_of(Y), m, (Fr*)q, (Fr*)qpart));
}

// out[i] = [L_i(tau)] G (96 bytes each) from the context's commit key
int dke_lagrange_points(plonk_ctx* h, uint32_t log_n, void* out) {
  DOOR(h);
  if (log_n < 1 || log_n > 20) return PLONK_ERR_ARG;
  GlvScalar* tw = nullptr;
  int rc = kzd_twiddles_create(&c, log_n + 1, &tw);
  if (rc == PLONK_OK) rc = kze_lagrange_points(&c, log_n, tw, log_n + 1, (G1Affine*)out);
  rc = finish(c, rc);
  (void)hipFree(tw);
  return rc;
}

uint64_t dke_const(int which) {
  switch (which) {
    case 0: return KZE_GROUP;
    case 1: return kze_fold_waves(1);          // partials per KZE_FOLD_T * KZE_FOLD_E values
    case 2: return (uint64_t)KZE_FOLD_T * KZE_FOLD_E;
    case 3: return KZE_Q_T;
    default: return 0;
  }
}

}  // extern "C"
