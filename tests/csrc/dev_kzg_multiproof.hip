// extern "C" doors to the launchers of plonk_amd/csrc/kzg_multiproof.hip (kzg_multiproof.hpp) — the invd table, the gather, the
// per-group constants, the aggregation with its fix-up and the weights — for tests/test_gpu_kzg_multiproof.py.  No kernels here:
// the code that runs is libplonk_hip.so's own.  Every door takes the plonk_ctx* the Python binding holds (Context.handle), device
// pointers and plain host arguments, queues on the context's stream, waits for that stream and returns the product's code
// (PLONK_ERR_*, negative) or, when the product was content, the HIP error of the wait (positive).  Test code only.
#include <string.h>

#include "kzg_multiproof.hpp"
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

// invd[s] = 1 / (w^s - 1), invd[0] = 0; meta: 16 bytes of scratch
int dkm_invd(plonk_ctx* h, uint32_t log_n, void* invd, void* meta) {
  DOOR(h);
  if (log_n < 1 || log_n > 20) return PLONK_ERR_ARG;
  return finish(c, kmp_invd(&c, log_n, (Fr*)invd, (KzeMeta*)meta));
}

int dkm_gather(plonk_ctx* h, const void* vecs, const void* vidx, const void* midx, uint64_t K, void* yk) {
  DOOR(h);
  return finish(c, kmp_gather(&c, (const Fr* const*)vecs, (const uint32_t*)vidx, (const uint32_t*)midx, K, (Fr*)yk));
}

// The aggregation as the handle runs it: r^k as data and in twiddle form, the per-group constants, then every chunk of groups
// with its fix-up.  perm / group_m / group_off: kmp_sort_points' output on the device.
int dkm_aggregate(plonk_ctx* h, uint32_t log_n, const void* vecs, const void* vidx, const void* yk, uint64_t K, const uint64_t r[4],
                  const void* perm, const void* group_m, const void* group_off, uint64_t groups, const void* invd, void* rpow, void* rtw,
                  void* ym, void* cw, void* negw, void* g, void* partial) {
  DOOR(h);
  if (log_n < 1 || log_n > 20 || !K || K > KMP_MAX_ITEMS) return PLONK_ERR_ARG;
  int rc = poly_power_array(&c, (Fr*)rpow, K, fr_of(r));
  if (rc == PLONK_OK) rc = poly_kzg_powers(&c, rtw, (uint32_t)K, fr_of(r));
  if (rc == PLONK_OK)
    rc = kmp_groups(&c, log_n, (const Fr*)rpow, (const Fr*)yk, (const uint32_t*)perm, (const uint32_t*)group_m, (const uint32_t*)group_off,
                    groups, (Fr*)ym, cw, (Fr*)negw);
  KmpAggArgs a;
  a.vecs = (const Fr* const*)vecs;
  a.vector_index = (const uint32_t*)vidx;
  a.rtw = rtw;
  a.perm = (const uint32_t*)perm;
  a.group_m = (const uint32_t*)group_m;
  a.group_off = (const uint32_t*)group_off;
  a.ym = (const Fr*)ym;
  a.cw = cw;
  a.negw = (const Fr*)negw;
  a.invd = (const Fr*)invd;
  a.n = 1ull << log_n;
  a.log_n = log_n;
  a.g = (Fr*)g;
  a.partial = (Fr*)partial;
  if (rc == PLONK_OK) rc = kmp_aggregate(&c, a, groups);
  return finish(c, rc);
}

// rpow = r^k, then the weights: stw (48 M bytes), y_out (32), sc (32 (M + 3)), ids (4 (M + 3)); perm / off: the sort by vector
int dkm_weights(plonk_ctx* h, uint32_t log_n, const uint64_t r[4], const uint64_t t[4], const void* midx, const void* yk, const void* perm,
                const void* off, uint64_t K, uint64_t M, void* rpow, void* wt, void* stw, void* y_out, void* sc, void* ids) {
  DOOR(h);
  if (log_n < 1 || log_n > 20 || !K || K > KMP_MAX_ITEMS) return PLONK_ERR_ARG;
  int rc = poly_power_array(&c, (Fr*)rpow, K, fr_of(r));
  if (rc == PLONK_OK)
    rc = kmp_weights(&c, log_n, fr_of(t), (const uint32_t*)midx, (const Fr*)rpow, (const Fr*)yk, (const uint32_t*)perm, (const uint32_t*)off,
                     K, M, (Fr*)wt, stw, (Fr*)y_out, (uint32_t*)sc, (uint32_t*)ids);
  return finish(c, rc);
}

uint64_t dkm_const(int which) {
  switch (which) {
    case 0: return KMP_GROUP_CHUNK;
    case 1: return kze_fold_waves(1);          // partials per KMP_AGG_T * KMP_AGG_E values
    case 2: return (uint64_t)KMP_AGG_T * KMP_AGG_E;
    default: return 0;
  }
}

}  // extern "C"
