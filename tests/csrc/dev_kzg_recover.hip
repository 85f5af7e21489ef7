// extern "C" doors to the launchers of plonk_amd/csrc/kzg_recover.hip (kzg_recover.hpp) — the vanish, scatter, divide and tail
// kernels of the KZG10 cell recovery — for tests/test_gpu_kzg_recover.py.  No kernels here: the code that runs is
// libplonk_hip.so's own.  Every door takes the plonk_ctx* the Python binding holds (Context.handle), device pointers and plain
// host arguments, queues on the context's stream, waits for that stream and returns the product's code (PLONK_ERR_*,
// negative) or, when the product was content, the HIP error of the wait (positive).  Test code only.
#include "poly.hpp"
#include "kzg_recover.hpp"

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

// pw: r values of scratch the door fills with phi^i; miss: nmiss indexes; zdom, zcoset: r values each
int dkr_vanish(plonk_ctx* h, void* pw, const void* miss, uint32_t nmiss, uint32_t log_n, uint32_t log_cell, void* zdom, void* zcoset) {
  DOOR(h);
  if (kzc_check_cell(log_n, log_cell) || log_n - log_cell > KZR_MAX_LOG_R || !pw || !zdom || !zcoset) return PLONK_ERR_ARG;   // before the power table is written
  int rc = poly_power_array(&c, (Fr*)pw, 1ull << (log_n - log_cell), fr_domain_root(log_n - log_cell));
  if (!rc) rc = kzr_vanish(&c, (const Fr*)pw, (const uint32_t*)miss, nmiss, log_n, log_cell, (Fr*)zdom, (Fr*)zcoset);
  return finish(c, rc);
}

// vecs: device table of `batch` device pointers
int dkr_scatter(plonk_ctx* h, const void* vecs, const void* slot, const void* zdom, uint32_t log_n, uint32_t log_cell, uint32_t batch,
                void* out) {
  DOOR(h);
  return finish(c, kzr_scatter(&c, (const Fr* const*)vecs, (const int32_t*)slot, (const Fr*)zdom, log_n, log_cell, batch, (Fr*)out));
}

int dkr_divide(plonk_ctx* h, void* v, const void* zinv, uint32_t log_n, uint32_t log_cell, uint32_t batch) {
  DOOR(h);
  return finish(c, kzr_divide(&c, (Fr*)v, (const Fr*)zinv, log_n, log_cell, batch));
}

int dkr_tail(plonk_ctx* h, const void* coeffs, uint32_t log_n, uint64_t max_len, uint32_t batch, void* flags) {
  DOOR(h);
  return finish(c, kzr_tail(&c, (const Fr*)coeffs, log_n, max_len, batch, (int32_t*)flags));
}

}  // extern "C"
