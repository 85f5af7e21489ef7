// extern "C" doors to the launchers of plonk_amd/csrc/kzg_cells.hip (kzg_cells.hpp) — the A^(u) table build, the gather and
// transpose kernels, the multiply-accumulate and its reduction — for tests/test_gpu_kzg_cells.py, and the test-only setter of
// the slice count.  No kernels here: the code that runs is libplonk_hip.so's own.  Every door takes the plonk_ctx* the Python
// binding holds (Context.handle), device pointers and plain host arguments, queues on the context's stream, waits for that
// stream and returns the product's code (PLONK_ERR_*, negative) or, when the product was content, the HIP error of the wait
// (positive).  Slots are loaded and read back through the doors of dev_kzg_domain.hip.  Test code only.
#include <string.h>

#include "kzg_cells.hpp"

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

// table: 2n slots; tw: dkd_twiddles' table for tw_log >= log_n - log_cell + 1
int dkc_table_build(plonk_ctx* h, uint32_t log_n, uint32_t log_cell, const void* tw, uint32_t tw_log, void* table) {
  DOOR(h);
  return finish(c, kzc_table_build(&c, log_n, log_cell, (const GlvScalar*)tw, tw_log, table));
}

int dkc_gather(plonk_ctx* h, const void* f, uint32_t log_n, uint32_t log_cell, uint32_t batch, void* g) {
  DOOR(h);
  return finish(c, kzc_gather(&c, (const Fr*)f, log_n, log_cell, batch, (Fr*)g));
}

// tw: 2^(log_size - 1) Montgomery values w^e
int dkc_ntt(plonk_ctx* h, void* g, uint32_t log_size, uint64_t vectors, uint32_t batch, const void* tw) {
  DOOR(h);
  return finish(c, kzc_ntt(&c, (Fr*)g, log_size, vectors, batch, (const Fr*)tw));
}

int dkc_transpose(plonk_ctx* h, const void* evals, uint32_t log_n, uint32_t log_cell, uint32_t batch, void* cells) {
  DOOR(h);
  return finish(c, kzc_transpose(&c, (const Fr*)evals, log_n, log_cell, batch, (Fr*)cells));
}

// scale: 4 Montgomery limbs
int dkc_mulacc(plonk_ctx* h, const void* table, const void* G, uint64_t g_stride, void* ws, uint64_t stride, uint32_t log_n,
               uint32_t log_cell, uint64_t slices, uint32_t batch, const uint64_t scale[4]) {
  DOOR(h);
  Fr s;
  memcpy(s.l, scale, 32);
  return finish(c, kzc_mulacc(&c, table, (const Fr*)G, g_stride, ws, stride, log_n, log_cell, slices, batch, s));
}

int dkc_reduce(plonk_ctx* h, void* ws, uint64_t stride, uint32_t log_r, uint64_t slices, uint32_t batch) {
  DOOR(h);
  return finish(c, kzc_reduce(&c, ws, stride, log_r, slices, batch));
}

// the slice count S of the handle's next plonk_kzg_open_cells calls (0 restores the plan's own choice)
int dkc_set_slices(plonk_kzg_domain* dom, uint64_t slices) {
  if (!dom) return PLONK_ERR_ARG;
  kzc_set_slices(dom, slices);
  return PLONK_OK;
}

}  // extern "C"
