// extern "C" doors to the launchers of plonk_amd/csrc/kzg_many.hip (kzg_many.hpp) — the window-table build, the dense and the
// sparse accumulation and the compression — for tests/test_gpu_kzg_many.py, and the test-only setter of the slice count.  No
// kernels here: the code that runs is libplonk_hip.so's own.  Every door takes the plonk_ctx* the Python binding holds
// (Context.handle), device pointers and plain host arguments, queues on the context's stream, waits for that stream and
// returns the product's code (PLONK_ERR_*, negative) or, when the product was content, the HIP error of the wait (positive).
// Test code only.
#include "kzg_handle.hpp"
#include "kzg_many.hpp"

using namespace plonk;

namespace {

int finish(Ctx& c, int rc) {
  const hipError_t e = hipStreamSynchronize(c.stream);
  if (rc) return rc;
  return (int)e;
}
KzmTables tables(const void* table, uint32_t log_n, uint32_t window_bits) {
  return KzmTables{(const G1AffineR*)table, log_n, window_bits, kzm_windows(window_bits)};
}

}  // namespace

#define DOOR(H) \
  Ctx& c = (H)->c; \
  std::lock_guard<std::mutex> lk(c.mu)

extern "C" {

// lag: n x 96 bytes (affine x || y, Montgomery; 96 zero bytes: the identity); table: kzm_table_bytes(log_n, window_bits)
int dkm_tables_fill(plonk_ctx* h, const void* lag, uint32_t log_n, uint32_t window_bits, void* table) {
  DOOR(h);
  return finish(c, kzm_tables_fill(&c, (const G1Affine*)lag, log_n, window_bits, (G1AffineR*)table));
}

// values: count x n Montgomery Fr; partial: count x slices slots of 256 bytes; out48: count x 48
int dkm_commit(plonk_ctx* h, const void* table, uint32_t log_n, uint32_t window_bits, const void* values, uint64_t count, uint32_t slices,
               void* partial, void* out48) {
  DOOR(h);
  int rc = kzm_accumulate(&c, tables(table, log_n, window_bits), (const Fr*)values, count, slices, (G1RSlot*)partial);
  if (!rc) rc = kzm_compress(&c, (const G1RSlot*)partial, slices, nullptr, nullptr, count, (uint8_t*)out48);
  return finish(c, rc);
}

// offsets: count + 1 (device); partial: count slots; out48: count x 48
int dkm_sparse(plonk_ctx* h, const void* table, uint32_t log_n, uint32_t window_bits, const void* offsets, const void* index,
               const void* deltas, uint64_t count, void* partial, void* out48) {
  DOOR(h);
  int rc = kzm_accumulate_sparse(&c, tables(table, log_n, window_bits), (const uint64_t*)offsets, (const uint32_t*)index, (const Fr*)deltas,
                                 count, (G1RSlot*)partial);
  if (!rc) rc = kzm_compress(&c, (const G1RSlot*)partial, 1, nullptr, nullptr, count, (uint8_t*)out48);
  return finish(c, rc);
}

// the slices of the handle's next plonk_kzg_commit_many calls (0 restores the plan's own rule)
int dkm_set_slices(plonk_kzg_domain* dom, uint32_t slices) {
  if (!dom) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(dom->ctx->c.mu);
  kzm_test_force_slices(dom->d, slices);
  return PLONK_OK;
}

uint64_t dkm_const(int which) {
  switch (which) {
    case 0: return KZM_RESIDENT_WAVES;
    case 1: return KZM_ENTRY_BYTES;
    case 2: return KZM_SLOT_BYTES;
    case 3: return KZM_CHUNK_MAX;
    default: return 0;
  }
}

}  // extern "C"
