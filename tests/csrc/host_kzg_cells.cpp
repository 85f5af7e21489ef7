// CPU harness for plonk_amd/csrc/kzg_cells_core.hpp (the index maps, the slice split, the chunk plan, the operation counts and
// the argument check of the KZG10 cell proofs), compiled with g++ by tests/test_kzg_cells_model_host.py and checked against
// the big-int model tests/kzg_cells_model.py.
#include "../../plonk_amd/csrc/kzg_cells_core.hpp"

using namespace plonk;

extern "C" {

uint64_t hkc_fill_lanes() { return KZC_FILL_LANES; }
int hkc_check_cell(uint32_t log_n, uint32_t log_cell) { return kzc_check_cell(log_n, log_cell); }
uint64_t hkc_a_src(uint32_t log_cell, uint64_t r, uint64_t u, uint64_t v) { return kzc_a_src(log_cell, r, u, v); }
uint64_t hkc_g_src(uint32_t log_cell, uint64_t r, uint64_t u, uint64_t t) { return kzc_g_src(log_cell, r, u, t); }
uint64_t hkc_cell_dst(uint32_t log_n, uint32_t log_cell, uint64_t i) { return kzc_cell_dst(log_n, log_cell, i); }
uint64_t hkc_slice_terms(uint32_t log_cell, uint64_t slices) { return kzc_slice_terms(log_cell, slices); }
uint64_t hkc_slice_first(uint32_t log_cell, uint64_t slices, uint64_t s) { return kzc_slice_first(log_cell, slices, s); }
uint64_t hkc_partial_slot(uint64_t r, uint64_t s, uint64_t p) { return kzc_partial_slot(r, s, p); }
void hkc_plan(uint32_t log_n, uint32_t log_cell, uint64_t count, uint64_t cap_bytes, uint64_t forced_slices, uint64_t out[7]) {
  const KzcPlan p = kzc_plan(log_n, log_cell, count, cap_bytes, forced_slices);
  out[0] = p.slices;
  out[1] = p.chunk_polys;
  out[2] = p.chunks;
  out[3] = p.ws_bytes;
  out[4] = p.table_bytes;
  out[5] = p.stage_launches;
  out[6] = p.scalar_muls;
}

}  // extern "C"
