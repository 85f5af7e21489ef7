// CPU harness for plonk_amd/csrc/kzg_recover_core.hpp (the index maps, the chunk plan, the counts and the argument checks of
// the KZG10 cell recovery), compiled with g++ by tests/test_kzg_recover_model_host.py and checked against the big-int model
// tests/kzg_recover_model.py.
#include "../../plonk_amd/csrc/kzg_recover_core.hpp"

using namespace plonk;

extern "C" {

uint32_t hkr_max_log_r() { return KZR_MAX_LOG_R; }
uint32_t hkr_vanish_slices() { return KZR_VANISH_SLICES; }
uint32_t hkr_vanish_first(uint32_t s) { return kzr_vanish_first(s); }
uint64_t hkr_scatter_src(uint32_t log_n, uint32_t log_cell, uint64_t i, const int32_t* slot) { return kzr_scatter_src(log_n, log_cell, i, slot); }
uint64_t hkr_period(uint32_t log_n, uint32_t log_cell, uint64_t i) { return kzr_period(log_n, log_cell, i); }
uint64_t hkr_point_exp(uint32_t log_r, uint64_t p) { return kzr_point_exp(log_r, p); }
int hkr_point_on_coset(uint32_t log_r, uint64_t p) { return kzr_point_on_coset(log_r, p) ? 1 : 0; }
uint64_t hkr_tail_first(uint64_t max_len) { return kzr_tail_first(max_len); }
int hkr_check_args(int has_domain, uint32_t log_n, uint32_t log_cell, uint64_t count, const uint32_t* cell_ids, uint64_t available,
                   int has_values, int values_all_set, uint64_t max_len, int any_output) {
  return kzr_check_args(has_domain != 0, log_n, log_cell, count, cell_ids, available, has_values != 0, values_all_set != 0, max_len,
                        any_output != 0);
}
int hkr_check_degree(uint32_t log_cell, uint64_t available, uint64_t max_len) { return kzr_check_degree(log_cell, available, max_len); }
void hkr_plan(uint32_t log_n, uint32_t log_cell, uint64_t count, uint64_t available, uint64_t cap_bytes, int want_values, uint64_t out[7]) {
  const KzrPlan p = kzr_plan(log_n, log_cell, count, available, cap_bytes, want_values != 0);
  out[0] = p.missing;
  out[1] = p.chunk_polys;
  out[2] = p.chunks;
  out[3] = p.ws_bytes;
  out[4] = p.passes;
  out[5] = p.transforms;
  out[6] = p.vanish_muls;
}

}  // extern "C"
