// CPU harness for plonk_amd/csrc/kzg_cell_verify_core.hpp (the argument checks, the packing of the twist kernel, the passes of
// the column sums, the term layout, the counting sort, the plan and the batch challenge of the KZG10 cell verifier), compiled
// with g++ by tests/test_kzg_cell_verify_model_host.py and checked against the big-int model tests/kzg_cell_verify_model.py.
#include <vector>

#include "../../plonk_amd/csrc/kzg_cell_verify_core.hpp"

using namespace plonk;

extern "C" {

int hkv_check_shape(uint32_t log_n, uint32_t log_cell) { return kzv_check_shape(log_n, log_cell); }
int hkv_check_items(uint32_t log_n, uint32_t log_cell, uint64_t M, const uint32_t* cidx, const uint32_t* kidx, uint64_t K) {
  return kzv_check_items(log_n, log_cell, M, cidx, kidx, K);
}
// the count limits alone (no index arrays of 2^20 entries in a test)
int hkv_check_counts(uint32_t log_n, uint32_t log_cell, uint64_t M, uint64_t K) {
  std::vector<uint32_t> zero(K < (1u << 21) ? K : 0, 0u);
  if (zero.size() != K) return PLONK_ERR_ARG;
  return kzv_check_items(log_n, log_cell, M, zero.data(), zero.data(), K);
}
int hkv_canonical(const uint64_t limbs[4]) {
  Fr v;
  memcpy(v.l, limbs, 32);
  return kzv_canonical(v) ? 1 : 0;
}
uint32_t hkv_items_per_group(uint32_t log_cell) { return kzv_items_per_group(log_cell); }
uint32_t hkv_lanes_per_item(uint32_t log_cell) { return kzv_lanes_per_item(log_cell); }
uint64_t hkv_twist_groups(uint32_t log_cell, uint64_t K) { return kzv_twist_groups(log_cell, K); }
uint64_t hkv_twist_lds_bytes(uint32_t log_cell) { return kzv_twist_lds_bytes(log_cell); }
uint64_t hkv_colsum_slices(uint64_t rows) { return kzv_colsum_slices(rows); }
uint32_t hkv_colsum_passes(uint64_t rows) { return kzv_colsum_passes(rows); }
void hkv_layout(uint32_t log_cell, uint64_t M, uint64_t K, uint64_t out[7]) {
  const KzvLayout t = kzv_layout(log_cell, M, K);
  out[0] = t.pt_commitment;
  out[1] = t.pt_proof;
  out[2] = t.points;
  out[3] = t.term_w;
  out[4] = t.term_x;
  out[5] = t.term_r;
  out[6] = t.terms;
}
void hkv_counting_sort(const uint32_t* cidx, uint64_t K, uint64_t M, uint32_t* perm, uint32_t* off) {
  kzv_counting_sort(cidx, K, M, perm, off);
}
void hkv_plan(uint32_t log_cell, uint64_t M, uint64_t K, int each, uint32_t min_left, uint32_t min_right, uint64_t out[9]) {
  const KzvPlan p = kzv_plan(log_cell, M, K, each != 0, min_left, min_right);
  out[0] = p.transforms;
  out[1] = p.twist_groups;
  out[2] = p.colsum_passes;
  out[3] = p.msm_terms_left;
  out[4] = p.msm_terms_right;
  out[5] = p.msm_path_left;
  out[6] = p.msm_path_right;
  out[7] = p.scalar_muls;
  out[8] = p.msm_terms_info;
}
// values: K x l x 4 Montgomery limbs; rho_out: the canonical 32 little-endian bytes
void hkv_challenge(const uint8_t* label, uint64_t label_len, uint32_t log_n, uint32_t log_cell, const uint8_t* key240,
                   const uint8_t* commitments48, uint64_t M, const uint32_t* cidx, const uint32_t* kidx, const uint64_t* values,
                   const uint8_t* proofs48, uint64_t K, uint8_t rho_out[32]) {
  std::vector<uint8_t> cell(32ull << log_cell);
  const Fr rho = kzv_challenge(label, label_len, log_n, log_cell, key240, commitments48, M, cidx, kidx, values, proofs48, K, cell.data());
  fr_to_bytes(rho, rho_out);
}
}  // extern "C"
