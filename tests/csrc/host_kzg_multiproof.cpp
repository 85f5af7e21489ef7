// CPU harness for plonk_amd/csrc/kzg_multiproof_core.hpp (the argument checks, the two counting sorts, the plan and the two
// challenges of the KZG10 multiproofs), compiled with g++ by tests/test_kzg_multiproof_model_host.py and checked against the
// big-int model tests/kzg_multiproof_model.py.
#include <vector>

#include "../../plonk_amd/csrc/kzg_multiproof_core.hpp"

using namespace plonk;

extern "C" {

int hkm_check_items(uint32_t log_n, uint64_t M, const uint32_t* vidx, const uint32_t* midx, uint64_t K, int host_form, int check) {
  return kmp_check_items(log_n, M, vidx, midx, K, host_form != 0, check != 0);
}
// the count limits alone (no index arrays of 2^20 entries in a test)
int hkm_check_counts(uint32_t log_n, uint64_t M, uint64_t K, int host_form, int check) {
  std::vector<uint32_t> zero(K < (1u << 21) ? K : 0, 0u);
  if (zero.size() != K) return PLONK_ERR_ARG;
  return kmp_check_items(log_n, M, zero.data(), zero.data(), K, host_form != 0, check != 0);
}
// override: 8 limbs or null; out: r then t as the function loaded them
int hkm_check_override(const uint64_t* override8, uint32_t log_n, uint64_t out[8]) {
  Fr r = Fr::zero(), t = Fr::zero();
  const int rc = kmp_check_override(override8, log_n, &r, &t);
  memcpy(out, r.l, 32);
  memcpy(out + 4, t.l, 32);
  return rc;
}
void hkm_counting_sort(const uint32_t* key, uint64_t K, uint64_t buckets, uint32_t* perm, uint32_t* off) {
  kmp_counting_sort(key, K, buckets, perm, off);
}
uint64_t hkm_sort_points(const uint32_t* midx, uint64_t K, uint64_t n, uint32_t* perm, uint32_t* group_m, uint32_t* group_off) {
  std::vector<uint32_t> scratch(n + 1);
  return kmp_sort_points(midx, K, n, perm, group_m, group_off, scratch.data());
}
void hkm_plan(uint32_t log_n, uint64_t M, uint64_t K, uint64_t groups, int compute, int host_form, uint64_t out[11]) {
  const KmpPlan p = kmp_plan(log_n, M, K, groups, compute != 0, host_form != 0);
  out[0] = p.point_groups;
  out[1] = p.agg_launches;
  out[2] = p.agg_blocks;
  out[3] = p.waves;
  out[4] = p.partial_values;
  out[5] = p.products;
  out[6] = p.fold_launches;
  out[7] = p.commitments_computed;
  out[8] = p.msm_launches;
  out[9] = p.msm_terms;
  out[10] = p.stage_values;
}
// values: K x 4 Montgomery limbs; out: r then t, the canonical 32 little-endian bytes each
void hkm_challenges(const uint8_t* label, uint64_t label_len, uint32_t log_n, const uint8_t* commitments48, uint64_t M,
                    const uint32_t* vidx, const uint32_t* midx, const uint64_t* values, uint64_t K, const uint8_t d48[48],
                    uint8_t out[64]) {
  Transcript tr(label, label_len);
  const Fr r = kmp_challenge_r(tr, log_n, commitments48, M, vidx, midx, values, K);
  const Fr t = kmp_challenge_t(tr, d48);
  fr_to_bytes(r, out);
  fr_to_bytes(t, out + 32);
}
}  // extern "C"
