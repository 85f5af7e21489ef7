// CPU harness for plonk_amd/csrc/kzg_evals_core.hpp (the argument checks, the launch geometry, the plan, the in-domain test
// and the factor of the barycentric sum of KZG10 in evaluation form), compiled with g++ by tests/test_kzg_evals_model_host.py
// and checked against the big-int model tests/kzg_evals_model.py.
#include <string.h>

#include "../../plonk_amd/csrc/kzg_evals_core.hpp"

using namespace plonk;

extern "C" {

uint64_t hke_const(int which) {
  switch (which) {
    case 0: return KZE_MAX_COUNT;
    case 1: return KZE_GROUP;
    case 2: return KZE_FOLD_T;
    case 3: return KZE_FOLD_E;
    case 4: return KZE_Q_T;
    case 5: return KZE_STAGE_MIN;
    case 6: return KZE_POINT_BYTES;
    case 7: return KZE_NONE;
    default: return 0;
  }
}
uint32_t hke_fold_waves(uint64_t n) { return kze_fold_waves(n); }
uint32_t hke_fold_blocks(uint64_t n) { return kze_fold_blocks(n); }
uint32_t hke_quotient_blocks(uint64_t n) { return kze_quotient_blocks(n); }
// z: 4 canonical limbs
int hke_in_domain(const uint64_t z[4], uint32_t log_n) {
  Fr t;
  memcpy(t.l, z, 32);
  return kze_in_domain(t.to_mont(), log_n) ? 1 : 0;
}
void hke_eval_scale(const uint64_t z[4], uint32_t log_n, uint64_t out[4]) {
  Fr t;
  memcpy(t.l, z, 32);
  const Fr s = kze_eval_scale(t.to_mont(), log_n).from_mont();
  memcpy(out, s.l, 32);
}
void hke_plan(uint32_t log_n, uint64_t count, int commitments, int witness, int host_form, uint64_t out[6]) {
  const KzePlan p = kze_plan(log_n, count, commitments != 0, witness != 0, host_form != 0);
  out[0] = p.group_vectors;
  out[1] = p.groups;
  out[2] = p.stage_values;
  out[3] = p.msm_launches;
  out[4] = p.msm_terms;
  out[5] = p.lagrange_bytes;
}
int hke_check_commit(int has_domain, int has_evals, int has_out, uint64_t count) {
  return kze_check_commit(has_domain != 0, has_evals != 0, has_out != 0, count);
}
int hke_check_open(int has_domain, int has_evals, int has_point, int has_v, int has_evaluations, uint64_t count) {
  return kze_check_open(has_domain != 0, has_evals != 0, has_point != 0, has_v != 0, has_evaluations != 0, count);
}

}  // extern "C"
