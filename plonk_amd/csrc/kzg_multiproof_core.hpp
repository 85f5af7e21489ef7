// KZG10 multiproofs (kzg_multiproof.hip): what the host decides before a kernel runs — the caps and the argument checks in the
// order the header documents them, the two counting sorts of the items, the two challenges and the plan
// plonk_kzg_multiproof_last reports — __host__ __device__ in place like kzg_cell_verify_core.hpp: the driver calls these
// functions, tests/csrc/host_kzg_multiproof.cpp compiles them with g++ against the big-int model tests/kzg_multiproof_model.py.
//
// n = 2^L, w the size-n generator, e_j[i] = p_j(w^i) the M vectors, C_j their commitments.  Items k < K: (j_k < M, m_k < n),
// y_k = e_(j_k)[m_k], weight r^k:
//   g(X) = sum_k r^k (p_(j_k)(X) - y_k) / (X - w^(m_k))          D = commit(g)
//   s_j  = sum_(k : j_k = j) r^k / (t - w^(m_k))                 h = sum_j s_j e_j
//   y    = sum_k r^k y_k / (t - w^(m_k))                         pi = commit(((h - g)[i] - y) / (w^i - t))
//   accept iff e(pi, [tau] h) == e(sum_j s_j C_j - D - [y] g + t pi, h)
// g in evaluation form, the items grouped by point index m (invd[s] = 1 / (w^s - 1), invd[0] = 0):
//   A_m[i] = sum_(k : m_k = m) r^k e_(j_k)[i]        Y_m = sum_(k : m_k = m) r^k y_k
//   q_m[i] = (A_m[i] - Y_m) w^(-m) invd[(i - m) mod n]  (i != m)       q_m[m] = -w^(-m) sum_(i != m) q_m[i] w^i
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/plonk_hip.h"
#include "field.cuh"
#include "transcript.hpp"
#include "kzg_evals_core.hpp"

namespace plonk {

static constexpr uint32_t KMP_MAX_LOG_N = 20;                  // plonk_kzg_multiproof_check (a domain handle has its own range)
static constexpr uint64_t KMP_MAX_ITEMS = 1ull << 20;          // items per call
static constexpr uint64_t KMP_MAX_VECTORS = 65536;             // vectors (commitments) per call
static constexpr uint64_t KMP_MAX_HOST_VALUES = 1ull << 28;    // nvectors * n of the host form (8 GiB staged on the device)
static constexpr uint32_t KMP_AGG_T = KZE_FOLD_T, KMP_AGG_E = KZE_FOLD_E;   // kmp_aggregate_kernel: kze_fold_kernel's shape
static constexpr uint32_t KMP_GROUP_CHUNK = 64;                // point groups one launch of kmp_aggregate_kernel takes
static constexpr uint32_t KMP_LANES = 64;                      // one wave per workgroup in the small kernels

HD bool kmp_canonical(const Fr& v) {
  for (int i = 7; i >= 0; --i) {
    if (v.l[i] < FrP::MOD[i]) return true;
    if (v.l[i] > FrP::MOD[i]) return false;
  }
  return false;   // == q
}

// The counts and the indexes of a call (the pointers are looked at by the entry point).  host_form: plonk_kzg_multiproof_open,
// which stages all the vectors; check: plonk_kzg_multiproof_check, which also bounds log_n.
HD int kmp_check_items(uint32_t log_n, uint64_t nvectors, const uint32_t* vector_index, const uint32_t* point_index, uint64_t count,
                       bool host_form, bool check) {
  if (check && (log_n < 1 || log_n > KMP_MAX_LOG_N)) return PLONK_ERR_ARG;
  if (count == 0 || count > KMP_MAX_ITEMS) return PLONK_ERR_ARG;
  if (nvectors == 0 || nvectors > KMP_MAX_VECTORS) return PLONK_ERR_ARG;
  const uint64_t n = 1ull << log_n;
  for (uint64_t k = 0; k < count; ++k)
    if (vector_index[k] >= nvectors || point_index[k] >= n) return PLONK_ERR_ARG;
  if (host_form && nvectors * n > KMP_MAX_HOST_VALUES) return PLONK_ERR_ARG;
  return PLONK_OK;
}

// r and t as the caller or the transcript gave them: PLONK_ERR_DATA for a non-canonical override or an override t inside the
// domain (override: 8 limbs, r then t, Montgomery; NULL: nothing to check yet)
HD int kmp_check_override(const uint64_t* challenges_override, uint32_t log_n, Fr* r, Fr* t) {
  if (!challenges_override) return PLONK_OK;
  memcpy(r->l, challenges_override, 32);
  memcpy(t->l, challenges_override + 4, 32);
  if (!kmp_canonical(*r) || !kmp_canonical(*t)) return PLONK_ERR_DATA;
  if (kze_in_domain(*t, log_n)) return PLONK_ERR_DATA;
  return PLONK_OK;
}

// perm: the items ordered by key (stable), off[b] .. off[b + 1]: the items with key b; off has buckets + 1 entries
HD void kmp_counting_sort(const uint32_t* key, uint64_t K, uint64_t buckets, uint32_t* perm, uint32_t* off) {
  for (uint64_t b = 0; b <= buckets; ++b) off[b] = 0;
  for (uint64_t k = 0; k < K; ++k) ++off[key[k] + 1];
  for (uint64_t b = 0; b < buckets; ++b) off[b + 1] += off[b];
  for (uint64_t k = 0; k < K; ++k) perm[off[key[k]]++] = (uint32_t)k;   // off[b] has moved to the end of b
  for (uint64_t b = buckets; b > 0; --b) off[b] = off[b - 1];
  off[0] = 0;
}
// The sort by point index, compacted to the point groups: perm as above, group_m[g] the g-th distinct point index (ascending),
// group_off[g] .. group_off[g + 1] its items in perm.  scratch: n + 1 words.  Returns the number of groups.
HD uint64_t kmp_sort_points(const uint32_t* point_index, uint64_t K, uint64_t n, uint32_t* perm, uint32_t* group_m, uint32_t* group_off,
                            uint32_t* scratch) {
  kmp_counting_sort(point_index, K, n, perm, scratch);
  uint64_t groups = 0;
  for (uint64_t m = 0; m < n; ++m)
    if (scratch[m + 1] != scratch[m]) {
      group_m[groups] = (uint32_t)m;
      group_off[groups] = scratch[m];
      ++groups;
    }
  group_off[groups] = (uint32_t)K;
  return groups;
}

struct KmpPlan {
  uint64_t point_groups;        // distinct point indexes
  uint64_t agg_launches;        // launches of kmp_aggregate_kernel (and of kmp_fix_kernel): ceil(point_groups / KMP_GROUP_CHUNK)
  uint64_t agg_blocks;          // workgroups of each: kze_fold_blocks(n)
  uint64_t waves;               // partials per group: kze_fold_waves(n)
  uint64_t partial_values;      // the partials buffer: min(point_groups, KMP_GROUP_CHUNK) * waves
  uint64_t products;            // field products of the aggregation pass: (K + 2 point_groups) n
  uint64_t fold_launches;       // kze_fold_eval launches of h: ceil(M / KZE_GROUP)
  uint64_t commitments_computed;
  uint64_t msm_launches;        // commitments_computed + 2 (D and pi)
  uint64_t msm_terms;           // n
  uint64_t stage_values;        // host form: M n values staged on the device
};
HD KmpPlan kmp_plan(uint32_t log_n, uint64_t M, uint64_t K, uint64_t point_groups, bool compute_commitments, bool host_form) {
  const uint64_t n = 1ull << log_n;
  KmpPlan p;
  p.point_groups = point_groups;
  p.agg_launches = (point_groups + KMP_GROUP_CHUNK - 1) / KMP_GROUP_CHUNK;
  p.agg_blocks = kze_fold_blocks(n);
  p.waves = kze_fold_waves(n);
  p.partial_values = (point_groups < KMP_GROUP_CHUNK ? point_groups : KMP_GROUP_CHUNK) * p.waves;
  p.products = (K + 2 * point_groups) * n;
  p.fold_launches = (M + KZE_GROUP - 1) / KZE_GROUP;
  p.commitments_computed = compute_commitments ? M : 0;
  p.msm_launches = p.commitments_computed + 2;
  p.msm_terms = n;
  p.stage_values = host_form ? M * n : 0;
  return p;
}

// The two challenges on a fresh Transcript::new(label).  values: K x 4 Montgomery limbs (canonical).  kmp_challenge_r leaves the
// transcript ready for kmp_challenge_t, which binds D.
HD Fr kmp_challenge_r(Transcript& tr, uint32_t log_n, const uint8_t* commitments48, uint64_t M, const uint32_t* vector_index,
                      const uint32_t* point_index, const uint64_t* values, uint64_t K) {
  tr.append_message("dom-sep", (const uint8_t*)"kzg10-multiproof-v1", 19);
  tr.append_u64("log-n", log_n);
  tr.append_u64("commitments", M);
  tr.append_u64("items", K);
  for (uint64_t j = 0; j < M; ++j) tr.append_commitment("commitment", commitments48 + 48 * j);
  for (uint64_t k = 0; k < K; ++k) {
    Fr v;
    memcpy(v.l, values + 4 * k, 32);
    tr.append_u64("vector-index", vector_index[k]);
    tr.append_u64("point-index", point_index[k]);
    tr.append_scalar("value", v);
  }
  return tr.challenge_scalar("multiproof-r");
}
HD Fr kmp_challenge_t(Transcript& tr, const uint8_t d48[48]) {
  tr.append_commitment("multiproof-d", d48);
  return tr.challenge_scalar("multiproof-t");
}

}  // namespace plonk
