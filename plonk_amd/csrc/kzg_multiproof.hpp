// Launchers of kzg_multiproof.hip: the aggregation of the K quotients in evaluation form and the weights of the opening at t.
// Shared with the doors of the per-kernel tests (tests/csrc/dev_kzg_multiproof.hip).  Every pointer is device memory unless
// said otherwise, everything is queued on the context's stream, nothing synchronises.
#pragma once
#include "plonk_internal.hpp"
#include "kzg_evals.hpp"
#include "kzg_multiproof_core.hpp"

namespace plonk {

// invd[s] = 1 / (w^s - 1), s < n = 2^log_n, invd[0] = 0: kze_denominators at z = 1 and poly_batch_inverse, which leaves the
// zero alone.  meta: a KzeMeta the caller owns (its m becomes 0).
int kmp_invd(Ctx* c, uint32_t log_n, Fr* invd, KzeMeta* meta);

// yk[k] = vecs[vector_index[k]][point_index[k]], k < K: the values the prover claims, read from the vectors themselves
int kmp_gather(Ctx* c, const Fr* const* vecs, const uint32_t* vector_index, const uint32_t* point_index, uint64_t K, Fr* yk);

// Per point group g < groups (kmp_sort_points' perm / group_m / group_off): ym[g] = sum of rpow[k] yk[k] over its items,
// cw[g] = 32 w^(-m) in twiddle form (Fr29Slot: the factor that also takes the product with invd back to the R form) and
// negw[g] = -w^(-m).  rpow: r^k as data (poly_power_array).
int kmp_groups(Ctx* c, uint32_t log_n, const Fr* rpow, const Fr* yk, const uint32_t* perm, const uint32_t* group_m,
               const uint32_t* group_off, uint64_t groups, Fr* ym, void* cw, Fr* negw);

struct KmpAggArgs {
  const Fr* const* vecs;        // device table of the call's vectors
  const uint32_t* vector_index; // [K]
  const void* rtw;              // r^k, k < K, twiddle form (Fr29Slot, poly_kzg_powers)
  const uint32_t* perm;         // the items by point index
  const uint32_t* group_m;      // [groups]
  const uint32_t* group_off;    // [groups + 1]
  const Fr* ym;                 // [groups]
  const void* cw;               // [groups] Fr29Slot
  const Fr* negw;               // [groups]
  const Fr* invd;               // [n]
  uint64_t n;
  uint32_t log_n;
  Fr* g;                        // [n] out
  Fr* partial;                  // [min(groups, KMP_GROUP_CHUNK)][kze_fold_waves(n)]
};
// g[i] = sum over all the groups of q_m[i]: ceil(groups / KMP_GROUP_CHUNK) launches of kmp_aggregate_kernel, each followed by
// kmp_fix_kernel for the entries g[m] of its groups
int kmp_aggregate(Ctx* c, const KmpAggArgs& a, uint64_t groups);

// wt[k] = 1 / (t - w^(m_k)) (t outside the domain), then per vector j < M over kmp_counting_sort's perm / off by vector index
// s_j = sum rpow[k] wt[k], and y = sum_k rpow[k] wt[k] yk[k].  Outputs, each may be null: stw[j] = s_j in twiddle form
// (Fr29Slot, the weights kze_fold_eval takes), y_out = y as data, and the terms of the check in msm_run's layout:
// sc = [s_0 .. s_(M-1) | -1 | t | -y] canonical, 8 words each, ids[i] = i, i < M + 3.
int kmp_weights(Ctx* c, uint32_t log_n, const Fr& t, const uint32_t* point_index, const Fr* rpow, const Fr* yk, const uint32_t* perm,
                const uint32_t* off, uint64_t K, uint64_t M, Fr* wt, void* stw, Fr* y_out, uint32_t* sc, uint32_t* ids);

// plonk_kzg_multiproof_open_dev (given commitments, no commitments_out) for a caller that is inside the handle already —
// kzg_tree.hip, which holds the context's mutex and has made the KZD_WORK checks: the argument checks, then the same body
struct KzgDomain;
int kmp_open_entered(const char* api_fn, KzgDomain* d, const void* const* vecs_dev, uint64_t nvectors, const uint8_t* commitments_in,
                     const uint32_t* vector_index, const uint32_t* point_index, uint64_t count, const uint8_t* label, uint64_t label_len,
                     const uint64_t* challenges_override, uint64_t* values, uint8_t* proof96);

void kmp_check_release(void* ws);   // the workspace plonk_kzg_multiproof_check hangs off its key

}  // namespace plonk
