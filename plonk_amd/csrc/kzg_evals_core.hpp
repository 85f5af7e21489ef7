// KZG10 in evaluation form (kzg_evals.hip): everything the host decides before a kernel runs — the argument checks in the
// order the header documents them, whether the point lies in the domain, the factor of the barycentric sum, the geometry of
// the fold and quotient launches and the plan a call reports.  Like kzg_domain_core.hpp everything is __host__ __device__ in
// place (the HD convention of field.cuh): the handle calls these functions, tests/csrc/host_kzg_evals.cpp compiles them with
// g++ against the big-int model tests/kzg_evals_model.py.
//
// e_j[i] = p_j(w^i), i < n = 2^L, w the generator of the size-n domain, z the point, v the fold challenge:
//   d_i = 1 / (w^i - z)                                   one batch inversion per call; lane m with w^m = z stays 0
//   u_i = w^i / (z - w^i) = -(1 + z d_i)                  so the weights need no second table of w^i
//   y_j = (z^n - 1) / n * sum_i e_j[i] u_i                z outside the domain;  y_j = e_j[m] inside
//   F[i] = sum_j v^j e_j[i],  Y = sum_j v^j y_j
//   q[i] = (F[i] - Y) d_i  (i != m),   q[m] = -w^(-m) sum_(i != m) q[i] w^i
//   commit_j = sum_i e_j[i] [L_i(tau)] G,   witness = sum_i q[i] [L_i(tau)] G
#pragma once
#include <stdint.h>

#include "../../include/plonk_hip.h"
#include "field.cuh"

namespace plonk {

static constexpr uint64_t KZE_MAX_COUNT = 65536;              // vectors per call, as plonk_kzg_open
static constexpr uint32_t KZE_GROUP = 64;                     // vectors per launch of the fold kernel
static constexpr uint32_t KZE_FOLD_T = 256, KZE_FOLD_E = 4;   // lanes per workgroup, values per lane (strided by KZE_FOLD_T)
static constexpr uint32_t KZE_Q_T = 256;                      // lanes (= values) per workgroup of the quotient kernel
static constexpr uint64_t KZE_STAGE_MIN = 1ull << 16;         // values a staging buffer of the host form holds at least
static constexpr uint64_t KZE_POINT_BYTES = 96;               // one Lagrange point: affine x || y, Montgomery
static constexpr uint64_t KZE_NONE = ~0ull;                   // in_domain_index of a point outside the domain

// evaluation partials a fold launch over n values writes per vector: one per wave
HD uint32_t kze_fold_waves(uint64_t n) {
  const uint64_t per = (uint64_t)KZE_FOLD_T * KZE_FOLD_E;
  return (uint32_t)((n + per - 1) / per) * (KZE_FOLD_T / 64);
}
HD uint32_t kze_fold_blocks(uint64_t n) { return kze_fold_waves(n) / (KZE_FOLD_T / 64); }
HD uint32_t kze_quotient_blocks(uint64_t n) { return (uint32_t)((n + KZE_Q_T - 1) / KZE_Q_T); }

// z^n == 1 by log_n squarings
HD bool kze_in_domain(const Fr& z, uint32_t log_n) {
  Fr t = z;
  for (uint32_t i = 0; i < log_n; ++i) t = t.sqr();
  return t == Fr::one();
}
// the factor of sum_i e[i] (1 + z d_i): -(z^n - 1) / n outside the domain; inside, the weights select e[m] and the factor is 1
HD Fr kze_eval_scale(const Fr& z, uint32_t log_n) {
  Fr t = z;
  for (uint32_t i = 0; i < log_n; ++i) t = t.sqr();
  if (t == Fr::one()) return t;
  return (Fr::one() - t) * Fr::from_u64(1ull << log_n).inv();
}

struct KzePlan {
  uint64_t group_vectors;    // vectors per fold launch (host form: also what one staging buffer holds)
  uint64_t groups;           // fold launches (open) / staged groups (host form of either call)
  uint64_t stage_values;     // values per staging buffer of the host form (0 for the resident form)
  uint64_t msm_launches;     // msm_points_run calls: one per commitment asked for, one for the witness
  uint64_t msm_terms;        // terms of each: n
  uint64_t lagrange_bytes;   // the n Lagrange points: 96 n bytes (0 when the call needs none)
};
// commitments / witness: the call asks for them (plonk_kzg_commit_evals: commitments only)
HD KzePlan kze_plan(uint32_t log_n, uint64_t count, bool commitments, bool witness, bool host_form) {
  const uint64_t n = 1ull << log_n;
  KzePlan p;
  p.stage_values = host_form ? (n > KZE_STAGE_MIN ? n : KZE_STAGE_MIN) : 0;
  uint64_t g = KZE_GROUP;
  if (host_form && p.stage_values / n < g) g = p.stage_values / n;
  if (g > count) g = count;
  p.group_vectors = g;
  p.groups = count ? (count + g - 1) / g : 0;
  p.msm_launches = count ? (commitments ? count : 0) + (witness ? 1 : 0) : 0;
  p.msm_terms = n;
  p.lagrange_bytes = p.msm_launches ? KZE_POINT_BYTES * n : 0;
  return p;
}

// ---- a handle that holds Lagrange-basis tables (plonk_kzg_evals_tables_build) ------------------------------------------------
// The MSMs of a call run as grouped table launches (msm_batch_device over the handle's tables), KZE_TABLE_GROUP vectors per
// launch.  The commitments are grouped inside the groups the call makes its vectors resident by (`group_vectors` at a time:
// KzePlan::group_vectors for the evaluation-form calls, all M at once for a multiproof), so a staging buffer is never read
// after it was handed back.  `joined` MSMs follow the commitments in the same run, one launch each (the witness of an
// opening); `separate` MSMs are needed by the host before the next can start (D and pi of a multiproof feed the transcript)
// and are a run of their own each.  A run of ONE launch is finished on the host; a longer run queues all its launches, their
// bit sums side by side, and finishes and compresses them on the device, KZE_FINISH_CHUNK commitments per kernel launch.
static constexpr uint32_t KZE_TABLE_GROUP = 4;        // MSM_MAX_BATCH (kzg_evals.hip asserts it)
static constexpr uint32_t KZE_FINISH_CHUNK = 4096;    // commitments whose bit sums the handle holds at a time
static constexpr uint32_t KZE_FINISH_LANES = 64;      // lanes (= commitments) per workgroup of the finish kernel

struct KzeTablesPlan {
  uint64_t msms;              // commitments + joined + separate
  uint64_t group_launches;    // msm_batch_device calls
  uint32_t device_finished;   // the run of the commitments (and the joined MSMs) is finished on the device
  uint64_t finish_launches;   // finish kernel launches (= copies = synchronisations of the device finish): one per chunk
  uint64_t last_chunk;        // commitments of the last of them
};
HD KzeTablesPlan kze_tables_plan(uint64_t commitments, uint64_t group_vectors, uint64_t joined, uint64_t separate) {
  KzeTablesPlan p;
  p.msms = commitments + joined + separate;
  uint64_t run = joined;
  if (commitments) {
    const uint64_t g = group_vectors ? group_vectors : 1, full = commitments / g, rem = commitments % g;
    run += full * ((g + KZE_TABLE_GROUP - 1) / KZE_TABLE_GROUP) + (rem + KZE_TABLE_GROUP - 1) / KZE_TABLE_GROUP;
  }
  p.group_launches = run + separate;
  p.device_finished = run > 1 ? 1u : 0u;
  const uint64_t entries = commitments + joined;
  p.finish_launches = p.device_finished ? (entries + KZE_FINISH_CHUNK - 1) / KZE_FINISH_CHUNK : 0;
  p.last_chunk = p.device_finished ? entries - (p.finish_launches - 1) * KZE_FINISH_CHUNK : 0;
  return p;
}

// plonk_kzg_commit_evals' pointer checks: PLONK_ERR_ARG or PLONK_OK
HD int kze_check_commit(bool has_domain, bool has_evals, bool has_out, uint64_t count) {
  if (!has_domain) return PLONK_ERR_ARG;
  if (count > KZE_MAX_COUNT) return PLONK_ERR_ARG;
  if (count && (!has_evals || !has_out)) return PLONK_ERR_ARG;
  return PLONK_OK;
}
// plonk_kzg_open_evals' pointer checks (commitments48 and witness48 may be NULL)
HD int kze_check_open(bool has_domain, bool has_evals, bool has_point, bool has_v, bool has_evaluations, uint64_t count) {
  if (!has_domain || !has_point) return PLONK_ERR_ARG;
  if (count > KZE_MAX_COUNT) return PLONK_ERR_ARG;
  if (count && (!has_evals || !has_evaluations)) return PLONK_ERR_ARG;
  if (count > 1 && !has_v) return PLONK_ERR_ARG;
  return PLONK_OK;
}

}  // namespace plonk
