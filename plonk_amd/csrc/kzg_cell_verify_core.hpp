// KZG10 cell verification (kzg_cell_verify.hip): what the host decides before a kernel runs — the argument checks, the
// packing of the twist kernel, the passes of the column sums, the term and point layout of the two folded sums, the counting
// sort of the commitment indexes, the plan plonk_kzg_cell_verifier_last reports and the batch challenge — __host__ __device__
// in place like kzg_cells_core.hpp: the kernels and the driver call these functions, tests/csrc/host_kzg_cell_verify.cpp
// compiles them with g++ against the big-int model tests/kzg_cell_verify_model.py.
//
// n = 2^L, l = 2^c, r = n / l; w the size-n generator, x_k = w^(l k), s_j = [tau^j] g.  Items i < K: (c_i < M, k_i < r, l
// values v_i, a proof pi_i); weights rho^i:
//   c_ij = w^(-k_i j) * (size-l inverse NTT of v_i)_j                  the remainder of cell k_i from its values
//   R_j  = sum_i rho^i c_ij          W_c = sum_(i : c_i = c) rho^i     L = sum_i rho^i pi_i
//   Rhs  = sum_c W_c C_c + sum_i (rho^i x_(k_i)) pi_i - sum_(j < l) R_j s_j
//   accept iff e(L, [tau^l] h) == e(Rhs, h)
// Per item (weight 1): A_i = pi_i, B_i = C_(c_i) + x_(k_i) pi_i - sum_j c_ij s_j, e(A_i, [tau^l] h) == e(B_i, h).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/plonk_hip.h"
#include "field.cuh"
#include "transcript.hpp"
#include "kzg_cells_core.hpp"
#include "msm_points_core.hpp"

namespace plonk {

static constexpr uint32_t KZV_MAX_LOG_N = 20;
static constexpr uint64_t KZV_MAX_ITEMS = 1ull << 20;          // items per call
static constexpr uint64_t KZV_MAX_VALUES = 1ull << 25;         // count * l per call (1 GiB of values)
static constexpr uint64_t KZV_MAX_COMMITMENTS = 65536;
static constexpr uint32_t KZV_LANES = 256;                     // kzv_twist_kernel's workgroup
static constexpr uint32_t KZV_PACK_MAX_LOG = 6;                // cells of up to 64 values share a workgroup, one item per l lanes
static constexpr uint32_t KZV_COLSUM_ROWS = 64;                // rows one lane of kzv_colsum_kernel adds
static constexpr uint32_t KZV_COLSUM_LANES = 64;
static constexpr uint32_t KZV_SUMS_LANES = 64;                 // kzv_cell_sums_kernel: one wave per item

// is the value (Montgomery limbs of the ABI) a canonical residue, < q?
HD bool kzv_canonical(const Fr& v) {
  for (int i = 7; i >= 0; --i) {
    if (v.l[i] < FrP::MOD[i]) return true;
    if (v.l[i] > FrP::MOD[i]) return false;
  }
  return false;   // == q
}

// plonk_kzg_cell_verifier_create: log_n in [2, 20], log_cell in [1, min(log_n - 1, KZC_NTT_MAX_LOG)]
HD int kzv_check_shape(uint32_t log_n, uint32_t log_cell) {
  if (log_n < 2 || log_n > KZV_MAX_LOG_N) return PLONK_ERR_ARG;
  if (log_cell < 1 || log_cell >= log_n || log_cell > KZC_NTT_MAX_LOG) return PLONK_ERR_ARG;
  return PLONK_OK;
}
// the counts and the indexes of a call (the pointers are looked at by the entry point)
HD int kzv_check_items(uint32_t log_n, uint32_t log_cell, uint64_t ncommitments, const uint32_t* commitment_index,
                       const uint32_t* cell_index, uint64_t count) {
  if (count > KZV_MAX_ITEMS || (count << log_cell) > KZV_MAX_VALUES || ncommitments > KZV_MAX_COMMITMENTS) return PLONK_ERR_ARG;
  const uint64_t r = 1ull << (log_n - log_cell);
  for (uint64_t i = 0; i < count; ++i)
    if (commitment_index[i] >= ncommitments || cell_index[i] >= r) return PLONK_ERR_ARG;
  return PLONK_OK;
}

// kzv_twist_kernel: items per workgroup, lanes per item, the number of workgroups and the LDS bytes of one
HD uint32_t kzv_items_per_group(uint32_t log_cell) { return log_cell <= KZV_PACK_MAX_LOG ? KZV_LANES >> log_cell : 1u; }
HD uint32_t kzv_lanes_per_item(uint32_t log_cell) { return log_cell <= KZV_PACK_MAX_LOG ? 1u << log_cell : KZV_LANES; }
HD uint64_t kzv_twist_groups(uint32_t log_cell, uint64_t count) {
  const uint64_t per = kzv_items_per_group(log_cell);
  return (count + per - 1) / per;
}
HD uint64_t kzv_twist_lds_bytes(uint32_t log_cell) { return (uint64_t)kzv_items_per_group(log_cell) * (32ull << log_cell); }

// kzv_colsum_kernel: pass p turns `rows` rows into ceil(rows / KZV_COLSUM_ROWS); the last pass (one row out) writes the terms
HD uint64_t kzv_colsum_slices(uint64_t rows) { return (rows + KZV_COLSUM_ROWS - 1) / KZV_COLSUM_ROWS; }
HD uint32_t kzv_colsum_passes(uint64_t rows) {
  uint32_t p = 1;
  while (rows > KZV_COLSUM_ROWS) {
    rows = kzv_colsum_slices(rows);
    ++p;
  }
  return p;
}

// The point table [s_0 .. s_(l-1) | C_0 .. C_(M-1) | pi_0 .. pi_(K-1)] and the terms of the two sums over it:
//   L   terms [0, K)                    rho^i            pi_i
//   Rhs terms [K, K + M)                W_c              C_c
//             [K + M, 2K + M)           rho^i x_(k_i)    pi_i
//             [2K + M, 2K + M + l)      -R_j             s_j
struct KzvLayout {
  uint64_t pt_commitment, pt_proof, points;
  uint64_t term_w, term_x, term_r, terms;
};
HD KzvLayout kzv_layout(uint32_t log_cell, uint64_t M, uint64_t K) {
  const uint64_t l = 1ull << log_cell;
  KzvLayout t;
  t.pt_commitment = l;
  t.pt_proof = l + M;
  t.points = l + M + K;
  t.term_w = K;
  t.term_x = K + M;
  t.term_r = 2 * K + M;
  t.terms = 2 * K + M + l;
  return t;
}

// perm: the items ordered by commitment index (stable), off[c] .. off[c + 1]: the items of commitment c; off has M + 1 entries
HD void kzv_counting_sort(const uint32_t* commitment_index, uint64_t K, uint64_t M, uint32_t* perm, uint32_t* off) {
  for (uint64_t c = 0; c <= M; ++c) off[c] = 0;
  for (uint64_t i = 0; i < K; ++i) ++off[commitment_index[i] + 1];
  for (uint64_t c = 0; c < M; ++c) off[c + 1] += off[c];
  for (uint64_t i = 0; i < K; ++i) perm[off[commitment_index[i]]++] = (uint32_t)i;   // off[c] has moved to the end of c
  for (uint64_t c = M; c > 0; --c) off[c] = off[c - 1];
  off[0] = 0;
}

struct KzvPlan {
  uint64_t transforms, twist_groups;
  uint32_t colsum_passes;
  uint64_t msm_terms_left, msm_terms_right;
  uint32_t msm_path_left, msm_path_right;   // 0 per-term, 1 buckets (msm_points' own rule)
  uint64_t scalar_muls;                     // the each path: K (l + 1)
  uint64_t msm_terms_info;                  // plonk_verify_info.msm_terms of the folded call
};
// min_left / min_right: the test door's forced thresholds (0: msm_points' own)
HD KzvPlan kzv_plan(uint32_t log_cell, uint64_t M, uint64_t K, bool each, uint32_t min_left, uint32_t min_right) {
  const uint64_t l = 1ull << log_cell;
  KzvPlan p;
  p.transforms = K;
  p.twist_groups = kzv_twist_groups(log_cell, K);
  p.colsum_passes = each ? 0 : kzv_colsum_passes(K);
  p.msm_terms_left = each ? 0 : K;
  p.msm_terms_right = each ? 0 : M + K + l;
  p.msm_path_left = each ? 0 : mp_plan(p.msm_terms_left, 0, 0, min_left).path;
  p.msm_path_right = each ? 0 : mp_plan(p.msm_terms_right, 0, 0, min_right).path;
  p.scalar_muls = each ? K * (l + 1) : 0;
  p.msm_terms_info = 2 * K + M + l;
  return p;
}

// rho of plonk_kzg_verify_cells on a fresh Transcript::new(label); values: K x l Montgomery residues (canonical)
HD Fr kzv_challenge(const uint8_t* label, size_t label_len, uint32_t log_n, uint32_t log_cell, const uint8_t opening_key[240],
                    const uint8_t* commitments48, uint64_t M, const uint32_t* commitment_index, const uint32_t* cell_index,
                    const uint64_t* values, const uint8_t* proofs48, uint64_t K, uint8_t* cell_bytes /* l x 32 scratch */) {
  const uint64_t l = 1ull << log_cell;
  Transcript tr(label, label_len);
  tr.append_message("dom-sep", (const uint8_t*)"kzg10-cell-batch-check-v1", 25);
  tr.append_u64("log-n", log_n);
  tr.append_u64("log-cell", log_cell);
  tr.append_u64("commitments", M);
  tr.append_u64("items", K);
  tr.append_message("opening-key", opening_key, 240);
  for (uint64_t c = 0; c < M; ++c) tr.append_commitment("commitment", commitments48 + 48 * c);
  for (uint64_t i = 0; i < K; ++i) {
    tr.append_u64("commitment-index", commitment_index[i]);
    tr.append_u64("cell-index", cell_index[i]);
    for (uint64_t j = 0; j < l; ++j) {
      Fr v;
      memcpy(v.l, values + 4 * (i * l + j), 32);
      fr_to_bytes(v, cell_bytes + 32 * j);
    }
    tr.append_message("cell", cell_bytes, 32 * l);
    tr.append_commitment("cell-proof", proofs48 + 48 * i);
  }
  return tr.challenge_scalar("cell-batch-challenge");
}

}  // namespace plonk
