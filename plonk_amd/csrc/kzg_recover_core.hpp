// KZG10 cell recovery (kzg_recover.hip): a polynomial, its missing cells and their proofs rebuilt from a subset of its cells.
// Everything the host decides before a kernel runs — the index maps, the chunk plan, the counts, the argument checks —
// __host__ __device__ in place like kzg_cells_core.hpp: the kernels and the driver call these functions,
// tests/csrc/host_kzg_recover.cpp compiles them with g++ against the big-int model tests/kzg_recover_model.py.
//
// Notation of kzg_cells_core.hpp: n = 2^L, l = 2^c, r = n / l, w the size-n generator, phi = w^l, cell k = { w^(k + r j) }, the
// y with y^l = phi^k.  Given: a distinct cells (a l values per polynomial, packed in the order of cell_ids) of a polynomial f
// of at most d = max_len <= a l coefficients.  M = the r - a missing cells.
//   Z(X) = Z_r(X^l), Z_r(Y) = prod_(m in M) (Y - phi^m): constant on a cell, Z(w^(k + r j)) = Z_r(phi^k), and periodic on the
//     coset of 7, Z(7 w^i) = Z_r(7^l phi^(i mod r)), never zero there (7^n != 1).  Only these 2r values are made.
//   E = the values with 0 in the missing cells: E Z = f Z on the domain, deg(f Z) < d + l |M| <= n, so the inverse transform of
//     E Z is P = f Z exactly;  f = coset^-1( coset(P)_i / Z_r(7^l phi^(i mod r)) ).
//   The result g has g_i = 0 for all i >= d iff the values come from a polynomial of at most d coefficients (g Z = P on n points,
//     both of degree < n): the consistency verdict.  With a l = d there is no redundancy and every input is consistent.
// r <= 2^KZR_MAX_LOG_R: Z_r is evaluated by direct products, 2r |M| multiplications.
#pragma once
#include <stdint.h>

#include "../../include/plonk_hip.h"
#include "field.cuh"
#include "kzg_domain_core.hpp"
#include "kzg_cells_core.hpp"

namespace plonk {

static constexpr uint32_t KZR_MAX_LOG_R = 11;      // r <= 2048: above it Z_r wants a product tree
static constexpr uint32_t KZR_POLY_ARRAYS = 3;     // length-n arrays of workspace per polynomial of a chunk
static constexpr int32_t KZR_MISSING = -1;         // slot table: the cell is not among the given ones
static constexpr uint32_t KZR_VANISH_SLICES = 64;  // lanes per point of the vanish kernel: slice s takes the factors s, s + 64, ...
HD uint32_t kzr_vanish_first(uint32_t s) { return s; }

// the packed value position i of the natural-order array reads: i = k + r j -> slot[k] l + j (KZD_NONE: zero, a missing cell)
HD uint64_t kzr_scatter_src(uint32_t log_n, uint32_t log_cell, uint64_t i, const int32_t* slot) {
  const uint32_t log_r = log_n - log_cell;
  const int32_t s = slot[i & ((1ull << log_r) - 1)];
  return s < 0 ? KZD_NONE : ((uint64_t)s << log_cell) + (i >> log_r);
}
// the entry of Zdom / Zcoset^-1 element i of a length-n array takes
HD uint64_t kzr_period(uint32_t log_n, uint32_t log_cell, uint64_t i) { return i & ((1ull << (log_n - log_cell)) - 1); }
// the exponent e of point p < 2r of the vanish kernel: phi^e for p < r, 7^l phi^e above
HD uint64_t kzr_point_exp(uint32_t log_r, uint64_t p) { return p & ((1ull << log_r) - 1); }
HD bool kzr_point_on_coset(uint32_t log_r, uint64_t p) { return (p >> log_r) != 0; }
// the coefficients the tail kernel looks at: [first, n)
HD uint64_t kzr_tail_first(uint64_t max_len) { return max_len; }

// plonk_kzg_recover_cells' argument checks (all PLONK_ERR_ARG); cell_ids may be NULL only with count == 0
HD int kzr_check_args(bool has_domain, uint32_t log_n, uint32_t log_cell, uint64_t count, const uint32_t* cell_ids, uint64_t available,
                      bool has_values, bool values_all_set, uint64_t max_len, bool any_output) {
  if (!has_domain) return PLONK_ERR_ARG;
  if (kzc_check_cell(log_n, log_cell)) return PLONK_ERR_ARG;
  const uint32_t log_r = log_n - log_cell;
  if (log_r > KZR_MAX_LOG_R) return PLONK_ERR_ARG;
  if (count > KZD_MAX_COUNT) return PLONK_ERR_ARG;
  const uint64_t r = 1ull << log_r;
  if (!available || available > r) return PLONK_ERR_ARG;
  if (cell_ids) {
    uint64_t seen[(1u << KZR_MAX_LOG_R) / 64] = {};
    for (uint64_t i = 0; i < available; ++i) {
      const uint32_t k = cell_ids[i];
      if (k >= r || ((seen[k >> 6] >> (k & 63)) & 1)) return PLONK_ERR_ARG;
      seen[k >> 6] |= 1ull << (k & 63);
    }
  }
  if (count && (!cell_ids || !has_values || !values_all_set)) return PLONK_ERR_ARG;
  if (!max_len || max_len > (1ull << log_n)) return PLONK_ERR_ARG;
  if (!any_output) return PLONK_ERR_ARG;
  return PLONK_OK;
}
// too few cells for that length (after the state checks and count == 0)
HD int kzr_check_degree(uint32_t log_cell, uint64_t available, uint64_t max_len) {
  return max_len > (available << log_cell) ? PLONK_ERR_DEGREE : PLONK_OK;
}

struct KzrPlan {
  uint64_t missing;        // r - a
  uint64_t chunk_polys;    // polynomials per chunk (the last chunk may be shorter)
  uint64_t chunks;
  uint64_t ws_bytes;       // KZR_POLY_ARRAYS length-n arrays per polynomial of a chunk
  uint64_t passes;         // 1: the coefficients of the only chunk wait for the verdict; 2: several chunks, made again after it
  uint64_t transforms;     // size-n transforms: 3 per polynomial and pass, + 1 when cell values (or proofs, which bring them) are asked for
  uint64_t vanish_muls;    // 2r |M|
};
// kzd_plan's rule over the polynomial workspace: what fits under the cap, at least one, at most KZD_MAX_CHUNK
HD KzrPlan kzr_plan(uint32_t log_n, uint32_t log_cell, uint64_t count, uint64_t available, uint64_t cap_bytes, bool want_values) {
  const uint64_t n = 1ull << log_n, r = n >> log_cell, per_poly = KZR_POLY_ARRAYS * n * sizeof(Fr);
  KzrPlan p;
  uint64_t chunk = cap_bytes / per_poly;
  if (chunk < 1) chunk = 1;
  if (chunk > KZD_MAX_CHUNK) chunk = KZD_MAX_CHUNK;
  if (chunk > count) chunk = count;
  p.missing = r - available;
  p.chunk_polys = chunk;
  p.chunks = count ? (count + chunk - 1) / chunk : 0;
  p.ws_bytes = chunk * per_poly;
  p.passes = p.chunks > 1 ? 2 : 1;
  p.transforms = count * (3 * p.passes + (want_values ? 1 : 0));
  p.vanish_muls = 2 * r * p.missing;
  return p;
}

}  // namespace plonk
