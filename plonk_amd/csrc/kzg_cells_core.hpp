// KZG10 cell proofs (kzg_cells.hip): one proof per coset of the domain, opening all l values of the coset at once
// (Feist-Khovratovich section 3).  Everything the host decides before a kernel runs — the index maps, the slice split, the
// chunk plan, the operation counts, the argument checks — __host__ __device__ in place like kzg_domain_core.hpp: the kernels
// and the driver call these functions, tests/csrc/host_kzg_cells.cpp compiles them with g++ against the big-int model
// tests/kzg_cells_model.py.
//
// n = 2^L, l = 2^c (1 <= c <= L - 1), r = n / l, N' = 2r; w the size-n generator, phi = w^l; s_i = [tau^i] g; f_0 .. f_(n-1):
//   cell k (k < r) = { w^(k + r j) : j < l }, vanishing polynomial X^l - x_k, x_k = phi^k;  cells[k l + j] = f(w^(k + r j))
//   proof_k = commit(q_k), f = q_k (X^l - x_k) + r_k, deg r_k < l;   proofs = DFT_r(H), H_m = sum_j f_(j + (m+1) l) s_j
//   a^(u)_v = s_(u + l v) (v <= r-2), O elsewhere;  A^(u) = DFT_N'(a^(u))              per (handle, c): l x 2r slots
//   g^(u)_t = f_(u + l (r-1-t)) (t <= r-2), 0 elsewhere;  G^(u) = NTT_N'(g^(u))
//   P_i = sum_(u < l) [G^(u)_i / N'] A^(u)_i;  c = DFT_N'^-1(P);  H_m = c_(r-2-m) (m <= r-2), H_(r-1) = O
// The orders are those of kzg_domain_core.hpp with n replaced by r: A^(u) stays bit-reversed, P is made at bit-reversed
// positions p (i = rev(p)), c comes out in natural order in the lower half of the first 2r slots of a polynomial, H goes to
// the upper half, is transformed there, and the finishing kernel reads slot r + rev(k).
// The sum over u is cut into S slices of l / S consecutive u: lane (p, s) accumulates its slice in registers and stores one
// partial at slot s * 2r + p of the polynomial's workspace; the reduction adds the partials s = 1 .. S-1 IN THAT ORDER onto
// the partial of slice 0, which is the slot the inverse transform reads.
#pragma once
#include <stdint.h>

#include "../../include/plonk_hip.h"
#include "field.cuh"
#include "kzg_domain_core.hpp"

namespace plonk {

static constexpr uint64_t KZC_FILL_LANES = 65536;   // one wave on each of the chip's 1024 SIMDs
static constexpr uint32_t KZC_NTT_MAX_LOG = 11;     // the scalar transforms of a polynomial are one launch up to 2r = 2048 (64 KiB of LDS)
static constexpr uint32_t KZC_NTT_LANES = 256;

HD int kzc_check_cell(uint32_t log_n, uint32_t log_cell) {
  return (log_cell < 1 || log_cell >= log_n) ? PLONK_ERR_ARG : PLONK_OK;
}
// the key point a^(u)_v reads (KZD_NONE: the identity), v < 2r
HD uint64_t kzc_a_src(uint32_t log_cell, uint64_t r, uint64_t u, uint64_t v) { return v + 2 <= r ? u + (v << log_cell) : KZD_NONE; }
// the coefficient g^(u)_t reads (KZD_NONE: zero), t < 2r
HD uint64_t kzc_g_src(uint32_t log_cell, uint64_t r, uint64_t u, uint64_t t) {
  const uint64_t v = kzd_g_src(r, t);
  return v == KZD_NONE ? KZD_NONE : u + (v << log_cell);
}
// cells[kzc_cell_dst] = evaluations[i]: i = k + r j -> k l + j
HD uint64_t kzc_cell_dst(uint32_t log_n, uint32_t log_cell, uint64_t i) {
  const uint64_t r = 1ull << (log_n - log_cell);
  return ((i & (r - 1)) << log_cell) + (i >> (log_n - log_cell));
}
// the first term of slice s and the terms per slice
HD uint64_t kzc_slice_terms(uint32_t log_cell, uint64_t slices) { return (1ull << log_cell) / slices; }
HD uint64_t kzc_slice_first(uint32_t log_cell, uint64_t slices, uint64_t s) { return s * kzc_slice_terms(log_cell, slices); }
// the slot of partial (s, p) in a polynomial's workspace
HD uint64_t kzc_partial_slot(uint64_t r, uint64_t s, uint64_t p) { return s * 2 * r + p; }

struct KzcPlan {
  uint64_t slices;           // S: a power of two dividing l
  uint64_t chunk_polys;      // polynomials per chunk (the last chunk may be shorter)
  uint64_t chunks;
  uint64_t ws_bytes;         // point workspace: S * 2r slots per polynomial of a chunk
  uint64_t table_bytes;      // the A^(u) of this cell size: 2n slots
  uint64_t stage_launches;   // group-FFT stage launches of the call: (2 log r + 1) per chunk
  uint64_t scalar_muls;      // per polynomial 2n in the accumulate + the butterflies with a twiddle != 1
};
// forced_slices != 0 (tests): that S, when it is a power of two <= l; otherwise the smallest S for which 2r * S * (the
// polynomials a chunk could hold at most) covers KZC_FILL_LANES, at most l
HD KzcPlan kzc_plan(uint32_t log_n, uint32_t log_cell, uint64_t count, uint64_t cap_bytes, uint64_t forced_slices) {
  const uint64_t n = 1ull << log_n, l = 1ull << log_cell, r = n >> log_cell;
  const uint32_t log_r = log_n - log_cell;
  KzcPlan p;
  uint64_t polys = count < KZD_MAX_CHUNK ? count : KZD_MAX_CHUNK;
  if (polys < 1) polys = 1;
  uint64_t S = 1;
  while (S < l && 2 * r * S * polys < KZC_FILL_LANES) S <<= 1;
  if (forced_slices && forced_slices <= l && !(forced_slices & (forced_slices - 1))) S = forced_slices;
  const uint64_t per_poly = S * 2 * r * KZD_SLOT_BYTES;
  uint64_t chunk = cap_bytes / per_poly;
  if (chunk < 1) chunk = 1;
  if (chunk > KZD_MAX_CHUNK) chunk = KZD_MAX_CHUNK;
  if (chunk > count) chunk = count;
  p.slices = S;
  p.chunk_polys = chunk;
  p.chunks = count ? (count + chunk - 1) / chunk : 0;
  p.ws_bytes = chunk * per_poly;
  p.table_bytes = 2 * n * KZD_SLOT_BYTES;
  p.stage_launches = p.chunks * (2ull * log_r + 1);
  p.scalar_muls = count * (2 * n + kzd_transform_muls(log_r + 1) + kzd_transform_muls(log_r));
  return p;
}

}  // namespace plonk
