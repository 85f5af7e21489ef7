// Launchers of kzg_cell_verify.hip: the kernels of the KZG10 cell verifier.  Shared with the doors of the per-kernel tests
// (tests/csrc/dev_kzg_cell_verify.hip).  Every pointer is device memory, everything is queued on the context's stream,
// nothing synchronises.  l = 2^log_cell values per cell; the layouts are those of kzg_cell_verify_core.hpp.
#pragma once
#include "plonk_internal.hpp"
#include "kzg_cell_verify_core.hpp"

namespace plonk {

// out[i] = point i of the context's commit key as x || y (Montgomery, 96 bytes), i < count <= srs_n
int kzv_key_copy(Ctx* c, uint64_t count, G1Affine* out);
// out[i][j] = l_inv * weight_i * winv[cell_index[i]]^j * (size-l inverse DIT of values[i])_j; weights == nullptr: weight 1.
// winv[k] = w^(-k); itw[e] = w_l^(-e), e < l / 2.  An item with a value that is not a canonical residue gets flags[i] = 1
// (the caller zeroes flags) and a row of zeros.
int kzv_twist(Ctx* c, const Fr* values, const uint32_t* cell_index, const Fr* weights, uint64_t count, uint32_t log_cell,
              const Fr* winv, const Fr* itw, Fr* out, uint32_t* flags);
// sc[8 j ..] = the canonical words of -(sum_i rows[i][j]), ids[j] = j, j < l: kzv_colsum_passes(count) launches, the partial
// rows alternating between part0 and part1 (each kzv_colsum_slices(count) x l values)
int kzv_colsum(Ctx* c, const Fr* rows, uint64_t count, uint32_t log_cell, Fr* part0, Fr* part1, uint32_t* sc, uint32_t* ids);
// the terms [0, K) (rho^i, pi_i), [K, K + M) (W_c, C_c) and [K + M, 2K + M) (rho^i x_k, pi_i) of kzv_layout; pw[i] = rho^i
int kzv_weights(Ctx* c, const Fr* pw, const uint32_t* cell_index, const Fr* xk, const uint32_t* perm, const uint32_t* off, uint64_t K,
                uint64_t M, uint32_t log_cell, uint32_t* sc, uint32_t* ids);
// pairs[2 i] = pi_i, pairs[2 i + 1] = C_(c_i) + x_(k_i) pi_i - sum_j coeffs[i][j] s_j, pre[i] = 0 — or pre[i] =
// PLONK_ERR_DATA (flags[i]) / PLONK_ERR_POINT (a point of the item did not decode) and the pairs left alone; pts / kind: the
// point table of kzv_layout
int kzv_cell_sums(Ctx* c, const Fr* coeffs, const uint32_t* commitment_index, const uint32_t* cell_index, const Fr* xk,
                  const uint32_t* flags, const G1Affine* pts, const int32_t* kind, uint64_t K, uint64_t M, uint32_t log_cell, G1* pairs,
                  int32_t* pre);

}  // namespace plonk
