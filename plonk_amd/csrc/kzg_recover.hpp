// Launchers of kzg_recover.hip: the four kernels of the KZG10 cell recovery around the transforms of ntt.hip.  Shared with the
// doors of the per-kernel tests (tests/csrc/dev_kzg_recover.hip).  Every pointer is device memory, everything is queued on
// the context's stream, nothing synchronises.  n = 2^log_n, l = 2^log_cell, r = n / l <= 2^KZR_MAX_LOG_R.
#pragma once
#include "plonk_internal.hpp"
#include "kzg_recover_core.hpp"

namespace plonk {

// zdom[k] = Z_r(phi^k), zcoset[k] = Z_r(7^l phi^k), k < r, Z_r(Y) = prod_(m < nmiss) (Y - pw[miss[m]]); pw[i] = phi^i, i < r
// (poly_power_array); miss: nmiss distinct indexes < r (may be NULL when nmiss == 0)
int kzr_vanish(Ctx* c, const Fr* pw, const uint32_t* miss, uint32_t nmiss, uint32_t log_n, uint32_t log_cell, Fr* zdom, Fr* zcoset);
// out[b][k + r j] = vecs[b][slot[k] l + j] * zdom[k], 0 where slot[k] < 0; vecs: device table of `batch` pointers to packed
// cell values; slot: r entries
int kzr_scatter(Ctx* c, const Fr* const* vecs, const int32_t* slot, const Fr* zdom, uint32_t log_n, uint32_t log_cell, uint32_t batch, Fr* out);
// v[b][i] *= zinv[i mod r], i < n
int kzr_divide(Ctx* c, Fr* v, const Fr* zinv, uint32_t log_n, uint32_t log_cell, uint32_t batch);
// flags[b] = 1 when one of coeffs[b][max_len .. n) is not zero, else 0 (max_len <= n; an empty range gives 0)
int kzr_tail(Ctx* c, const Fr* coeffs, uint32_t log_n, uint64_t max_len, uint32_t batch, int32_t* flags);

}  // namespace plonk
