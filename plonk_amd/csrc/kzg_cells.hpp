// Launchers of kzg_cells.hip: the kernels of the KZG10 cell proofs around the group transform of kzg_domain.hip.  Shared with
// the doors of the per-kernel tests (tests/csrc/dev_kzg_cells.hip).  Every pointer is device memory, everything is queued on
// the context's stream, nothing synchronises.  Slots are those of kzg_domain.hpp; n = 2^log_n, l = 2^log_cell, r = n / l.
#pragma once
#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "kzg_cells_core.hpp"

namespace plonk {

// table[u * 2r + p] = DFT_2r(a^(u))_rev(p), u < l: 2n slots, from row 0 of the context's commit-key tables; tw: the handle's
// split twiddles (kzd_twiddles_create) for tw_log >= log_n - log_cell + 1
int kzc_table_build(Ctx* c, uint32_t log_n, uint32_t log_cell, const GlvScalar* tw, uint32_t tw_log, void* table);
// g[b][u][t] = f[b][u + l (r - 1 - t)] for t <= r - 2, 0 up to 2r; f: n coefficients per polynomial, g: 2n values
int kzc_gather(Ctx* c, const Fr* f, uint32_t log_n, uint32_t log_cell, uint32_t batch, Fr* g);
// every one of the batch x vectors consecutive vectors of 2^log_size values at g (log_size <= KZC_NTT_MAX_LOG) replaced by
// its forward NTT in natural order; tw[e] = w^e, e < 2^(log_size - 1), Montgomery, w the generator plonk_ntt uses for that size
int kzc_ntt(Ctx* c, Fr* g, uint32_t log_size, uint64_t vectors, uint32_t batch, const Fr* tw);
// cells[b][k l + j] = evals[b][k + r j]
int kzc_transpose(Ctx* c, const Fr* evals, uint32_t log_n, uint32_t log_cell, uint32_t batch, Fr* cells);
// ws[b][s * 2r + p] = sum over the l / slices terms u of slice s of [G[b][u][rev(p)] * scale] table[u][p]; g_stride in values
// (2n), stride in slots (>= slices * 2r) per polynomial
int kzc_mulacc(Ctx* c, const void* table, const Fr* G, uint64_t g_stride, void* ws, uint64_t stride, uint32_t log_n, uint32_t log_cell,
               uint64_t slices, uint32_t batch, const Fr& scale);
// ws[b][p] += ws[b][s * 2r + p], s = 1 .. slices - 1 in that order
int kzc_reduce(Ctx* c, void* ws, uint64_t stride, uint32_t log_r, uint64_t slices, uint32_t batch);

// kzg_recover.hip: the body of plonk_kzg_open_cells_dev after its checks, for polynomials resident on the device whose
// trimmed lengths the caller knows (at most n, canonical coefficients).  cells may be NULL (the values are not copied out);
// the outputs go through hipMemcpyDefault, so either side of the call may own them.  *built_table is set to 1 when the call
// built the A^(u) of its cell size; plonk_kzg_cells_last reports the call.  Synchronises the stream per chunk.
struct KzgDomain;   // kzg_handle.hpp
int kzc_open_resident(KzgDomain* d, uint32_t log_cell, const void* const* polys_dev, const uint64_t* trimmed, uint64_t count, void* cells,
                      void* proofs48, void* commitments48, uint32_t* built_table);

// test hook (tests/csrc/dev_kzg_cells.hip): the slice count of the handle's next calls, 0 restores the plan's own; takes the
// context's mutex
void kzc_set_slices(plonk_kzg_domain* dom, uint64_t slices);

}  // namespace plonk
