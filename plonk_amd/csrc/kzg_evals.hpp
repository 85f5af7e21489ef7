// Launchers of kzg_evals.hip: the scalar stage of KZG10 in evaluation form and the Lagrange points it commits over.  Shared
// with the doors of the per-kernel tests (tests/csrc/dev_kzg_evals.hip).  Every pointer is device memory unless said
// otherwise, everything is queued on the context's stream, nothing synchronises (kze_lagrange_points does: it frees its
// workspace).
#pragma once
#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "kzg_evals_core.hpp"

namespace plonk {

struct KzeMeta {              // what the host reads back before anything else of a call is queued
  unsigned long long m;       // the lane with w^m == z (KZE_NONE: none)
  unsigned long long bad;     // != 0: a resident value is not a canonical residue
};

// den[i] = w^i - z, i < n = 2^log_n; meta->m = the lane where that is zero (the caller presets KZE_NONE)
int kze_denominators(Ctx* c, uint32_t log_n, const Fr& z, Fr* den, KzeMeta* meta);
// meta->bad |= 1 when one of the n values of vecs[first .. first + cnt) is >= q (any cnt: a launch per 32768 vectors)
int kze_scan(Ctx* c, const Fr* const* vecs, uint32_t first, uint32_t cnt, uint64_t n, KzeMeta* meta);

struct KzeFoldArgs {
  const Fr* const* vecs;   // device table of the call's vectors; the launch covers vecs[first, first + count), count <= KZE_GROUP
  const void* vpow;        // v^j, j < (all vectors of the call), twiddle form (Fr29Slot, poly_kzg_powers)
  uint32_t first, count;
  uint64_t n;
  int accumulate;          // 0: fold[i] = sum; 1: fold[i] += sum
  const Fr* inv;           // 1 / (w^i - z), 0 at lane m
  uint64_t m;              // KZE_NONE: z outside the domain
  Fr* fold;                // n
  Fr* partial;             // [count][kze_fold_waves(n)]
  Fr z, scale;             // scale: kze_eval_scale
};
// fold += sum_j v^j e_j and evals[j] = y_(first + j), j < count: one pass over the values
int kze_fold_eval(Ctx* c, const KzeFoldArgs& a, Fr* evals);
// q[i] = (fold[i] - Y) inv[i]; with m != KZE_NONE also q[m] = -w^(-m) sum_(i != m) q[i] w^i (qpart: kze_quotient_blocks(n) values)
int kze_quotient(Ctx* c, uint32_t log_n, const Fr* fold, const Fr* inv, const Fr& Y, uint64_t m, Fr* q, Fr* qpart);
// out[i] = [L_i(tau)] G, i < n, as affine x || y (96 zero bytes: the identity) from row 0 of the context's commit-key tables
// (n points are enough); tw: kzd_twiddles_create's table for tw_log > log_n.  Returns with the stream synchronised.
int kze_lagrange_points(Ctx* c, uint32_t log_n, const GlvScalar* tw, uint32_t tw_log, G1Affine* out);

// every one of the n values (4 limbs each) of the `count` HOST vectors is a canonical residue
bool kze_host_canonical(const void* const* vecs, uint64_t count, uint64_t n);

// What kzg_multiproof.hip shares with the evaluation-form calls of the handle (kzg_handle.hpp): the resident Lagrange points
// (built by whichever call commits first; *built = 1 when this one did) and the commitment over them, sum_i s[i] [L_i(tau)] G
// as 48 compressed bytes (returns with the stream synchronised; plonk_ctx_last_msm_points keeps reporting the caller's own
// last call).
struct KzgDomain;
int kze_points_ready(KzgDomain* d, uint32_t* built);
const G1Affine* kze_points(KzgDomain* d);   // the n resident points once kze_points_ready returned PLONK_OK (kzg_many.hip builds its window tables over them)
int kze_commit_values(KzgDomain* d, const Fr* s, uint8_t out48[48]);
// the same for `count` resident vectors, out48[48 j] for s[j]: one after the other on a handle without tables, as ONE run of
// grouped table launches on a handle that holds them (kzg_evals_core.hpp kze_tables_plan)
int kze_commit_list(KzgDomain* d, const Fr* const* s, uint64_t count, uint8_t* out48);
// a call that may use the handle's tables starts here: what plonk_kzg_evals_tables_last reports of "the last call" is
// counted from this point on (kze_commit_values / kze_commit_list add to it)
void kze_tables_call_begin(KzgDomain* d);

// kze_finish_kernel: out48[48 i] = the compressed commitment of bits[MSM_BIT_SUMS i ...], i < count — the chain of
// finish_bit_sums (rb row bits, bitpos: 2 W - S), the affine normalisation and G1Affine::to_bytes, one lane per commitment
int kze_finish(Ctx* c, const G1* bits, uint32_t count, int rb, bool bitpos, uint8_t* out48);

}  // namespace plonk
