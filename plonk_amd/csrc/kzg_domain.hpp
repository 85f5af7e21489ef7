// Launchers of kzg_domain.hip: the batched group transform on XYZZ slots and the kernels around it.  Shared with the doors of
// the per-kernel tests (tests/csrc/dev_kzg_domain.hip).  Every pointer is device memory, everything is queued on the
// context's stream, nothing synchronises.  A "slot" is one XYZZ point over Fp28, KZD_SLOT_BYTES (256) bytes, 16-byte aligned;
// polynomial b of a batch lives at slots + b * stride (in slots).
#pragma once
#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "kzg_domain_core.hpp"

namespace plonk {

// w^e as GLV halves, e < 2^(tw_log - 1), w the 2^tw_log-th root of unity plonk_ntt uses; the caller frees *out_dev (hipFree)
int kzd_twiddles_create(Ctx* c, uint32_t tw_log, GlvScalar** out_dev);
// size 2^size_log per polynomial, `batch` polynomials (grid.y); tw: a table of kzd_twiddles_create for tw_log >= size_log.
// forward: decimation in frequency, natural order in, bit-reversed out.  inverse: decimation in time, bit-reversed in, natural
// out, WITHOUT the 1/size factor.  stage_launches / scalar_muls (may be NULL) are added to.
int kzd_transform(Ctx* c, void* slots, uint64_t stride, uint32_t size_log, uint32_t batch, bool inverse, const GlvScalar* tw,
                  uint32_t tw_log, uint64_t* stage_launches, uint64_t* scalar_muls);
// out[b][p] = [G[b][rev(p)] * scale] A[p], p < 2^size_log (A is shared by the batch; a zero scalar gives the identity)
int kzd_pointwise(Ctx* c, const void* A, const Fr* G, uint64_t g_stride, void* out_slots, uint64_t stride, uint32_t size_log,
                  uint32_t batch, const Fr& scale);
// slots[b][n + k] = slots[b][n - 2 - k] for k <= n - 2, the identity for k = n - 1 (n = 2^log_n, 2n slots per polynomial)
int kzd_extract(Ctx* c, void* slots, uint64_t stride, uint32_t log_n, uint32_t batch);
// out48[b][i] = the 48-byte compressed encoding of slots[b][offset + (bitrev ? rev(i) : i)], i < 2^log_n
int kzd_finish(Ctx* c, const void* slots, uint64_t stride, uint64_t offset, uint32_t log_n, uint32_t batch, bool bitrev,
               uint8_t* out48);
// slots[i] = the affine point xy96[i] (Montgomery x || y, 96 zero bytes = the identity), i < count
int kzd_load_raw(Ctx* c, const G1Affine* xy96, uint64_t count, void* slots);

// ---- the chunk steps the openings on a handle (kzg_domain.hip, kzg_cells.hip, kzg_recover.hip) share ----
// f[b] = the trimmed[b] coefficients of polys[b] (either side's memory), zero-padded to n, b < cnt
int kzd_stage(Ctx* c, Fr* f, uint64_t n, const void* const* polys, const uint64_t* trimmed, uint32_t cnt);
// from the transformed products of a chunk (2^(log_w + 1) slots per polynomial at slots + b * stride) to its 2^log_w witnesses
// per polynomial as 48 bytes each: inverse transform, kzd_extract, forward transform of the upper half, kzd_finish in
// bit-reversed order.  The two counters are added to.
int kzd_witnesses(Ctx* c, void* slots, uint64_t stride, uint32_t log_w, uint32_t cnt, const GlvScalar* tw, uint32_t tw_log,
                  uint64_t* stage_launches, uint64_t* scalar_muls, uint8_t* out48);
// an error of a call's body leaves nothing of the call queued: the copy stream, if the context has one, and the main stream
// are drained; passes rc on
int kzd_drained(Ctx* c, int rc);

struct KzdDesc {   // a resident polynomial as the scan kernel takes it
  const Fr* p;
  uint64_t len;
};
// trimmed[i] = the length of polynomial i without trailing zeros; PLONK_ERR_DATA for a coefficient that is not a canonical
// residue, then PLONK_ERR_DEGREE for more than 2^log_n coefficients.  Host form: polys are host pointers, nothing is queued.
// Resident form: a scan on the device (desc_dev: count descriptors, meta_dev: 2 x count words, both the caller's); returns
// with the stream drained.
int kzd_lengths(const char* api_fn, Ctx* c, uint32_t log_n, const void* const* polys, const uint64_t* lens, uint64_t count, bool resident,
                KzdDesc* desc_dev, unsigned long long* meta_dev, uint64_t* trimmed);
// dst48[i] (either side's memory) = the commitment of row i of f (n coefficients per row, trimmed length m[i]) through the
// ordinary commitment path; the caller has reserved the MSM scratch (msm_reserve).  The copy to dst48 is queued from `comm`,
// which the caller keeps alive until it has synchronised the stream.
int kzd_commit(Ctx* c, const Fr* f, uint64_t n, const uint64_t* m, uint32_t cnt, std::vector<uint8_t>& comm, void* dst48);

}  // namespace plonk
