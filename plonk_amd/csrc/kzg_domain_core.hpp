// KZG10 openings over a whole domain (kzg_domain.hip): everything the host decides before a kernel runs — the index maps of
// the six steps, the twiddle a butterfly takes, the chunk plan, the workspace and the operation counts, the argument checks.
// Like kzg_core.hpp everything is __host__ __device__ in place (the HD convention of field.cuh): the kernels and the handle
// call these functions, tests/csrc/host_kzg_domain.cpp compiles them with g++ against the big-int model
// tests/kzg_domain_model.py.
//
// f has coefficients f_0 .. f_(n-1), n = 2^L, N = 2n, s_i = [tau^i] g, w the generator of the size-n domain:
//   a_l = s_l (l <= n-2), O elsewhere;  A = DFT_N(a)                       once per handle
//   g_t = f_(n-1-t) (t <= n-2), 0 elsewhere;  G = NTT_N(g)
//   P_i = [G_i / N] A_i;  c = DFT_N^-1(P) (the 1/N of the inverse rides on the scalars of this step)
//   h_k = c_(n-2-k) (k <= n-2), h_(n-1) = O;  pi = DFT_n(h)                 pi_i = the witness at w^i
// The forward transforms are decimation in frequency (natural order in, bit-reversed out), the inverse is decimation in
// time (bit-reversed in, natural out): A stays bit-reversed, P_p = [G_rev(p) / N] A_rev(p) is made in that order, c comes
// out in natural order in the LOWER half of the 2n slots, h is written to the UPPER half, transformed there, and the
// finishing kernel reads slot n + rev(i).  No pass only permutes.
#pragma once
#include <stdint.h>

#include "../../include/plonk_hip.h"
#include "field.cuh"

namespace plonk {

static constexpr uint32_t KZD_MIN_LOG = 1, KZD_MAX_LOG = 20;
static constexpr uint64_t KZD_MAX_COUNT = 65536;              // polynomials per call, as plonk_kzg_open
static constexpr uint64_t KZD_SLOT_BYTES = 256;               // one XYZZ point over Fp28: 4 coordinates of 64 B
static constexpr uint64_t KZD_WS_CAP_DEFAULT = 2ull << 30;    // bytes of point workspace a call may hold (one polynomial is always allowed)
static constexpr uint64_t KZD_MAX_CHUNK = 4096;               // polynomials per chunk: grid.y of the batched launches
static constexpr uint32_t KZD_LANES = 64;                     // one wave per workgroup in every point kernel
static constexpr uint64_t KZD_NONE = ~0ull;

HD uint64_t kzd_rev(uint64_t i, uint32_t bits) {
  uint64_t r = 0;
  for (uint32_t b = 0; b < bits; ++b) r |= ((i >> b) & 1ull) << (bits - 1 - b);
  return r;
}
// g_t = f[kzd_g_src(n, t)], or 0 for KZD_NONE; t < 2n
HD uint64_t kzd_g_src(uint64_t n, uint64_t t) { return t + 2 <= n ? n - 1 - t : KZD_NONE; }
// h_k = c[kzd_h_src(n, k)], or the identity for KZD_NONE; k < n
HD uint64_t kzd_h_src(uint64_t n, uint64_t k) { return k + 2 <= n ? n - 2 - k : KZD_NONE; }

// The twiddle of lane j (< half) of the stage with butterfly span `half` of a size-2^size_log transform, read from a table
// of the 2^(tw_log - 1) powers w^e, e < 2^(tw_log - 1), of a primitive 2^tw_log-th root (size_log <= tw_log).  Returns the
// table index; *negate says that the factor is MINUS that entry (the inverse: w^-e = -w^(T - e), T = 2^(tw_log - 1)).
// KZD_NONE: the factor is 1 and the butterfly multiplies nothing.
HD uint64_t kzd_twiddle(uint32_t size_log, uint64_t half, uint64_t j, uint32_t tw_log, bool inverse, bool* negate) {
  const uint64_t e = (j * ((1ull << size_log) / (2 * half))) << (tw_log - size_log);
  *negate = false;
  if (!e) return KZD_NONE;
  if (!inverse) return e;
  *negate = true;
  return (1ull << (tw_log - 1)) - e;
}
// butterflies of one stage that multiply (j != 0), and of a whole transform
HD uint64_t kzd_stage_muls(uint32_t size_log, uint64_t half) { return (1ull << size_log) / 2 - (1ull << size_log) / (2 * half); }
HD uint64_t kzd_transform_muls(uint32_t size_log) {
  uint64_t s = 0;
  for (uint64_t half = 1; half < (1ull << size_log); half <<= 1) s += kzd_stage_muls(size_log, half);
  return s;
}

struct KzdPlan {
  uint64_t chunk_polys;      // polynomials per chunk (the last chunk may be shorter)
  uint64_t chunks;
  uint64_t ws_bytes;         // point workspace: 2n slots per polynomial of a chunk
  uint64_t stage_launches;   // group-FFT stage launches of the call: (2 L + 1) per chunk
  uint64_t scalar_muls;      // full-width scalar multiplications issued: per polynomial N pointwise + the butterflies with a twiddle != 1
};
HD KzdPlan kzd_plan(uint32_t log_n, uint64_t count, uint64_t cap_bytes) {
  const uint64_t n = 1ull << log_n, per_poly = 2 * n * KZD_SLOT_BYTES;
  KzdPlan p;
  uint64_t chunk = cap_bytes / per_poly;
  if (chunk < 1) chunk = 1;
  if (chunk > KZD_MAX_CHUNK) chunk = KZD_MAX_CHUNK;
  if (chunk > count) chunk = count;
  p.chunk_polys = chunk;
  p.chunks = count ? (count + chunk - 1) / chunk : 0;
  p.ws_bytes = chunk * per_poly;
  p.stage_launches = p.chunks * (2ull * log_n + 1);
  p.scalar_muls = count * (2 * n + kzd_transform_muls(log_n + 1) + kzd_transform_muls(log_n));
  return p;
}

// plonk_kzg_domain_create's checks, in the order the header documents them
HD int kzd_check_create(uint32_t log_n, bool has_comm, bool has_srs, uint64_t srs_n) {
  if (log_n < KZD_MIN_LOG || log_n > KZD_MAX_LOG) return PLONK_ERR_ARG;
  if (has_comm) return PLONK_ERR_STATE;
  if (!has_srs) return PLONK_ERR_NO_SRS;
  if (srs_n < (1ull << log_n)) return PLONK_ERR_DEGREE;
  return PLONK_OK;
}
// a polynomial's trimmed length against the domain
HD int kzd_check_len(uint32_t log_n, uint64_t trimmed) { return trimmed > (1ull << log_n) ? PLONK_ERR_DEGREE : PLONK_OK; }

}  // namespace plonk
