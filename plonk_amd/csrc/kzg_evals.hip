// KZG10 in evaluation form: commitments and openings of polynomials given by their values on a plonk_kzg_domain.  The
// formulas, the argument checks and the plan are in kzg_evals_core.hpp; DESIGN.md section 15 has the resources and the
// measurements.
//
//   kze_load_kernel       once per handle: the first n points of the commit key (row 0 of its tables) as XYZZ slots
//   kze_points_kernel     once per handle: slot rev((n - i) mod n) of the forward group transform (kzd_transform) times 1/n,
//                         normalised: [L_i(tau)] G as 96 affine bytes, the layout msm_points_run reads
//   kze_scan_kernel       resident vectors: the canonical-form check
//   kze_denoms_kernel     w^i - z per lane and the lane m where it vanishes; poly_batch_inverse inverts in place and
//                         leaves that zero alone, so lane m cannot poison its block
//   kze_fold_kernel       one pass over the values: F[i] += v^j e_j[i] and the partial of y_j with the weight
//                         1 + z / (w^i - z) = w^i / (w^i - z) (inside the domain: 1 at lane m, 0 elsewhere); a wave's partials
//                         are summed by shuffles, kze_final_kernel adds them per vector and applies -(z^n - 1) / n
//   kze_quotient_kernel   q[i] = (F[i] - Y) / (w^i - z); inside the domain also the block partials of sum q[i] w^i, from
//   kze_qfix_kernel       which one lane writes q[m] = -w^(-m) sum
//   kze_finish_kernel     a handle with tables, a call of more than one MSM group: the bit sums of up to KZE_FINISH_CHUNK
//                         commitments -> their 48 compressed bytes, one lane per commitment (kzg_evals_finish.cuh, g1codec.cuh)
// Commitments and the witness go through msm_points_run over the resident Lagrange points: no tables, nothing of the
// context's table budget.  A handle that was given tables (plonk_kzg_evals_tables_build) runs them as
// grouped launches of msm_batch_device over those tables instead: same bytes out.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "poly.hpp"
#include "devmem.cuh"
#include "hostg1.hpp"
#include "g1codec.cuh"
#include "kzg_core.hpp"
#include "kzg_handle.hpp"
#include "kzg_evals.hpp"
#include "kzg_evals_finish.cuh"

namespace plonk {

namespace {

static_assert(sizeof(G1Affine) == KZE_POINT_BYTES, "point size");
static_assert(KZE_TABLE_GROUP == (uint32_t)MSM_MAX_BATCH, "vectors per table launch");

constexpr uint32_t KZE_POINT_LANES = 64;   // one wave per workgroup in the point kernels, as kzg_domain.hip

}  // namespace

// ---- the Lagrange points ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KZE_POINT_LANES) kze_load_kernel(const G1AffineR* __restrict__ row0, uint64_t n,
                                                                   G1RSlot* __restrict__ v) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_g1r(v + i, G1R::from_affine(ld_f28(&row0[i].x), ld_f28(&row0[i].y)));
}

// the forward transform leaves sum_j w^(jk) s_j = n [L_(-k)(tau)] G in slot rev(k)
__global__ void __launch_bounds__(KZE_POINT_LANES) kze_points_kernel(const G1RSlot* __restrict__ v, uint32_t log_n, Fr n_inv_canonical,
                                                                     G1Affine* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = 1ull << log_n;
  if (i >= n) return;
  const G1R s = ld_g1r(v + kzd_rev((n - i) & (n - 1), log_n));
  uint32_t w[24];
#pragma unroll
  for (int k = 0; k < 24; ++k) w[k] = 0;
  if (!s.is_identity()) {   // (tau a point of the domain makes all but one of them the identity)
    const G1R p = g1r_mul_glv(s, n_inv_canonical.l);
    Fp28 x, y;
    g1r_to_affine(p, &x, &y);
    const Fp xf = x.to_fp(), yf = y.to_fp();
#pragma unroll
    for (int k = 0; k < 12; ++k) { w[k] = xf.l[k]; w[12 + k] = yf.l[k]; }
  }
  uint4* q = reinterpret_cast<uint4*>(out + i);
#pragma unroll
  for (int k = 0; k < 6; ++k) q[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// ---- the scalar stage --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) kze_scan_kernel(const Fr* const* __restrict__ vecs, uint64_t n, KzeMeta* __restrict__ meta) {
  const Fr* p = vecs[blockIdx.y];
  unsigned long long bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const Fr x = ld_fr(p + i);
    bool lt = false;
    for (int k = 7; k >= 0; --k)
      if (x.l[k] != FrP::MOD[k]) { lt = x.l[k] < FrP::MOD[k]; break; }
    if (!lt) bad = 1;
  }
  if (bad) atomicOr(&meta->bad, bad);
}

__global__ void __launch_bounds__(256) kze_denoms_kernel(Fr w, Fr z, uint64_t n, Fr* __restrict__ den, KzeMeta* __restrict__ meta) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr d = w.pow_u64(i) - z;
  st_fr(den + i, d);
  if (d.is_zero()) meta->m = i;   // at most one lane: the w^i are distinct
}

// A lane owns the KZE_FOLD_E values base + k * KZE_FOLD_T (coalesced).  Per vector it loads each value ONCE and uses it
// twice: f[k] += v^j e (the fold) and h += e u_k (the partial of y_j).  Values stay in data form: data x twiddle -> data.
__global__ void __launch_bounds__(KZE_FOLD_T) kze_fold_kernel(KzeFoldArgs a, Tw zt_, Tw conv_, Tw one_plain, Tw one_t, uint32_t nwaves) {
  const uint64_t base = (uint64_t)blockIdx.x * (KZE_FOLD_T * KZE_FOLD_E) + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * KZE_FOLD_T + threadIdx.x) >> 6;
  static_assert(KZE_FOLD_E == 4, "the fold kernel is written out for four values per lane");
  // written out per value so that the accumulators have constant names and stay in registers
  const uint64_t i0 = base, i1 = base + KZE_FOLD_T, i2 = base + 2 * KZE_FOLD_T, i3 = base + 3 * KZE_FOLD_T;
  Fr29 f0 = Fr29::zero(), f1 = f0, f2 = f0, f3 = f0, u0 = f0, u1 = f0, u2 = f0, u3 = f0;
  if (a.m != KZE_NONE) {
    const Fr29 one = tw29(one_t);
    if (i0 == a.m) u0 = one;
    if (i1 == a.m) u1 = one;
    if (i2 == a.m) u2 = one;
    if (i3 == a.m) u3 = one;
  } else {   // (1 + z d_i) in data form, then into twiddle form
    const Fr29 zt = tw29(zt_), conv = tw29(conv_), one = tw29(one_plain);
#define KZE_WEIGHT(k) \
  if (i##k < a.n) u##k = Fr29::mul(Fr29::add_csub(Fr29::mul(Fr29::from_fr(ld_fr(a.inv + i##k)), zt), one), conv);
    KZE_WEIGHT(0) KZE_WEIGHT(1) KZE_WEIGHT(2) KZE_WEIGHT(3)
#undef KZE_WEIGHT
  }
  for (uint32_t j = 0; j < a.count; ++j) {
    const Fr* p = a.vecs[a.first + j];
    const Fr29 vt = ld_slot(a.vpow, a.first + j);
    Fr29 h = Fr29::zero();
#define KZE_STEP(k)                                   \
  if (i##k < a.n) {                                   \
    const Fr29 e = Fr29::from_fr(ld_fr(p + i##k));    \
    f##k = Fr29::add_csub(f##k, Fr29::mul(e, vt));    \
    h = Fr29::add_csub(h, Fr29::mul(e, u##k));        \
  }
    KZE_STEP(0) KZE_STEP(1) KZE_STEP(2) KZE_STEP(3)
#undef KZE_STEP
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      Fr29 o;
#pragma unroll
      for (int w = 0; w < 9; ++w) o.l[w] = __shfl_down(h.l[w], off, 64);
      h = Fr29::add_csub(h, o);
    }
    if (!lane) st_fr(a.partial + (uint64_t)j * nwaves + wave, h.to_fr());
  }
#define KZE_STORE(k)                                                                  \
  if (i##k < a.n) {                                                                   \
    Fr29 r = f##k;                                                                    \
    if (a.accumulate) r = Fr29::add_csub(r, Fr29::from_fr(ld_fr(a.fold + i##k)));     \
    st_fr(a.fold + i##k, r.to_fr());                                                  \
  }
  KZE_STORE(0) KZE_STORE(1) KZE_STORE(2) KZE_STORE(3)
#undef KZE_STORE
}
// one workgroup per vector of the launch: evals[j] = scale * the sum of its nwaves partials
__global__ void __launch_bounds__(256) kze_final_kernel(const Fr* __restrict__ partial, uint32_t nwaves, Fr scale, Fr* __restrict__ evals) {
  __shared__ Fr sh[256];
  const uint32_t t = threadIdx.x;
  Fr acc = Fr::zero();
  for (uint32_t w = t; w < nwaves; w += 256) acc = acc + ld_fr(partial + (uint64_t)blockIdx.x * nwaves + w);
  sh[t] = acc;
  __syncthreads();
  for (uint32_t h = 128; h; h >>= 1) {
    if (t < h) sh[t] = sh[t] + sh[t + h];
    __syncthreads();
  }
  if (!t) st_fr(evals + blockIdx.x, sh[0] * scale);
}

// in_domain: lane m has inv == 0, so its q is 0 for now and contributes nothing to the sum
__global__ void __launch_bounds__(KZE_Q_T) kze_quotient_kernel(const Fr* __restrict__ fold, const Fr* __restrict__ inv, Fr Y, uint64_t n,
                                                               Fr w, int in_domain, Fr* __restrict__ q, Fr* __restrict__ qpart) {
  __shared__ Fr sh[KZE_Q_T];
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * KZE_Q_T + t;
  Fr v = Fr::zero();
  if (i < n) {
    v = (ld_fr(fold + i) - Y) * ld_fr(inv + i);
    st_fr(q + i, v);
  }
  if (!in_domain) return;   // (uniform over the grid)
  sh[t] = i < n ? v * w.pow_u64(i) : Fr::zero();
  __syncthreads();
  for (uint32_t h = KZE_Q_T / 2; h; h >>= 1) {
    if (t < h) sh[t] = sh[t] + sh[t + h];
    __syncthreads();
  }
  if (!t) st_fr(qpart + blockIdx.x, sh[0]);
}
__global__ void __launch_bounds__(256) kze_qfix_kernel(const Fr* __restrict__ qpart, uint32_t nblocks, Fr neg_w_inv_m, uint64_t m,
                                                       Fr* __restrict__ q) {
  __shared__ Fr sh[256];
  const uint32_t t = threadIdx.x;
  Fr acc = Fr::zero();
  for (uint32_t b = t; b < nblocks; b += 256) acc = acc + ld_fr(qpart + b);
  sh[t] = acc;
  __syncthreads();
  for (uint32_t h = 128; h; h >>= 1) {
    if (t < h) sh[t] = sh[t] + sh[t + h];
    __syncthreads();
  }
  if (!t) st_fr(q + m, sh[0] * neg_w_inv_m);
}

// ---- the commitments of a call on a handle with tables --------------------------------------------------------------------
// A lane owns a commitment: the Horner chain over its MSM_BIT_SUMS slots (one accumulator, the addend loaded where it is
// used), one safegcd inverse, the encoding.  A slot is read once, 192 bytes by 16-byte words; a launch moves at most
// 4096 x 21 x 192 B = 16.5 MB and runs ~36 point operations per lane: it is bound by the chain's latency, not by memory.
namespace {
struct KzeBitsLoad {
  const G1* b;
  __device__ G1R operator()(int slot) const { return g1r_of_g1(ld_g1(b + slot)); }
};
}  // namespace
__global__ void __launch_bounds__(KZE_FINISH_LANES) kze_finish_kernel(const G1* __restrict__ bits, uint32_t count, int rb, int bitpos,
                                                                      uint8_t* __restrict__ out48) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const KzeBitsLoad ld = {bits + (uint64_t)i * MSM_BIT_SUMS};
  const G1R acc = kze_finish_chain(ld, rb, bitpos != 0);
  uint32_t w[12];
  g1r_compress48_words(acc, w);
  uint4* q = reinterpret_cast<uint4*>(out48 + 48ull * i);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
  q[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// ---- launchers (kzg_evals.hpp) -----------------------------------------------------------------------------------------------
int kze_lagrange_points(Ctx* c, uint32_t log_n, const GlvScalar* tw, uint32_t tw_log, G1Affine* out) {
  const uint64_t n = 1ull << log_n;
  if (!c->srs_table || c->srs_n < n || log_n < 1 || log_n > tw_log) return PLONK_ERR_ARG;
  G1RSlot* v = nullptr;
  HIP_TRY(hipMalloc((void**)&v, sizeof(G1RSlot) * n));
  const dim3 grid((uint32_t)((n + KZE_POINT_LANES - 1) / KZE_POINT_LANES));
  hipLaunchKernelGGL(kze_load_kernel, grid, dim3(KZE_POINT_LANES), 0, c->stream, (const G1AffineR*)c->srs_table, n, v);
  int rc = hipGetLastError() == hipSuccess ? PLONK_OK : PLONK_ERR_HIP;
  if (rc == PLONK_OK) rc = kzd_transform(c, v, n, log_n, 1, false, tw, tw_log, nullptr, nullptr);
  if (rc == PLONK_OK) {
    hipLaunchKernelGGL(kze_points_kernel, grid, dim3(KZE_POINT_LANES), 0, c->stream, (const G1RSlot*)v, log_n,
                       Fr::from_u64(n).inv().from_mont(), out);
    if (hipGetLastError() != hipSuccess) rc = PLONK_ERR_HIP;
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess && rc == PLONK_OK) rc = PLONK_ERR_HIP;
  (void)hipFree(v);
  if (rc == PLONK_ERR_HIP) set_last_error("kze_lagrange_points", "a launch of the Lagrange-point build failed", __FILE__, __LINE__);
  return rc;
}

int kze_scan(Ctx* c, const Fr* const* vecs, uint32_t first, uint32_t cnt, uint64_t n, KzeMeta* meta) {
  const uint32_t blocks = (uint32_t)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  for (uint32_t done = 0; done < cnt; done += 32768) {   // grid.y
    hipLaunchKernelGGL(kze_scan_kernel, dim3(blocks, cnt - done < 32768 ? cnt - done : 32768), dim3(256), 0, c->stream, vecs + first + done, n, meta);
    HIP_TRY(hipGetLastError());
  }
  return PLONK_OK;
}

bool kze_host_canonical(const void* const* vecs, uint64_t count, uint64_t n) {
  Fr t;
  for (uint64_t i = 0; i < count; ++i)
    for (uint64_t k = 0; k < n; ++k)
      if (!kzg_fr_load((const uint64_t*)vecs[i] + 4 * k, &t)) return false;
  return true;
}

int kze_denominators(Ctx* c, uint32_t log_n, const Fr& z, Fr* den, KzeMeta* meta) {
  const uint64_t n = 1ull << log_n;
  hipLaunchKernelGGL(kze_denoms_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, fr_domain_root(log_n), z, n, den, meta);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kze_fold_eval(Ctx* c, const KzeFoldArgs& a, Fr* evals) {
  if (!a.count || a.count > KZE_GROUP || !a.n) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  const uint32_t nwaves = kze_fold_waves(a.n);
  // R''^2 / R = (R'' / R) in twiddle form; R'' / R = 2^5 (poly_batch_inverse's constant)
  hipLaunchKernelGGL(kze_fold_kernel, dim3(kze_fold_blocks(a.n)), dim3(KZE_FOLD_T), 0, c->stream, a, tw_of(a.z), tw_of(Fr::from_u64(32)),
                     tw_plain(Fr::one()), tw_of(Fr::one()), nwaves);
  hipLaunchKernelGGL(kze_final_kernel, dim3(a.count), dim3(256), 0, c->stream, (const Fr*)a.partial, nwaves, a.scale, evals);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kze_quotient(Ctx* c, uint32_t log_n, const Fr* fold, const Fr* inv, const Fr& Y, uint64_t m, Fr* q, Fr* qpart) {
  const uint64_t n = 1ull << log_n;
  if (m != KZE_NONE && m >= n) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  const Fr w = fr_domain_root(log_n);
  const uint32_t blocks = kze_quotient_blocks(n);
  hipLaunchKernelGGL(kze_quotient_kernel, dim3(blocks), dim3(KZE_Q_T), 0, c->stream, fold, inv, Y, n, w, m != KZE_NONE ? 1 : 0, q, qpart);
  if (m != KZE_NONE)
    hipLaunchKernelGGL(kze_qfix_kernel, dim3(1), dim3(256), 0, c->stream, (const Fr*)qpart, blocks, w.pow_u64(m).inv().neg(), m, q);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kze_finish(Ctx* c, const G1* bits, uint32_t count, int rb, bool bitpos, uint8_t* out48) {
  // rb + 9 slots are read of the MSM_BIT_SUMS a commitment has
  if (!bits || !out48 || !count || rb < 8 || rb + 9 > MSM_BIT_SUMS) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kze_finish_kernel, dim3((count + KZE_FINISH_LANES - 1) / KZE_FINISH_LANES), dim3(KZE_FINISH_LANES), 0, c->stream, bits,
                     count, rb, bitpos ? 1 : 0, out48);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the state a handle holds for these calls ------------------------------------------------------------------------------
struct KzeBufs {
  enum { DEN, FOLD, Q, PARTIAL, EVALS, VPOW, VECS, META, QPART, BITS, FIN48, NBUF };   // grow-only
};
struct KzgEvals : KzeBufs, DevBufs<KzeBufs::NBUF> {
  G1Affine* lag = nullptr;      // [L_i(tau)] G, i < n
  uint64_t lag_bytes = 0;
  plonk_kzg_evals_info last = {};
  // opt-in (plonk_kzg_evals_tables_build): table rows over `lag`, held against the context's table budget
  Ctx* tab_ctx = nullptr;
  void* table = nullptr;
  uint32_t tab_rows = 0;
  uint64_t tab_n = 0;
  plonk_kzg_evals_tables_info tl = {};   // built, bucket_bits and the counters of the last call that used the tables
  std::vector<uint8_t> fin_host;         // the compressed commitments of a chunk on their way to the caller
  void drop_tables() {
    if (!table) return;
    (void)hipStreamSynchronize(tab_ctx->stream);
    srs_table_release(tab_ctx, table, tab_rows, tab_n);
    table = nullptr;
    tab_rows = 0;
    tl = {};
  }
  ~KzgEvals() {
    drop_tables();
    (void)hipFree(lag);
  }
};

void kze_release(KzgEvals* evals) { delete evals; }

namespace {

// the points, built by the first call that commits
int lagrange_ready(KzgDomain* d, KzgEvals* e, uint32_t* built) {
  if (e->lag) return PLONK_OK;
  const uint64_t bytes = KZE_POINT_BYTES << d->log_n;
  G1Affine* pts = nullptr;
  HIP_TRY(hipMalloc((void**)&pts, bytes));
  const int rc = kze_lagrange_points(d->c, d->log_n, d->tw, d->log_n + 1, pts);
  if (rc != PLONK_OK) {
    (void)hipFree(pts);
    return rc;
  }
  e->lag = pts;
  e->lag_bytes = bytes;
  *built = 1;
  return PLONK_OK;
}

// sum_i s[i] [L_i(tau)] G as 48 compressed bytes (returns with the stream synchronised); plonk_ctx_last_msm_points keeps
// reporting the caller's own last call
int commit_values_points(Ctx* c, const KzgEvals* e, const Fr* s, uint64_t n, uint8_t out48[48]) {
  const plonk_msm_points_info keep = c->last_points;
  const bool keep_valid = c->last_points_valid;
  MpInput in;
  in.points = reinterpret_cast<const uint8_t*>(e->lag);
  in.scalars = s;
  G1 sum;
  const int rc = msm_points_run(c, in, n, nullptr, &sum);
  c->last_points = keep;
  c->last_points_valid = keep_valid;
  PTRY(rc);
  uint8_t aff[1][97];
  batch_xyzz_to_affine97(&sum, 1, aff);
  g1_compress97(aff[0], out48);
  return PLONK_OK;
}

// One run of table MSMs of a call on a handle that holds tables (kzg_evals_core.hpp kze_tables_plan): add() queues the
// grouped launches of the vectors it is given, finish() ends the run.  A run planned as ONE launch is finished on the host,
// as msm_group_sums does for the commit key.  A longer run writes the bit sums of its launches side by side into the handle's
// array and turns a full chunk (and what is left at the end) into compressed bytes by kze_finish_kernel, one copy and one
// synchronisation.  While the run lives the context's last_plan and acc_done are put aside: plonk_ctx_last_msm keeps
// describing the caller's own last MSM, and no event of a prover is recorded by these launches.
struct TableRun {
  Ctx* c = nullptr;
  KzgEvals* e = nullptr;
  uint64_t n = 0;
  bool device = false;
  uint32_t cap = 0, pending = 0;   // commitments the bit-sum array holds / that wait in it
  int rb = 0;
  std::vector<uint8_t*> dest;      // where the 48 bytes of each waiting commitment go
  plonk_msm_plan_internal keep_plan;
  hipEvent_t keep_acc = nullptr;
  TableRun() = default;
  TableRun(const TableRun&) = delete;
  TableRun& operator=(const TableRun&) = delete;
  ~TableRun() {
    if (!c) return;
    c->last_plan = keep_plan;
    c->acc_done = keep_acc;
  }
  // launches / entries: of the whole run, as planned
  int begin(Ctx* ctx, KzgEvals* ev, uint64_t points, uint64_t launches, uint64_t entries) {
    e = ev;
    n = points;
    device = launches > 1;
    PTRY(msm_reserve(ctx, n));   // msm_group_sums reads the scratch's result slots before its launch reserves anything
    if (device) {
      cap = (uint32_t)(entries < KZE_FINISH_CHUNK ? entries : KZE_FINISH_CHUNK);
      PTRY(e->need(KzgEvals::BITS, sizeof(G1) * MSM_BIT_SUMS * cap));
      PTRY(e->need(KzgEvals::FIN48, 48ull * cap));
      e->fin_host.resize(48ull * cap);
      dest.reserve(cap);
    }
    c = ctx;
    keep_plan = c->last_plan;
    keep_acc = c->acc_done;
    c->acc_done = nullptr;
    return PLONK_OK;
  }
  // out48[k]: where the commitment of s[k] goes, k < cnt
  int add(const Fr* const* s, uint32_t cnt, uint8_t* const* out48) {
    uint64_t m[MSM_MAX_BATCH];
    for (int k = 0; k < MSM_MAX_BATCH; ++k) m[k] = n;
    for (uint32_t k0 = 0; k0 < cnt;) {
      uint32_t g = cnt - k0 < (uint32_t)MSM_MAX_BATCH ? cnt - k0 : (uint32_t)MSM_MAX_BATCH;
      if (!device) {
        G1 sums[MSM_MAX_BATCH];
        uint8_t aff[MSM_MAX_BATCH][97];
        PTRY(msm_group_sums(c, s + k0, m, (int)g, sums, e->table, e->tab_n, e->tab_rows));
        batch_xyzz_to_affine97(sums, (int)g, aff);
        for (uint32_t k = 0; k < g; ++k) g1_compress97(aff[k], out48[k0 + k]);
      } else {
        if (g > cap - pending) g = cap - pending;   // (chunks end on a launch boundary for every plan; the array's bound)
        G1* out[MSM_MAX_BATCH];
        for (uint32_t k = 0; k < g; ++k) {
          out[k] = e->at<G1>(KzgEvals::BITS) + (uint64_t)(pending + k) * MSM_BIT_SUMS;
          dest.push_back(out48[k0 + k]);
        }
        PTRY(msm_batch_device(c, s + k0, m, (int)g, out, true, e->table, e->tab_n, nullptr, nullptr, e->tab_rows));
        if (rb && rb != c->msm.last_rowbits) return (set_last_error("kzg_evals", "the launches of a run disagree on the layout of their bit sums", __FILE__, __LINE__), PLONK_ERR_STATE);
        rb = c->msm.last_rowbits;
        pending += g;
      }
      e->tl.bucket_bits = c->last_plan.bucket_bits;
      e->tl.msms += g;
      ++e->tl.group_launches;
      k0 += g;
      if (device && pending == cap) PTRY(flush());
    }
    return PLONK_OK;
  }
  int flush() {
    if (!pending) return PLONK_OK;
    PTRY(kze_finish(c, e->at<G1>(KzgEvals::BITS), pending, rb, e->tab_rows == MSM_ROWS_BITPOS, e->at<uint8_t>(KzgEvals::FIN48)));
    HIP_TRY(hipMemcpyAsync(e->fin_host.data(), e->p[KzgEvals::FIN48], 48ull * pending, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < pending; ++k) memcpy(dest[k], e->fin_host.data() + 48ull * k, 48);
    dest.clear();
    pending = 0;
    e->tl.device_finished = 1;
    return PLONK_OK;
  }
  int finish() { return device ? flush() : PLONK_OK; }
};

// the counters plonk_kzg_evals_tables_last reports of "the last call that used the tables" start here
void tables_call_begin(KzgEvals* e) {
  e->tl.msms = 0;
  e->tl.group_launches = 0;
  e->tl.device_finished = 0;
}

// commitments of `count` resident vectors, out48 + 48 j for s[j]: one after the other over the points, or one run over the tables
int commit_list(Ctx* c, KzgEvals* e, const Fr* const* s, uint64_t count, uint64_t n, uint8_t* out48) {
  if (!e->table) {
    for (uint64_t j = 0; j < count; ++j) PTRY(commit_values_points(c, e, s[j], n, out48 + 48 * j));
    return PLONK_OK;
  }
  const KzeTablesPlan tp = kze_tables_plan(count, count, 0, 0);
  TableRun run;
  PTRY(run.begin(c, e, n, tp.group_launches, count));
  std::vector<uint8_t*> out(count);
  for (uint64_t j = 0; j < count; ++j) out[j] = out48 + 48 * j;
  for (uint64_t j = 0; j < count; j += KZE_GROUP) {   // (add() takes a 32-bit count)
    const uint32_t cnt = (uint32_t)(count - j < KZE_GROUP ? count - j : KZE_GROUP);
    PTRY(run.add(s + j, cnt, out.data() + j));
  }
  return run.finish();
}
int commit_values(Ctx* c, KzgEvals* e, const Fr* s, uint64_t n, uint8_t out48[48]) { return commit_list(c, e, &s, 1, n, out48); }

// The call's vectors made resident group after group, `per` at most at a time: fn(first, cnt, ptrs) runs with ptrs[k] the
// device address of vector first + k.  The resident form passes the caller's pointers through; the host form packs a group
// into one of the context's two upload buffers, the upload of group g + 1 (copy stream) queued under what fn queued for group
// g (main stream); a buffer is reused once the work that read it has finished.
template <class F>
int for_groups(Ctx* c, const void* const* vecs, uint64_t count, uint64_t n, bool resident, const KzePlan& plan, F fn) {
  const uint32_t per = (uint32_t)plan.group_vectors;
  std::vector<const Fr*> ptrs(per);
  if (resident) {
    for (uint64_t first = 0; first < count; first += per) {
      const uint32_t cnt = (uint32_t)(count - first < per ? count - first : per);
      for (uint32_t k = 0; k < cnt; ++k) ptrs[k] = (const Fr*)vecs[first + k];
      PTRY(fn((uint32_t)first, cnt, ptrs.data()));
    }
    return PLONK_OK;
  }
  Fr* stage[2];
  hipEvent_t up[2], done[2];
  PTRY(kzg_stage_reserve(c, plan.stage_values, stage, up, done));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the copy stream is not ordered behind what the main stream still runs
  uint64_t g = 0;
  for (uint64_t first = 0; first < count; first += per, ++g) {
    const int b = (int)(g & 1);
    const uint32_t cnt = (uint32_t)(count - first < per ? count - first : per);
    if (g >= 2) HIP_TRY(hipStreamWaitEvent(c->copy_stream, done[b], 0));
    for (uint32_t k = 0; k < cnt; ++k) {
      ptrs[k] = stage[b] + (uint64_t)k * n;
      HIP_TRY(hipMemcpyAsync((void*)ptrs[k], vecs[first + k], sizeof(Fr) * n, hipMemcpyHostToDevice, c->copy_stream));
    }
    HIP_TRY(hipEventRecord(up[b], c->copy_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, up[b], 0));
    PTRY(fn((uint32_t)first, cnt, ptrs.data()));
    HIP_TRY(hipEventRecord(done[b], c->stream));
  }
  return PLONK_OK;
}

struct EvalsCall {
  const void* const* vecs;
  uint64_t count;
  bool resident;
  bool open;                 // plonk_kzg_open_evals (false: plonk_kzg_commit_evals)
  Fr z, v;
  uint64_t* evaluations;
  uint8_t* commitments48;
  uint8_t* witness48;
};

int evals_body(const char* api_fn, KzgDomain* d, KzgEvals* e, const EvalsCall& a) {
  Ctx& c = *d->c;
  const uint32_t L = d->log_n;
  const uint64_t n = 1ull << L, count = a.count;
  const bool in_domain = a.open && kze_in_domain(a.z, L);
  const KzePlan plan = kze_plan(L, count, a.commitments48 != nullptr, a.witness48 != nullptr, !a.resident);
  plonk_kzg_evals_info info = {};
  info.log_n = L;
  info.count = count;
  info.in_domain_index = KZE_NONE;
  info.msm_launches = plan.msm_launches;
  info.msm_terms = plan.msm_terms;
  // ---- checks that need the device: canonical values of the resident form, the lane m ----
  PTRY(e->need(KzgEvals::META, sizeof(KzeMeta)));
  PTRY(e->need(KzgEvals::VECS, sizeof(Fr*) * count));
  if (a.open) PTRY(e->need(KzgEvals::DEN, sizeof(Fr) * n));
  KzeMeta mh = {KZE_NONE, 0};
  if (a.resident || in_domain) {
    HIP_TRY(hipMemcpyAsync(e->p[KzgEvals::META], &mh, sizeof mh, hipMemcpyHostToDevice, c.stream));
    if (a.resident) {
      HIP_TRY(hipMemcpyAsync(e->p[KzgEvals::VECS], a.vecs, sizeof(Fr*) * count, hipMemcpyHostToDevice, c.stream));
      PTRY(kze_scan(&c, e->at<const Fr*>(KzgEvals::VECS), 0, (uint32_t)count, n, e->at<KzeMeta>(KzgEvals::META)));
    }
    if (a.open) PTRY(kze_denominators(&c, L, a.z, e->at<Fr>(KzgEvals::DEN), e->at<KzeMeta>(KzgEvals::META)));
    HIP_TRY(hipMemcpyAsync(&mh, e->p[KzgEvals::META], sizeof mh, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (mh.bad) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
    if (in_domain != (mh.m != KZE_NONE) || (in_domain && mh.m >= n)) API_FAIL(PLONK_ERR_STATE, "the device and the host disagree on whether the point lies in the domain");
  } else if (a.open) {
    PTRY(kze_denominators(&c, L, a.z, e->at<Fr>(KzgEvals::DEN), e->at<KzeMeta>(KzgEvals::META)));
  }
  info.in_domain_index = mh.m;
  // ---- from here on the call writes ----
  if (plan.msm_launches) PTRY(lagrange_ready(d, e, &info.built_points));
  // the MSMs of the call: per vector over the points, or ONE run over the handle's tables — the commitments group after
  // group as their vectors become resident, the witness last
  const bool tabled = e->table && plan.msm_launches;
  TableRun run;
  if (tabled) {
    const KzeTablesPlan tp = kze_tables_plan(a.commitments48 ? count : 0, plan.group_vectors, a.witness48 ? 1 : 0, 0);
    tables_call_begin(e);
    PTRY(run.begin(&c, e, n, tp.group_launches, tp.msms));
  }
  auto commit_group = [&](uint32_t first, uint32_t cnt, const Fr* const* ptrs) -> int {
    if (!tabled) {
      for (uint32_t k = 0; k < cnt; ++k) PTRY(commit_values_points(&c, e, ptrs[k], n, a.commitments48 + 48ull * (first + k)));
      return PLONK_OK;
    }
    uint8_t* out[KZE_GROUP];
    for (uint32_t k = 0; k < cnt; ++k) out[k] = a.commitments48 + 48ull * (first + k);
    return run.add(ptrs, cnt, out);
  };
  if (!a.open) {
    PTRY(for_groups(&c, a.vecs, count, n, a.resident, plan, commit_group));
    if (tabled) PTRY(run.finish());
    info.lagrange_bytes = e->lag_bytes;
    e->last = info;
    return PLONK_OK;
  }
  const uint32_t nwaves = kze_fold_waves(n);
  PTRY(e->need(KzgEvals::FOLD, sizeof(Fr) * n));
  PTRY(e->need(KzgEvals::PARTIAL, sizeof(Fr) * KZE_GROUP * nwaves));
  PTRY(e->need(KzgEvals::EVALS, sizeof(Fr) * count));
  PTRY(e->need(KzgEvals::VPOW, sizeof(Fr29Slot) * count));
  PTRY(poly_batch_inverse(&c, e->at<Fr>(KzgEvals::DEN), n));
  PTRY(poly_kzg_powers(&c, e->p[KzgEvals::VPOW], (uint32_t)count, a.v));
  KzeFoldArgs fa;
  fa.vecs = e->at<const Fr*>(KzgEvals::VECS);
  fa.vpow = e->p[KzgEvals::VPOW];
  fa.n = n;
  fa.inv = e->at<Fr>(KzgEvals::DEN);
  fa.m = mh.m;
  fa.fold = e->at<Fr>(KzgEvals::FOLD);
  fa.partial = e->at<Fr>(KzgEvals::PARTIAL);
  fa.z = a.z;
  fa.scale = kze_eval_scale(a.z, L);
  std::vector<const Fr*> staged(a.resident ? 0 : count);   // the host form's device addresses, alive until the call's last copy has run
  PTRY(for_groups(&c, a.vecs, count, n, a.resident, plan, [&](uint32_t first, uint32_t cnt, const Fr* const* ptrs) -> int {
    if (!a.resident) {
      for (uint32_t k = 0; k < cnt; ++k) staged[first + k] = ptrs[k];
      HIP_TRY(hipMemcpyAsync(e->at<const Fr*>(KzgEvals::VECS) + first, staged.data() + first, sizeof(Fr*) * cnt, hipMemcpyHostToDevice, c.stream));
    }
    fa.first = first;
    fa.count = cnt;
    fa.accumulate = first ? 1 : 0;
    PTRY(kze_fold_eval(&c, fa, e->at<Fr>(KzgEvals::EVALS) + first));
    if (a.commitments48) PTRY(commit_group(first, cnt, ptrs));
    return PLONK_OK;
  }));
  std::vector<Fr> y(count);
  HIP_TRY(hipMemcpyAsync(y.data(), e->p[KzgEvals::EVALS], sizeof(Fr) * count, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  if (a.witness48) {
    Fr Y = Fr::zero(), vp = Fr::one();
    for (uint64_t j = 0; j < count; ++j) {
      Y = Y + vp * y[j];
      vp = vp * a.v;
    }
    PTRY(e->need(KzgEvals::Q, sizeof(Fr) * n));
    PTRY(e->need(KzgEvals::QPART, sizeof(Fr) * kze_quotient_blocks(n)));
    PTRY(kze_quotient(&c, L, e->at<Fr>(KzgEvals::FOLD), e->at<Fr>(KzgEvals::DEN), Y, mh.m, e->at<Fr>(KzgEvals::Q), e->at<Fr>(KzgEvals::QPART)));
    if (tabled) {
      const Fr* q = e->at<Fr>(KzgEvals::Q);
      uint8_t* out = a.witness48;
      PTRY(run.add(&q, 1, &out));
    } else {
      PTRY(commit_values_points(&c, e, e->at<Fr>(KzgEvals::Q), n, a.witness48));
    }
  }
  if (tabled) PTRY(run.finish());
  memcpy(a.evaluations, y.data(), sizeof(Fr) * count);
  info.lagrange_bytes = e->lag_bytes;
  e->last = info;
  return PLONK_OK;
}

int evals_impl(const char* api_fn, plonk_kzg_domain* dom, const void* const* vecs, uint64_t count, bool resident, bool open,
               const uint64_t* point, const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments48, uint8_t* witness48) {
  const int arg = open ? kze_check_open(dom != nullptr, vecs != nullptr, point != nullptr, v_challenge != nullptr, evaluations != nullptr, count)
                       : kze_check_commit(dom != nullptr, vecs != nullptr, commitments48 != nullptr, count);
  if (arg != PLONK_OK) API_FAIL(PLONK_ERR_ARG, count > KZE_MAX_COUNT ? "invalid argument: at most 65536 vectors per call"
                                                                      : "invalid argument: a required pointer is NULL");
  for (uint64_t i = 0; i < count; ++i)
    if (!vecs[i]) API_FAIL(PLONK_ERR_ARG, "invalid argument: evals[i] is NULL");
  EvalsCall a = {vecs, count, resident, open, Fr::zero(), Fr::one(), evaluations, commitments48, witness48};
  if (open && (!kzg_fr_load(point, &a.z) || (v_challenge && !kzg_fr_load(v_challenge, &a.v)))) API_FAIL(PLONK_ERR_DATA, "non-canonical scalar");
  KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_WORK);
  // before anything is queued or written
  if (!resident && !kze_host_canonical(vecs, count, 1ull << d->log_n)) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
  KzgEvals* e = kzd_state(d->evals);
  if (!count) {
    if (witness48) identity48(witness48);
    plonk_kzg_evals_info info = {};
    info.log_n = d->log_n;
    info.in_domain_index = KZE_NONE;
    info.msm_terms = 1ull << d->log_n;
    info.lagrange_bytes = e->lag_bytes;
    e->last = info;
    return PLONK_OK;
  }
  return kzd_drained(d->c, evals_body(api_fn, d, e, a));
}

}  // namespace

int kze_points_ready(KzgDomain* d, uint32_t* built) { return lagrange_ready(d, kzd_state(d->evals), built); }
const G1Affine* kze_points(KzgDomain* d) { return kzd_state(d->evals)->lag; }
int kze_commit_values(KzgDomain* d, const Fr* s, uint8_t out48[48]) {
  return commit_values(d->c, kzd_state(d->evals), s, 1ull << d->log_n, out48);
}
int kze_commit_list(KzgDomain* d, const Fr* const* s, uint64_t count, uint8_t* out48) {
  return commit_list(d->c, kzd_state(d->evals), s, count, 1ull << d->log_n, out48);
}
void kze_tables_call_begin(KzgDomain* d) {
  KzgEvals* e = kzd_state(d->evals);
  if (e->table) tables_call_begin(e);
}

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_kzg_commit_evals(plonk_kzg_domain* dom, const uint64_t* const* evals, uint64_t count, uint8_t* commitments48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::evals_impl(api_fn, dom, (const void* const*)evals, count, false, false, nullptr, nullptr, nullptr, commitments48, nullptr);
  });
}

int plonk_kzg_commit_evals_dev(plonk_kzg_domain* dom, const void* const* evals_dev, uint64_t count, uint8_t* commitments48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::evals_impl(api_fn, dom, evals_dev, count, true, false, nullptr, nullptr, nullptr, commitments48, nullptr);
  });
}

int plonk_kzg_open_evals(plonk_kzg_domain* dom, const uint64_t* const* evals, uint64_t count, const uint64_t point[4],
                         const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments48, uint8_t* witness48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::evals_impl(api_fn, dom, (const void* const*)evals, count, false, true, point, v_challenge, evaluations, commitments48,
                             witness48);
  });
}

int plonk_kzg_open_evals_dev(plonk_kzg_domain* dom, const void* const* evals_dev, uint64_t count, const uint64_t point[4],
                             const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments48, uint8_t* witness48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::evals_impl(api_fn, dom, evals_dev, count, true, true, point, v_challenge, evaluations, commitments48, witness48);
  });
}

int plonk_kzg_evals_last(plonk_kzg_domain* dom, plonk_kzg_evals_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_KEY);
  const KzgEvals* e = d->evals;
  plonk_kzg_evals_info info = {};
  info.log_n = d->log_n;
  info.in_domain_index = KZE_NONE;
  info.msm_terms = 1ull << d->log_n;
  if (e) {
    info = e->last.log_n ? e->last : info;
    info.lagrange_bytes = e->lag_bytes;
  }
  *out = info;
  return PLONK_OK;
  });
}

int plonk_kzg_evals_tables_build(plonk_kzg_domain* dom) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  Ctx& c = *d->c;
  KZD_ENTER(d, api_fn, KZD_WORK);
  KzgEvals* e = kzd_state(d->evals);
  if (e->table) {
    e->tl.built = 0;
    return PLONK_OK;
  }
  const uint64_t n = 1ull << d->log_n;
  // srs_table_build's refusal, before the points are allocated
  if ((uint64_t)msm_table_rows(&c, n, true) * n > (1ull << 31)) API_FAIL(PLONK_ERR_ARG, "invalid argument: table rows * points must be <= 2^31");
  uint32_t built_points = 0;
  PTRY(lagrange_ready(d, e, &built_points));
  void* t = nullptr;
  uint32_t rows = 0;
  PTRY(srs_table_build(&c, e->lag, n, &t, &rows));
  e->tab_ctx = &c;
  e->table = t;
  e->tab_rows = rows;
  e->tab_n = n;
  e->tl = {};
  e->tl.built = 1;
  return PLONK_OK;
  });
}

int plonk_kzg_evals_tables_drop(plonk_kzg_domain* dom) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_SET_DEVICE);
  if (d->evals) d->evals->drop_tables();
  return PLONK_OK;
  });
}

int plonk_kzg_evals_tables_last(plonk_kzg_domain* dom, plonk_kzg_evals_tables_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, 0);
  const KzgEvals* e = d->evals;
  plonk_kzg_evals_tables_info info = {};
  if (e && e->table) {
    info = e->tl;
    info.table_rows = e->tab_rows;
    info.table_bytes = sizeof(G1AffineR) * (uint64_t)e->tab_rows * e->tab_n;
  }
  info.log_n = d->log_n;
  *out = info;
  return PLONK_OK;
  });
}

}  // extern "C"
