// KZG10 multiproofs: many (vector, domain point) openings of polynomials in evaluation form behind one 96-byte proof.  The
// formulas, the argument checks, the sorts, the challenges and the plan are in kzg_multiproof_core.hpp; DESIGN.md section 19
// has the derivation, the resources and the measurements.  The Lagrange points, the weighted fold (kze_fold_eval), the
// quotient at t (kze_denominators / poly_batch_inverse / kze_quotient), the commitments (msm_points_run over the Lagrange
// points), the decoding, the verifier's sum (msm_points_run in the term layout) and the host pairing are those the other
// calls use; new here:
//
//   kmp_gather_kernel       y_k = e_(j_k)[m_k]: the prover reads the values it proves from the vectors themselves
//   kmp_groups_kernel       one wave per point group: Y_m over the group's items, 32 w^(-m) in twiddle form, -w^(-m)
//   kmp_aggregate_kernel    the hot path, kze_fold_kernel's shape: a lane owns four values one workgroup-width apart; per
//                           point group it sums r^k e_(j_k)[i] over the group's items (one load and one product per item and
//                           value), multiplies (A - Y_m) by invd[(i - m) mod n] (contiguous across the lanes) and by 32 w^(-m),
//                           adds q into g and reduces the wave's partial of sum q w^i by shuffles; up to KMP_GROUP_CHUNK
//                           groups per launch, so the partials buffer is bounded
//   kmp_fix_kernel          one workgroup per group of the launch: g[m] += -w^(-m) * the sum of its partials; distinct groups
//                           have distinct m, nothing races
//   kmp_weights_den_kernel  t - w^(m_k) per item; poly_batch_inverse inverts
//   kmp_weights_kernel      one wave per vector over the sort by vector index: s_j; one more wave: y; shared by the prover (s_j
//                           in twiddle form for the fold) and the verifier (the canonical scalars of its sum)
// invd is kze_denominators at z = 1 and poly_batch_inverse, once per handle.
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "poly.hpp"
#include "devmem.cuh"
#include "hostg1.hpp"
#include "kzg_core.hpp"
#include "kzg_key.hpp"
#include "kzg_handle.hpp"
#include "kzg_evals.hpp"
#include "kzg_multiproof.hpp"

namespace plonk {

namespace {

// x^e by squarings over the bits of e held in a register (Fr::pow_u64 indexes a local array of words)
__device__ __forceinline__ Fr kmp_pow(const Fr& x, uint64_t e) {
  Fr acc = Fr::one();
  if (!e) return acc;
  int b = 63 - __clzll((long long)e);
  acc = x;
  for (--b; b >= 0; --b) {
    acc = acc.sqr();
    if ((e >> b) & 1) acc = acc * x;
  }
  return acc;
}

// the sum of one value per lane over a wave of KMP_LANES, in lane 0
__device__ __forceinline__ Fr kmp_wave_sum(Fr acc, Fr* sh, uint32_t lane) {
  sh[lane] = acc;
  __syncthreads();
  for (uint32_t s = KMP_LANES / 2; s; s >>= 1) {
    if (lane < s) sh[lane] = sh[lane] + sh[lane + s];
    __syncthreads();
  }
  return sh[0];
}

}  // namespace

__global__ void __launch_bounds__(256) kmp_gather_kernel(const Fr* const* __restrict__ vecs, const uint32_t* __restrict__ vector_index,
                                                         const uint32_t* __restrict__ point_index, uint32_t K, Fr* __restrict__ yk) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  st_fr(yk + k, ld_fr(vecs[vector_index[k]] + point_index[k]));
}

__global__ void __launch_bounds__(KMP_LANES) kmp_groups_kernel(Fr w_inv, Fr c32, const Fr* __restrict__ rpow, const Fr* __restrict__ yk,
                                                               const uint32_t* __restrict__ perm, const uint32_t* __restrict__ group_m,
                                                               const uint32_t* __restrict__ group_off, Fr* __restrict__ ym,
                                                               void* __restrict__ cw, Fr* __restrict__ negw) {
  __shared__ Fr sh[KMP_LANES];
  const uint32_t g = blockIdx.x, lane = threadIdx.x, end = group_off[g + 1];
  Fr acc = Fr::zero();
  for (uint32_t t = group_off[g] + lane; t < end; t += KMP_LANES) {
    const uint32_t k = perm[t];
    acc = acc + ld_fr(rpow + k) * ld_fr(yk + k);
  }
  const Fr sum = kmp_wave_sum(acc, sh, lane);
  if (lane) return;
  const Fr wm = kmp_pow(w_inv, group_m[g]);
  st_fr(ym + g, sum);
  st_fr(negw + g, wm.neg());
  st_slot(cw, g, Fr29::twiddle_from_fr(wm * c32));
}

// A lane owns the KMP_AGG_E values base + k * KMP_AGG_T (coalesced).  The accumulators are written out per value so that they
// have constant names and stay in registers (as kze_fold_kernel's).  Values stay in data form: data x twiddle -> data; the
// product of two data-form values (A - Y_m and invd) comes back to data form through the factor 32 = R'' / R inside cw.
__global__ void __launch_bounds__(KMP_AGG_T) kmp_aggregate_kernel(KmpAggArgs a, uint32_t first, uint32_t count, int accumulate, Fr w,
                                                                  Fr w_step, uint32_t nwaves) {
  static_assert(KMP_AGG_E == 4, "the aggregate kernel is written out for four values per lane");
  const uint64_t base = (uint64_t)blockIdx.x * (KMP_AGG_T * KMP_AGG_E) + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * KMP_AGG_T + threadIdx.x) >> 6;
  const uint64_t i0 = base, i1 = base + KMP_AGG_T, i2 = base + 2 * KMP_AGG_T, i3 = base + 3 * KMP_AGG_T;
  const uint64_t mask = a.n - 1;
  // w^i in twiddle form, for the partial of sum q w^i
  Fr29 p0 = Fr29::zero(), p1 = p0, p2 = p0, p3 = p0;
  {
    Fr x = kmp_pow(w, i0 & mask);
    p0 = Fr29::twiddle_from_fr(x);
    x = x * w_step;
    p1 = Fr29::twiddle_from_fr(x);
    x = x * w_step;
    p2 = Fr29::twiddle_from_fr(x);
    x = x * w_step;
    p3 = Fr29::twiddle_from_fr(x);
  }
  Fr29 g0 = Fr29::zero(), g1 = g0, g2 = g0, g3 = g0;
  for (uint32_t gi = 0; gi < count; ++gi) {
    const uint32_t grp = first + gi;
    const uint64_t m = a.group_m[grp];
    const uint32_t end = a.group_off[grp + 1];
    Fr29 a0 = Fr29::zero(), a1 = a0, a2 = a0, a3 = a0;
    for (uint32_t t = a.group_off[grp]; t < end; ++t) {
      const uint32_t k = a.perm[t];
      const Fr* p = a.vecs[a.vector_index[k]];
      const Fr29 rt = ld_slot(a.rtw, k);
#define KMP_STEP(k) \
  if (i##k < a.n) a##k = Fr29::add_csub(a##k, Fr29::mul(Fr29::from_fr(ld_fr(p + i##k)), rt));
      KMP_STEP(0) KMP_STEP(1) KMP_STEP(2) KMP_STEP(3)
#undef KMP_STEP
    }
    const Fr29 ym = Fr29::from_fr(ld_fr(a.ym + grp)), cw = ld_slot(a.cw, grp);
    Fr29 h = Fr29::zero();
    // lane i == m reads invd[0] = 0: its q is 0 for now and adds nothing to the partial
#define KMP_Q(k)                                                                                                               \
  if (i##k < a.n) {                                                                                                            \
    const Fr29 d = Fr29::from_fr(ld_fr(a.invd + ((i##k - m) & mask)));                                                         \
    const Fr29 q = Fr29::mul(Fr29::mul(Fr29::sub_lazy(a##k, ym), d), cw);                                                      \
    g##k = Fr29::add_csub(g##k, q);                                                                                            \
    h = Fr29::add_csub(h, Fr29::mul(q, p##k));                                                                                 \
  }
    KMP_Q(0) KMP_Q(1) KMP_Q(2) KMP_Q(3)
#undef KMP_Q
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      Fr29 o;
#pragma unroll
      for (int x = 0; x < 9; ++x) o.l[x] = __shfl_down(h.l[x], off, 64);
      h = Fr29::add_csub(h, o);
    }
    if (!lane) st_fr(a.partial + (uint64_t)gi * nwaves + wave, h.to_fr());
  }
#define KMP_STORE(k)                                                                \
  if (i##k < a.n) {                                                                 \
    Fr29 r = g##k;                                                                  \
    if (accumulate) r = Fr29::add_csub(r, Fr29::from_fr(ld_fr(a.g + i##k)));        \
    st_fr(a.g + i##k, r.to_fr());                                                   \
  }
  KMP_STORE(0) KMP_STORE(1) KMP_STORE(2) KMP_STORE(3)
#undef KMP_STORE
}

// one workgroup per group of the launch
__global__ void __launch_bounds__(256) kmp_fix_kernel(const Fr* __restrict__ partial, uint32_t nwaves, uint32_t first,
                                                      const uint32_t* __restrict__ group_m, const Fr* __restrict__ negw, Fr* __restrict__ g) {
  __shared__ Fr sh[256];
  const uint32_t t = threadIdx.x, grp = first + blockIdx.x;
  Fr acc = Fr::zero();
  for (uint32_t x = t; x < nwaves; x += 256) acc = acc + ld_fr(partial + (uint64_t)blockIdx.x * nwaves + x);
  sh[t] = acc;
  __syncthreads();
  for (uint32_t h = 128; h; h >>= 1) {
    if (t < h) sh[t] = sh[t] + sh[t + h];
    __syncthreads();
  }
  if (!t) {
    Fr* at = g + group_m[grp];
    st_fr(at, ld_fr(at) + sh[0] * ld_fr(negw + grp));
  }
}

__global__ void __launch_bounds__(256) kmp_weights_den_kernel(Fr w, Fr t, const uint32_t* __restrict__ point_index, uint32_t K,
                                                              Fr* __restrict__ wt) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  st_fr(wt + k, t - kmp_pow(w, point_index[k]));
}

// blocks [0, M): vector j = blockIdx.x; block M: y
__global__ void __launch_bounds__(KMP_LANES) kmp_weights_kernel(const Fr* __restrict__ wt, const Fr* __restrict__ rpow, const Fr* __restrict__ yk,
                                                                const uint32_t* __restrict__ perm, const uint32_t* __restrict__ off, uint32_t K,
                                                                uint32_t M, Fr t, void* __restrict__ stw, Fr* __restrict__ y_out,
                                                                uint32_t* __restrict__ sc, uint32_t* __restrict__ ids) {
  __shared__ Fr sh[KMP_LANES];
  const uint32_t j = blockIdx.x, lane = threadIdx.x;
  Fr acc = Fr::zero();
  if (j < M) {
    const uint32_t end = off[j + 1];
    for (uint32_t x = off[j] + lane; x < end; x += KMP_LANES) {
      const uint32_t k = perm[x];
      acc = acc + ld_fr(rpow + k) * ld_fr(wt + k);
    }
  } else {
    for (uint32_t k = lane; k < K; k += KMP_LANES) acc = acc + ld_fr(rpow + k) * ld_fr(wt + k) * ld_fr(yk + k);
  }
  const Fr sum = kmp_wave_sum(acc, sh, lane);
  if (lane) return;
  if (j < M) {
    if (stw) st_slot(stw, j, Fr29::twiddle_from_fr(sum));
    if (sc) {
      st_fr(reinterpret_cast<Fr*>(sc + 8ull * j), sum.from_mont());
      ids[j] = j;
    }
    return;
  }
  if (y_out) st_fr(y_out, sum);
  if (sc) {
    st_fr(reinterpret_cast<Fr*>(sc + 8ull * M), Fr::one().neg().from_mont());
    st_fr(reinterpret_cast<Fr*>(sc + 8ull * (M + 1)), t.from_mont());
    st_fr(reinterpret_cast<Fr*>(sc + 8ull * (M + 2)), sum.neg().from_mont());
    ids[M] = M;
    ids[M + 1] = M + 1;
    ids[M + 2] = M + 2;
  }
}

// ---- launchers (kzg_multiproof.hpp) ------------------------------------------------------------------------------------------
int kmp_invd(Ctx* c, uint32_t log_n, Fr* invd, KzeMeta* meta) {
  if (log_n < 1 || log_n > 32) return kzg_bad_args("kmp_invd");
  PTRY(kze_denominators(c, log_n, Fr::one(), invd, meta));
  return poly_batch_inverse(c, invd, 1ull << log_n);
}

int kmp_gather(Ctx* c, const Fr* const* vecs, const uint32_t* vector_index, const uint32_t* point_index, uint64_t K, Fr* yk) {
  if (!K || K > KMP_MAX_ITEMS) return kzg_bad_args("kmp_gather");
  hipLaunchKernelGGL(kmp_gather_kernel, dim3((uint32_t)((K + 255) / 256)), dim3(256), 0, c->stream, vecs, vector_index, point_index,
                     (uint32_t)K, yk);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kmp_groups(Ctx* c, uint32_t log_n, const Fr* rpow, const Fr* yk, const uint32_t* perm, const uint32_t* group_m,
               const uint32_t* group_off, uint64_t groups, Fr* ym, void* cw, Fr* negw) {
  if (!groups || groups > KMP_MAX_ITEMS || log_n < 1 || log_n > 32) return kzg_bad_args("kmp_groups");
  hipLaunchKernelGGL(kmp_groups_kernel, dim3((uint32_t)groups), dim3(KMP_LANES), 0, c->stream, fr_domain_root(log_n).inv(),
                     Fr::from_u64(32), rpow, yk, perm, group_m, group_off, ym, cw, negw);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kmp_aggregate(Ctx* c, const KmpAggArgs& a, uint64_t groups) {
  if (!groups || groups > KMP_MAX_ITEMS || a.n != (1ull << a.log_n) || a.log_n < 1 || a.log_n > 32) return kzg_bad_args("kmp_aggregate");
  const uint32_t nwaves = kze_fold_waves(a.n), blocks = kze_fold_blocks(a.n);
  const Fr w = fr_domain_root(a.log_n), w_step = w.pow_u64(KMP_AGG_T);
  prof_begin(c, 12);   // slot 12: every aggregate and fix launch of the call
  for (uint64_t first = 0; first < groups; first += KMP_GROUP_CHUNK) {
    const uint32_t cnt = (uint32_t)(groups - first < KMP_GROUP_CHUNK ? groups - first : KMP_GROUP_CHUNK);
    hipLaunchKernelGGL(kmp_aggregate_kernel, dim3(blocks), dim3(KMP_AGG_T), 0, c->stream, a, (uint32_t)first, cnt, first ? 1 : 0, w, w_step,
                       nwaves);
    hipLaunchKernelGGL(kmp_fix_kernel, dim3(cnt), dim3(256), 0, c->stream, (const Fr*)a.partial, nwaves, (uint32_t)first, a.group_m, a.negw, a.g);
  }
  prof_end(c, 12);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kmp_weights(Ctx* c, uint32_t log_n, const Fr& t, const uint32_t* point_index, const Fr* rpow, const Fr* yk, const uint32_t* perm,
                const uint32_t* off, uint64_t K, uint64_t M, Fr* wt, void* stw, Fr* y_out, uint32_t* sc, uint32_t* ids) {
  if (!K || K > KMP_MAX_ITEMS || !M || M > KMP_MAX_VECTORS || log_n < 1 || log_n > 32) return kzg_bad_args("kmp_weights");
  hipLaunchKernelGGL(kmp_weights_den_kernel, dim3((uint32_t)((K + 255) / 256)), dim3(256), 0, c->stream, fr_domain_root(log_n), t,
                     point_index, (uint32_t)K, wt);
  HIP_TRY(hipGetLastError());
  PTRY(poly_batch_inverse(c, wt, K));
  hipLaunchKernelGGL(kmp_weights_kernel, dim3((uint32_t)M + 1), dim3(KMP_LANES), 0, c->stream, (const Fr*)wt, rpow, yk, perm, off, (uint32_t)K,
                     (uint32_t)M, t, stw, y_out, sc, ids);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the state a domain handle holds for plonk_kzg_multiproof_open ------------------------------------------------------------
struct KmpBufs {
  enum { VECS, STAGE, VIDX, MIDX, PERM_M, GROUP_M, GROUP_OFF, PERM_V, OFF_V, YK, RPOW, RTW, YM, CW, NEGW, G, PARTIAL, WT, STW, YOUT, DEN,
         FOLD_PARTIAL, EVALS, Q, QPART, META, NBUF };   // grow-only
};
struct KzgMulti : KmpBufs, DevBufs<KmpBufs::NBUF> {
  Fr* invd = nullptr;           // 1 / (w^s - 1), s < n; built by the first call
  uint64_t invd_bytes = 0;
  Fr last_r = Fr::zero(), last_t = Fr::zero();
  plonk_kzg_multiproof_info last = {};
  ~KzgMulti() { (void)hipFree(invd); }
};

void kmp_release(KzgMulti* multi) { delete multi; }

namespace {

struct StreamDrain {   // an error leaves nothing of the call queued, and nothing reads the host vectors of the call after they are gone
  Ctx& c;
  ~StreamDrain() { (void)hipStreamSynchronize(c.stream); }
};

struct OpenCall {
  const void* const* vecs;
  uint64_t M;
  const uint8_t* commitments_in;
  const uint32_t* vector_index;
  const uint32_t* point_index;
  uint64_t K;
  const uint8_t* label;
  uint64_t label_len;
  bool has_override;
  Fr r, t;
  bool resident;
  uint64_t* values;
  uint8_t* commitments_out;
  uint8_t* proof96;
};

int open_body(const char* api_fn, KzgDomain* d, KzgMulti* s, const OpenCall& a) {
  Ctx& c = *d->c;
  const uint32_t L = d->log_n;
  const uint64_t n = 1ull << L, M = a.M, K = a.K;
  // the host side of the call: sorted before anything is queued
  std::vector<uint32_t> perm_m(K), group_m(K < n ? K : n), group_off((K < n ? K : n) + 1), scratch(n + 1), perm_v(K), off_v(M + 1);
  std::vector<const Fr*> table(M);
  std::vector<Fr> yk(K);
  std::vector<uint8_t> cm(48 * M);
  const uint64_t groups = kmp_sort_points(a.point_index, K, n, perm_m.data(), group_m.data(), group_off.data(), scratch.data());
  kmp_counting_sort(a.vector_index, K, M, perm_v.data(), off_v.data());
  const KmpPlan plan = kmp_plan(L, M, K, groups, a.commitments_in == nullptr, !a.resident);
  StreamDrain drain{c};
  plonk_kzg_multiproof_info info = {};
  info.log_n = L;
  info.items = K;
  info.vectors = M;
  info.point_groups = groups;
  info.commitments_computed = plan.commitments_computed;
  info.msm_launches = plan.msm_launches;
  info.msm_terms = plan.msm_terms;
  info.products = plan.products;
  // ---- the vectors on the device, the canonical-form check of the resident form, the claimed values ----
  PTRY(s->need(KzgMulti::META, sizeof(KzeMeta)));
  PTRY(s->need(KzgMulti::VECS, sizeof(Fr*) * M));
  PTRY(s->need(KzgMulti::VIDX, 4 * K));
  PTRY(s->need(KzgMulti::MIDX, 4 * K));
  PTRY(s->need(KzgMulti::YK, sizeof(Fr) * K));
  if (a.resident) {
    for (uint64_t j = 0; j < M; ++j) table[j] = (const Fr*)a.vecs[j];
  } else {
    PTRY(s->need(KzgMulti::STAGE, sizeof(Fr) * plan.stage_values));
    for (uint64_t j = 0; j < M; ++j) {
      table[j] = s->at<Fr>(KzgMulti::STAGE) + j * n;
      HIP_TRY(hipMemcpyAsync((void*)table[j], a.vecs[j], sizeof(Fr) * n, hipMemcpyHostToDevice, c.stream));
    }
  }
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::VECS], table.data(), sizeof(Fr*) * M, hipMemcpyHostToDevice, c.stream));
  const Fr* const* vecs = s->at<const Fr*>(KzgMulti::VECS);
  if (a.resident) {
    KzeMeta mh = {KZE_NONE, 0};
    HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::META], &mh, sizeof mh, hipMemcpyHostToDevice, c.stream));
    PTRY(kze_scan(&c, vecs, 0, (uint32_t)M, n, s->at<KzeMeta>(KzgMulti::META)));
    HIP_TRY(hipMemcpyAsync(&mh, s->p[KzgMulti::META], sizeof mh, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (mh.bad) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
  }
  if (!s->invd) {
    Fr* t = nullptr;
    HIP_TRY(hipMalloc((void**)&t, sizeof(Fr) * n));
    const int rc = kmp_invd(&c, L, t, s->at<KzeMeta>(KzgMulti::META));
    if (rc != PLONK_OK) {
      (void)hipStreamSynchronize(c.stream);
      (void)hipFree(t);
      return rc;
    }
    s->invd = t;
    s->invd_bytes = sizeof(Fr) * n;
  }
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::VIDX], a.vector_index, 4 * K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::MIDX], a.point_index, 4 * K, hipMemcpyHostToDevice, c.stream));
  PTRY(kmp_gather(&c, vecs, s->at<const uint32_t>(KzgMulti::VIDX), s->at<const uint32_t>(KzgMulti::MIDX), K, s->at<Fr>(KzgMulti::YK)));
  HIP_TRY(hipMemcpyAsync(yk.data(), s->p[KzgMulti::YK], sizeof(Fr) * K, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  // ---- the commitments and r ----
  PTRY(kze_points_ready(d, &info.built_points));
  kze_tables_call_begin(d);   // (a handle with tables: the M commitments are one run of grouped launches, D and pi one launch each)
  if (a.commitments_in) {
    memcpy(cm.data(), a.commitments_in, 48 * M);
  } else {
    PTRY(kze_commit_list(d, table.data(), M, cm.data()));
  }
  Transcript tr(a.label, a.label_len);
  Fr r = a.r, t = a.t;
  if (!a.has_override) r = kmp_challenge_r(tr, L, cm.data(), M, a.vector_index, a.point_index, (const uint64_t*)yk.data(), K);
  // ---- g and D ----
  const uint64_t chunk = groups < KMP_GROUP_CHUNK ? groups : KMP_GROUP_CHUNK;
  PTRY(s->need(KzgMulti::PERM_M, 4 * K));
  PTRY(s->need(KzgMulti::GROUP_M, 4 * groups));
  PTRY(s->need(KzgMulti::GROUP_OFF, 4 * (groups + 1)));
  PTRY(s->need(KzgMulti::PERM_V, 4 * K));
  PTRY(s->need(KzgMulti::OFF_V, 4 * (M + 1)));
  PTRY(s->need(KzgMulti::RPOW, sizeof(Fr) * K));
  PTRY(s->need(KzgMulti::RTW, sizeof(Fr29Slot) * K));
  PTRY(s->need(KzgMulti::YM, sizeof(Fr) * groups));
  PTRY(s->need(KzgMulti::CW, sizeof(Fr29Slot) * groups));
  PTRY(s->need(KzgMulti::NEGW, sizeof(Fr) * groups));
  PTRY(s->need(KzgMulti::G, sizeof(Fr) * n));
  PTRY(s->need(KzgMulti::PARTIAL, sizeof(Fr) * chunk * plan.waves));
  PTRY(s->need(KzgMulti::WT, sizeof(Fr) * K));
  PTRY(s->need(KzgMulti::STW, sizeof(Fr29Slot) * M));
  PTRY(s->need(KzgMulti::YOUT, sizeof(Fr)));
  PTRY(s->need(KzgMulti::DEN, sizeof(Fr) * n));
  PTRY(s->need(KzgMulti::FOLD_PARTIAL, sizeof(Fr) * KZE_GROUP * plan.waves));
  PTRY(s->need(KzgMulti::EVALS, sizeof(Fr) * M));
  PTRY(s->need(KzgMulti::Q, sizeof(Fr) * n));
  PTRY(s->need(KzgMulti::QPART, sizeof(Fr) * kze_quotient_blocks(n)));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::PERM_M], perm_m.data(), 4 * K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::GROUP_M], group_m.data(), 4 * groups, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::GROUP_OFF], group_off.data(), 4 * (groups + 1), hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::PERM_V], perm_v.data(), 4 * K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMulti::OFF_V], off_v.data(), 4 * (M + 1), hipMemcpyHostToDevice, c.stream));
  PTRY(poly_power_array(&c, s->at<Fr>(KzgMulti::RPOW), K, r));
  PTRY(poly_kzg_powers(&c, s->p[KzgMulti::RTW], (uint32_t)K, r));
  PTRY(kmp_groups(&c, L, s->at<const Fr>(KzgMulti::RPOW), s->at<const Fr>(KzgMulti::YK), s->at<const uint32_t>(KzgMulti::PERM_M),
                    s->at<const uint32_t>(KzgMulti::GROUP_M), s->at<const uint32_t>(KzgMulti::GROUP_OFF), groups, s->at<Fr>(KzgMulti::YM),
                    s->p[KzgMulti::CW], s->at<Fr>(KzgMulti::NEGW)));
  KmpAggArgs ag;
  ag.vecs = vecs;
  ag.vector_index = s->at<const uint32_t>(KzgMulti::VIDX);
  ag.rtw = s->p[KzgMulti::RTW];
  ag.perm = s->at<const uint32_t>(KzgMulti::PERM_M);
  ag.group_m = s->at<const uint32_t>(KzgMulti::GROUP_M);
  ag.group_off = s->at<const uint32_t>(KzgMulti::GROUP_OFF);
  ag.ym = s->at<const Fr>(KzgMulti::YM);
  ag.cw = s->p[KzgMulti::CW];
  ag.negw = s->at<const Fr>(KzgMulti::NEGW);
  ag.invd = s->invd;
  ag.n = n;
  ag.log_n = L;
  ag.g = s->at<Fr>(KzgMulti::G);
  ag.partial = s->at<Fr>(KzgMulti::PARTIAL);
  PTRY(kmp_aggregate(&c, ag, groups));
  uint8_t proof[96];
  PTRY(kze_commit_values(d, ag.g, proof));
  // ---- t, h - g, the opening at t ----
  if (!a.has_override) {
    t = kmp_challenge_t(tr, proof);
    if (kze_in_domain(t, L)) API_FAIL(PLONK_ERR_STATE, "the transcript's challenge t lies in the domain (probability n / q): open again under another label");
  }
  PTRY(kmp_weights(&c, L, t, s->at<const uint32_t>(KzgMulti::MIDX), s->at<const Fr>(KzgMulti::RPOW), s->at<const Fr>(KzgMulti::YK),
                     s->at<const uint32_t>(KzgMulti::PERM_V), s->at<const uint32_t>(KzgMulti::OFF_V), K, M, s->at<Fr>(KzgMulti::WT),
                     s->p[KzgMulti::STW], s->at<Fr>(KzgMulti::YOUT), nullptr, nullptr));
  PTRY(kze_denominators(&c, L, t, s->at<Fr>(KzgMulti::DEN), s->at<KzeMeta>(KzgMulti::META)));
  PTRY(poly_batch_inverse(&c, s->at<Fr>(KzgMulti::DEN), n));
  PTRY(poly_scale_array(&c, ag.g, n, Fr::one().neg()));   // the fold below adds h to -g
  KzeFoldArgs fa;
  fa.vecs = vecs;
  fa.vpow = s->p[KzgMulti::STW];
  fa.n = n;
  fa.accumulate = 1;
  fa.inv = s->at<Fr>(KzgMulti::DEN);
  fa.m = KZE_NONE;
  fa.fold = ag.g;
  fa.partial = s->at<Fr>(KzgMulti::FOLD_PARTIAL);
  fa.z = t;
  fa.scale = kze_eval_scale(t, L);
  for (uint64_t first = 0; first < M; first += KZE_GROUP) {
    fa.first = (uint32_t)first;
    fa.count = (uint32_t)(M - first < KZE_GROUP ? M - first : KZE_GROUP);
    PTRY(kze_fold_eval(&c, fa, s->at<Fr>(KzgMulti::EVALS) + first));
  }
  Fr y;
  HIP_TRY(hipMemcpyAsync(&y, s->p[KzgMulti::YOUT], sizeof y, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  PTRY(kze_quotient(&c, L, ag.g, s->at<Fr>(KzgMulti::DEN), y, KZE_NONE, s->at<Fr>(KzgMulti::Q), s->at<Fr>(KzgMulti::QPART)));
  PTRY(kze_commit_values(d, s->at<Fr>(KzgMulti::Q), proof + 48));
  // ---- the call's outputs ----
  memcpy(a.values, yk.data(), sizeof(Fr) * K);
  if (a.commitments_out) memcpy(a.commitments_out, cm.data(), 48 * M);
  memcpy(a.proof96, proof, 96);
  s->last_r = r;
  s->last_t = t;
  s->last = info;
  return PLONK_OK;
}

int open_impl(const char* api_fn, plonk_kzg_domain* dom, const void* const* vecs, uint64_t nvectors, const uint8_t* commitments_in,
              const uint32_t* vector_index, const uint32_t* point_index, uint64_t count, const uint8_t* label, uint64_t label_len,
              const uint64_t* challenges_override, uint64_t* values, uint8_t* commitments_out, uint8_t* proof96, bool resident) {
  if (!dom || !vecs || !vector_index || !point_index || !values || !proof96 || (label_len && !label))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  if (kmp_check_items(d->log_n, nvectors, vector_index, point_index, count, !resident, false))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 2^20], nvectors in [1, 65536], every index in range and (host form) nvectors * n <= 2^28");
  for (uint64_t j = 0; j < nvectors; ++j)
    if (!vecs[j]) API_FAIL(PLONK_ERR_ARG, "invalid argument: evals[j] is NULL");
  OpenCall a = {vecs, nvectors, commitments_in, vector_index, point_index, count, label, label_len, challenges_override != nullptr,
                Fr::zero(), Fr::zero(), resident, values, commitments_out, proof96};
  if (kmp_check_override(challenges_override, d->log_n, &a.r, &a.t))
    API_FAIL(PLONK_ERR_DATA, "the challenges override is not canonical, or its t lies in the domain");
  if (!resident && !kze_host_canonical(vecs, nvectors, 1ull << d->log_n)) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
  KZD_ENTER(d, api_fn, KZD_WORK);
  return open_body(api_fn, d, kzd_state(d->multi), a);
}

// ---- plonk_kzg_multiproof_check: the workspace hangs off the key ----------------------------------------------------------------
struct KmcBufs {
  enum { COMP, PTS, KIND, SC, IDS, MIDX, PERM_V, OFF_V, YK, RPOW, WT, NBUF };   // grow-only
};
struct KzgMultiCheck : KmcBufs, DevBufs<KmcBufs::NBUF> {};

struct CheckCall {
  uint32_t log_n;
  const uint8_t* commitments48;
  uint64_t M;
  const uint32_t* vector_index;
  const uint32_t* point_index;
  const uint64_t* values;
  uint64_t K;
  const uint8_t* proof96;
  const uint8_t* label;
  uint64_t label_len;
  bool has_override;
  Fr r, t;
};

int check_body(const char* api_fn, KzgKey* kk, const CheckCall& a, plonk_verify_info* info) {
  Ctx& c = *kk->c;
  if (!kk->multiproof) kk->multiproof = new KzgMultiCheck();
  KzgMultiCheck* s = (KzgMultiCheck*)kk->multiproof;
  const uint64_t M = a.M, K = a.K, npts = M + 3;
  std::vector<uint32_t> perm_v(K), off_v(M + 1);
  std::vector<uint8_t> comp(48 * npts);
  std::vector<int32_t> st;
  StreamDrain drain{c};
  const auto t0 = std::chrono::steady_clock::now();
  // the point table [C_0 .. C_(M-1) | D | pi | g]: decoded and subgroup-checked on the device
  PTRY(s->need(KzgMultiCheck::COMP, 48 * npts));
  PTRY(s->need(KzgMultiCheck::PTS, sizeof(G1Affine) * npts));
  PTRY(s->need(KzgMultiCheck::KIND, 4 * npts));
  memcpy(comp.data(), a.commitments48, 48 * M);
  memcpy(comp.data() + 48 * M, a.proof96, 96);
  memcpy(comp.data() + 48 * (M + 2), kk->opening_key, 48);
  PTRY(decode_points(&c, comp.data(), (uint32_t)npts, s->at<uint8_t>(KzgMultiCheck::COMP), s->at<G1Affine>(KzgMultiCheck::PTS),
                       s->at<int32_t>(KzgMultiCheck::KIND), &st));
  for (uint64_t i = 0; i < npts; ++i)
    if (st[i] == VDEC_BAD) API_FAIL(PLONK_ERR_POINT, "a commitment, D or pi is not a valid compressed point of G1");
  const auto t1 = std::chrono::steady_clock::now();
  Fr r = a.r, t = a.t;
  if (!a.has_override) {
    Transcript tr(a.label, a.label_len);
    r = kmp_challenge_r(tr, a.log_n, a.commitments48, M, a.vector_index, a.point_index, a.values, K);
    t = kmp_challenge_t(tr, a.proof96);
    if (kze_in_domain(t, a.log_n)) API_FAIL(PLONK_ERR_VERIFY, "the transcript's challenge t lies in the domain: no prover returns such a proof");
  }
  kmp_counting_sort(a.vector_index, K, M, perm_v.data(), off_v.data());
  PTRY(s->need(KzgMultiCheck::SC, 32 * npts));
  PTRY(s->need(KzgMultiCheck::IDS, 4 * npts));
  PTRY(s->need(KzgMultiCheck::MIDX, 4 * K));
  PTRY(s->need(KzgMultiCheck::PERM_V, 4 * K));
  PTRY(s->need(KzgMultiCheck::OFF_V, 4 * (M + 1)));
  PTRY(s->need(KzgMultiCheck::YK, sizeof(Fr) * K));
  PTRY(s->need(KzgMultiCheck::RPOW, sizeof(Fr) * K));
  PTRY(s->need(KzgMultiCheck::WT, sizeof(Fr) * K));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMultiCheck::MIDX], a.point_index, 4 * K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMultiCheck::PERM_V], perm_v.data(), 4 * K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMultiCheck::OFF_V], off_v.data(), 4 * (M + 1), hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(s->p[KzgMultiCheck::YK], a.values, sizeof(Fr) * K, hipMemcpyHostToDevice, c.stream));
  PTRY(poly_power_array(&c, s->at<Fr>(KzgMultiCheck::RPOW), K, r));
  PTRY(kmp_weights(&c, a.log_n, t, s->at<const uint32_t>(KzgMultiCheck::MIDX), s->at<const Fr>(KzgMultiCheck::RPOW),
                     s->at<const Fr>(KzgMultiCheck::YK), s->at<const uint32_t>(KzgMultiCheck::PERM_V), s->at<const uint32_t>(KzgMultiCheck::OFF_V),
                     K, M, s->at<Fr>(KzgMultiCheck::WT), nullptr, nullptr, s->at<uint32_t>(KzgMultiCheck::SC), s->at<uint32_t>(KzgMultiCheck::IDS)));
  G1Affine pi_aff;
  HIP_TRY(hipMemcpyAsync(&pi_aff, s->at<G1Affine>(KzgMultiCheck::PTS) + M + 1, sizeof pi_aff, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  const auto t2 = std::chrono::steady_clock::now();
  // one launch of msm_points' kernels; plonk_ctx_last_msm_points keeps describing the caller's own last call
  const plonk_msm_points_info keep = c.last_points;
  const bool keep_valid = c.last_points_valid;
  MpInput in;
  in.sc = s->at<const uint32_t>(KzgMultiCheck::SC);
  in.ids = s->at<const uint32_t>(KzgMultiCheck::IDS);
  in.pts = s->at<const G1Affine>(KzgMultiCheck::PTS);
  in.kind = s->at<const int32_t>(KzgMultiCheck::KIND);
  G1 sum;
  const int rc = msm_points_run(&c, in, npts, nullptr, &sum);
  c.last_points = keep;
  c.last_points_valid = keep_valid;
  PTRY(rc);
  const auto t3 = std::chrono::steady_clock::now();
  const H1 sums[2] = {h1_of_g1(st[M + 1] == VDEC_OK ? G1::from_affine(pi_aff) : G1::identity()), h1_of_g1(sum)};
  const bool ok = pairing_check(sums, kk->x_h, kk->h);
  const auto t4 = std::chrono::steady_clock::now();
  if (info) {
    info->proofs = K;
    info->msm_terms = npts;
    info->pairing_checks = 1;
    info->rejected = ok ? 0 : (uint32_t)K;
    info->ms_decode = ms_between(t0, t1);
    info->ms_scalars = ms_between(t1, t2);
    info->ms_msm = ms_between(t2, t3);
    info->ms_pairing = ms_between(t3, t4);
  }
  if (!ok) API_FAIL(PLONK_ERR_VERIFY, "the multiproof does not verify");
  return PLONK_OK;
}

}  // namespace

int kmp_open_entered(const char* api_fn, KzgDomain* d, const void* const* vecs_dev, uint64_t nvectors, const uint8_t* commitments_in,
                     const uint32_t* vector_index, const uint32_t* point_index, uint64_t count, const uint8_t* label, uint64_t label_len,
                     const uint64_t* challenges_override, uint64_t* values, uint8_t* proof96) {
  if (!vecs_dev || !commitments_in || !vector_index || !point_index || !values || !proof96 || (label_len && !label))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (kmp_check_items(d->log_n, nvectors, vector_index, point_index, count, false, false))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 2^20], nvectors in [1, 65536] and every index in range");
  OpenCall a = {vecs_dev, nvectors, commitments_in, vector_index, point_index, count, label, label_len, challenges_override != nullptr,
                Fr::zero(), Fr::zero(), true, values, nullptr, proof96};
  if (kmp_check_override(challenges_override, d->log_n, &a.r, &a.t))
    API_FAIL(PLONK_ERR_DATA, "the challenges override is not canonical, or its t lies in the domain");
  return open_body(api_fn, d, kzd_state(d->multi), a);
}

void kmp_check_release(void* ws) { delete (KzgMultiCheck*)ws; }

KzgKey::~KzgKey() {
  (void)hipFree(pair_tables);
  kmp_check_release(multiproof);
}

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_kzg_multiproof_open(plonk_kzg_domain* domain, const uint64_t* const* evals, uint64_t nvectors, const uint8_t* commitments_in,
                              const uint32_t* vector_index, const uint32_t* point_index, uint64_t count, const uint8_t* label,
                              uint64_t label_len, const uint64_t* challenges_override, uint64_t* values, uint8_t* commitments_out,
                              uint8_t proof96[96]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::open_impl(api_fn, domain, (const void* const*)evals, nvectors, commitments_in, vector_index, point_index, count, label,
                            label_len, challenges_override, values, commitments_out, proof96, false);
  });
}

int plonk_kzg_multiproof_open_dev(plonk_kzg_domain* domain, const void* const* evals_dev, uint64_t nvectors, const uint8_t* commitments_in,
                                  const uint32_t* vector_index, const uint32_t* point_index, uint64_t count, const uint8_t* label,
                                  uint64_t label_len, const uint64_t* challenges_override, uint64_t* values, uint8_t* commitments_out,
                                  uint8_t proof96[96]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::open_impl(api_fn, domain, evals_dev, nvectors, commitments_in, vector_index, point_index, count, label, label_len,
                            challenges_override, values, commitments_out, proof96, true);
  });
}

int plonk_kzg_multiproof_last(plonk_kzg_domain* domain, plonk_kzg_multiproof_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!domain || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgDomain* d = domain->d;
  KZD_ENTER(d, api_fn, KZD_KEY);
  const KzgMulti* s = d->multi;
  plonk_kzg_multiproof_info info = {};
  info.log_n = d->log_n;
  info.msm_terms = 1ull << d->log_n;
  if (s) {
    if (s->last.log_n) info = s->last;
    info.device_bytes = s->invd_bytes + s->bytes();
  }
  *out = info;
  return PLONK_OK;
  });
}

int plonk_kzg_multiproof_check(plonk_kzg_key* key, uint32_t log_n, const uint8_t* commitments48, uint64_t ncommitments,
                               const uint32_t* vector_index, const uint32_t* point_index, const uint64_t* values, uint64_t count,
                               const uint8_t proof96[96], const uint8_t* label, uint64_t label_len, const uint64_t* challenges_override,
                               plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!key || !commitments48 || !vector_index || !point_index || !values || !proof96 || (label_len && !label))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (kmp_check_items(log_n, ncommitments, vector_index, point_index, count, false, true))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: log_n must be in [1, 20], count in [1, 2^20], ncommitments in [1, 65536] and every index in range");
  CheckCall a = {log_n, commitments48, ncommitments, vector_index, point_index, values, count, proof96, label, label_len,
                 challenges_override != nullptr, Fr::zero(), Fr::zero()};
  Fr x;
  for (uint64_t k = 0; k < count; ++k)
    if (!kzg_fr_load(values + 4 * k, &x)) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
  if (kmp_check_override(challenges_override, log_n, &a.r, &a.t))
    API_FAIL(PLONK_ERR_DATA, "the challenges override is not canonical, or its t lies in the domain");
  if (info) memset(info, 0, sizeof *info);
  Ctx& c = *key->k->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  return check_body(api_fn, key->k, a, info);
  });
}

// Test hook (not in include/plonk_hip.h, not part of the API), for tests/test_gpu_kzg_multiproof.py through the binding's
// KzgDomain._multi_last_challenges: r and t of the handle's last plonk_kzg_multiproof_open (Montgomery limbs).
int plonk_test_kzg_multiproof_last_challenges(plonk_kzg_domain* domain, uint64_t out[8]) {
  if (!domain || !out) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(domain->d->c->mu);
  const KzgMulti* s = domain->d->multi;
  if (!s) return PLONK_ERR_STATE;
  memcpy(out, s->last_r.l, 32);
  memcpy(out + 4, s->last_t.l, 32);
  return PLONK_OK;
}

}  // extern "C"
