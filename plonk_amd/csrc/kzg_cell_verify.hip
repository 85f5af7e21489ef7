// KZG10 cell verification: the checking side of kzg_cells.hip.  The equations, the layouts and the plan are in
// kzg_cell_verify_core.hpp; DESIGN.md section 17 has the derivation, the resources and the measurements.  The decoding, the
// two folded sums (msm_points_run in the term layout), the host pairing and the per-item pairing kernel are those the other
// checks use; new here:
//
//   kzv_key_kernel        once per handle: the first l points of the commit key as the 96-byte affine points msm_points_run reads
//   kzv_twist_kernel      one item per workgroup (256 / l items where l <= 64): the cell's values into LDS bit-reversed, the
//                         inverse decimation in time of kzc_ntt_kernel with the inverse twiddles, element j times
//                         l^-1 * weight_i * (w^(-k_i))^j; lane j builds that power from log l squarings the item shares in LDS
//   kzv_colsum_kernel     R_j = sum_i c'_ij: lane (j, slice) adds 64 rows, the passes repeat until one row is left; no atomics
//                         (field addition is exact, any order gives the same bytes); the last pass writes the terms -R_j s_j
//   kzv_weights_kernel    one wave per commitment: W_c over its segment of the host's counting sort; one lane per item: rho^i
//                         and rho^i x_(k_i)
//   kzv_cell_sums_kernel  the per-item path, one wave per item: lane t takes the terms -c_ij s_j, j = t, t + 64, ... one after
//                         the other through the split double-and-add into an accumulator that stays in registers (as
//                         kzc_mulacc_kernel), lane 0 adds C, lane 1 takes x_k pi as one more term, an LDS tree over the 64
//                         partials; (A_i, B_i) and the pre-verdict in the layout pairing_each_launch reads
// Every addition is the complete law (G1R::add).  A zero scalar or an identity operand multiplies nothing.
#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "poly.hpp"
#include "kzg_core.hpp"
#include "kzg_key.hpp"
#include "kzg_cell_verify.hpp"
#include "devmem.cuh"

namespace plonk {

__global__ void __launch_bounds__(64) kzv_key_kernel(const G1AffineR* __restrict__ row0, uint32_t count, G1Affine* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  G1Affine a;
  a.x = ld_f28(&row0[i].x).to_fp();
  a.y = ld_f28(&row0[i].y).to_fp();
  st_aff(out + i, a);
}

// dynamic LDS: kzv_twist_lds_bytes(log_cell), l values per item of the workgroup
__global__ void __launch_bounds__(KZV_LANES) kzv_twist_kernel(const Fr* __restrict__ values, const uint32_t* __restrict__ cell_index,
                                                              const Fr* __restrict__ weights, uint32_t count, uint32_t log_cell,
                                                              const Fr* __restrict__ winv, const Fr* __restrict__ itw, Fr l_inv,
                                                              Fr* __restrict__ out, uint32_t* flags) {
  extern __shared__ uint4 kzv_twist_lds[];
  const uint32_t l = 1u << log_cell;
  const uint32_t lpi = kzv_lanes_per_item(log_cell), per = kzv_items_per_group(log_cell);
  const uint32_t sub = per > 1 ? threadIdx.x >> log_cell : 0u, t = threadIdx.x - sub * lpi;
  const uint64_t item = (uint64_t)blockIdx.x * per + sub;
  const bool live = item < count;
  Fr* sh = reinterpret_cast<Fr*>(kzv_twist_lds) + ((uint64_t)sub << log_cell);
  // (w^(-k))^(2^s), s < log l, in the item's first slots; each lane multiplies its power together, then the slots are free
  if (live && t == 0) {
    Fr b = ld_fr(winv + cell_index[item]);
    for (uint32_t s = 0; s < log_cell; ++s) {
      sh[s] = b;
      b = b * b;
    }
  }
  __syncthreads();
  Fr p = l_inv, step = Fr::one();
  if (live) {
    if (weights) p = p * ld_fr(weights + item);
    for (uint32_t s = 0; s < log_cell && (t >> s); ++s)
      if ((t >> s) & 1u) p = p * sh[s];
    if (l > KZV_LANES) step = sh[8];   // (w^(-k))^256: from element j to element j + 256
  }
  __syncthreads();
  bool bad = false;
  if (live)
    for (uint32_t j = t; j < l; j += lpi) {
      const Fr v = ld_fr(values + item * l + j);
      bad |= !kzv_canonical(v);
      sh[kzd_rev(j, log_cell)] = v;
    }
  // the item's lanes agree through its flag: a workgroup-scope fence and the barrier order the store before the load
  if (bad) flags[item] = 1u;
  __threadfence_block();
  __syncthreads();
  const bool item_bad = live && *reinterpret_cast<const volatile uint32_t*>(flags + item) != 0;
  const bool work = live && !item_bad;
  for (uint32_t s = 0; s < log_cell; ++s) {
    const uint32_t half = 1u << s;
    if (work)
      for (uint32_t e = t; e < l / 2; e += lpi) {
        const uint32_t j = e & (half - 1), lo = ((e - j) << 1) + j, hi = lo + half;
        Fr b = sh[hi];
        if (j) b = b * ld_fr(itw + ((uint64_t)j << (log_cell - 1 - s)));
        const Fr a = sh[lo];
        sh[lo] = a + b;
        sh[hi] = a - b;
      }
    __syncthreads();
  }
  if (live)
    for (uint32_t j = t; j < l; j += lpi) {
      st_fr(out + item * l + j, work ? sh[j] * p : Fr::zero());
      p = p * step;
    }
}

// grid = (ceil(l / 64), slices); sc == nullptr: out[slice][j] = the sum of the slice's rows; otherwise (one slice) the terms
__global__ void __launch_bounds__(KZV_COLSUM_LANES) kzv_colsum_kernel(const Fr* __restrict__ rows, uint64_t nrows, uint32_t log_cell,
                                                                      Fr* __restrict__ out, uint32_t* __restrict__ sc,
                                                                      uint32_t* __restrict__ ids) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >> log_cell) return;
  const uint64_t first = (uint64_t)blockIdx.y * KZV_COLSUM_ROWS;
  const uint64_t last = first + KZV_COLSUM_ROWS < nrows ? first + KZV_COLSUM_ROWS : nrows;
  Fr acc = Fr::zero();
  for (uint64_t i = first; i < last; ++i) acc = acc + ld_fr(rows + (i << log_cell) + j);
  if (sc) {
    st_fr(reinterpret_cast<Fr*>(sc + 8ull * j), acc.neg().from_mont());
    ids[j] = j;
  } else {
    st_fr(out + ((uint64_t)blockIdx.y << log_cell) + j, acc);
  }
}

// blocks [0, M): commitment c = blockIdx.x; blocks from M on: 64 items each
__global__ void __launch_bounds__(64) kzv_weights_kernel(const Fr* __restrict__ pw, const uint32_t* __restrict__ cell_index,
                                                         const Fr* __restrict__ xk, const uint32_t* __restrict__ perm,
                                                         const uint32_t* __restrict__ off, uint32_t K, uint32_t M, uint32_t log_cell,
                                                         uint32_t* __restrict__ sc, uint32_t* __restrict__ ids) {
  __shared__ Fr sh[64];
  const uint32_t lane = threadIdx.x, l = 1u << log_cell;
  if (blockIdx.x < M) {
    const uint32_t c = blockIdx.x, end = off[c + 1];
    Fr acc = Fr::zero();
    for (uint32_t t = off[c] + lane; t < end; t += 64) acc = acc + ld_fr(pw + perm[t]);
    sh[lane] = acc;
    __syncthreads();
    for (uint32_t s = 32; s; s >>= 1) {
      if (lane < s) sh[lane] = sh[lane] + sh[lane + s];
      __syncthreads();
    }
    if (!lane) {
      st_fr(reinterpret_cast<Fr*>(sc + 8ull * (K + c)), sh[0].from_mont());
      ids[K + c] = l + c;
    }
    return;
  }
  const uint32_t i = (blockIdx.x - M) * 64 + lane;
  if (i >= K) return;
  const Fr w = ld_fr(pw + i);
  st_fr(reinterpret_cast<Fr*>(sc + 8ull * i), w.from_mont());
  ids[i] = l + M + i;
  st_fr(reinterpret_cast<Fr*>(sc + 8ull * ((uint64_t)K + M + i)), (w * ld_fr(xk + cell_index[i])).from_mont());
  ids[K + M + i] = l + M + i;
}

// glv_split (curve28.cuh) and kzd_mul_split (devmem.cuh) with the scalar's words picked by compile-time indexes: inside
// kzv_cell_sums_kernel the compiler leaves the run-time indexed words of the originals in private memory (72 bytes of scratch
// per lane); here they stay in registers.  The same arithmetic, step for step.
__device__ __forceinline__ GlvScalar kzv_glv_split(const Fr& k) {
  constexpr uint64_t LH = 0xac45a4010001a402ull, LL = 0x00000000ffffffffull;   // LAMBDA
  uint64_t rh = 0, rl = 0, qh = 0, ql = 0;
#pragma unroll
  for (int w = 7; w >= 0; --w) {
    const uint32_t word = k.l[w];
    for (int b = w == 7 ? 30 : 31; b >= 0; --b) {   // bits 254 .. 0
      const uint64_t top = rh >> 63;
      rh = (rh << 1) | (rl >> 63);
      rl = (rl << 1) | ((word >> b) & 1u);
      const bool ge = top || rh > LH || (rh == LH && rl >= LL);
      if (ge) {
        const uint64_t borrow = rl < LL ? 1u : 0u;
        rl -= LL;
        rh -= LH + borrow;
      }
      qh = (qh << 1) | (ql >> 63);
      ql = (ql << 1) | (ge ? 1u : 0u);
    }
  }
  GlvScalar g;
  g.k1[0] = rl; g.k1[1] = rh; g.k2[0] = ql; g.k2[1] = qh;
  return g;
}
__device__ __forceinline__ G1R kzv_mul_steps(G1R acc, uint64_t k1, uint64_t k2, const G1R& p, const G1R& p2, const G1R& p3) {
  for (int b = 63; b >= 0; --b) {
    acc = acc.dbl();
    const uint32_t s = (uint32_t)((k1 >> b) & 1u) | ((uint32_t)((k2 >> b) & 1u) << 1);
    if (s) acc = acc.add(s == 1 ? p : (s == 2 ? p2 : p3));
  }
  return acc;
}
__device__ __forceinline__ G1R kzv_mul_split(const G1R& p, const GlvScalar& g) {
  if (p.is_identity()) return p;
  G1R p2 = p;
  p2.X = Fp28::mul(p.X, glv_beta());
  const G1R p3 = p.add(p2);
  return kzv_mul_steps(kzv_mul_steps(G1R::identity(), g.k1[1], g.k2[1], p, p2, p3), g.k1[0], g.k2[0], p, p2, p3);
}

__global__ void __launch_bounds__(KZV_SUMS_LANES) kzv_cell_sums_kernel(const Fr* __restrict__ coeffs, const uint32_t* __restrict__ commitment_index,
                                                                       const uint32_t* __restrict__ cell_index, const Fr* __restrict__ xk,
                                                                       const uint32_t* __restrict__ flags, const G1Affine* __restrict__ pts,
                                                                       const int32_t* __restrict__ kind, uint32_t M, uint32_t log_cell,
                                                                       G1* __restrict__ pairs, int32_t* __restrict__ pre) {
  __shared__ G1R sh[KZV_SUMS_LANES];
  const uint32_t i = blockIdx.x, lane = threadIdx.x, l = 1u << log_cell;
  const uint32_t pc = l + commitment_index[i], pp = l + M + i;
  const int32_t kc = kind[pc], kp = kind[pp];
  int32_t verdict = 0;
  if (kc == VDEC_BAD || kp == VDEC_BAD) verdict = PLONK_ERR_POINT;
  if (flags[i]) verdict = PLONK_ERR_DATA;   // the values are looked at first, as the folded call does
  if (verdict) {   // the whole wave
    if (!lane) pre[i] = verdict;
    return;
  }
  // lane t: the terms j = t, t + 64, ... < l; lane 1 takes x_k pi as one more
  const uint32_t mine = (l > lane ? (l - lane + KZV_SUMS_LANES - 1) / KZV_SUMS_LANES : 0u) + (lane == 1 ? 1u : 0u);
  G1R acc = G1R::identity();
  for (uint32_t it = 0; it < mine; ++it) {
    const uint32_t j = lane + KZV_SUMS_LANES * it;
    const bool extra = j >= l;
    if (extra && kp != VDEC_OK) continue;   // the identity proof
    const Fr raw = ld_fr(extra ? xk + cell_index[i] : coeffs + ((uint64_t)i << log_cell) + j);
    const Fr s = (extra ? raw : raw.neg()).from_mont();
    const uint32_t p = extra ? pp : j;
    if (s.is_zero()) continue;
    const G1Affine a = ld_aff(pts + p);
    const G1R term = kzv_mul_split(G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)), kzv_glv_split(s));
    if (!term.is_identity()) acc = acc.add(term);
  }
  if (lane == 0 && kc == VDEC_OK) {
    const G1Affine a = ld_aff(pts + pc);
    acc = acc.add(G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)));
  }
  sh[lane] = acc;
  __syncthreads();
  for (uint32_t s = KZV_SUMS_LANES / 2; s; s >>= 1) {
    if (lane < s) sh[lane] = sh[lane].add(sh[lane + s]);
    __syncthreads();
  }
  if (!lane) {
    pre[i] = 0;
    st_g1(pairs + 2ull * i, kp == VDEC_OK ? G1::from_affine(ld_aff(pts + pp)) : G1::identity());
    st_g1(pairs + 2ull * i + 1, sh[0].to_g1());
  }
}

// ---- launchers (kzg_cell_verify.hpp) ------------------------------------------------------------------------------------------
int kzv_key_copy(Ctx* c, uint64_t count, G1Affine* out) {
  if (!c->srs_table || !count || count > c->srs_n) return kzg_bad_args("kzv_key_copy");
  hipLaunchKernelGGL(kzv_key_kernel, dim3((uint32_t)((count + 63) / 64)), dim3(64), 0, c->stream, (const G1AffineR*)c->srs_table,
                     (uint32_t)count, out);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzv_twist(Ctx* c, const Fr* values, const uint32_t* cell_index, const Fr* weights, uint64_t count, uint32_t log_cell,
              const Fr* winv, const Fr* itw, Fr* out, uint32_t* flags) {
  if (log_cell < 1 || log_cell > KZC_NTT_MAX_LOG || !count || count > KZV_MAX_ITEMS || (count << log_cell) > KZV_MAX_VALUES)
    return kzg_bad_args("kzv_twist");
  hipLaunchKernelGGL(kzv_twist_kernel, dim3((uint32_t)kzv_twist_groups(log_cell, count)), dim3(KZV_LANES), kzv_twist_lds_bytes(log_cell),
                     c->stream, values, cell_index, weights, (uint32_t)count, log_cell, winv, itw, Fr::from_u64(1ull << log_cell).inv(),
                     out, flags);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzv_colsum(Ctx* c, const Fr* rows, uint64_t count, uint32_t log_cell, Fr* part0, Fr* part1, uint32_t* sc, uint32_t* ids) {
  if (log_cell < 1 || log_cell > KZC_NTT_MAX_LOG || !count || count > KZV_MAX_ITEMS) return kzg_bad_args("kzv_colsum");
  const uint32_t gx = ((1u << log_cell) + KZV_COLSUM_LANES - 1) / KZV_COLSUM_LANES;
  Fr* part[2] = {part0, part1};
  int b = 0;
  while (count > KZV_COLSUM_ROWS) {
    const uint64_t slices = kzv_colsum_slices(count);
    hipLaunchKernelGGL(kzv_colsum_kernel, dim3(gx, (uint32_t)slices), dim3(KZV_COLSUM_LANES), 0, c->stream, rows, count, log_cell,
                       part[b], (uint32_t*)nullptr, (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    rows = part[b];
    count = slices;
    b ^= 1;
  }
  hipLaunchKernelGGL(kzv_colsum_kernel, dim3(gx, 1), dim3(KZV_COLSUM_LANES), 0, c->stream, rows, count, log_cell, (Fr*)nullptr, sc, ids);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzv_weights(Ctx* c, const Fr* pw, const uint32_t* cell_index, const Fr* xk, const uint32_t* perm, const uint32_t* off, uint64_t K,
                uint64_t M, uint32_t log_cell, uint32_t* sc, uint32_t* ids) {
  if (!K || K > KZV_MAX_ITEMS || M > KZV_MAX_COMMITMENTS) return kzg_bad_args("kzv_weights");
  hipLaunchKernelGGL(kzv_weights_kernel, dim3((uint32_t)(M + (K + 63) / 64)), dim3(64), 0, c->stream, pw, cell_index, xk, perm, off,
                     (uint32_t)K, (uint32_t)M, log_cell, sc, ids);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzv_cell_sums(Ctx* c, const Fr* coeffs, const uint32_t* commitment_index, const uint32_t* cell_index, const Fr* xk,
                  const uint32_t* flags, const G1Affine* pts, const int32_t* kind, uint64_t K, uint64_t M, uint32_t log_cell, G1* pairs,
                  int32_t* pre) {
  if (log_cell < 1 || log_cell > KZC_NTT_MAX_LOG || !K || K > KZV_MAX_ITEMS || M > KZV_MAX_COMMITMENTS) return kzg_bad_args("kzv_cell_sums");
  hipLaunchKernelGGL(kzv_cell_sums_kernel, dim3((uint32_t)K), dim3(KZV_SUMS_LANES), 0, c->stream, coeffs, commitment_index, cell_index, xk,
                     flags, pts, kind, (uint32_t)M, log_cell, pairs, pre);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the handle -------------------------------------------------------------------------------------------------------------
namespace {

struct KzvBufs {
  enum { VALUES, CIDX, KIDX, PERM, OFF, FLAGS, POW, COEFFS, PART0, PART1, COMP, PTS, KIND, SC, IDS, PAIRS, PRE, VERDICT, NBUF };   // grow-only
};
struct KzgCellVerifier : KzvBufs, DevBufs<KzvBufs::NBUF> {
  plonk_kzg_key* key = nullptr;
  uint32_t log_n = 0, log_cell = 0, key_checked = 0;
  G1Affine* key_pts = nullptr;   // s_0 .. s_(l-1) (and s_l while the key is checked)
  Fr* xk = nullptr;              // w^(l k), k < r
  Fr* winv = nullptr;            // w^(-k), k < r
  Fr* itw = nullptr;             // w_l^(-e), e < l / 2
  uint64_t fixed_bytes = 0;
  Fr last_rho = Fr::zero();
  uint32_t forced_min[2] = {0, 0};   // test door: opts.min_bucket_terms of the left / right sum
  plonk_kzg_cell_verify_info last = {};
  ~KzgCellVerifier() {
    (void)hipFree(key_pts);
    (void)hipFree(xk);
    (void)hipFree(winv);
    (void)hipFree(itw);
  }
};

int create_body(const char* api_fn, KzgCellVerifier* v, KzgKey* kk) {
  Ctx& c = *kk->c;
  const uint32_t log_r = v->log_n - v->log_cell;
  const uint64_t l = 1ull << v->log_cell, r = 1ull << log_r;
  const bool check = c.srs_n > l;
  const uint64_t npts = l + (check ? 1 : 0);
  HIP_TRY(hipMalloc((void**)&v->key_pts, sizeof(G1Affine) * npts));
  HIP_TRY(hipMalloc((void**)&v->xk, sizeof(Fr) * r));
  HIP_TRY(hipMalloc((void**)&v->winv, sizeof(Fr) * r));
  HIP_TRY(hipMalloc((void**)&v->itw, sizeof(Fr) * (l / 2)));
  v->fixed_bytes = sizeof(G1Affine) * npts + sizeof(Fr) * (2 * r + l / 2);
  PTRY(kzv_key_copy(&c, npts, v->key_pts));
  PTRY(poly_power_array(&c, v->xk, r, fr_domain_root(log_r)));
  PTRY(poly_power_array(&c, v->winv, r, fr_domain_root(v->log_n).inv()));
  PTRY(poly_power_array(&c, v->itw, l / 2, fr_domain_root(v->log_cell).inv()));
  G1Affine s0, sl;
  HIP_TRY(hipMemcpyAsync(&s0, v->key_pts, sizeof s0, hipMemcpyDeviceToHost, c.stream));
  if (check) HIP_TRY(hipMemcpyAsync(&sl, v->key_pts + l, sizeof sl, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  if (memcmp(s0.x.l, kk->g_aff.x.l, 48) || memcmp(s0.y.l, kk->g_aff.y.l, 48))
    API_FAIL(PLONK_ERR_VERIFY, "the first point of the commit key is not the opening key's g");
  if (check) {   // e(-s_0, x_h) e(s_l, h) == 1: x_h is [tau^l] h
    const H1 sums[2] = {h1_of_g1(G1::from_affine(s0)), h1_of_g1(G1::from_affine(sl))};
    if (!pairing_check(sums, kk->x_h, kk->h))
      API_FAIL(PLONK_ERR_VERIFY, "the key's third element is not [tau^l] h for the commit key's tau and this cell size");
    v->key_checked = 1;
  }
  return PLONK_OK;
}

struct CallArgs {
  const uint8_t* commitments48;
  uint64_t M;
  const uint32_t* commitment_index;
  const uint32_t* cell_index;
  const uint64_t* values;
  const uint8_t* proofs48;
  uint64_t K;
};

// the point table [s | C | pi] decoded, the values and the cell indexes on the device; st: the kinds of the M + K decoded points
int stage_inputs(KzgCellVerifier* v, Ctx& c, const CallArgs& a, std::vector<int32_t>* st) {
  const uint64_t l = 1ull << v->log_cell;
  const KzvLayout lay = kzv_layout(v->log_cell, a.M, a.K);
  PTRY(v->need(KzgCellVerifier::COMP, 48 * (a.M + a.K)));
  PTRY(v->need(KzgCellVerifier::PTS, sizeof(G1Affine) * lay.points));
  PTRY(v->need(KzgCellVerifier::KIND, 4 * lay.points));
  PTRY(v->need(KzgCellVerifier::VALUES, sizeof(Fr) * l * a.K));
  PTRY(v->need(KzgCellVerifier::COEFFS, sizeof(Fr) * l * a.K));
  PTRY(v->need(KzgCellVerifier::KIDX, 4 * a.K));
  PTRY(v->need(KzgCellVerifier::FLAGS, 4 * a.K));
  std::vector<uint8_t> comp(48 * (a.M + a.K));
  if (a.M) memcpy(comp.data(), a.commitments48, 48 * a.M);
  memcpy(comp.data() + 48 * a.M, a.proofs48, 48 * a.K);
  HIP_TRY(hipMemcpyAsync(v->p[KzgCellVerifier::PTS], v->key_pts, sizeof(G1Affine) * l, hipMemcpyDeviceToDevice, c.stream));
  HIP_TRY(hipMemsetAsync(v->p[KzgCellVerifier::KIND], 0, 4 * l, c.stream));   // VDEC_OK
  PTRY(decode_points(&c, comp.data(), (uint32_t)(a.M + a.K), v->at<uint8_t>(KzgCellVerifier::COMP),
                       v->at<G1Affine>(KzgCellVerifier::PTS) + l, v->at<int32_t>(KzgCellVerifier::KIND) + l, st));
  HIP_TRY(hipMemcpyAsync(v->p[KzgCellVerifier::VALUES], a.values, sizeof(Fr) * l * a.K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(v->p[KzgCellVerifier::KIDX], a.cell_index, 4 * a.K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemsetAsync(v->p[KzgCellVerifier::FLAGS], 0, 4 * a.K, c.stream));
  return PLONK_OK;
}

void fill_last(KzgCellVerifier* v, const CallArgs& a, bool each) {
  const KzvPlan p = kzv_plan(v->log_cell, a.M, a.K, each, v->forced_min[0], v->forced_min[1]);
  plonk_kzg_cell_verify_info& o = v->last;
  o = {};
  o.path_each = each ? 1 : 0;
  o.items = a.K;
  o.commitments = a.M;
  o.transforms = p.transforms;
  o.msm_terms_left = p.msm_terms_left;
  o.msm_terms_right = p.msm_terms_right;
  o.msm_path_left = p.msm_path_left;
  o.msm_path_right = p.msm_path_right;
  o.scalar_muls = p.scalar_muls;
}

// one of the two folded sums; plonk_ctx_last_msm_points keeps describing the caller's own last call
int folded_sum(KzgCellVerifier* v, Ctx& c, uint64_t first_term, uint64_t terms, uint32_t min_bucket_terms, H1* out) {
  const plonk_msm_points_info keep = c.last_points;
  const bool keep_valid = c.last_points_valid;
  MpInput in;
  in.sc = v->at<const uint32_t>(KzgCellVerifier::SC) + 8 * first_term;
  in.ids = v->at<const uint32_t>(KzgCellVerifier::IDS) + first_term;
  in.pts = v->at<const G1Affine>(KzgCellVerifier::PTS);
  in.kind = v->at<const int32_t>(KzgCellVerifier::KIND);
  plonk_msm_points_opts opts = {};
  opts.struct_size = sizeof opts;
  opts.min_bucket_terms = min_bucket_terms;
  G1 sum;
  const int rc = msm_points_run(&c, in, terms, &opts, &sum);
  c.last_points = keep;
  c.last_points_valid = keep_valid;
  PTRY(rc);
  *out = h1_of_g1(sum);
  return PLONK_OK;
}

int folded_body(const char* api_fn, KzgCellVerifier* v, Ctx& c, const CallArgs& a, const uint8_t* label, uint64_t label_len,
                const Fr* rho_override, plonk_verify_info* info) {
  KzgKey* kk = v->key->k;
  const uint64_t l = 1ull << v->log_cell, K = a.K, M = a.M;
  const KzvLayout lay = kzv_layout(v->log_cell, M, K);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> st;
  PTRY(stage_inputs(v, c, a, &st));
  for (uint64_t i = 0; i < M + K; ++i)
    if (st[i] == VDEC_BAD) API_FAIL(PLONK_ERR_POINT, "a commitment or a proof is not a valid compressed point of G1");
  const auto t1 = std::chrono::steady_clock::now();
  Fr rho;
  if (rho_override) {
    rho = *rho_override;
  } else {
    std::vector<uint8_t> cell(32 * l);
    rho = kzv_challenge(label, label_len, v->log_n, v->log_cell, kk->opening_key, a.commitments48, M, a.commitment_index, a.cell_index,
                        a.values, a.proofs48, K, cell.data());
  }
  v->last_rho = rho;
  std::vector<uint32_t> perm(K), off(M + 1);
  kzv_counting_sort(a.commitment_index, K, M, perm.data(), off.data());
  PTRY(v->need(KzgCellVerifier::PERM, 4 * K));
  PTRY(v->need(KzgCellVerifier::OFF, 4 * (M + 1)));
  PTRY(v->need(KzgCellVerifier::POW, sizeof(Fr) * K));
  const uint64_t slices = kzv_colsum_slices(K);
  PTRY(v->need(KzgCellVerifier::PART0, sizeof(Fr) * l * slices));
  PTRY(v->need(KzgCellVerifier::PART1, sizeof(Fr) * l * kzv_colsum_slices(slices)));
  PTRY(v->need(KzgCellVerifier::SC, 32 * lay.terms));
  PTRY(v->need(KzgCellVerifier::IDS, 4 * lay.terms));
  HIP_TRY(hipMemcpyAsync(v->p[KzgCellVerifier::PERM], perm.data(), 4 * K, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(v->p[KzgCellVerifier::OFF], off.data(), 4 * (M + 1), hipMemcpyHostToDevice, c.stream));
  PTRY(poly_power_array(&c, v->at<Fr>(KzgCellVerifier::POW), K, rho));
  PTRY(kzv_twist(&c, v->at<const Fr>(KzgCellVerifier::VALUES), v->at<const uint32_t>(KzgCellVerifier::KIDX), v->at<const Fr>(KzgCellVerifier::POW),
                   K, v->log_cell, v->winv, v->itw, v->at<Fr>(KzgCellVerifier::COEFFS), v->at<uint32_t>(KzgCellVerifier::FLAGS)));
  uint32_t* sc = v->at<uint32_t>(KzgCellVerifier::SC);
  uint32_t* ids = v->at<uint32_t>(KzgCellVerifier::IDS);
  PTRY(kzv_colsum(&c, v->at<const Fr>(KzgCellVerifier::COEFFS), K, v->log_cell, v->at<Fr>(KzgCellVerifier::PART0),
                    v->at<Fr>(KzgCellVerifier::PART1), sc + 8 * lay.term_r, ids + lay.term_r));
  PTRY(kzv_weights(&c, v->at<const Fr>(KzgCellVerifier::POW), v->at<const uint32_t>(KzgCellVerifier::KIDX), v->xk,
                     v->at<const uint32_t>(KzgCellVerifier::PERM), v->at<const uint32_t>(KzgCellVerifier::OFF), K, M, v->log_cell, sc, ids));
  HIP_TRY(hipStreamSynchronize(c.stream));   // perm / off are host vectors
  const auto t2 = std::chrono::steady_clock::now();
  H1 sums[2];
  PTRY(folded_sum(v, c, 0, K, v->forced_min[0], &sums[0]));
  PTRY(folded_sum(v, c, K, lay.terms - K, v->forced_min[1], &sums[1]));
  const auto t3 = std::chrono::steady_clock::now();
  const bool ok = pairing_check(sums, kk->x_h, kk->h);
  const auto t4 = std::chrono::steady_clock::now();
  fill_last(v, a, false);
  if (info) {
    info->proofs = K;
    info->msm_terms = lay.terms;
    info->pairing_checks = 1;
    info->rejected = ok ? 0 : (uint32_t)K;
    info->ms_decode = ms_between(t0, t1);
    info->ms_scalars = ms_between(t1, t2);
    info->ms_msm = ms_between(t2, t3);
    info->ms_pairing = ms_between(t3, t4);
  }
  if (!ok) API_FAIL(PLONK_ERR_VERIFY, "the batch of cells does not verify");
  return PLONK_OK;
}

int each_body(KzgCellVerifier* v, Ctx& c, const CallArgs& a, int32_t* verdicts, plonk_verify_info* info) {
  KzgKey* kk = v->key->k;
  const uint64_t l = 1ull << v->log_cell, K = a.K, M = a.M;
  PTRY(pairing_tables_create(&c, kk->x_h, kk->h, &kk->pair_tables));
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> st;
  PTRY(stage_inputs(v, c, a, &st));
  const auto t1 = std::chrono::steady_clock::now();
  PTRY(v->need(KzgCellVerifier::CIDX, 4 * K));
  PTRY(v->need(KzgCellVerifier::PAIRS, sizeof(G1) * 2 * K));
  PTRY(v->need(KzgCellVerifier::PRE, 4 * K));
  PTRY(v->need(KzgCellVerifier::VERDICT, 4 * K));
  HIP_TRY(hipMemcpyAsync(v->p[KzgCellVerifier::CIDX], a.commitment_index, 4 * K, hipMemcpyHostToDevice, c.stream));
  PTRY(kzv_twist(&c, v->at<const Fr>(KzgCellVerifier::VALUES), v->at<const uint32_t>(KzgCellVerifier::KIDX), nullptr, K, v->log_cell,
                   v->winv, v->itw, v->at<Fr>(KzgCellVerifier::COEFFS), v->at<uint32_t>(KzgCellVerifier::FLAGS)));
  HIP_TRY(hipStreamSynchronize(c.stream));
  const auto t2 = std::chrono::steady_clock::now();
  PTRY(kzv_cell_sums(&c, v->at<const Fr>(KzgCellVerifier::COEFFS), v->at<const uint32_t>(KzgCellVerifier::CIDX),
                       v->at<const uint32_t>(KzgCellVerifier::KIDX), v->xk, v->at<const uint32_t>(KzgCellVerifier::FLAGS),
                       v->at<const G1Affine>(KzgCellVerifier::PTS), v->at<const int32_t>(KzgCellVerifier::KIND), K, M, v->log_cell,
                       v->at<G1>(KzgCellVerifier::PAIRS), v->at<int32_t>(KzgCellVerifier::PRE)));
  HIP_TRY(hipStreamSynchronize(c.stream));
  const auto t3 = std::chrono::steady_clock::now();
  PTRY(pairing_each_launch(&c, kk->pair_tables, v->at<const G1>(KzgCellVerifier::PAIRS), v->at<const int32_t>(KzgCellVerifier::PRE), K,
                             v->at<int32_t>(KzgCellVerifier::VERDICT), nullptr));
  uint32_t checked = 0, rejected = 0;
  PTRY(each_finish(&c, v->at<const int32_t>(KzgCellVerifier::VERDICT), v->at<const int32_t>(KzgCellVerifier::PRE), K, verdicts, &checked,
                     &rejected));
  const auto t4 = std::chrono::steady_clock::now();
  fill_last(v, a, true);
  if (info) {
    info->proofs = K;
    info->msm_terms = (l + 2) * checked;
    info->pairing_checks = checked;
    info->rejected = rejected;
    info->ms_decode = ms_between(t0, t1);
    info->ms_scalars = ms_between(t1, t2);
    info->ms_msm = ms_between(t2, t3);
    info->ms_pairing = ms_between(t3, t4);
  }
  return rejected ? PLONK_ERR_VERIFY : PLONK_OK;
}

}  // namespace
}  // namespace plonk

struct plonk_kzg_cell_verifier {
  plonk::KzgCellVerifier* v;
  plonk_kzg_key* key;
};

using namespace plonk;

extern "C" {

int plonk_kzg_cell_verifier_create(plonk_kzg_key* key_l, uint32_t log_n, uint32_t log_cell, plonk_kzg_cell_verifier** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!key_l || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  *out = nullptr;
  if (kzv_check_shape(log_n, log_cell))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: log_n must be in [2, 20] and log_cell in [1, min(log_n - 1, 11)]");
  KzgKey* kk = key_l->k;
  Ctx& c = *kk->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  if (c.nccl_comm) API_FAIL(PLONK_ERR_STATE, "a context with a communicator holds only a range of the commit key");
  if (!c.srs_table || !c.srs_n) return PLONK_ERR_NO_SRS;
  if (c.srs_n < (1ull << log_cell)) API_FAIL(PLONK_ERR_DEGREE, "the commit key has fewer points than a cell has values");
  std::unique_ptr<KzgCellVerifier> v(new KzgCellVerifier());
  v->key = key_l;
  v->log_n = log_n;
  v->log_cell = log_cell;
  const int rc = create_body(api_fn, v.get(), kk);
  if (rc != PLONK_OK) {
    (void)hipStreamSynchronize(c.stream);
    return rc;
  }
  *out = new plonk_kzg_cell_verifier{v.release(), key_l};
  return PLONK_OK;
  });
}

void plonk_kzg_cell_verifier_destroy(plonk_kzg_cell_verifier* v) {
  if (!v) return;
  (void)plonk::api_guard(__func__, [&]() -> int {
    std::lock_guard<std::mutex> lk(v->key->ctx->c.mu);
    delete v->v;
    return PLONK_OK;
  });
  delete v;
}

static int kzv_entry_checks(const char* api_fn, plonk_kzg_cell_verifier* v, const CallArgs& a) {
  if (!v || !a.commitment_index || !a.cell_index || !a.values || !a.proofs48 || (a.M && !a.commitments48))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (kzv_check_items(v->v->log_n, v->v->log_cell, a.M, a.commitment_index, a.cell_index, a.K))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: count > 2^20, count * l > 2^25, ncommitments > 65536 or an index out of range");
  return PLONK_OK;
}

int plonk_kzg_verify_cells(plonk_kzg_cell_verifier* v, const uint8_t* commitments48, uint64_t ncommitments,
                           const uint32_t* commitment_index, const uint32_t* cell_index, const uint64_t* values, const uint8_t* proofs48,
                           uint64_t count, const uint8_t* label, uint64_t label_len, const uint64_t* rho_override, plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  const CallArgs a = {commitments48, ncommitments, commitment_index, cell_index, values, proofs48, count};
  if (!v || (label_len && !label)) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count) PTRY(kzv_entry_checks(api_fn, v, a));
  else if (ncommitments > KZV_MAX_COMMITMENTS) API_FAIL(PLONK_ERR_ARG, "invalid argument: ncommitments > 65536");
  if (info) memset(info, 0, sizeof *info);
  if (count == 0) API_FAIL(PLONK_ERR_VERIFY, "empty batch");
  Fr rho = Fr::one();
  bool canon = true;
  if (rho_override) {
    memcpy(rho.l, rho_override, 32);
    canon = kzv_canonical(rho);
  }
  const uint64_t nvalues = count << v->v->log_cell;
  for (uint64_t i = 0; i < nvalues && canon; ++i) {
    Fr x;
    memcpy(x.l, values + 4 * i, 32);
    canon = kzv_canonical(x);
  }
  if (!canon) API_FAIL(PLONK_ERR_DATA, "non-canonical scalar");
  Ctx& c = *v->key->k->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  const int rc = folded_body(api_fn, v->v, c, a, label, label_len, rho_override ? &rho : nullptr, info);
  if (rc != PLONK_OK && rc != PLONK_ERR_VERIFY) (void)hipStreamSynchronize(c.stream);   // nothing of the call stays queued
  return rc;
  });
}

int plonk_kzg_verify_cells_each(plonk_kzg_cell_verifier* v, const uint8_t* commitments48, uint64_t ncommitments,
                                const uint32_t* commitment_index, const uint32_t* cell_index, const uint64_t* values,
                                const uint8_t* proofs48, uint64_t count, int32_t* verdicts, plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  const CallArgs a = {commitments48, ncommitments, commitment_index, cell_index, values, proofs48, count};
  if (!v || !verdicts) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count == 0) API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 2^20]");
  PTRY(kzv_entry_checks(api_fn, v, a));
  if (info) memset(info, 0, sizeof *info);
  Ctx& c = *v->key->k->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  const int rc = each_body(v->v, c, a, verdicts, info);
  if (rc != PLONK_OK && rc != PLONK_ERR_VERIFY) (void)hipStreamSynchronize(c.stream);
  if (rc == PLONK_ERR_VERIFY) set_last_error(api_fn, "at least one cell does not verify", __FILE__, __LINE__);
  return rc;
  });
}

int plonk_kzg_cell_verifier_last(plonk_kzg_cell_verifier* v, plonk_kzg_cell_verify_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!v || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  std::lock_guard<std::mutex> lk(v->key->ctx->c.mu);
  plonk_kzg_cell_verify_info info = v->v->last;
  info.log_n = v->v->log_n;
  info.log_cell = v->v->log_cell;
  info.key_checked = v->v->key_checked;
  info.device_bytes = v->v->fixed_bytes + v->v->bytes();
  *out = info;
  return PLONK_OK;
  });
}

// Test hooks (not in include/plonk_hip.h, not part of the API), for tests/test_gpu_kzg_cell_verify.py through the binding's
// KzgCellVerifier._last_rho / _force_paths: the challenge of the handle's last folded call (Montgomery limbs), and
// plonk_msm_points_opts.min_bucket_terms of the left / right sum of its next calls (0 restores msm_points' own rule).
int plonk_test_kzg_cell_verify_last_rho(plonk_kzg_cell_verifier* v, uint64_t rho_out[4]) {
  if (!v || !rho_out) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(v->key->ctx->c.mu);
  memcpy(rho_out, v->v->last_rho.l, 32);
  return PLONK_OK;
}

int plonk_test_kzg_cell_verify_force_paths(plonk_kzg_cell_verifier* v, uint32_t min_left, uint32_t min_right) {
  if (!v) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(v->key->ctx->c.mu);
  v->v->forced_min[0] = min_left;
  v->v->forced_min[1] = min_right;
  return PLONK_OK;
}

}  // extern "C"
