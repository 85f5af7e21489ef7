// KZG10 openings over a whole evaluation domain: the n witnesses of one polynomial at the n roots of unity by group FFTs
// (Feist-Khovratovich) instead of n MSMs.  The derivation, the index maps and the plan are in kzg_domain_core.hpp; DESIGN.md
// section 14 has the resources and the measurements.
//
//   kzd_twiddle_kernel    once per handle: w^e, e < n, reduced to canonical form and split through the endomorphism
//                         (glv_split), so that a butterfly starts at the 128-step double-and-add
//   kzd_load_kernel       once per handle: a = (s_0 .. s_(n-2), O ...) from row 0 of the commit-key tables
//   kzd_dif_kernel        one stage of a forward transform: (a, b) -> (a + b, [w^e] (a - b)); grid.y = polynomial
//   kzd_dit_kernel        one stage of an inverse transform: (a, b) -> (a + [w^-e] b, a - [w^-e] b)
//   kzd_reverse_kernel    g_t = f_(n-1-t): the scalar side of the Toeplitz product, transformed by the existing NTT
//   kzd_pointwise_kernel  P_p = [G_rev(p) / N] A_p, the scalar split per lane
//   kzd_extract_kernel    h_k = c_(n-2-k) from the lower half of a polynomial's slots into the upper half, h_(n-1) = O
//   kzd_finish_kernel     per witness: slot n + rev(i), safegcd inverse, the 48-byte compressed encoding on the device
//   kzd_scan_kernel       resident polynomials: trimmed length and the canonical-form check
// Every addition is the complete law (G1R::add): identities, equal and opposite points occur for real inputs (zero
// polynomials, G_i = 0, degenerate keys).  A twiddle of 1 multiplies nothing.  One wave per workgroup: the butterfly keeps
// four points live (the operand, its image under the endomorphism, their sum, the accumulator) — the 256-VGPR class of
// verify_msm_kernel.  A stage is a launch: a butterfly is ~224 point operations against four 256-byte accesses, the pass is
// bound by integer-VALU issue, not by HBM, and fusing stages would buy nothing.
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "hostg1.hpp"
#include "g1codec.cuh"
#include "kzg_core.hpp"
#include "kzg_handle.hpp"
#include "devmem.cuh"

namespace plonk {

__global__ void __launch_bounds__(KZD_LANES) kzd_twiddle_kernel(Fr w, uint64_t count, GlvScalar* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const Fr k = w.pow_u64(e).from_mont();
  out[e] = glv_split(k.l);
}

__global__ void __launch_bounds__(KZD_LANES) kzd_load_kernel(const G1AffineR* __restrict__ row0, uint64_t valid, uint64_t total,
                                                             G1RSlot* __restrict__ v) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  st_g1r(v + i, i < valid ? G1R::from_affine(ld_f28(&row0[i].x), ld_f28(&row0[i].y)) : G1R::identity());
}

__global__ void __launch_bounds__(KZD_LANES) kzd_load_raw_kernel(const G1Affine* __restrict__ pts, uint64_t count,
                                                                 G1RSlot* __restrict__ v) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const G1Affine a = pts[i];
  st_g1r(v + i, (a.x.is_zero() && a.y.is_zero()) ? G1R::identity() : G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)));
}

// stage with butterfly span `half` of a forward transform: pairs (blk * 2 half + j, + half)
__global__ void __launch_bounds__(KZD_LANES) kzd_dif_kernel(G1RSlot* __restrict__ v, uint64_t stride, uint32_t size_log, uint64_t half,
                                                            const GlvScalar* __restrict__ tw, uint32_t tw_log) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (1ull << size_log) / 2) return;
  G1RSlot* base = v + (uint64_t)blockIdx.y * stride;
  const uint64_t j = t & (half - 1), lo = ((t - j) << 1) + j, hi = lo + half;
  const G1R a = ld_g1r(base + lo), b = ld_g1r(base + hi);
  st_g1r(base + lo, a.add(b));
  G1R d = a.add(g1r_neg(b));
  bool negate;
  const uint64_t e = kzd_twiddle(size_log, half, j, tw_log, false, &negate);
  if (e != KZD_NONE) d = kzd_mul_split(d, ld_glv(tw + e));
  st_g1r(base + hi, d);
}

// stage with butterfly span `half` of an inverse transform; the factor w^-e is minus the table's w^(T - e)
__global__ void __launch_bounds__(KZD_LANES) kzd_dit_kernel(G1RSlot* __restrict__ v, uint64_t stride, uint32_t size_log, uint64_t half,
                                                            const GlvScalar* __restrict__ tw, uint32_t tw_log) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (1ull << size_log) / 2) return;
  G1RSlot* base = v + (uint64_t)blockIdx.y * stride;
  const uint64_t j = t & (half - 1), lo = ((t - j) << 1) + j, hi = lo + half;
  G1R b = ld_g1r(base + hi);
  bool negate;
  const uint64_t e = kzd_twiddle(size_log, half, j, tw_log, true, &negate);
  if (e != KZD_NONE) b = kzd_mul_split(g1r_neg(b), ld_glv(tw + e));
  const G1R a = ld_g1r(base + lo);
  st_g1r(base + lo, a.add(b));
  st_g1r(base + hi, a.add(g1r_neg(b)));
}

// g[b][t] = f[b][n - 1 - t] for t <= n - 2, 0 up to 2n; f is zero-padded to n coefficients
__global__ void kzd_reverse_kernel(const Fr* __restrict__ f, uint64_t n, Fr* __restrict__ g) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * n) return;
  const uint64_t src = kzd_g_src(n, t);
  st_fr(g + (uint64_t)blockIdx.y * 2 * n + t, src == KZD_NONE ? Fr::zero() : ld_fr(f + (uint64_t)blockIdx.y * n + src));
}

__global__ void __launch_bounds__(KZD_LANES) kzd_pointwise_kernel(const G1RSlot* __restrict__ A, const Fr* __restrict__ G,
                                                                  uint64_t g_stride, G1RSlot* __restrict__ out, uint64_t stride,
                                                                  uint32_t size_log, Fr scale) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (1ull << size_log)) return;
  const uint64_t i = kzd_rev(p, size_log);
  const Fr s = (ld_fr(G + (uint64_t)blockIdx.y * g_stride + i) * scale).from_mont();
  G1R r = G1R::identity();
  if (!s.is_zero()) r = kzd_mul_split(ld_g1r(A + p), glv_split(s.l));
  st_g1r(out + (uint64_t)blockIdx.y * stride + p, r);
}

__global__ void __launch_bounds__(KZD_LANES) kzd_extract_kernel(G1RSlot* __restrict__ v, uint64_t stride, uint64_t n) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  G1RSlot* base = v + (uint64_t)blockIdx.y * stride;
  const uint64_t src = kzd_h_src(n, k);
  st_g1r(base + n + k, src == KZD_NONE ? G1R::identity() : ld_g1r(base + src));
}

// G1Affine::to_bytes on the device: big-endian x, 0x80 compressed | 0x40 infinity | 0x20 y is the larger root
__global__ void __launch_bounds__(KZD_LANES) kzd_finish_kernel(const G1RSlot* __restrict__ v, uint64_t stride, uint64_t offset,
                                                               uint32_t log_n, int bitrev, uint8_t* __restrict__ out48) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = 1ull << log_n;
  if (i >= n) return;
  const G1R p = ld_g1r(v + (uint64_t)blockIdx.y * stride + offset + (bitrev ? kzd_rev(i, log_n) : i));
  uint32_t w[12];
  g1r_compress48_words(p, w);
  uint4* q = reinterpret_cast<uint4*>(out48 + 48ull * ((uint64_t)blockIdx.y * n + i));
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
  q[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// meta[2 b] = trimmed length of polynomial b (atomicMax over its lanes), meta[2 b + 1] != 0: a coefficient >= q
__global__ void kzd_scan_kernel(const KzdDesc* __restrict__ desc, unsigned long long* __restrict__ meta) {
  const KzdDesc d = desc[blockIdx.y];
  unsigned long long top = 0, bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.len; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(d.p + i);
    uint32_t nz = 0;
    bool lt = false;
    for (int k = 7; k >= 0; --k) nz |= w[k];
    for (int k = 7; k >= 0; --k)
      if (w[k] != FrP::MOD[k]) { lt = w[k] < FrP::MOD[k]; break; }
    if (nz) top = i + 1;
    if (!lt) bad = 1;
  }
  if (top) atomicMax(meta + 2 * blockIdx.y, top);
  if (bad) atomicOr(meta + 2 * blockIdx.y + 1, bad);
}

// ---- launchers (kzg_domain.hpp) ------------------------------------------------------------------------------------------
static dim3 kzd_grid(uint64_t lanes, uint32_t batch) { return dim3((uint32_t)((lanes + KZD_LANES - 1) / KZD_LANES), batch); }

int kzd_twiddles_create(Ctx* c, uint32_t tw_log, GlvScalar** out_dev) {
  const uint64_t count = 1ull << (tw_log - 1);
  GlvScalar* t = nullptr;
  HIP_TRY(hipMalloc((void**)&t, sizeof(GlvScalar) * count));
  hipLaunchKernelGGL(kzd_twiddle_kernel, kzd_grid(count, 1), dim3(KZD_LANES), 0, c->stream, fr_domain_root(tw_log), count, t);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    (void)hipFree(t);
    set_last_error("kzd_twiddles_create", hipGetErrorString(e), __FILE__, __LINE__);
    return PLONK_ERR_HIP;
  }
  *out_dev = t;
  return PLONK_OK;
}

int kzd_transform(Ctx* c, void* slots, uint64_t stride, uint32_t size_log, uint32_t batch, bool inverse, const GlvScalar* tw,
                  uint32_t tw_log, uint64_t* stage_launches, uint64_t* scalar_muls) {
  if (size_log < 1 || size_log > tw_log || !batch || batch > KZD_MAX_CHUNK) return PLONK_ERR_ARG;
  const uint64_t size = 1ull << size_log;
  const dim3 grid = kzd_grid(size / 2, batch);
  for (uint32_t s = 0; s < size_log; ++s) {
    const uint64_t half = inverse ? 1ull << s : size >> (s + 1);
    if (inverse) hipLaunchKernelGGL(kzd_dit_kernel, grid, dim3(KZD_LANES), 0, c->stream, (G1RSlot*)slots, stride, size_log, half, tw, tw_log);
    else hipLaunchKernelGGL(kzd_dif_kernel, grid, dim3(KZD_LANES), 0, c->stream, (G1RSlot*)slots, stride, size_log, half, tw, tw_log);
    HIP_TRY(hipGetLastError());
    if (stage_launches) ++*stage_launches;
    if (scalar_muls) *scalar_muls += kzd_stage_muls(size_log, half) * batch;
  }
  return PLONK_OK;
}

int kzd_pointwise(Ctx* c, const void* A, const Fr* G, uint64_t g_stride, void* out_slots, uint64_t stride, uint32_t size_log,
                  uint32_t batch, const Fr& scale) {
  if (!batch || batch > KZD_MAX_CHUNK) return PLONK_ERR_ARG;
  hipLaunchKernelGGL(kzd_pointwise_kernel, kzd_grid(1ull << size_log, batch), dim3(KZD_LANES), 0, c->stream, (const G1RSlot*)A, G,
                     g_stride, (G1RSlot*)out_slots, stride, size_log, scale);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzd_extract(Ctx* c, void* slots, uint64_t stride, uint32_t log_n, uint32_t batch) {
  if (!batch || batch > KZD_MAX_CHUNK) return PLONK_ERR_ARG;
  hipLaunchKernelGGL(kzd_extract_kernel, kzd_grid(1ull << log_n, batch), dim3(KZD_LANES), 0, c->stream, (G1RSlot*)slots, stride,
                     1ull << log_n);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzd_finish(Ctx* c, const void* slots, uint64_t stride, uint64_t offset, uint32_t log_n, uint32_t batch, bool bitrev,
               uint8_t* out48) {
  if (!batch || batch > KZD_MAX_CHUNK) return PLONK_ERR_ARG;
  hipLaunchKernelGGL(kzd_finish_kernel, kzd_grid(1ull << log_n, batch), dim3(KZD_LANES), 0, c->stream, (const G1RSlot*)slots, stride,
                     offset, log_n, bitrev ? 1 : 0, out48);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzd_load_raw(Ctx* c, const G1Affine* xy96, uint64_t count, void* slots) {
  if (!count) return PLONK_OK;
  hipLaunchKernelGGL(kzd_load_raw_kernel, kzd_grid(count, 1), dim3(KZD_LANES), 0, c->stream, xy96, count, (G1RSlot*)slots);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the handle ------------------------------------------------------------------------------------------------------------
static const char KZD_NEEDS_WHOLE_KEY[] = "a context with a communicator holds only a range of the commit key";

int kzd_enter_checks(const char* api_fn, const KzgDomain* d, uint32_t checks) {
  const Ctx& c = *d->c;
  if (checks & KZD_SET_DEVICE) HIP_TRY(hipSetDevice(c.device));
  if ((checks & KZD_KEY) && d->srs_gen != c.srs_gen) API_FAIL(PLONK_ERR_STATE, "the domain is bound to a commit key that was replaced on its context");
  if ((checks & KZD_WHOLE_KEY) && c.nccl_comm) API_FAIL(PLONK_ERR_STATE, KZD_NEEDS_WHOLE_KEY);
  return PLONK_OK;
}

static int domain_create_body(Ctx& c, uint32_t log_n, KzgDomain* d) {
  const uint64_t n = 1ull << log_n, N = 2 * n;
  d->c = &c;
  d->log_n = log_n;
  d->srs_gen = c.srs_gen;
  HIP_TRY(hipMalloc((void**)&d->A, sizeof(G1RSlot) * N));
  d->fixed_bytes = sizeof(G1RSlot) * N + sizeof(GlvScalar) * n;
  PTRY(kzd_twiddles_create(&c, log_n + 1, &d->tw));
  hipLaunchKernelGGL(kzd_load_kernel, kzd_grid(N, 1), dim3(KZD_LANES), 0, c.stream, (const G1AffineR*)c.srs_table, n - 1, N, d->A);
  HIP_TRY(hipGetLastError());
  PTRY(kzd_transform(&c, d->A, N, log_n + 1, 1, false, d->tw, log_n + 1, nullptr, nullptr));
  HIP_TRY(hipStreamSynchronize(c.stream));
  d->last.log_n = log_n;
  d->last.workspace_cap_bytes = d->ws_cap;
  d->last.device_bytes = d->device_bytes();
  return PLONK_OK;
}

// ---- the chunk steps (kzg_domain.hpp) ----------------------------------------------------------------------------------------
int kzd_stage(Ctx* c, Fr* f, uint64_t n, const void* const* polys, const uint64_t* trimmed, uint32_t cnt) {
  HIP_TRY(hipMemsetAsync(f, 0, sizeof(Fr) * n * cnt, c->stream));
  for (uint32_t b = 0; b < cnt; ++b)
    if (trimmed[b]) HIP_TRY(hipMemcpyAsync(f + (uint64_t)b * n, polys[b], sizeof(Fr) * trimmed[b], hipMemcpyDefault, c->stream));
  return PLONK_OK;
}

int kzd_witnesses(Ctx* c, void* slots, uint64_t stride, uint32_t log_w, uint32_t cnt, const GlvScalar* tw, uint32_t tw_log,
                  uint64_t* stage_launches, uint64_t* scalar_muls, uint8_t* out48) {
  const uint64_t w = 1ull << log_w;
  PTRY(kzd_transform(c, slots, stride, log_w + 1, cnt, true, tw, tw_log, stage_launches, scalar_muls));
  PTRY(kzd_extract(c, slots, stride, log_w, cnt));
  PTRY(kzd_transform(c, (G1RSlot*)slots + w, stride, log_w, cnt, false, tw, tw_log, stage_launches, scalar_muls));
  return kzd_finish(c, slots, stride, w, log_w, cnt, true, out48);
}

int kzd_drained(Ctx* c, int rc) {
  if (rc != PLONK_OK) {
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->stream);
  }
  return rc;
}

int kzd_commit(Ctx* c, const Fr* f, uint64_t n, const uint64_t* m, uint32_t cnt, std::vector<uint8_t>& comm, void* dst48) {
  comm.resize(48ull * cnt);
  uint8_t* out48 = comm.data();
  const Fr* sc[MSM_MAX_BATCH];
  uint64_t mm[MSM_MAX_BATCH];
  uint32_t which[MSM_MAX_BATCH];
  G1 sums[MSM_MAX_BATCH];
  uint8_t aff[MSM_MAX_BATCH][97];
  int g = 0;
  for (uint32_t i = 0; i <= cnt; ++i) {
    if (i < cnt) {
      if (!m[i]) { identity48(out48 + 48ull * i); continue; }
      sc[g] = f + (uint64_t)i * n; mm[g] = m[i]; which[g] = i; ++g;
    }
    if (g == MSM_MAX_BATCH || (i == cnt && g)) {
      PTRY(msm_group_sums(c, sc, mm, g, sums));
      batch_xyzz_to_affine97(sums, g, aff);
      for (int k = 0; k < g; ++k) g1_compress97(aff[k], out48 + 48ull * which[k]);
      g = 0;
    }
  }
  HIP_TRY(hipMemcpyAsync(dst48, out48, 48ull * cnt, hipMemcpyDefault, c->stream));
  return PLONK_OK;
}

static int domain_open_body(KzgDomain* d, const void* const* polys, const uint64_t* trimmed, uint64_t count, void* evaluations,
                            void* witnesses48, void* commitments48) {
  Ctx& c = *d->c;
  const uint32_t L = d->log_n;
  const uint64_t n = 1ull << L, N = 2 * n;
  const KzdPlan plan = kzd_plan(L, count, d->ws_cap);
  const uint64_t chunk = plan.chunk_polys;
  PTRY(d->need(KzgDomain::WS, plan.ws_bytes));
  PTRY(d->need(KzgDomain::F, sizeof(Fr) * n * chunk));
  PTRY(d->need(KzgDomain::G, sizeof(Fr) * N * chunk));
  PTRY(d->need(KzgDomain::EVALS, sizeof(Fr) * n * chunk));
  PTRY(d->need(KzgDomain::TMP, sizeof(Fr) * N));
  PTRY(d->need(KzgDomain::OUT48, 48 * n * chunk));
  if (commitments48) PTRY(msm_reserve(&c, n));
  G1RSlot* ws = d->at<G1RSlot>(KzgDomain::WS);
  Fr* f = d->at<Fr>(KzgDomain::F);
  Fr* g = d->at<Fr>(KzgDomain::G);
  Fr* ev = d->at<Fr>(KzgDomain::EVALS);
  Fr* tmp = d->at<Fr>(KzgDomain::TMP);
  uint8_t* out48 = d->at<uint8_t>(KzgDomain::OUT48);
  const Fr n_inv = Fr::from_u64(N).inv();
  plonk_kzg_domain_info info = {};
  info.log_n = L;
  info.count = count;
  info.workspace_cap_bytes = d->ws_cap;
  info.chunk_polys = chunk;
  std::vector<uint8_t> comm;
  for (uint64_t first = 0; first < count; first += chunk) {
    const uint32_t cnt = (uint32_t)(count - first < chunk ? count - first : chunk);
    PTRY(kzd_stage(&c, f, n, polys + first, trimmed + first, cnt));
    // evaluations: the ordinary forward transform; G = NTT_N of the reversed coefficients
    hipLaunchKernelGGL(kzd_reverse_kernel, dim3((uint32_t)((N + 255) / 256), cnt), dim3(256), 0, c.stream, (const Fr*)f, n, g);
    HIP_TRY(hipGetLastError());
    for (uint32_t b = 0; b < cnt; ++b) {
      PTRY(ntt_device(&c, f + (uint64_t)b * n, ev + (uint64_t)b * n, tmp, L, false, false, n));
      PTRY(ntt_device(&c, g + (uint64_t)b * N, g + (uint64_t)b * N, tmp, L + 1, false, false, N));
    }
    PTRY(kzd_pointwise(&c, d->A, g, N, ws, N, L + 1, cnt, n_inv));
    info.scalar_muls += N * cnt;
    PTRY(kzd_witnesses(&c, ws, N, L, cnt, d->tw, L + 1, &info.stage_launches, &info.scalar_muls, out48));
    HIP_TRY(hipMemcpyAsync((uint8_t*)evaluations + sizeof(Fr) * n * first, ev, sizeof(Fr) * n * cnt, hipMemcpyDefault, c.stream));
    HIP_TRY(hipMemcpyAsync((uint8_t*)witnesses48 + 48 * n * first, out48, 48 * n * cnt, hipMemcpyDefault, c.stream));
    if (commitments48) PTRY(kzd_commit(&c, f, n, trimmed + first, cnt, comm, (uint8_t*)commitments48 + 48 * first));
    HIP_TRY(hipStreamSynchronize(c.stream));   // the chunk's buffers are reused by the next one
    ++info.chunks;
  }
  info.device_bytes = d->device_bytes();
  d->last = info;
  return PLONK_OK;
}

// The trimmed lengths of a call's polynomials and the checks that go with them (canonical coefficients: PLONK_ERR_DATA,
// then more than n coefficients: PLONK_ERR_DEGREE), before anything is written.  The resident form scans on the device
// (desc_dev: count descriptors, meta_dev: 2 x count words, the caller's) and returns with the stream drained.
int kzd_lengths(const char* api_fn, Ctx* c, uint32_t log_n, const void* const* polys, const uint64_t* lens, uint64_t count, bool resident,
                KzdDesc* desc_dev, unsigned long long* meta_dev, uint64_t* trimmed) {
  // lengths without trailing zeros and the canonical-form check, before anything is queued or written
  if (resident) {
    std::vector<KzdDesc> desc(count);
    for (uint64_t i = 0; i < count; ++i) desc[i] = KzdDesc{(const Fr*)polys[i], lens[i]};
    std::vector<unsigned long long> meta(2 * count);
    uint64_t longest = 1;
    for (uint64_t i = 0; i < count; ++i) longest = lens[i] > longest ? lens[i] : longest;
    const uint32_t blocks = (uint32_t)((longest + 255) / 256 < 1024 ? (longest + 255) / 256 : 1024);
    // whatever fails, the stream is drained before the call returns: nothing stays queued
    hipError_t e = hipMemcpyAsync(desc_dev, desc.data(), sizeof(KzdDesc) * count, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(meta_dev, 0, 16 * count, c->stream);
    for (uint64_t first = 0; first < count && e == hipSuccess; first += 32768) {   // grid.y
      const uint32_t cnt = (uint32_t)(count - first < 32768 ? count - first : 32768);
      hipLaunchKernelGGL(kzd_scan_kernel, dim3(blocks, cnt), dim3(256), 0, c->stream, (const KzdDesc*)desc_dev + first,
                         meta_dev + 2 * first);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(meta.data(), meta_dev, 16 * count, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) API_FAIL(PLONK_ERR_HIP, hipGetErrorString(e));
    for (uint64_t i = 0; i < count; ++i) {
      if (meta[2 * i + 1]) API_FAIL(PLONK_ERR_DATA, "non-canonical coefficient");
      trimmed[i] = meta[2 * i];
    }
  } else {
    for (uint64_t i = 0; i < count; ++i) {
      const uint64_t* p = (const uint64_t*)polys[i];
      trimmed[i] = host_trimmed(p, lens[i]);
      Fr t;
      for (uint64_t k = 0; k < trimmed[i]; ++k)
        if (!kzg_fr_load(p + 4 * k, &t)) API_FAIL(PLONK_ERR_DATA, "non-canonical coefficient");
    }
  }
  for (uint64_t i = 0; i < count; ++i)
    if (kzd_check_len(log_n, trimmed[i])) return PLONK_ERR_DEGREE;
  return PLONK_OK;
}

static int domain_open_impl(const char* api_fn, plonk_kzg_domain* dom, const void* const* polys, const uint64_t* lens, uint64_t count,
                            void* evaluations, void* witnesses48, void* commitments48, bool resident) {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count > KZD_MAX_COUNT) API_FAIL(PLONK_ERR_ARG, "invalid argument: at most 65536 polynomials per call");
  if (count && (!polys || !lens || !evaluations || !witnesses48)) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  for (uint64_t i = 0; i < count; ++i)
    if (lens[i] && !polys[i]) API_FAIL(PLONK_ERR_ARG, "invalid argument: polys[i] is NULL with lens[i] > 0");
  KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_WORK);
  if (!count) return PLONK_OK;
  // lengths without trailing zeros and the canonical-form check, before anything is queued or written
  std::vector<uint64_t> trimmed(count);
  PTRY(kzd_lengths_on(api_fn, d->c, d, d->log_n, polys, lens, count, resident, trimmed.data()));
  return kzd_drained(d->c, domain_open_body(d, polys, trimmed.data(), count, evaluations, witnesses48, commitments48));
}

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_kzg_domain_create(plonk_ctx* ctx, uint32_t log_n, plonk_kzg_domain** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  *out = nullptr;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  switch (kzd_check_create(log_n, c.nccl_comm != nullptr, c.srs_table != nullptr && c.srs_n != 0, c.srs_n)) {
    case PLONK_ERR_ARG: API_FAIL(PLONK_ERR_ARG, "invalid argument: log_n must be in [1, 20]");
    case PLONK_ERR_STATE: API_FAIL(PLONK_ERR_STATE, KZD_NEEDS_WHOLE_KEY);
    case PLONK_ERR_NO_SRS: return PLONK_ERR_NO_SRS;
    case PLONK_ERR_DEGREE: return PLONK_ERR_DEGREE;
    default: break;
  }
  std::unique_ptr<KzgDomain> d(new KzgDomain());
  const int rc = domain_create_body(c, log_n, d.get());
  if (rc != PLONK_OK) {
    (void)hipStreamSynchronize(c.stream);
    return rc;
  }
  *out = new plonk_kzg_domain{d.release(), ctx};
  return PLONK_OK;
  });
}

void plonk_kzg_domain_destroy(plonk_kzg_domain* dom) {
  if (!dom) return;
  (void)plonk::api_guard(__func__, [&]() -> int {
    std::lock_guard<std::mutex> lk(dom->ctx->c.mu);
    delete dom->d;
    return PLONK_OK;
  });
  delete dom;
}

int plonk_kzg_domain_points(plonk_kzg_domain* dom, uint64_t* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_KEY);
  const Fr w = fr_domain_root(d->log_n);
  Fr x = Fr::one();
  for (uint64_t i = 0; i < (1ull << d->log_n); ++i) {
    memcpy(out + 4 * i, x.l, 32);
    x = x * w;
  }
  return PLONK_OK;
  });
}

int plonk_kzg_open_domain(plonk_kzg_domain* dom, const uint64_t* const* polys, const uint64_t* lens, uint64_t count,
                          uint64_t* evaluations, uint8_t* witnesses48, uint8_t* commitments48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::domain_open_impl(api_fn, dom, (const void* const*)polys, lens, count, evaluations, witnesses48, commitments48, false);
  });
}

int plonk_kzg_open_domain_dev(plonk_kzg_domain* dom, const void* const* polys_dev, const uint64_t* lens, uint64_t count,
                              void* evaluations_dev, void* witnesses48_dev, void* commitments48_dev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::domain_open_impl(api_fn, dom, polys_dev, lens, count, evaluations_dev, witnesses48_dev, commitments48_dev, true);
  });
}

int plonk_kzg_domain_last(plonk_kzg_domain* dom, plonk_kzg_domain_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_KEY);
  *out = d->last;
  out->device_bytes = d->device_bytes();
  out->workspace_cap_bytes = d->ws_cap;
  return PLONK_OK;
  });
}

// Test hook (not in include/plonk_hip.h, not part of the API): the cap on the point workspace of the handle's next calls, so
// that a small call runs in several chunks (0 restores the default).  The binding's KzgDomain._set_workspace_cap calls it for
// tests/test_gpu_kzg_domain.py.
int plonk_test_kzg_domain_set_cap(plonk_kzg_domain* dom, uint64_t bytes) {
  if (!dom) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(dom->ctx->c.mu);
  dom->d->ws_cap = bytes ? bytes : KZD_WS_CAP_DEFAULT;
  return PLONK_OK;
}

}  // extern "C"
