// Proof verification: Verifier::try_from_bytes / Verifier::verify of the reference (src/compiler/verifier.rs:121-253,
// src/proof_system/proof.rs:218-513) for a batch of proofs of one circuit, folded into ONE pairing check.
//
//   plonk_verifier_from_bytes   parse + validate the Verifier::to_bytes blob, decode the 15 VK points and g on the device
//                               (decode kernel below), prepare h and x_h for the Miller loop (hostpairing.hpp)
//   plonk_verify                decode + subgroup-check the 11 K commitments (device), replay the K transcripts on host
//                               threads (verify_core.hpp), aggregate the K checks with powers of a batch challenge rho,
//                               one grouped MSM for L and R (device), one two-pair pairing check (host); a failing batch is
//                               bisected with a fresh challenge per sub-batch, so b bad proofs cost O(b log K) checks.
//
// Device work:
//   verify_decode_kernel   one lane per compressed commitment: g1_decompress48 + g1r_on_curve_in_subgroup
//   verify_msm_kernel      grid (blocks, 2 sums): lane-strided [s] P through the endomorphism (g1r_mul_glv, 128
//                          doublings + ~96 general additions) accumulated per lane, then a tree over the wave in LDS;
//                          the host adds the per-block partial sums.  Every addition is G1R::add, the general XYZZ law
//                          that doubles equal points and cancels opposite ones: adversarial commitments (duplicates,
//                          P and -P, the identity) and scalars 0 / q - 1 need no special case.
// The SRS MSM of msm.hip is not used: its speed comes from per-key tables of row multiples, which would cost more to build
// for one call's points than the sum itself.
#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "curve28.cuh"
#include "g1codec.cuh"
#include "finish_pool.hpp"
#include "hostpairing.hpp"
#include "verify_core.hpp"

#define PTRY_V(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

namespace plonk {

FinishPool* finish_pool_acquire(Ctx* c);   // prover.hip: the context's host helper threads (cfg.host_threads), or null

enum : int { VDEC_OK = 0, VDEC_IDENTITY = 1, VDEC_BAD = 2 };

__global__ void __launch_bounds__(64) verify_decode_kernel(const uint8_t* __restrict__ comp, uint32_t n, G1Affine* __restrict__ out,
                                     int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine a;
  const int rc = g1_decompress48(comp + 48ull * i, &a);
  int st = VDEC_BAD;
  if (rc == G1DEC_IDENTITY) {
    st = VDEC_IDENTITY;
    a.x = Fp::zero();
    a.y = Fp::zero();
  } else if (rc == G1DEC_OK) {
    st = g1r_on_curve_in_subgroup(Fp28::from_fp(a.x), Fp28::from_fp(a.y)) ? VDEC_OK : VDEC_BAD;
  } else {
    a.x = Fp::zero();
    a.y = Fp::zero();
  }
  out[i] = a;
  status[i] = st;
}

constexpr int VMSM_LANES = 64;   // one wave per block: the LDS tree needs no barrier beyond the wave's own
constexpr uint32_t VMSM_MAX_BLOCKS = 512;

// sum 0 (L) takes terms [0, n0), sum 1 (R) terms [n0, n0 + n1).  sc: canonical scalars (8 words each); id: point index
// into pts / kind (VDEC_*).  part: [2][gridDim.x] partial sums (XYZZ, canonical Montgomery coordinates).
__global__ void __launch_bounds__(VMSM_LANES) verify_msm_kernel(const uint32_t* __restrict__ sc, const uint32_t* __restrict__ id,
                                                                 uint32_t n0, uint32_t n1, const G1Affine* __restrict__ pts,
                                                                 const int32_t* __restrict__ kind, G1* __restrict__ part) {
  __shared__ G1R sh[VMSM_LANES];
  const uint32_t g = blockIdx.y, lane = threadIdx.x;
  const uint32_t begin = g ? n0 : 0, count = g ? n1 : n0;
  G1R acc = G1R::identity();
  for (uint32_t t = blockIdx.x * VMSM_LANES + lane; t < count; t += gridDim.x * VMSM_LANES) {
    const uint32_t j = begin + t, p = id[j];
    if (kind[p] != VDEC_OK) continue;   // the identity (a bad point never reaches a sum)
    uint32_t k[8];
    uint32_t nz = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) { k[w] = sc[8ull * j + w]; nz |= k[w]; }
    if (!nz) continue;
    const G1Affine a = pts[p];
    acc = acc.add(g1r_mul_glv(G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)), k));
  }
  sh[lane] = acc;
  __syncthreads();
  for (uint32_t s = VMSM_LANES / 2; s; s >>= 1) {
    if (lane < s) sh[lane] = sh[lane].add(sh[lane + s]);
    __syncthreads();
  }
  if (!lane) part[g * gridDim.x + blockIdx.x] = sh[0].to_g1();
}

// ---- the verifier object --------------------------------------------------------------------------------------------
struct Verifier {
  Ctx* c = nullptr;
  VerifierCore core;
  G2Prepared h, x_h;
  uint8_t g48[48];
  // device: points [0, 16) = VK (PolyId order) and g, then 11 per proof of the current call
  G1Affine* pts = nullptr;
  int32_t* kind = nullptr;
  uint8_t* comp = nullptr;
  uint32_t* sc = nullptr;
  uint32_t* ids = nullptr;
  G1* part = nullptr;
  uint64_t cap_proofs = 0, cap_terms = 0;
  plonk_verify_info last;
  ~Verifier() {
    (void)hipFree(pts); (void)hipFree(kind); (void)hipFree(comp);
    (void)hipFree(sc); (void)hipFree(ids); (void)hipFree(part);
  }
  int reserve(uint64_t proofs) {
    if (proofs > cap_proofs) {   // the decoded VK points and g ([0, 16)) move to the larger buffers
      const uint64_t npts = 16 + PC_COUNT * proofs;
      G1Affine* npts_dev = nullptr;
      int32_t* nkind = nullptr;
      uint8_t* ncomp = nullptr;
      hipError_t e = hipMalloc((void**)&npts_dev, sizeof(G1Affine) * npts);
      if (e == hipSuccess) e = hipMalloc((void**)&nkind, sizeof(int32_t) * npts);
      if (e == hipSuccess) e = hipMalloc((void**)&ncomp, 48 * npts);
      if (e == hipSuccess && pts) e = hipMemcpyAsync(npts_dev, pts, sizeof(G1Affine) * 16, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess && kind) e = hipMemcpyAsync(nkind, kind, sizeof(int32_t) * 16, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) {
        (void)hipFree(npts_dev); (void)hipFree(nkind); (void)hipFree(ncomp);
        HIP_TRY(e);
      }
      (void)hipFree(pts); (void)hipFree(kind); (void)hipFree(comp);
      pts = npts_dev; kind = nkind; comp = ncomp;
      cap_proofs = proofs;
    }
    const uint64_t terms = 13 * proofs + 16;
    if (terms > cap_terms) {
      (void)hipFree(sc); (void)hipFree(ids);
      sc = nullptr; ids = nullptr;
      cap_terms = 0;
      HIP_TRY(hipMalloc((void**)&sc, 32 * terms));
      HIP_TRY(hipMalloc((void**)&ids, 4 * terms));
      cap_terms = terms;
    }
    if (!part) HIP_TRY(hipMalloc((void**)&part, sizeof(G1) * 2 * VMSM_MAX_BLOCKS));
    return PLONK_OK;
  }
};

static int decode_points(Verifier* v, const uint8_t* comp_host, uint32_t first, uint32_t n, std::vector<int32_t>* st) {
  Ctx* c = v->c;
  HIP_TRY(hipMemcpyAsync(v->comp + 48ull * first, comp_host, 48ull * n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(verify_decode_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, v->comp + 48ull * first, n,
                     v->pts + first, v->kind + first);
  HIP_TRY(hipGetLastError());
  st->resize(n);
  HIP_TRY(hipMemcpyAsync(st->data(), v->kind + first, 4ull * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PLONK_OK;
}

static G1Aff64 xyzz_to_aff(const H1& p) {
  G1Aff64 a;
  memset(&a, 0, sizeof a);
  if (p.inf()) { a.inf = true; return a; }
  const Fp64 inv = fp64_inv(fp64_mul(p.ZZ, p.ZZZ));
  a.x = fp64_mul(p.X, fp64_mul(inv, p.ZZZ));
  a.y = fp64_mul(p.Y, fp64_mul(inv, p.ZZ));
  return a;
}

static void put_scalar(uint32_t* dst, const Fr& s_mont) {
  const Fr s = s_mont.from_mont();
  memcpy(dst, s.l, 32);
}

struct BatchState {
  Verifier* v;
  const uint8_t* proofs;
  const Fr* pi;
  uint64_t pi_count;
  std::vector<ProofScalars> ps;
  std::vector<uint32_t> sc_host, id_host;
  double ms_pack = 0, ms_msm = 0, ms_pairing = 0;
  uint64_t first_terms = 0;
  uint32_t checks = 0;
};

// the two sums of a check on the device: terms [0, nL) (L) and [nL, nL + nR) (R) of the host arrays (canonical scalars,
// 8 words each; point ids into v->pts); the host adds the per-block partial sums
static int msm_device(Verifier* v, const uint32_t* sc_host, const uint32_t* id_host, uint64_t nL, uint64_t nR, H1 sums[2]) {
  Ctx* c = v->c;
  const uint64_t nmax = nR > nL ? nR : nL;
  uint32_t blocks = (uint32_t)((nmax + 4 * VMSM_LANES - 1) / (4 * VMSM_LANES));   // ~4 terms per lane
  if (blocks > VMSM_MAX_BLOCKS) blocks = VMSM_MAX_BLOCKS;
  if (!blocks) blocks = 1;
  HIP_TRY(hipMemcpyAsync(v->sc, sc_host, 32 * (nL + nR), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(v->ids, id_host, 4 * (nL + nR), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(verify_msm_kernel, dim3(blocks, 2), dim3(VMSM_LANES), 0, c->stream, v->sc, v->ids, (uint32_t)nL,
                     (uint32_t)nR, v->pts, v->kind, v->part);
  HIP_TRY(hipGetLastError());
  std::vector<G1> part(2 * blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), v->part, sizeof(G1) * 2 * blocks, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int g = 0; g < 2; ++g) {
    memset(&sums[g], 0, sizeof(H1));
    for (uint32_t k = 0; k < blocks; ++k) {
      const G1& q = part[g * blocks + k];
      if (q.is_identity()) continue;
      H1 h;
      memcpy(h.X.l, q.X.l, 48); memcpy(h.Y.l, q.Y.l, 48); memcpy(h.ZZ.l, q.ZZ.l, 48); memcpy(h.ZZZ.l, q.ZZZ.l, 48);
      sums[g] = h1_add(sums[g], h);
    }
  }
  return PLONK_OK;
}

// e(-L, x_h) e(R, h) == 1 for the proofs `which` (all with status VS_OK), weighted by rho^i
static int batch_check(BatchState& b, const uint32_t* which, size_t m, bool* ok) {
  Verifier* v = b.v;
  Ctx* c = v->c;
  const auto t0 = std::chrono::steady_clock::now();
  const Fr rho = m == 1 ? Fr::one() : batch_challenge(b.proofs, b.pi, b.pi_count, which, m);
  Fr vk_sum[P_COUNT], g_sum = Fr::zero();
  for (int j = 0; j < P_COUNT; ++j) vk_sum[j] = Fr::zero();
  const uint64_t nL = 2 * m, nR = 16 + PC_COUNT * m;
  b.sc_host.resize(8 * (nL + nR));
  b.id_host.resize(nL + nR);
  uint32_t* scL = b.sc_host.data();
  uint32_t* scR = scL + 8 * nL;
  uint32_t* idL = b.id_host.data();
  uint32_t* idR = idL + nL;
  Fr w = Fr::one();
  for (size_t i = 0; i < m; ++i) {
    const ProofScalars& p = b.ps[which[i]];
    const uint32_t base = 16 + PC_COUNT * which[i];
    put_scalar(scL + 8 * (2 * i), w);
    idL[2 * i] = base + PC_WZ;
    put_scalar(scL + 8 * (2 * i + 1), w * p.u);
    idL[2 * i + 1] = base + PC_WZW;
    for (int cc = 0; cc < PC_COUNT; ++cc) {
      put_scalar(scR + 8 * (16 + PC_COUNT * i + cc), w * p.comm[cc]);
      idR[16 + PC_COUNT * i + cc] = base + cc;
    }
    for (int j = 0; j < P_COUNT; ++j) vk_sum[j] = vk_sum[j] + w * p.vk[j];
    g_sum = g_sum + w * p.g;
    w = w * rho;
  }
  for (int j = 0; j < P_COUNT; ++j) { put_scalar(scR + 8 * j, vk_sum[j]); idR[j] = j; }
  put_scalar(scR + 8 * 15, g_sum);
  idR[15] = 15;
  const auto tp = std::chrono::steady_clock::now();   // rho and the packing are host scalar work (ms_scalars), not MSM
  H1 sums[2];
  PTRY_V(msm_device(v, b.sc_host.data(), b.id_host.data(), nL, nR, sums));
  const auto t1 = std::chrono::steady_clock::now();
  G1Aff64 pairs[2] = {xyzz_to_aff(sums[0]), xyzz_to_aff(sums[1])};
  if (!pairs[0].inf) {   // -L
    Fp64 z;
    memset(&z, 0, sizeof z);
    pairs[0].y = fp64_sub(z, pairs[0].y);
  }
  const G2Prepared* qs[2] = {&v->x_h, &v->h};
  *ok = f12_is_one(final_exponentiation(multi_miller_loop(pairs, qs, 2)));
  const auto t2 = std::chrono::steady_clock::now();
  if (!b.checks) b.first_terms = nL + nR;
  ++b.checks;
  b.ms_pack += std::chrono::duration<double, std::milli>(tp - t0).count();
  b.ms_msm += std::chrono::duration<double, std::milli>(t1 - tp).count();
  b.ms_pairing += std::chrono::duration<double, std::milli>(t2 - t1).count();
  return PLONK_OK;
}

// every proof of `which` gets VS_OK or VS_REJECT: one check for the set, halves of a failing set checked on their own
static int bisect(BatchState& b, std::vector<uint32_t>& which, size_t lo, size_t hi) {
  if (lo >= hi) return PLONK_OK;
  bool ok = false;
  PTRY_V(batch_check(b, which.data() + lo, hi - lo, &ok));
  if (ok) return PLONK_OK;
  if (hi - lo == 1) {
    b.ps[which[lo]].status = VS_REJECT;
    return PLONK_OK;
  }
  const size_t mid = lo + (hi - lo) / 2;
  PTRY_V(bisect(b, which, lo, mid));
  return bisect(b, which, mid, hi);
}

struct ReplayArg {
  const Verifier* v;
  const uint8_t* proofs;
  const Fr* pi;
  uint64_t pi_count, count;
  int tasks;
  ProofScalars* out;
};
static void replay_task(void* arg, int index) {
  const ReplayArg* a = (const ReplayArg*)arg;
  for (uint64_t k = (uint64_t)index; k < a->count; k += (uint64_t)a->tasks) {
    if (a->out[k].status != VS_OK) continue;   // a commitment already failed to decode
    a->out[k] = verify_scalars(a->v->core, a->proofs + PROOF_BYTES * k, a->pi + a->pi_count * k);
  }
}

}  // namespace plonk

using namespace plonk;

struct plonk_verifier {
  plonk::Verifier* v;
  plonk_ctx* ctx;
};


extern "C" {

int plonk_verifier_from_bytes(plonk_ctx* ctx, const uint8_t* blob, uint64_t len, plonk_verifier** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out || (len && !blob)) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  *out = nullptr;
  uint8_t h96[96], xh96[96];
  std::unique_ptr<plonk::Verifier> v(new plonk::Verifier());
  PTRY_V(plonk::parse_verifier_blob(blob, len, &v->core, v->g48, h96, xh96));
  v->h = plonk::g2_prepare(plonk::g2_decode_valid(h96));
  v->x_h = plonk::g2_prepare(plonk::g2_decode_valid(xh96));
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  v->c = &ctx->c;
  PTRY_V(v->reserve(1));
  uint8_t comp16[16 * 48];
  for (int j = 0; j < 15; ++j) memcpy(comp16 + 48 * j, v->core.vk[j], 48);
  memcpy(comp16 + 15 * 48, v->g48, 48);
  std::vector<int32_t> st;
  PTRY_V(plonk::decode_points(v.get(), comp16, 0, 16, &st));
  for (int j = 0; j < 16; ++j)   // the host validated them: the device must agree
    if (st[j] == plonk::VDEC_BAD || (j == 15 && st[j] != plonk::VDEC_OK))
      return (plonk::set_last_error(api_fn, "device decoding of a verifier-key point disagrees with the host", __FILE__, __LINE__), PLONK_ERR_STATE);
  memset(&v->last, 0, sizeof v->last);
  *out = new plonk_verifier{v.release(), ctx};
  return PLONK_OK;
  });
}

void plonk_verifier_destroy(plonk_verifier* v) {
  if (!v) return;
  (void)plonk::api_guard(__func__, [&]() -> int {
    std::lock_guard<std::mutex> lk(v->ctx->c.mu);
    (void)hipSetDevice(v->ctx->c.device);
    delete v->v;
    return PLONK_OK;
  });
  delete v;
}

int plonk_verifier_set_version(plonk_verifier* v, int version) {
  if (!v) return (plonk::set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  if (version != 2 && version != 3) return (plonk::set_last_error("invalid argument", "PlonkVersion: 2 (legacy) or 3; V1 is not supported", __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(v->ctx->c.mu);   // not under a running plonk_verify
  v->v->core.version = version;
  return PLONK_OK;
}

int plonk_verify(plonk_verifier* vh, const uint8_t* proofs, const uint64_t* pi, uint64_t pi_count, uint64_t count,
                 int32_t* verdicts) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!vh || !proofs || count == 0 || (pi_count && !pi) || (count > 1 && !verdicts))
    return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  plonk::Verifier* v = vh->v;
  if (pi_count != v->core.pi_idx.size())
    return (plonk::set_last_error("invalid argument", "public input count differs from the verifier's (Error::InconsistentPublicInputsLen)", __FILE__, __LINE__), PLONK_ERR_ARG);
  if (count > (1ull << 24)) return (plonk::set_last_error("invalid argument", "at most 2^24 proofs per call", __FILE__, __LINE__), PLONK_ERR_ARG);
  CTX_ENTER(vh->ctx->c, api_fn);
  Ctx* c = v->c;
  HIP_TRY(hipSetDevice(c->device));
  PTRY_V(v->reserve(count));
  const auto t0 = std::chrono::steady_clock::now();
  // the 11 commitments of every proof, decoded and subgroup-checked on the device
  std::vector<uint8_t> comp(48ull * plonk::PC_COUNT * count);
  for (uint64_t k = 0; k < count; ++k) memcpy(comp.data() + 48ull * plonk::PC_COUNT * k, proofs + plonk::PROOF_BYTES * k, 48 * plonk::PC_COUNT);
  // the context's host threads are woken now, while this thread waits for the decode; they take the transcript replays
  plonk::FinishPool* pool = count > 1 ? plonk::finish_pool_acquire(c) : nullptr;
  plonk::Armed helpers(pool);
  std::vector<int32_t> st;
  PTRY_V(plonk::decode_points(v, comp.data(), 16, (uint32_t)(plonk::PC_COUNT * count), &st));
  plonk::BatchState b;
  b.v = v;
  b.proofs = proofs;
  b.pi = (const Fr*)pi;
  b.pi_count = pi_count;
  b.ps.resize(count);
  for (uint64_t k = 0; k < count; ++k)
    for (int cc = 0; cc < plonk::PC_COUNT; ++cc)
      if (st[plonk::PC_COUNT * k + cc] == plonk::VDEC_BAD) b.ps[k].status = plonk::VS_POINT;
  const auto t1 = std::chrono::steady_clock::now();
  // transcript replays on the context's host threads and this one
  plonk::ReplayArg ra{v, proofs, (const Fr*)pi, pi_count, count, 1, b.ps.data()};
  uint64_t tasks = pool ? 4 * ((uint64_t)pool->workers() + 1) : 1;   // a few per thread: replays of rejected proofs end early
  if (tasks > count) tasks = count;
  if (tasks > 255) tasks = 255;
  ra.tasks = (int)tasks;
  helpers.run(plonk::replay_task, &ra, ra.tasks);
  const auto t2 = std::chrono::steady_clock::now();
  std::vector<uint32_t> which;
  for (uint64_t k = 0; k < count; ++k)
    if (b.ps[k].status == plonk::VS_OK) which.push_back((uint32_t)k);
  PTRY_V(plonk::bisect(b, which, 0, which.size()));
  uint32_t rejected = 0;
  int rc = PLONK_OK;
  for (uint64_t k = 0; k < count; ++k) {
    const int s = b.ps[k].status;
    const int32_t code = s == plonk::VS_OK ? PLONK_OK : s == plonk::VS_DATA ? PLONK_ERR_DATA : s == plonk::VS_POINT ? PLONK_ERR_POINT : PLONK_ERR_VERIFY;
    if (verdicts) verdicts[k] = code;
    if (code != PLONK_OK) { ++rejected; rc = PLONK_ERR_VERIFY; }
  }
  plonk_verify_info& li = v->last;
  li.proofs = count;
  li.msm_terms = b.first_terms;
  li.pairing_checks = b.checks;
  li.rejected = rejected;
  li.ms_decode = std::chrono::duration<double, std::milli>(t1 - t0).count();
  li.ms_scalars = std::chrono::duration<double, std::milli>(t2 - t1).count() + b.ms_pack;
  li.ms_msm = b.ms_msm;
  li.ms_pairing = b.ms_pairing;
  if (rc != PLONK_OK) plonk::set_last_error(api_fn, "proof verification failed (Error::ProofVerificationError)", __FILE__, __LINE__);
  return rc;
  });
}

int plonk_verifier_last(plonk_verifier* v, plonk_verify_info* out) {
  if (!v || !out) return (plonk::set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(v->ctx->c.mu);
  *out = v->v->last;
  return PLONK_OK;
}

// Test hook (not in include/plonk_hip.h, not part of the API): the device MSM of plonk_verify on caller-chosen points —
// n compressed G1 points (decoded and subgroup-checked by verify_decode_kernel; a bad one gives PLONK_ERR_POINT) and n
// canonical scalars (8 x 32-bit words each) -> sum as 97 bytes (Montgomery x || y || infinity flag).  The binding's
// Context._verify_msm calls it for tests/test_gpu_verify.py.
int plonk_test_verify_msm(plonk_ctx* ctx, const uint8_t* comp48, const uint32_t* scalars, uint64_t n, uint8_t out97[97]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out97 || !n || !comp48 || !scalars || n > (1ull << 24)) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  plonk::Verifier v;
  v.c = &ctx->c;
  PTRY_V(v.reserve((n + plonk::PC_COUNT - 1) / plonk::PC_COUNT));
  std::vector<int32_t> st;
  PTRY_V(plonk::decode_points(&v, comp48, 16, (uint32_t)n, &st));
  for (uint64_t i = 0; i < n; ++i)
    if (st[i] == plonk::VDEC_BAD) return (plonk::set_last_error(api_fn, "not a valid compressed point of G1", __FILE__, __LINE__), PLONK_ERR_POINT);
  std::vector<uint32_t> ids(n);
  for (uint64_t i = 0; i < n; ++i) ids[i] = (uint32_t)(16 + i);
  plonk::H1 sums[2];
  PTRY_V(plonk::msm_device(&v, scalars, ids.data(), n, 0, sums));
  memset(out97, 0, 97);
  const plonk::G1Aff64 a = plonk::xyzz_to_aff(sums[0]);
  if (a.inf) { out97[96] = 1; return PLONK_OK; }
  memcpy(out97, a.x.l, 48);
  memcpy(out97 + 48, a.y.l, 48);
  return PLONK_OK;
  });
}

}  // extern "C"

