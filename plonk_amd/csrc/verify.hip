// Proof verification: Verifier::try_from_bytes / Verifier::verify of the reference (src/compiler/verifier.rs:121-253,
// src/proof_system/proof.rs:218-513) for a batch of proofs of one circuit, folded into ONE pairing check.
//
//   plonk_verifier_from_bytes   parse + validate the Verifier::to_bytes blob, decode the 15 VK points and g on the device
//                               (decode kernel below), prepare h and x_h for the Miller loop (hostpairing.hpp)
//   plonk_verify                decode + subgroup-check the 11 K commitments (device), replay the K transcripts on host
//                               threads (verify_core.hpp), aggregate the K checks with powers of a batch challenge rho,
//                               one grouped MSM for L and R (device), one two-pair pairing check (host); a failing batch is
//                               bisected with a fresh challenge per sub-batch, so b bad proofs cost O(b log K) checks.
//   plonk_verify_mixed          the same check for proofs of several circuits that share one opening key: the transcript
//                               replays run on the device (replay kernel below, the shared verify_core.hpp code), rho is
//                               drawn from 32-byte digests, the weighting and the per-circuit VK sums stay on the device.
//
// Device work:
//   verify_decode_kernel   one lane per compressed commitment: g1_decompress48 + g1r_on_curve_in_subgroup
//   verify_msm_kernel      grid (blocks, 2 sums): lane-strided [s] P through the endomorphism (g1r_mul_glv, 128
//                          doublings + ~96 general additions) accumulated per lane, then a tree over the wave in LDS;
//                          the host adds the per-block partial sums.  Every addition is G1R::add, the general XYZZ law
//                          that doubles equal points and cancels opposite ones: adversarial commitments (duplicates,
//                          P and -P, the identity) and scalars 0 / q - 1 need no special case.
//   verify_gather_kernel   plonk_verify_mixed: the 11 commitments of every proof out of the uploaded proofs, for decode
//   verify_replay_kernel   plonk_verify_mixed: one lane per proof, replay_scalars (verify_core.hpp) from its circuit's
//                          pre-seeded transcript -> status, the 28 scalars of ProofScalars and the 32-byte proof digest
//   verify_weight_kernel   one lane per proof of a sub-batch: rho^i, the 13 weighted proof terms of the MSM, and the 16
//                          weighted VK / g scalars in a column per scalar for
//   verify_vksum_kernel    one block per (circuit of the sub-batch, VK scalar): the segmented sum over that circuit's proofs
//   verify_gsum_kernel     one block: the g scalar summed over the circuits
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

namespace plonk { struct Verifier; }
struct plonk_verifier {
  plonk::Verifier* v;
  plonk_ctx* ctx;
};

namespace plonk {

FinishPool* finish_pool_acquire(Ctx* c);   // prover.hip: the context's host helper threads (cfg.host_threads), or null

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
constexpr uint32_t VMSM_MAX_BLOCKS = VERIFY_MSM_MAX_BLOCKS;

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

// ---- plonk_verify_mixed: device replay and weighting ----------------------------------------------------------------
// One circuit of a mixed call on the device: its constants and its transcript after the label and seed_transcript_vk
// (identical for every proof of the circuit, so the host seeds it once per slot).
struct MixedSlot {
  SlotConst k;
  Transcript tr;
};

constexpr uint32_t PROOF_COMM_WORDS = PC_COUNT * 48 / 4;   // 132 words of commitments at the start of Proof::to_bytes

// comp[k][0, 528) = proofs[k][0, 528): the layout verify_decode_kernel reads (1008 and 528 are multiples of 4)
__global__ void __launch_bounds__(256) verify_gather_kernel(const uint32_t* __restrict__ proofs, uint64_t count,
                                                            uint32_t* __restrict__ comp) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * PROOF_COMM_WORDS) return;
  const uint64_t k = t / PROOF_COMM_WORDS, w = t - k * PROOF_COMM_WORDS;
  comp[t] = proofs[(PROOF_BYTES / 4) * k + w];
}

// one lane per proof: a proof with a commitment that failed to decode gets VS_POINT, every other one is replayed from its
// circuit's seeded transcript.  kind: decode statuses of the combined point table, the proofs' 11 each from pt_proof0.
__global__ void __launch_bounds__(64) verify_replay_kernel(const uint8_t* __restrict__ proofs, const uint32_t* __restrict__ slot,
                                                           const uint64_t* __restrict__ pi_off, const Fr* __restrict__ pi,
                                                           const MixedSlot* __restrict__ slots, const Fr* __restrict__ pi_root,
                                                           const int32_t* __restrict__ kind, uint32_t pt_proof0, uint32_t count,
                                                           int32_t* __restrict__ status, ProofScalars* __restrict__ ps,
                                                           uint8_t* __restrict__ digest) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < PC_COUNT; ++c) bad |= kind[pt_proof0 + (uint64_t)PC_COUNT * k + c] == VDEC_BAD;
  if (bad) {
    ps[k].status = VS_POINT;
    status[k] = VS_POINT;
    memset(digest + 32ull * k, 0, 32);
    return;
  }
  const MixedSlot& s = slots[slot[k]];
  Transcript tr = s.tr;
  replay_scalars(s.k, pi_root + s.k.pi_root_off, tr, proofs + PROOF_BYTES * k, pi + pi_off[k], ps + k, digest + 32ull * k);
  status[k] = ps[k].status;
}

__device__ __forceinline__ void put_canonical(uint32_t* dst, const Fr& s_mont) {
  const Fr s = s_mont.from_mont();
#pragma unroll
  for (int w = 0; w < 8; ++w) dst[w] = s.l[w];
}

// One lane per proof of a sub-batch, taken in slot-grouped order: p -> sub-batch position i = order[p], proof which[i],
// weight rho^i.  Writes the proof's 2 L terms (2i, 2i + 1) and 11 R terms (nL + r0 + 11 i + c) with their point ids, and its
// 15 weighted VK scalars and g scalar into wv[j][p] (column j, m per column) for the segmented sums.
__global__ void __launch_bounds__(256) verify_weight_kernel(const uint32_t* __restrict__ which, const uint32_t* __restrict__ order,
                                                            uint32_t m, Fr rho, const ProofScalars* __restrict__ ps,
                                                            uint32_t pt_proof0, uint32_t nL, uint32_t r0,
                                                            uint32_t* __restrict__ sc, uint32_t* __restrict__ ids,
                                                            Fr* __restrict__ wv) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const uint32_t i = order[p], k = which[i];
  const Fr w = rho.pow_u64(i);
  const ProofScalars& s = ps[k];
  const uint32_t base = pt_proof0 + PC_COUNT * k;
  put_canonical(sc + 16ull * i, w);
  ids[2 * i] = base + PC_WZ;
  put_canonical(sc + 16ull * i + 8, w * s.u);
  ids[2 * i + 1] = base + PC_WZW;
#pragma unroll
  for (int c = 0; c < PC_COUNT; ++c) {
    const uint64_t t = (uint64_t)nL + r0 + (uint64_t)PC_COUNT * i + c;
    put_canonical(sc + 8 * t, w * s.comm[c]);
    ids[t] = base + c;
  }
#pragma unroll
  for (int j = 0; j < P_COUNT; ++j) wv[(uint64_t)j * m + p] = w * s.vk[j];
  wv[(uint64_t)P_COUNT * m + p] = w * s.g;
}

constexpr int VSUM_LANES = 256;

template <int LANES>
__device__ __forceinline__ Fr block_sum(Fr acc, Fr* sh) {
  const uint32_t t = threadIdx.x;
  sh[t] = acc;
  __syncthreads();
  for (uint32_t h = LANES / 2; h; h >>= 1) {
    if (t < h) sh[t] = sh[t] + sh[t + h];
    __syncthreads();
  }
  return sh[0];
}

// grid (circuits of the sub-batch, 16): block (s, j) sums column j of wv over segment s = positions [seg[s], seg[s + 1])
// (the proofs of one circuit).  j < 15: the R term nL + 15 s + j with the circuit's VK point j (seg_pt[s] + j); j = 15:
// the circuit's share of the g scalar, to gpart[s].
__global__ void __launch_bounds__(VSUM_LANES) verify_vksum_kernel(const Fr* __restrict__ wv, uint32_t m,
                                                                  const uint32_t* __restrict__ seg,
                                                                  const uint32_t* __restrict__ seg_pt, uint32_t nL,
                                                                  uint32_t* __restrict__ sc, uint32_t* __restrict__ ids,
                                                                  Fr* __restrict__ gpart) {
  __shared__ Fr sh[VSUM_LANES];
  const uint32_t s = blockIdx.x, j = blockIdx.y;
  Fr acc = Fr::zero();
  for (uint32_t p = seg[s] + threadIdx.x; p < seg[s + 1]; p += VSUM_LANES) acc = acc + wv[(uint64_t)j * m + p];
  acc = block_sum<VSUM_LANES>(acc, sh);
  if (threadIdx.x) return;
  if (j < P_COUNT) {
    const uint64_t t = (uint64_t)nL + P_COUNT * s + j;
    put_canonical(sc + 8 * t, acc);
    ids[t] = seg_pt[s] + j;
  } else {
    gpart[s] = acc;
  }
}

// one block: the g scalar, summed over the ns circuits' shares, as R term nL + 15 ns with point pt_g
__global__ void __launch_bounds__(VSUM_LANES) verify_gsum_kernel(const Fr* __restrict__ gpart, uint32_t ns, uint32_t nL,
                                                                 uint32_t pt_g, uint32_t* __restrict__ sc,
                                                                 uint32_t* __restrict__ ids) {
  __shared__ Fr sh[VSUM_LANES];
  Fr acc = Fr::zero();
  for (uint32_t s = threadIdx.x; s < ns; s += VSUM_LANES) acc = acc + gpart[s];
  acc = block_sum<VSUM_LANES>(acc, sh);
  if (threadIdx.x) return;
  const uint64_t t = (uint64_t)nL + (uint64_t)P_COUNT * ns;
  put_canonical(sc + 8 * t, acc);
  ids[t] = pt_g;
}

// ---- the verifier object --------------------------------------------------------------------------------------------
struct Verifier {
  Ctx* c = nullptr;
  VerifierCore core;
  G2Prepared h, x_h;
  uint8_t g48[48];
  uint8_t opening_key[OPENING_KEY_LEN];   // g || h || x_h as in the blob: plonk_verify_mixed compares and digests them
  // device: points [0, 16) = VK (PolyId order) and g, then 11 per proof of the current call
  G1Affine* pts = nullptr;
  int32_t* kind = nullptr;
  uint8_t* comp = nullptr;
  uint32_t* sc = nullptr;
  uint32_t* ids = nullptr;
  G1* part = nullptr;
  uint64_t cap_proofs = 0, cap_terms = 0;
  plonk_verify_info last;
  void* pair_tables = nullptr;   // the lines of x_h and h for the pairing kernel (pairing.hip), made by the first plonk_verify_each
  ~Verifier() {
    (void)hipFree(pts); (void)hipFree(kind); (void)hipFree(comp);
    (void)hipFree(sc); (void)hipFree(ids); (void)hipFree(part); (void)hipFree(pair_tables);
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

// n compressed commitments from the host -> comp_dev, decoded and subgroup-checked into pts_dev / kind_dev; st: the kinds
int decode_points(Ctx* c, const uint8_t* comp_host, uint32_t n, uint8_t* comp_dev, G1Affine* pts_dev, int32_t* kind_dev,
                  std::vector<int32_t>* st) {
  st->resize(n);
  if (!n) return PLONK_OK;
  HIP_TRY(hipMemcpyAsync(comp_dev, comp_host, 48ull * n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(verify_decode_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, comp_dev, n, pts_dev, kind_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(st->data(), kind_dev, 4ull * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PLONK_OK;
}
static int decode_points(Verifier* v, const uint8_t* comp_host, uint32_t first, uint32_t n, std::vector<int32_t>* st) {
  return decode_points(v->c, comp_host, n, v->comp + 48ull * first, v->pts + first, v->kind + first, st);
}

G1Aff64 xyzz_to_aff(const H1& p) {
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

// the two sums of a check from term arrays on the device: terms [0, nL) (L) and [nL, nL + nR) (R) (canonical scalars, 8
// words each; point ids into pts / kind); the host adds the per-block partial sums
int msm_run(Ctx* c, const uint32_t* sc, const uint32_t* ids, uint64_t nL, uint64_t nR, const G1Affine* pts,
                   const int32_t* kind, G1* part_dev, H1 sums[2]) {
  const uint64_t nmax = nR > nL ? nR : nL;
  uint32_t blocks = (uint32_t)((nmax + 4 * VMSM_LANES - 1) / (4 * VMSM_LANES));   // ~4 terms per lane
  if (blocks > VMSM_MAX_BLOCKS) blocks = VMSM_MAX_BLOCKS;
  if (!blocks) blocks = 1;
  hipLaunchKernelGGL(verify_msm_kernel, dim3(blocks, 2), dim3(VMSM_LANES), 0, c->stream, sc, ids, (uint32_t)nL,
                     (uint32_t)nR, pts, kind, part_dev);
  HIP_TRY(hipGetLastError());
  std::vector<G1> part(2 * blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), part_dev, sizeof(G1) * 2 * blocks, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int g = 0; g < 2; ++g) {
    memset(&sums[g], 0, sizeof(H1));
    for (uint32_t k = 0; k < blocks; ++k) {
      const G1& q = part[g * blocks + k];
      if (q.is_identity()) continue;
      sums[g] = h1_add(sums[g], h1_of_g1(q));
    }
  }
  return PLONK_OK;
}

// the same from host term arrays (plonk_verify): uploaded to the verifier's buffers first
static int msm_device(Verifier* v, const uint32_t* sc_host, const uint32_t* id_host, uint64_t nL, uint64_t nR, H1 sums[2]) {
  Ctx* c = v->c;
  HIP_TRY(hipMemcpyAsync(v->sc, sc_host, 32 * (nL + nR), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(v->ids, id_host, 4 * (nL + nR), hipMemcpyHostToDevice, c->stream));
  return msm_run(c, v->sc, v->ids, nL, nR, v->pts, v->kind, v->part, sums);
}

// e(-L, x_h) e(R, h) == 1 for the two sums of a check
bool pairing_check(const H1 sums[2], const G2Prepared& x_h, const G2Prepared& h) {
  G1Aff64 pairs[2] = {xyzz_to_aff(sums[0]), xyzz_to_aff(sums[1])};
  if (!pairs[0].inf) {   // -L
    Fp64 z;
    memset(&z, 0, sizeof z);
    pairs[0].y = fp64_sub(z, pairs[0].y);
  }
  const G2Prepared* qs[2] = {&x_h, &h};
  return f12_is_one(final_exponentiation(multi_miller_loop(pairs, qs, 2)));
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
  PTRY(msm_device(v, b.sc_host.data(), b.id_host.data(), nL, nR, sums));
  const auto t1 = std::chrono::steady_clock::now();
  *ok = pairing_check(sums, v->x_h, v->h);
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
  PTRY(batch_check(b, which.data() + lo, hi - lo, &ok));
  if (ok) return PLONK_OK;
  if (hi - lo == 1) {
    b.ps[which[lo]].status = VS_REJECT;
    return PLONK_OK;
  }
  const size_t mid = lo + (hi - lo) / 2;
  PTRY(bisect(b, which, lo, mid));
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

// ---- plonk_verify_mixed: the host side --------------------------------------------------------------------------------
// The context's grow-only workspace of mixed calls (Ctx::verify_ws): a call whose sizes fit an earlier one allocates nothing.
struct MixedBufs {
  enum { PTS, KIND, COMP, PROOFS, SLOT, PI_OFF, PI, SLOTS, PI_ROOT, STATUS, SCALARS, DIGEST, WHICH, ORDER, SEG, SEG_PT,
         WV, GPART, SC, IDS, PART, E_PRE, E_SUMS, E_VERDICT, NBUF };   // E_*: plonk_verify_each (pairing.hip)
};
struct MixedWork : MixedBufs, DevBufs<MixedBufs::NBUF> {};

void verify_ws_release(Ctx* c) {
  delete (MixedWork*)c->verify_ws;
  c->verify_ws = nullptr;
}

// one plonk_verify_mixed call after its replay: what the checks and the bisection need
struct MixedState {
  Ctx* c;
  MixedWork* w;
  const uint32_t* circuit;            // per proof: its slot
  std::vector<uint32_t> dense;        // per proof: the slot's position among the used slots
  std::vector<uint32_t> used;         // the slots some proof references, ascending
  std::vector<uint8_t> slot_digest;   // 32 bytes per slot (verifier digests; used slots only)
  std::vector<int32_t> status;        // per proof (VerifyStatus)
  std::vector<uint8_t> digest;        // 32 bytes per proof
  const G2Prepared *h = nullptr, *x_h = nullptr;
  uint32_t pt_g = 0, pt_proof0 = 0;   // combined table: [15 per used slot | g | 11 per proof]
  double ms_decode = 0, ms_replay = 0, ms_weight = 0, ms_msm = 0, ms_pairing = 0;
  uint64_t first_terms = 0;
  uint32_t checks = 0;
  // per check (host staging of the small index arrays)
  std::vector<uint32_t> order, seg, seg_pt, sub_slots, cnt;
};

static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// Everything up to the checks: the combined point table (the verifiers' decoded VK points and g copied, the proofs'
// commitments decoded), the per-slot constants, the replay kernel; statuses and digests back to the host.
static int mixed_front(MixedState& b, plonk_verifier* const* verifiers, uint32_t nverifiers, const uint32_t* circuit,
                       const uint8_t* proofs, const uint64_t* pi, uint64_t pi_total, uint64_t count) {
  Ctx* c = b.c;
  if (!c->verify_ws) c->verify_ws = new MixedWork();
  MixedWork& w = *(MixedWork*)c->verify_ws;
  b.w = &w;
  b.circuit = circuit;
  std::vector<uint32_t> pos(nverifiers, UINT32_MAX);
  for (uint64_t k = 0; k < count; ++k) pos[circuit[k]] = 0;
  for (uint32_t s = 0; s < nverifiers; ++s)
    if (pos[s] == 0) { pos[s] = (uint32_t)b.used.size(); b.used.push_back(s); }
  const uint64_t nu = b.used.size();
  b.dense.resize(count);
  for (uint64_t k = 0; k < count; ++k) b.dense[k] = pos[circuit[k]];
  b.pt_g = (uint32_t)(P_COUNT * nu);
  b.pt_proof0 = b.pt_g + 1;
  const uint64_t npts = b.pt_proof0 + PC_COUNT * count, nterms = 13 * count + P_COUNT * nu + 1;
  // the slots' constants, seeded transcripts and public-input roots; the verifier digests
  std::vector<MixedSlot> slots;
  std::vector<Fr> roots;
  b.slot_digest.assign(32ull * nverifiers, 0);
  for (uint64_t u = 0; u < nu; ++u) {
    const Verifier* v = verifiers[b.used[u]]->v;
    slots.push_back(MixedSlot{slot_const(v->core, roots.size()), seeded_transcript(v->core)});
    roots.insert(roots.end(), v->core.pi_root.begin(), v->core.pi_root.end());
    verifier_digest(v->core, v->opening_key, b.slot_digest.data() + 32ull * b.used[u]);
  }
  std::vector<uint64_t> pi_off(count);
  uint64_t off = 0;
  for (uint64_t k = 0; k < count; ++k) {
    pi_off[k] = off;
    off += verifiers[circuit[k]]->v->core.pi_idx.size();
  }
  PTRY(w.need(MixedWork::PTS, sizeof(G1Affine) * npts));
  PTRY(w.need(MixedWork::KIND, 4 * npts));
  PTRY(w.need(MixedWork::COMP, 48ull * PC_COUNT * count));
  PTRY(w.need(MixedWork::PROOFS, PROOF_BYTES * count));
  PTRY(w.need(MixedWork::SLOT, 4 * count));
  PTRY(w.need(MixedWork::PI_OFF, 8 * count));
  PTRY(w.need(MixedWork::PI, 32 * (pi_total ? pi_total : 1)));
  PTRY(w.need(MixedWork::SLOTS, sizeof(MixedSlot) * nu));
  PTRY(w.need(MixedWork::PI_ROOT, 32 * (roots.empty() ? 1 : roots.size())));
  PTRY(w.need(MixedWork::STATUS, 4 * count));
  PTRY(w.need(MixedWork::SCALARS, sizeof(ProofScalars) * count));
  PTRY(w.need(MixedWork::DIGEST, 32 * count));
  PTRY(w.need(MixedWork::WHICH, 4 * count));
  PTRY(w.need(MixedWork::ORDER, 4 * count));
  PTRY(w.need(MixedWork::SEG, 4 * (nu + 1)));
  PTRY(w.need(MixedWork::SEG_PT, 4 * nu));
  PTRY(w.need(MixedWork::WV, 32ull * (P_COUNT + 1) * count));
  PTRY(w.need(MixedWork::GPART, 32 * nu));
  PTRY(w.need(MixedWork::SC, 32 * nterms));
  PTRY(w.need(MixedWork::IDS, 4 * nterms));
  PTRY(w.need(MixedWork::PART, sizeof(G1) * 2 * VMSM_MAX_BLOCKS));
  const hipStream_t st = c->stream;
  const auto t0 = std::chrono::steady_clock::now();
  // decode: the verifiers' VK points and g device to device, the proofs' commitments through verify_decode_kernel
  G1Affine* pts = w.at<G1Affine>(MixedWork::PTS);
  int32_t* kind = w.at<int32_t>(MixedWork::KIND);
  for (uint64_t u = 0; u < nu; ++u) {
    const Verifier* v = verifiers[b.used[u]]->v;
    HIP_TRY(hipMemcpyAsync(pts + P_COUNT * u, v->pts, sizeof(G1Affine) * P_COUNT, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(kind + P_COUNT * u, v->kind, 4 * P_COUNT, hipMemcpyDeviceToDevice, st));
  }
  const Verifier* v0 = verifiers[b.used[0]]->v;
  HIP_TRY(hipMemcpyAsync(pts + b.pt_g, v0->pts + P_COUNT, sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(kind + b.pt_g, v0->kind + P_COUNT, 4, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::PROOFS], proofs, PROOF_BYTES * count, hipMemcpyHostToDevice, st));
  const uint64_t words = PROOF_COMM_WORDS * count, ncomp = PC_COUNT * count;
  hipLaunchKernelGGL(verify_gather_kernel, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, st,
                     w.at<const uint32_t>(MixedWork::PROOFS), count, w.at<uint32_t>(MixedWork::COMP));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(verify_decode_kernel, dim3((uint32_t)((ncomp + 63) / 64)), dim3(64), 0, st, w.at<const uint8_t>(MixedWork::COMP),
                     (uint32_t)ncomp, pts + b.pt_proof0, kind + b.pt_proof0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  b.ms_decode = ms_since(t0);
  // replay
  const auto t1 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::SLOT], b.dense.data(), 4 * count, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::PI_OFF], pi_off.data(), 8 * count, hipMemcpyHostToDevice, st));
  if (pi_total) HIP_TRY(hipMemcpyAsync(w.p[MixedWork::PI], pi, 32 * pi_total, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::SLOTS], slots.data(), sizeof(MixedSlot) * nu, hipMemcpyHostToDevice, st));
  if (!roots.empty()) HIP_TRY(hipMemcpyAsync(w.p[MixedWork::PI_ROOT], roots.data(), 32 * roots.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(verify_replay_kernel, dim3((uint32_t)((count + 63) / 64)), dim3(64), 0, st, w.at<const uint8_t>(MixedWork::PROOFS),
                     w.at<const uint32_t>(MixedWork::SLOT), w.at<const uint64_t>(MixedWork::PI_OFF), w.at<const Fr>(MixedWork::PI),
                     w.at<const MixedSlot>(MixedWork::SLOTS), w.at<const Fr>(MixedWork::PI_ROOT), kind, b.pt_proof0,
                     (uint32_t)count, w.at<int32_t>(MixedWork::STATUS), w.at<ProofScalars>(MixedWork::SCALARS),
                     w.at<uint8_t>(MixedWork::DIGEST));
  HIP_TRY(hipGetLastError());
  b.status.resize(count);
  b.digest.resize(32 * count);
  HIP_TRY(hipMemcpyAsync(b.status.data(), w.p[MixedWork::STATUS], 4 * count, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(b.digest.data(), w.p[MixedWork::DIGEST], 32 * count, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  b.ms_replay = ms_since(t1);
  b.h = &v0->h;
  b.x_h = &v0->x_h;
  return PLONK_OK;
}

// one aggregated check of the proofs `which` (all VS_OK): rho from the digests, the weighting and the VK / g sums on the
// device, the MSM, the pairing
static int mixed_check(MixedState& b, const uint32_t* which, size_t m, bool* ok) {
  Ctx* c = b.c;
  MixedWork& w = *b.w;
  const hipStream_t st = c->stream;
  const auto t0 = std::chrono::steady_clock::now();
  // the sub-batch's slots (ascending) and its positions grouped by slot (a counting sort, stable)
  const size_t nu = b.used.size();
  b.cnt.assign(nu + 1, 0);
  for (size_t i = 0; i < m; ++i) ++b.cnt[b.dense[which[i]] + 1];
  b.sub_slots.clear();
  b.seg.assign(1, 0);
  b.seg_pt.clear();
  std::vector<uint32_t> first(nu + 1);   // where slot u's positions start in the grouped order
  for (size_t u = 0; u < nu; ++u) {
    first[u] = b.seg.back();
    if (!b.cnt[u + 1]) continue;
    b.sub_slots.push_back(b.used[u]);
    b.seg.push_back(b.seg.back() + b.cnt[u + 1]);
    b.seg_pt.push_back((uint32_t)(P_COUNT * u));
  }
  b.order.resize(m);
  for (size_t i = 0; i < m; ++i) b.order[first[b.dense[which[i]]]++] = (uint32_t)i;
  const uint32_t ns = (uint32_t)b.sub_slots.size();
  const Fr rho = m == 1 ? Fr::one()
                        : mixed_batch_challenge(b.sub_slots.data(), ns, b.slot_digest.data(), b.circuit, b.digest.data(), which, m);
  const uint32_t nL = (uint32_t)(2 * m), r0 = P_COUNT * ns + 1;
  const uint64_t nR = r0 + (uint64_t)PC_COUNT * m;
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::WHICH], which, 4 * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::ORDER], b.order.data(), 4 * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::SEG], b.seg.data(), 4 * (ns + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.p[MixedWork::SEG_PT], b.seg_pt.data(), 4 * ns, hipMemcpyHostToDevice, st));
  uint32_t* sc = w.at<uint32_t>(MixedWork::SC);
  uint32_t* ids = w.at<uint32_t>(MixedWork::IDS);
  hipLaunchKernelGGL(verify_weight_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, w.at<const uint32_t>(MixedWork::WHICH),
                     w.at<const uint32_t>(MixedWork::ORDER), (uint32_t)m, rho, w.at<const ProofScalars>(MixedWork::SCALARS),
                     b.pt_proof0, nL, r0, sc, ids, w.at<Fr>(MixedWork::WV));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(verify_vksum_kernel, dim3(ns, P_COUNT + 1), dim3(VSUM_LANES), 0, st, w.at<const Fr>(MixedWork::WV), (uint32_t)m,
                     w.at<const uint32_t>(MixedWork::SEG), w.at<const uint32_t>(MixedWork::SEG_PT), nL, sc, ids,
                     w.at<Fr>(MixedWork::GPART));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(verify_gsum_kernel, dim3(1), dim3(VSUM_LANES), 0, st, w.at<const Fr>(MixedWork::GPART), ns, nL, b.pt_g, sc, ids);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));   // the weighting is scalar work (ms_scalars), not MSM
  const auto tp = std::chrono::steady_clock::now();
  H1 sums[2];
  PTRY(msm_run(c, sc, ids, nL, nR, w.at<const G1Affine>(MixedWork::PTS), w.at<const int32_t>(MixedWork::KIND),
                 w.at<G1>(MixedWork::PART), sums));
  const auto t1 = std::chrono::steady_clock::now();
  *ok = pairing_check(sums, *b.x_h, *b.h);
  const auto t2 = std::chrono::steady_clock::now();
  if (!b.checks) b.first_terms = nL + nR;
  ++b.checks;
  b.ms_weight += std::chrono::duration<double, std::milli>(tp - t0).count();
  b.ms_msm += std::chrono::duration<double, std::milli>(t1 - tp).count();
  b.ms_pairing += std::chrono::duration<double, std::milli>(t2 - t1).count();
  return PLONK_OK;
}

// as bisect: a failing set is halved, each half with its own rho
static int mixed_bisect(MixedState& b, std::vector<uint32_t>& which, size_t lo, size_t hi) {
  if (lo >= hi) return PLONK_OK;
  bool ok = false;
  PTRY(mixed_check(b, which.data() + lo, hi - lo, &ok));
  if (ok) return PLONK_OK;
  if (hi - lo == 1) {
    b.status[which[lo]] = VS_REJECT;
    return PLONK_OK;
  }
  const size_t mid = lo + (hi - lo) / 2;
  PTRY(mixed_bisect(b, which, lo, mid));
  return mixed_bisect(b, which, mid, hi);
}

#define MIXED_ARG(msg) return (set_last_error(api_fn, msg, __FILE__, __LINE__), PLONK_ERR_ARG)

// the PLONK_ERR_ARG checks of plonk_verify_mixed (and of its test hook), each with its own text
static int mixed_args(const char* api_fn, plonk_verifier* const* verifiers, uint32_t nverifiers, const uint32_t* circuit,
                      const uint8_t* proofs, const uint64_t* pi, uint64_t pi_total, uint64_t count) {
  if (!verifiers || !circuit || !proofs || (pi_total && !pi)) MIXED_ARG("invalid argument: a required pointer is NULL");
  if (nverifiers == 0) MIXED_ARG("invalid argument: nverifiers == 0");
  for (uint32_t s = 0; s < nverifiers; ++s)
    if (!verifiers[s]) MIXED_ARG("invalid argument: verifiers[] holds a NULL verifier");
  if (count == 0 || count > (1ull << 24)) MIXED_ARG("invalid argument: count must be in [1, 2^24]");
  uint64_t sum = 0;
  for (uint64_t k = 0; k < count; ++k) {
    if (circuit[k] >= nverifiers) MIXED_ARG("invalid argument: circuit[k] >= nverifiers");
    sum += verifiers[circuit[k]]->v->core.pi_idx.size();
  }
  if (sum != pi_total) MIXED_ARG("invalid argument: pi_total differs from the sum of the proofs' public-input counts");
  for (uint32_t s = 1; s < nverifiers; ++s) {
    if (verifiers[s]->ctx != verifiers[0]->ctx) MIXED_ARG("invalid argument: the verifiers are on different contexts");
    if (memcmp(verifiers[s]->v->opening_key, verifiers[0]->v->opening_key, OPENING_KEY_LEN))
      MIXED_ARG("invalid argument: the verifiers' opening keys (g, h, x_h) differ");
  }
  return PLONK_OK;
}
#undef MIXED_ARG

}  // namespace plonk

using namespace plonk;


extern "C" {

int plonk_verifier_from_bytes(plonk_ctx* ctx, const uint8_t* blob, uint64_t len, plonk_verifier** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out || (len && !blob)) return (plonk::set_last_error("invalid argument", api_fn, __FILE__, __LINE__), PLONK_ERR_ARG);
  *out = nullptr;
  uint8_t h96[96], xh96[96];
  std::unique_ptr<plonk::Verifier> v(new plonk::Verifier());
  PTRY(plonk::parse_verifier_blob(blob, len, &v->core, v->g48, h96, xh96));
  memcpy(v->opening_key, v->g48, 48);
  memcpy(v->opening_key + 48, h96, 96);
  memcpy(v->opening_key + 144, xh96, 96);
  v->h = plonk::g2_prepare(plonk::g2_decode_valid(h96));
  v->x_h = plonk::g2_prepare(plonk::g2_decode_valid(xh96));
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  v->c = &ctx->c;
  PTRY(v->reserve(1));
  uint8_t comp16[16 * 48];
  for (int j = 0; j < 15; ++j) memcpy(comp16 + 48 * j, v->core.vk[j], 48);
  memcpy(comp16 + 15 * 48, v->g48, 48);
  std::vector<int32_t> st;
  PTRY(plonk::decode_points(v.get(), comp16, 0, 16, &st));
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
  PTRY(v->reserve(count));
  const auto t0 = std::chrono::steady_clock::now();
  // the 11 commitments of every proof, decoded and subgroup-checked on the device
  std::vector<uint8_t> comp(48ull * plonk::PC_COUNT * count);
  for (uint64_t k = 0; k < count; ++k) memcpy(comp.data() + 48ull * plonk::PC_COUNT * k, proofs + plonk::PROOF_BYTES * k, 48 * plonk::PC_COUNT);
  // the context's host threads are woken now, while this thread waits for the decode; they take the transcript replays
  plonk::FinishPool* pool = count > 1 ? plonk::finish_pool_acquire(c) : nullptr;
  plonk::Armed helpers(pool);
  std::vector<int32_t> st;
  PTRY(plonk::decode_points(v, comp.data(), 16, (uint32_t)(plonk::PC_COUNT * count), &st));
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
  PTRY(plonk::bisect(b, which, 0, which.size()));
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
  PTRY(v.reserve((n + plonk::PC_COUNT - 1) / plonk::PC_COUNT));
  std::vector<int32_t> st;
  PTRY(plonk::decode_points(&v, comp48, 16, (uint32_t)n, &st));
  for (uint64_t i = 0; i < n; ++i)
    if (st[i] == plonk::VDEC_BAD) return (plonk::set_last_error(api_fn, "not a valid compressed point of G1", __FILE__, __LINE__), PLONK_ERR_POINT);
  std::vector<uint32_t> ids(n);
  for (uint64_t i = 0; i < n; ++i) ids[i] = (uint32_t)(16 + i);
  plonk::H1 sums[2];
  PTRY(plonk::msm_device(&v, scalars, ids.data(), n, 0, sums));
  memset(out97, 0, 97);
  const plonk::G1Aff64 a = plonk::xyzz_to_aff(sums[0]);
  if (a.inf) { out97[96] = 1; return PLONK_OK; }
  memcpy(out97, a.x.l, 48);
  memcpy(out97 + 48, a.y.l, 48);
  return PLONK_OK;
  });
}

int plonk_verify_mixed(plonk_verifier* const* verifiers, uint32_t nverifiers, const uint32_t* circuit, const uint8_t* proofs,
                       const uint64_t* pi, uint64_t pi_total, uint64_t count, int32_t* verdicts, plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  PTRY(plonk::mixed_args(api_fn, verifiers, nverifiers, circuit, proofs, pi, pi_total, count));
  if (count > 1 && !verdicts) return (plonk::set_last_error(api_fn, "invalid argument: verdicts is NULL and count > 1", __FILE__, __LINE__), PLONK_ERR_ARG);
  CTX_ENTER(verifiers[0]->ctx->c, api_fn);
  plonk::MixedState b;
  b.c = &verifiers[0]->ctx->c;
  HIP_TRY(hipSetDevice(b.c->device));
  PTRY(plonk::mixed_front(b, verifiers, nverifiers, circuit, proofs, pi, pi_total, count));
  std::vector<uint32_t> which;
  for (uint64_t k = 0; k < count; ++k)
    if (b.status[k] == plonk::VS_OK) which.push_back((uint32_t)k);
  PTRY(plonk::mixed_bisect(b, which, 0, which.size()));
  uint32_t rejected = 0;
  int rc = PLONK_OK;
  for (uint64_t k = 0; k < count; ++k) {
    const int s = b.status[k];
    const int32_t code = s == plonk::VS_OK ? PLONK_OK : s == plonk::VS_DATA ? PLONK_ERR_DATA : s == plonk::VS_POINT ? PLONK_ERR_POINT : PLONK_ERR_VERIFY;
    if (verdicts) verdicts[k] = code;
    if (code != PLONK_OK) { ++rejected; rc = PLONK_ERR_VERIFY; }
  }
  if (info) {
    info->proofs = count;
    info->msm_terms = b.first_terms;
    info->pairing_checks = b.checks;
    info->rejected = rejected;
    info->ms_decode = b.ms_decode;
    info->ms_scalars = b.ms_replay + b.ms_weight;
    info->ms_msm = b.ms_msm;
    info->ms_pairing = b.ms_pairing;
  }
  if (rc != PLONK_OK) plonk::set_last_error(api_fn, "proof verification failed (Error::ProofVerificationError)", __FILE__, __LINE__);
  return rc;
  });
}

int plonk_verify_each(plonk_verifier* const* verifiers, uint32_t nverifiers, const uint32_t* circuit, const uint8_t* proofs,
                      const uint64_t* pi, uint64_t pi_total, uint64_t count, int32_t* verdicts, plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  std::vector<uint32_t> all_first;   // circuit == NULL: every proof belongs to verifiers[0]
  if (!circuit && count > 0 && count <= (1ull << 24)) {
    all_first.assign(count, 0);
    circuit = all_first.data();
  }
  if (!circuit && (count == 0 || count > (1ull << 24)))
    return (plonk::set_last_error(api_fn, "invalid argument: count must be in [1, 2^24]", __FILE__, __LINE__), PLONK_ERR_ARG);
  PTRY(plonk::mixed_args(api_fn, verifiers, nverifiers, circuit, proofs, pi, pi_total, count));
  if (!verdicts) return (plonk::set_last_error(api_fn, "invalid argument: verdicts is NULL", __FILE__, __LINE__), PLONK_ERR_ARG);
  if (info) memset(info, 0, sizeof *info);
  CTX_ENTER(verifiers[0]->ctx->c, api_fn);
  plonk::MixedState b;
  b.c = &verifiers[0]->ctx->c;
  Ctx* c = b.c;
  HIP_TRY(hipSetDevice(c->device));
  auto body = [&]() -> int {
    PTRY(plonk::mixed_front(b, verifiers, nverifiers, circuit, proofs, pi, pi_total, count));
    plonk::Verifier* v0 = verifiers[b.used[0]]->v;   // every verifier of the call has the same (g, h, x_h)
    PTRY(plonk::pairing_tables_create(c, v0->x_h, v0->h, &v0->pair_tables));
    plonk::MixedWork& w = *b.w;
    const uint64_t nterms = (uint64_t)plonk::VERIFY_EACH_TERMS * count;
    PTRY(w.need(plonk::MixedWork::SC, 32 * nterms));
    PTRY(w.need(plonk::MixedWork::IDS, 4 * nterms));
    PTRY(w.need(plonk::MixedWork::E_PRE, 4 * count));
    PTRY(w.need(plonk::MixedWork::E_SUMS, sizeof(G1) * 2 * count));
    PTRY(w.need(plonk::MixedWork::E_VERDICT, 4 * count));
    const auto t0 = std::chrono::steady_clock::now();
    PTRY(plonk::verify_each_pack_launch(c, w.p[plonk::MixedWork::SCALARS], w.at<const uint32_t>(plonk::MixedWork::SLOT), b.pt_g,
                                          b.pt_proof0, count, w.at<uint32_t>(plonk::MixedWork::SC), w.at<uint32_t>(plonk::MixedWork::IDS),
                                          w.at<int32_t>(plonk::MixedWork::E_PRE)));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double ms_pack = plonk::ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    PTRY(plonk::each_sums_launch(c, w.at<const uint32_t>(plonk::MixedWork::SC), w.at<const uint32_t>(plonk::MixedWork::IDS), 2,
                                   plonk::VERIFY_EACH_TERMS - 2, count, w.at<const G1Affine>(plonk::MixedWork::PTS),
                                   w.at<const int32_t>(plonk::MixedWork::KIND), w.at<const int32_t>(plonk::MixedWork::E_PRE),
                                   w.at<G1>(plonk::MixedWork::E_SUMS)));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double ms_msm = plonk::ms_since(t1);
    const auto t2 = std::chrono::steady_clock::now();
    PTRY(plonk::pairing_each_launch(c, v0->pair_tables, w.at<const G1>(plonk::MixedWork::E_SUMS),
                                      w.at<const int32_t>(plonk::MixedWork::E_PRE), count, w.at<int32_t>(plonk::MixedWork::E_VERDICT),
                                      nullptr));
    uint32_t checked = 0, rejected = 0;
    PTRY(plonk::each_finish(c, w.at<const int32_t>(plonk::MixedWork::E_VERDICT), w.at<const int32_t>(plonk::MixedWork::E_PRE), count,
                              verdicts, &checked, &rejected));
    if (info) {
      info->proofs = count;
      info->msm_terms = (uint64_t)plonk::VERIFY_EACH_TERMS * checked;
      info->pairing_checks = checked;
      info->rejected = rejected;
      info->ms_decode = b.ms_decode;
      info->ms_scalars = b.ms_replay + ms_pack;
      info->ms_msm = ms_msm;
      info->ms_pairing = plonk::ms_since(t2);
    }
    return rejected ? PLONK_ERR_VERIFY : PLONK_OK;
  };
  const int rc = body();
  if (rc != PLONK_OK && rc != PLONK_ERR_VERIFY) (void)hipStreamSynchronize(c->stream);   // nothing of the call stays queued
  if (rc == PLONK_ERR_VERIFY) plonk::set_last_error(api_fn, "proof verification failed (Error::ProofVerificationError)", __FILE__, __LINE__);
  return rc;
  });
}

// Test hook (not in include/plonk_hip.h, not part of the API): the front half of plonk_verify_mixed — decode and the device
// replay — with its arguments and checks, returning per proof the replay's status (VerifyStatus: 0 ok, 1 rejected by the
// barycentric evaluation, 2 non-canonical evaluation, 3 bad commitment), the 28 scalars of ProofScalars (vk[15] in PolyId
// order, g, comm[11], u; Montgomery, 8 words each) and the 32-byte proof digest.  The binding's Context._verify_replay
// calls it for tests/test_gpu_verify_mixed.py.
int plonk_test_verify_replay(plonk_verifier* const* verifiers, uint32_t nverifiers, const uint32_t* circuit,
                             const uint8_t* proofs, const uint64_t* pi, uint64_t pi_total, uint64_t count, int32_t* status,
                             uint32_t* scalars, uint8_t* digests) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  PTRY(plonk::mixed_args(api_fn, verifiers, nverifiers, circuit, proofs, pi, pi_total, count));
  if (!status || !scalars || !digests) return (plonk::set_last_error(api_fn, "invalid argument", __FILE__, __LINE__), PLONK_ERR_ARG);
  CTX_ENTER(verifiers[0]->ctx->c, api_fn);
  plonk::MixedState b;
  b.c = &verifiers[0]->ctx->c;
  HIP_TRY(hipSetDevice(b.c->device));
  PTRY(plonk::mixed_front(b, verifiers, nverifiers, circuit, proofs, pi, pi_total, count));
  std::vector<plonk::ProofScalars> ps(count);
  HIP_TRY(hipMemcpy(ps.data(), b.w->p[plonk::MixedWork::SCALARS], sizeof(plonk::ProofScalars) * count, hipMemcpyDeviceToHost));
  for (uint64_t k = 0; k < count; ++k) {
    status[k] = b.status[k];
    uint32_t* o = scalars + 28 * 8 * k;
    memcpy(o, ps[k].vk, 32 * plonk::P_COUNT);
    memcpy(o + 8 * 15, ps[k].g.l, 32);
    memcpy(o + 8 * 16, ps[k].comm, 32 * plonk::PC_COUNT);
    memcpy(o + 8 * 27, ps[k].u.l, 32);
  }
  memcpy(digests, b.digest.data(), 32 * count);
  return PLONK_OK;
  });
}

}  // extern "C"

