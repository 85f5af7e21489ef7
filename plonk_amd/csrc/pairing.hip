// Per-item verdicts: one pairing check per lane (plonk_kzg_pairing_check_each, plonk_kzg_check_each, plonk_verify_each;
// DESIGN.md section 9.2).  The entry points live with their objects (kzg.hip, verify.hip); this file holds what they share:
//
//   pairing_check_kernel     one lane per check: the two G1 points of the check normalised (one safegcd inverse each), the
//                            left one negated, ONE two-pair Miller loop over the prepared lines of x_h and h, one final
//                            exponentiation (pairing28.cuh, the code tests/csrc/host_pairing28.cpp runs on the host);
//                            verdict = is_one ? PLONK_OK : PLONK_ERR_VERIFY.  All lanes read the same line at the same step.
//   verify_each_sums_kernel  one wave per item, one term per lane: the item's L terms in lanes [0, 32), its R terms in lanes
//                            [32, 64), [s] P through the endomorphism and the general XYZZ addition (as verify_msm_kernel),
//                            an LDS tree per half; [item][2] sums stay in HBM for the pairing kernel
//   each_pairs_kernel        the bare pairing call: decoded affine points -> the pairing kernel's input
//   kzg_each_pack_kernel     one lane per opening: its 1 + 3 terms and its non-pairing verdict
//   verify_each_pack_kernel  one lane per proof: its 2 + 27 terms from the replay's ProofScalars
// An item whose `pre` verdict is non-zero (a point that does not decode, a non-canonical scalar, a proof the replay
// rejected) is skipped by the sums and the pairing kernel, which copies the verdict through.
#include <hip/hip_runtime.h>

#include <memory>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "pairing28.cuh"
#include "verify_core.hpp"
#include "kzg_core.hpp"

namespace plonk {

__global__ void __launch_bounds__(64) pairing_check_kernel(const PairingTables28* __restrict__ T, const G1* __restrict__ pairs,
                                                           const int32_t* __restrict__ pre, uint32_t count,
                                                           int32_t* __restrict__ verdict, uint64_t* __restrict__ values) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int32_t p = pre ? pre[k] : 0;
  if (p) {
    verdict[k] = p;
    if (values)
      for (int i = 0; i < 72; ++i) values[72ull * k + i] = 0;
    return;
  }
  F12r v;
  pairing_check_value_28(&v, T, pairs[2ull * k], pairs[2ull * k + 1]);
  verdict[k] = f12r_is_one(&v) ? PLONK_OK : PLONK_ERR_VERIFY;
  if (values) f12r_put(&v, values + 72ull * k);
}

// item k: terms [tpi k, tpi k + nL) (L) and the nR after them (R), tpi = nL + nR, nL, nR <= 32.  sc: canonical scalars (8
// words each); ids: point index into pts / kind.  sums[2 k] = L_k, sums[2 k + 1] = R_k (XYZZ, canonical coordinates).
__global__ void __launch_bounds__(EACH_LANES) verify_each_sums_kernel(const uint32_t* __restrict__ sc, const uint32_t* __restrict__ ids,
                                                                      uint32_t nL, uint32_t nR, const G1Affine* __restrict__ pts,
                                                                      const int32_t* __restrict__ kind, const int32_t* __restrict__ pre,
                                                                      G1* __restrict__ sums) {
  __shared__ G1R sh[EACH_LANES];
  const uint32_t k = blockIdx.x, lane = threadIdx.x, half = lane >> 5, t = lane & 31;
  if (pre[k]) return;   // the whole wave
  G1R acc = G1R::identity();
  if (t < (half ? nR : nL)) {
    const uint64_t j = (uint64_t)(nL + nR) * k + (half ? nL : 0) + t;
    const uint32_t p = ids[j];
    if (kind[p] == VDEC_OK) {   // the identity adds nothing (a bad point never reaches a sum)
      uint32_t s[8];
      uint32_t nz = 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) { s[w] = sc[8 * j + w]; nz |= s[w]; }
      if (nz) {
        const G1Affine a = pts[p];
        acc = g1r_mul_glv(G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)), s);
      }
    }
  }
  sh[lane] = acc;
  __syncthreads();
  for (uint32_t s = 16; s; s >>= 1) {
    if (t < s) sh[lane] = sh[lane].add(sh[lane + s]);
    __syncthreads();
  }
  if (!t) sums[2ull * k + half] = sh[lane].to_g1();
}

// decoded points [A_0 B_0 A_1 B_1 ...] -> pairs / pre: an item with a point that did not decode gets PLONK_ERR_POINT
__global__ void __launch_bounds__(256) each_pairs_kernel(const G1Affine* __restrict__ pts, const int32_t* __restrict__ kind,
                                                         uint32_t count, G1* __restrict__ pairs, int32_t* __restrict__ pre) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int32_t ka = kind[2ull * k], kb = kind[2ull * k + 1];
  pre[k] = (ka == VDEC_BAD || kb == VDEC_BAD) ? PLONK_ERR_POINT : 0;
  pairs[2ull * k] = ka == VDEC_OK ? G1::from_affine(pts[2ull * k]) : G1::identity();
  pairs[2ull * k + 1] = kb == VDEC_OK ? G1::from_affine(pts[2ull * k + 1]) : G1::identity();
}

// point table [g | C_0 W_0 | C_1 W_1 | ...]; opening k: L = {W_k: 1}, R = {C_k: 1, W_k: z_k, g: -v_k}
__global__ void __launch_bounds__(256) kzg_each_pack_kernel(const uint64_t* __restrict__ points, const plonk_kzg_proof* __restrict__ proofs,
                                                            const int32_t* __restrict__ kind, uint32_t count,
                                                            uint32_t* __restrict__ sc, uint32_t* __restrict__ ids,
                                                            int32_t* __restrict__ pre) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  Fr z, v;
  const bool canon = kzg_fr_load(points + 4ull * k, &z) & kzg_fr_load(proofs[k].evaluation, &v);
  const uint32_t c = 1 + 2 * k, w = 2 + 2 * k;
  int32_t p = 0;
  if (kind[c] == VDEC_BAD || kind[w] == VDEC_BAD) p = PLONK_ERR_POINT;
  if (!canon) p = PLONK_ERR_DATA;   // the scalars are looked at first, as plonk_kzg_batch_check does
  pre[k] = p;
  if (p) return;
  uint32_t* s = sc + 8ull * KZG_EACH_TERMS * k;
  uint32_t* id = ids + (uint64_t)KZG_EACH_TERMS * k;
  kzg_put_canonical(s, Fr::one());
  id[0] = w;
  kzg_put_canonical(s + 8, Fr::one());
  id[1] = c;
  kzg_put_canonical(s + 16, z);
  id[2] = w;
  kzg_put_canonical(s + 24, v.neg());
  id[3] = 0;
}

// proof k of slot slot[k] (point table [15 per slot | g | 11 per proof]): L = {W_z: 1, W_zw: u}, R = the 15 VK points of its
// slot, g and its 11 commitments with the replay's scalars, unweighted
__global__ void __launch_bounds__(64) verify_each_pack_kernel(const ProofScalars* __restrict__ ps, const uint32_t* __restrict__ slot,
                                                              uint32_t pt_g, uint32_t pt_proof0, uint32_t count,
                                                              uint32_t* __restrict__ sc, uint32_t* __restrict__ ids,
                                                              int32_t* __restrict__ pre) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const ProofScalars& s = ps[k];
  const int st = s.status;
  const int32_t p = st == VS_OK ? 0 : st == VS_DATA ? PLONK_ERR_DATA : st == VS_POINT ? PLONK_ERR_POINT : PLONK_ERR_VERIFY;
  pre[k] = p;
  if (p) return;
  uint32_t* o = sc + 8ull * VERIFY_EACH_TERMS * k;
  uint32_t* id = ids + (uint64_t)VERIFY_EACH_TERMS * k;
  const uint32_t base = pt_proof0 + PC_COUNT * k, vk0 = P_COUNT * slot[k];
  kzg_put_canonical(o, Fr::one());
  id[0] = base + PC_WZ;
  kzg_put_canonical(o + 8, s.u);
  id[1] = base + PC_WZW;
  for (int j = 0; j < P_COUNT; ++j) {
    kzg_put_canonical(o + 8 * (2 + j), s.vk[j]);
    id[2 + j] = vk0 + j;
  }
  kzg_put_canonical(o + 8 * (2 + P_COUNT), s.g);
  id[2 + P_COUNT] = pt_g;
  for (int c = 0; c < PC_COUNT; ++c) {
    kzg_put_canonical(o + 8 * (3 + P_COUNT + c), s.comm[c]);
    id[3 + P_COUNT + c] = base + c;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
int pairing_tables_create(Ctx* c, const G2Prepared& x_h, const G2Prepared& h, void** out_dev) {
  if (*out_dev) return PLONK_OK;
  std::unique_ptr<PairingTables28> T(new PairingTables28());
  if (!pairing_tables_fill(x_h, h, T.get())) {
    set_last_error("pairing_tables_create", "a prepared G2 point does not have the expected number of lines", __FILE__, __LINE__);
    return PLONK_ERR_STATE;
  }
  void* dev = nullptr;
  HIP_TRY(hipMalloc(&dev, sizeof(PairingTables28)));
  hipError_t e = hipMemcpyAsync(dev, T.get(), sizeof(PairingTables28), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    HIP_TRY(e);
  }
  *out_dev = dev;
  return PLONK_OK;
}

int each_pairs_launch(Ctx* c, const G1Affine* pts, const int32_t* kind, uint64_t count, G1* pairs, int32_t* pre) {
  hipLaunchKernelGGL(each_pairs_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, c->stream, pts, kind, (uint32_t)count,
                     pairs, pre);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzg_each_pack_launch(Ctx* c, const uint64_t* points, const plonk_kzg_proof* proofs, const int32_t* kind, uint64_t count,
                         uint32_t* sc, uint32_t* ids, int32_t* pre) {
  hipLaunchKernelGGL(kzg_each_pack_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, c->stream, points, proofs, kind,
                     (uint32_t)count, sc, ids, pre);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int verify_each_pack_launch(Ctx* c, const void* proof_scalars, const uint32_t* slot, uint32_t pt_g, uint32_t pt_proof0,
                            uint64_t count, uint32_t* sc, uint32_t* ids, int32_t* pre) {
  hipLaunchKernelGGL(verify_each_pack_kernel, dim3((uint32_t)((count + 63) / 64)), dim3(64), 0, c->stream,
                     (const ProofScalars*)proof_scalars, slot, pt_g, pt_proof0, (uint32_t)count, sc, ids, pre);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int each_sums_launch(Ctx* c, const uint32_t* sc, const uint32_t* ids, uint32_t nL, uint32_t nR, uint64_t count,
                     const G1Affine* pts, const int32_t* kind, const int32_t* pre, G1* sums) {
  if (nL > 32 || nR > 32 || !count) {
    set_last_error("each_sums_launch", "at most 32 terms per sum", __FILE__, __LINE__);
    return PLONK_ERR_ARG;
  }
  hipLaunchKernelGGL(verify_each_sums_kernel, dim3((uint32_t)count), dim3(EACH_LANES), 0, c->stream, sc, ids, nL, nR, pts, kind, pre,
                     sums);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int pairing_each_launch(Ctx* c, const void* tables, const G1* pairs, const int32_t* pre, uint64_t count, int32_t* verdict,
                        uint64_t* values) {
  hipLaunchKernelGGL(pairing_check_kernel, dim3((uint32_t)((count + 63) / 64)), dim3(64), 0, c->stream,
                     (const PairingTables28*)tables, pairs, pre, (uint32_t)count, verdict, values);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// verdicts to the host; the counts plonk_verify_info reports: checked = items that reached the pairing kernel (pre == 0)
int each_finish(Ctx* c, const int32_t* verdict_dev, const int32_t* pre_dev, uint64_t count, int32_t* verdicts, uint32_t* checked,
                uint32_t* rejected) {
  std::vector<int32_t> pre(count);
  HIP_TRY(hipMemcpyAsync(verdicts, verdict_dev, 4 * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(pre.data(), pre_dev, 4 * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *checked = 0;
  *rejected = 0;
  for (uint64_t k = 0; k < count; ++k) {
    if (!pre[k]) ++*checked;
    if (verdicts[k] != PLONK_OK) ++*rejected;
  }
  return PLONK_OK;
}

}  // namespace plonk
