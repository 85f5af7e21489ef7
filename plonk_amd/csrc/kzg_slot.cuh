// The XYZZ slot of the group transforms (kzg_domain.hip, kzg_cells.hip) and the device helpers around it: loads and stores by
// 16-byte words, the negation, and the double-and-add over scalar halves that are already split.  Internal linkage: every
// translation unit that includes this gets its own copy, inlined into its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "kzg_domain_core.hpp"

namespace plonk {

namespace {

// Fp28 / G1R in memory: each coordinate padded to 16 words (64 B), as the commit-key tables of msm.hip
struct alignas(16) G1RSlot {
  Fp28Slot X, Y, ZZ, ZZZ;
};
static_assert(sizeof(G1RSlot) == KZD_SLOT_BYTES, "slot size");
__device__ __forceinline__ Fp28 ld_f28(const Fp28Slot* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
  Fp28 r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = c.x; r.l[9] = c.y; r.l[10] = c.z; r.l[11] = c.w;
  r.l[12] = d.x; r.l[13] = d.y;
  return r;
}
__device__ __forceinline__ void st_f28(Fp28Slot* p, const Fp28& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
  q[2] = make_uint4(v.l[8], v.l[9], v.l[10], v.l[11]);
  q[3] = make_uint4(v.l[12], v.l[13], 0u, 0u);
}
__device__ __forceinline__ G1R ld_g1r(const G1RSlot* p) {
  G1R r;
  r.X = ld_f28(&p->X); r.Y = ld_f28(&p->Y); r.ZZ = ld_f28(&p->ZZ); r.ZZZ = ld_f28(&p->ZZZ);
  return r;
}
__device__ __forceinline__ void st_g1r(G1RSlot* p, const G1R& v) {
  st_f28(&p->X, v.X); st_f28(&p->Y, v.Y); st_f28(&p->ZZ, v.ZZ); st_f28(&p->ZZZ, v.ZZZ);
}
__device__ __forceinline__ G1R g1r_neg(const G1R& p) {   // -P: Y -> 16p - Y (Y < 8p), canonicalised
  G1R r = p;
  if (!p.is_identity()) r.Y = Fp28::sub<16>(Fp28::zero(), p.Y).canon();
  return r;
}
__device__ __forceinline__ Fr ld_fr(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_fr(Fr* p, const Fr& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ GlvScalar ld_glv(const GlvScalar* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  GlvScalar g;
  g.k1[0] = (uint64_t)a.x | ((uint64_t)a.y << 32); g.k1[1] = (uint64_t)a.z | ((uint64_t)a.w << 32);
  g.k2[0] = (uint64_t)b.x | ((uint64_t)b.y << 32); g.k2[1] = (uint64_t)b.z | ((uint64_t)b.w << 32);
  return g;
}

// [k1 + k2 LAMBDA] p for halves that are already split: g1r_mul_glv (curve28.cuh) from its double-and-add on
__device__ __forceinline__ G1R kzd_mul_split(const G1R& p, const GlvScalar& g) {
  if (p.is_identity()) return p;
  G1R p2 = p;
  p2.X = Fp28::mul(p.X, glv_beta());                          // 16 * 1 -> < 2p
  const G1R p3 = p.add(p2);
  G1R acc = G1R::identity();
  for (int b = 127; b >= 0; --b) {
    acc = acc.dbl();
    const uint32_t s = (uint32_t)((g.k1[b >> 6] >> (b & 63)) & 1u) | ((uint32_t)((g.k2[b >> 6] >> (b & 63)) & 1u) << 1);
    if (s) acc = acc.add(s == 1 ? p : (s == 2 ? p2 : p3));
  }
  return acc;
}

}  // namespace

}  // namespace plonk
