// How the kernels read and write field elements and points in HBM: by 16-byte words, one helper per type and one name per
// helper across the translation units.  Also the two padded layouts that exist only in memory (G1RSlot, and Fr29Slot of
// fr29.cuh as a kernel reads it), the reduced-radix kernel operand Tw, and the double-and-add of the group transforms
// over scalar halves that are already split.  The functions have internal linkage: every translation unit that includes
// this gets its own copy, inlined into its kernels.  The two structs are kernel-argument types and keep their plain names.
#pragma once
#include <hip/hip_runtime.h>

#include "plonk_internal.hpp"
#include "curve28.cuh"
#include "fr29.cuh"
#include "kzg_domain_core.hpp"

namespace plonk {

// Fp28 / G1R in memory: each coordinate padded to 16 words (64 B).  The slot of the MSM buckets and partial sums, of the
// group transforms and of the bucket method over caller-supplied points.
struct alignas(16) G1RSlot {
  Fp28Slot X, Y, ZZ, ZZZ;
};
static_assert(sizeof(G1RSlot) == KZD_SLOT_BYTES, "slot size");

// Reduced-radix operands as kernel arguments: x * R'' ("twiddle form", fr29.cuh) or the re-sliced R form.  Values in
// twiddle form are closed under Fr29::mul (x R'' * y R'' / R'' = xy R''), so chains of data x data products run there:
// one product converts in (twiddle_from_fr), one converts out (* R / R'').
struct Tw {
  uint32_t w[9];
};

namespace {

// ---- Fr, Fp and the points over them ----------------------------------------------------------------------------------------
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
__device__ __forceinline__ Fp ld_fp(const Fp* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1], c = q[2];
  Fp r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = c.x; r.l[9] = c.y; r.l[10] = c.z; r.l[11] = c.w;
  return r;
}
__device__ __forceinline__ void st_fp(Fp* p, const Fp& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
  q[2] = make_uint4(v.l[8], v.l[9], v.l[10], v.l[11]);
}
__device__ __forceinline__ G1Affine ld_aff(const G1Affine* p) {
  G1Affine a;
  a.x = ld_fp(&p->x);
  a.y = ld_fp(&p->y);
  return a;
}
__device__ __forceinline__ void st_aff(G1Affine* p, const G1Affine& a) {
  st_fp(&p->x, a.x);
  st_fp(&p->y, a.y);
}
__device__ __forceinline__ G1 ld_g1(const G1* p) {
  G1 r;
  r.X = ld_fp(&p->X); r.Y = ld_fp(&p->Y); r.ZZ = ld_fp(&p->ZZ); r.ZZZ = ld_fp(&p->ZZZ);
  return r;
}
__device__ __forceinline__ void st_g1(G1* p, const G1& v) {
  st_fp(&p->X, v.X); st_fp(&p->Y, v.Y); st_fp(&p->ZZ, v.ZZ); st_fp(&p->ZZZ, v.ZZZ);
}

// ---- Fp28 and the XYZZ slot ------------------------------------------------------------------------------------------------
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

// ---- Fr29: the 48-byte slot and the kernel operand --------------------------------------------------------------------------
__device__ __forceinline__ Fr29 ld_tw(const Fr29Slot* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  const uint32_t c = p->w[8];
  Fr29 r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = c;
  return r;
}
__device__ __forceinline__ void st_tw(Fr29Slot* p, const Fr29& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
  q[2] = make_uint4(v.l[8], 0u, 0u, 0u);
}
// the same for tables that travel as void* (NttTables, KzgFoldArgs): slot idx of base
__device__ __forceinline__ Fr29 ld_slot(const void* base, uint64_t idx) { return ld_tw(reinterpret_cast<const Fr29Slot*>(base) + idx); }
__device__ __forceinline__ void st_slot(void* base, uint64_t idx, const Fr29& v) { st_tw(reinterpret_cast<Fr29Slot*>(base) + idx, v); }

__device__ __forceinline__ Fr29 tw29(const Tw& t) {
  Fr29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = t.w[i];
  return r;
}
inline Tw tw_of(const Fr& x) {   // host: x (R form) -> x * R''
  const Fr29 t = Fr29::twiddle_from_fr(x);
  Tw r;
  for (int i = 0; i < 9; ++i) r.w[i] = t.l[i];
  return r;
}
inline Tw tw_plain(const Fr& x) {   // host: the re-sliced R-form value (multiplying a twiddle-form value by it converts back)
  const Fr29 t = Fr29::from_fr(x);
  Tw r;
  for (int i = 0; i < 9; ++i) r.w[i] = t.l[i];
  return r;
}

// ---- split scalars of the group transforms (kzg_domain.hip, kzg_cells.hip) ---------------------------------------------------
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
