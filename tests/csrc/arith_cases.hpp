// The arithmetic edge-case bodies, stated ONCE for both back ends of the test suite: tests/csrc/host_arith.cpp compiles
// them with g++ for the host, tests/csrc/dev_arith.hip with the product's hipcc flags into one small kernel per family.
// A case is a fixed-size input record and a fixed-size output record of plain uint32_t / uint8_t arrays (what
// tests/arith_vectors.py packs and checks against the big-int oracle); case_<family>(in, out) runs one case and touches
// nothing else, so lane i of a kernel can run case i straight from and to global memory.  Test code only.
#pragma once
#include "../../plonk_amd/csrc/curve.cuh"
#include "../../plonk_amd/csrc/fp28.cuh"
#include "../../plonk_amd/csrc/curve28.cuh"
#include "../../plonk_amd/csrc/fr29.cuh"
#include "../../plonk_amd/csrc/fp_safegcd.cuh"
#include "../../plonk_amd/csrc/g1codec.cuh"
#include "../../plonk_amd/csrc/msm_recode.cuh"
#include "../../plonk_amd/csrc/transcript.hpp"
#include "../../plonk_amd/csrc/composer_core.hpp"   // cg_inv: the inversion the executor kernel CALLS

namespace arith {
using namespace plonk;

// ---- record <-> value ------------------------------------------------------------------------------------------------
template <class T, int N>
HD T ld_limbs(const uint32_t* w) {
  T t;
#pragma unroll
  for (int i = 0; i < N; ++i) t.l[i] = w[i];
  return t;
}
template <class T, int N>
HD void st_limbs(uint32_t* w, const T& t) {
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = t.l[i];
}
HD Fr ld_fr(const uint32_t* w) { return ld_limbs<Fr, 8>(w); }
HD Fp ld_fp(const uint32_t* w) { return ld_limbs<Fp, 12>(w); }
HD Fp28 ld_fp28(const uint32_t* w) { return ld_limbs<Fp28, 14>(w); }
HD void st_fr(uint32_t* w, const Fr& x) { st_limbs<Fr, 8>(w, x); }
HD void st_fp(uint32_t* w, const Fp& x) { st_limbs<Fp, 12>(w, x); }
HD void st_fp28(uint32_t* w, const Fp28& x) { st_limbs<Fp28, 14>(w, x); }
// points: affine x || y, 2 x 12 Montgomery limbs (the 96-byte raw form)
HD G1Affine ld_aff(const uint32_t* w) {
  G1Affine a;
  a.x = ld_fp(w);
  a.y = ld_fp(w + 12);
  return a;
}
HD void st_aff(uint32_t* w, const G1Affine& a) {
  st_fp(w, a.x);
  st_fp(w + 12, a.y);
}
// result affine + 1, or (0, 0) + 0 for the identity
HD uint32_t out_aff(const G1& p, uint32_t* w) {
  G1Affine a;
  const bool ok = p.to_affine(&a);
  st_aff(w, a);
  return ok ? 1u : 0u;
}
HD uint32_t out_aff_r(const G1R& p, uint32_t* w) { return out_aff(p.to_g1(), w); }

// ---- Fr (field.cuh) --------------------------------------------------------------------------------------------------
enum : uint32_t { FR_MUL = 0, FR_ADD, FR_SUB, FR_INV, FR_FROM_MONT, FR_GENERATOR, FR_ROOT, FR_ONE };
struct FrIn { uint32_t op, a[8], b[8]; };
struct FrOut { uint32_t r[8]; };
HD void case_fr(const FrIn& in, FrOut& out) {
  const Fr x = ld_fr(in.a), y = ld_fr(in.b);
  Fr r = Fr::zero();
  switch (in.op) {
    case FR_MUL: r = x * y; break;
    case FR_ADD: r = x + y; break;
    case FR_SUB: r = x - y; break;
    case FR_INV: r = x.inv(); break;
    case FR_FROM_MONT: r = x.from_mont(); break;
    case FR_GENERATOR: r = fr_generator(); break;
    case FR_ROOT: r = fr_root_of_unity(); break;
    case FR_ONE: r = Fr::one(); break;
  }
  st_fr(out.r, r);
}

// ---- Fp (field.cuh) --------------------------------------------------------------------------------------------------
enum : uint32_t { FP_MUL = 0, FP_ADD, FP_SUB, FP_INV };
struct FpIn { uint32_t op, a[12], b[12]; };
struct FpOut { uint32_t r[12]; };
HD void case_fp(const FpIn& in, FpOut& out) {
  const Fp x = ld_fp(in.a), y = ld_fp(in.b);
  Fp r = Fp::zero();
  switch (in.op) {
    case FP_MUL: r = x * y; break;
    case FP_ADD: r = x + y; break;
    case FP_SUB: r = x - y; break;
    case FP_INV: r = x.inv(); break;
  }
  st_fp(out.r, r);
}

// ---- G1 in XYZZ over Fp (curve.cuh) ----------------------------------------------------------------------------------
// The mixed addition (P + Q, with P = Q: the doubling branch, and P + (-P) through the same call), and [k] P.
enum : uint32_t { G1_ADD_AFF = 0, G1_NEG_ADD, G1_MUL_U32 };
struct G1In { uint32_t op, k, a[24], b[24]; };
struct G1Out { uint32_t rc, p[24]; };
HD void case_g1(const G1In& in, G1Out& out) {
  const G1Affine x = ld_aff(in.a);
  G1 r;
  if (in.op == G1_MUL_U32) {
    r = G1::from_affine(x).mul_u32(in.k);
  } else {
    G1Affine y = ld_aff(in.b);
    if (in.op == G1_NEG_ADD) {
      y = x;
      y.y = x.y.neg();
    }
    r = G1::from_affine(x).add_affine(y);
  }
  out.rc = out_aff(r, out.p);
}

// The full addition on de-normalised operands (ZZ != 1), so that the general formulas are exercised.  A family (and a
// kernel) of its own, with the de-normalisation out of line: the fully unrolled 12-limb products of eleven point
// operations in one function are most of what this file would otherwise take to compile.
#if defined(__HIPCC__)
#define ARITH_NOINLINE __host__ __device__ __noinline__ inline
#else
#define ARITH_NOINLINE inline
#endif
ARITH_NOINLINE G1 g1_denormalised(G1Affine x) {   // = x, with ZZ != 1
  return G1::from_affine(x).dbl().add_affine(x).add(G1::from_affine(x).dbl().neg());
}
struct G1FullIn { uint32_t a[24], b[24]; };
struct G1FullOut { uint32_t rc, p[24]; };
HD void case_g1_full(const G1FullIn& in, G1FullOut& out) {
  const G1 p = g1_denormalised(ld_aff(in.a));
  const G1 q = g1_denormalised(ld_aff(in.b));
  out.rc = out_aff(p.add(q), out.p);
}

// ---- reduced-radix Fp (fp28.cuh), through the 12 x 32-bit R = 2^384 form ------------------------------------------------
enum : uint32_t { FP28_ROUNDTRIP = 0, FP28_MUL, FP28_CHAIN, FP28_ZERO_TEST };
struct Fp28In { uint32_t op, a[12], b[12]; };
struct Fp28Out { uint32_t flags, r[12]; };
HD void case_fp28(const Fp28In& in, Fp28Out& out) {
  const Fp28 A = Fp28::from_fp(ld_fp(in.a)), Bv = Fp28::from_fp(ld_fp(in.b));
  Fp r = Fp::zero();
  uint32_t flags = 0;
  switch (in.op) {
    case FP28_ROUNDTRIP: r = A.to_fp(); break;
    case FP28_MUL: r = Fp28::mul(A, Bv).to_fp(); break;
    case FP28_CHAIN: {
      // exercises lazy add/sub bounds: ((a + b) * (a - b + 4p)) - (a*a) + (b*b) ... = 0 ; returns a*b + that
      const Fp28 s = Fp28::add(A, Bv), d = Fp28::sub<4>(A, Bv);
      const Fp28 t = Fp28::mul(s, d);                         // a^2 - b^2
      const Fp28 u = Fp28::sub<4>(t, A.sqr());                // -b^2 (+4p)
      const Fp28 v = Fp28::add(u, Bv.sqr());                  // 0 mod p, value < 8p
      r = Fp28::add(Fp28::mul(A, Bv), v).to_fp();
      break;
    }
    case FP28_ZERO_TEST: {
      const Fp28 z = Fp28::sub<4>(A, A);
      const Fp28 z2 = Fp28::sub<32>(Fp28::add(Fp28::add(A, A), A.dbl().dbl()), Fp28::add(A.dbl(), A.dbl().dbl()));
      flags = (z.is_zero_mod() ? 1u : 0u) | (z2.is_zero_mod() ? 2u : 0u) | (A.is_zero_mod() ? 4u : 0u);
      break;
    }
  }
  out.flags = flags;
  st_fp(out.r, r);
}

// raw-limb access (14 x u32, possibly lazy): mul(a,b), a.sqr(), mul2(a,b,c,d); and the lazy helpers on normalised
// inputs: sub_lazy<32>(a,b), neg_lazy<16>(b), add_lazy(a,b)
enum : uint32_t { RAW_MUL = 0, RAW_SQR, RAW_MUL2, RAW_SUB_LAZY32, RAW_NEG_LAZY16, RAW_ADD_LAZY };
struct Fp28RawIn { uint32_t op, a[14], b[14], c[14], d[14]; };
struct Fp28RawOut { uint32_t r[14]; };
HD void case_fp28_raw(const Fp28RawIn& in, Fp28RawOut& out) {
  const Fp28 A = ld_fp28(in.a), Bv = ld_fp28(in.b), C = ld_fp28(in.c), D = ld_fp28(in.d);
  Fp28 r = Fp28::zero();
  switch (in.op) {
    case RAW_MUL: r = Fp28::mul(A, Bv); break;
    case RAW_SQR: r = A.sqr(); break;
    case RAW_MUL2: r = Fp28::mul2(A, Bv, C, D); break;
    case RAW_SUB_LAZY32: r = Fp28::sub_lazy<32>(A, Bv); break;
    case RAW_NEG_LAZY16: r = Fp28::neg_lazy<16>(Bv); break;
    case RAW_ADD_LAZY: r = Fp28::add_lazy(A, Bv); break;
  }
  st_fp28(out.r, r);
}

// ---- XYZZ over Fp28 (curve28.cuh) ------------------------------------------------------------------------------------
static constexpr int G1R_MAX_POINTS = 40;
enum : uint32_t { G1R_ACCUMULATE = 0, G1R_TREE, G1R_PAIR_FIRST, G1R_AFFINE_ROUNDTRIP };
struct G1rIn { uint32_t op, n, k, pts[24 * G1R_MAX_POINTS]; uint8_t neg[G1R_MAX_POINTS]; };
struct G1rOut { uint32_t rc, used_pair, p[24]; };
HD Fp28 signed_y28(const Fp28& y, bool ng) {   // the kernels' lazy sign: 4p - y
  Fp28 r;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) r.l[i] = ng ? Fp28::pad<4>(i) - y.l[i] : y.l[i];
  return r;
}
HD void case_g1r(const G1rIn& in, G1rOut& out) {
  const int n = (int)in.n < G1R_MAX_POINTS ? (int)in.n : G1R_MAX_POINTS;
  uint32_t used_pair = 0;
  switch (in.op) {
    case G1R_ACCUMULATE: {   // sum_{i<n} (neg[i] ? -P_i : P_i) with mixed additions
      G1R acc = G1R::identity();
      for (int i = 0; i < n; ++i) {
        const G1Affine a = ld_aff(in.pts + 24 * i);
        const Fp28 x = Fp28::from_fp(a.x);
        Fp28 y = Fp28::from_fp(a.y);
        if (in.neg[i]) y = Fp28::sub<4>(Fp28::zero(), y);
        acc = acc.add_affine(x, y);
      }
      out.rc = out_aff_r(acc, out.p);
      break;
    }
    case G1R_TREE: {   // (sum of first half) + (sum of second half) via the full addition; then * k
      G1R a = G1R::identity(), b = G1R::identity();
      for (int i = 0; i < n; ++i) {
        const G1Affine p = ld_aff(in.pts + 24 * i);
        const Fp28 x = Fp28::from_fp(p.x), y = Fp28::from_fp(p.y);
        if (i < n / 2) a = a.add_affine(x, y); else b = b.add_affine(x, y);
      }
      G1R s = a.add(b);
      s = s.add(s);            // doubling through add()
      out.rc = out_aff_r(s.mul_u32(in.k), out.p);
      break;
    }
    case G1R_PAIR_FIRST: {
      // The accumulation lanes' first step (msm.hip ACC_FIRST_PAIR): entries 0 and 1 through add_affine_pair when
      // their x differ (signs applied lazily as 4p - y, as the kernels do), then the rest through add_affine.
      G1R acc = G1R::identity();
      int k0 = 0;
      if (n >= 2) {
        const G1Affine a = ld_aff(in.pts), b = ld_aff(in.pts + 24);
        const Fp28 xa = Fp28::from_fp(a.x), ya = Fp28::from_fp(a.y), xb = Fp28::from_fp(b.x), yb = Fp28::from_fp(b.y);
        if (G1R::pair_distinct(xa, xb)) {
          acc = G1R::add_affine_pair(xa, signed_y28(ya, in.neg[0] != 0), xb, signed_y28(yb, in.neg[1] != 0));
          k0 = 2;
          used_pair = 1;
        }
      }
      for (int i = k0; i < n; ++i) {
        const G1Affine a = ld_aff(in.pts + 24 * i);
        acc = acc.add_affine(Fp28::from_fp(a.x), signed_y28(Fp28::from_fp(a.y), in.neg[i] != 0));
      }
      out.rc = out_aff_r(acc, out.p);
      break;
    }
    default: {   // G1R_AFFINE_ROUNDTRIP
      const G1Affine p = ld_aff(in.pts);
      const G1R q = G1R::from_affine(Fp28::from_fp(p.x), Fp28::from_fp(p.y)).dbl().dbl();
      Fp28 x, y;
      g1r_to_affine(q, &x, &y);
      G1Affine r;
      r.x = x.to_fp();
      r.y = y.to_fp();
      st_aff(out.p, r);
      out.rc = 1;
      break;
    }
  }
  out.used_pair = used_pair;
}

// [k] P through the endomorphism (g1r_mul_glv: the group FFT's scalar multiplication); k canonical, 8 x 32-bit limbs.
// pre = doublings applied to P first (an operand with the bounds the FFT's butterflies hand over, not a fresh affine
// point).  split = k1 || k2 of glv_split, 2 x 4 words.
enum : uint32_t { GLV_MUL = 0, GLV_SPLIT };
struct GlvIn { uint32_t op, pre, k[8], pt[24]; };
struct GlvOut { uint32_t rc, p[24], split[8]; };
HD void case_glv(const GlvIn& in, GlvOut& out) {
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = in.k[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) out.split[i] = 0;
  if (in.op == GLV_MUL) {
    const G1Affine p = ld_aff(in.pt);
    G1R q = G1R::from_affine(Fp28::from_fp(p.x), Fp28::from_fp(p.y));
    for (uint32_t i = 0; i < in.pre; ++i) q = q.add(q);
    out.rc = out_aff_r(g1r_mul_glv(q, k), out.p);
  } else {
    const GlvScalar g = glv_split(k);
    out.split[0] = (uint32_t)g.k1[0]; out.split[1] = (uint32_t)(g.k1[0] >> 32);
    out.split[2] = (uint32_t)g.k1[1]; out.split[3] = (uint32_t)(g.k1[1] >> 32);
    out.split[4] = (uint32_t)g.k2[0]; out.split[5] = (uint32_t)(g.k2[0] >> 32);
    out.split[6] = (uint32_t)g.k2[1]; out.split[7] = (uint32_t)(g.k2[1] >> 32);
    G1Affine z;
    z.x = Fp::zero();
    z.y = Fp::zero();
    st_aff(out.p, z);
    out.rc = 0;
  }
}

// ---- reduced-radix Fr (fr29.cuh): Montgomery (R = 2^256) in and out ------------------------------------------------------
enum : uint32_t { FR29_BUTTERFLY = 0, FR29_CHAIN, FR29_MUL2, FR29_SUB_REDUCE };
struct Fr29In { uint32_t op, stages, a[8], b[8], w[8]; };
struct Fr29Out { uint32_t o0[8], o1[8]; };
HD void case_fr29(const Fr29In& in, Fr29Out& out) {
  const Fr x = ld_fr(in.a), y = ld_fr(in.b), t = ld_fr(in.w);
  Fr r0 = Fr::zero(), r1 = Fr::zero();
  switch (in.op) {
    case FR29_BUTTERFLY: {   // DIF butterfly: out0 = a + b, out1 = (a - b) * w
      const Fr29 A = Fr29::from_fr(x), Bv = Fr29::from_fr(y), W = Fr29::twiddle_from_fr(t);
      r0 = Fr29::add_csub(A, Bv).to_fr();
      r1 = Fr29::mul(Fr29::sub_lazy(A, Bv), W).to_fr();
      break;
    }
    case FR29_CHAIN: {   // chained stages on a vector of 2 elements: the lazy ranges (sum path and product path)
      Fr29 A = Fr29::from_fr(x), Bv = Fr29::from_fr(y);
      const Fr29 W = Fr29::twiddle_from_fr(t);
      for (uint32_t s = 0; s < in.stages; ++s) {
        const Fr29 n0 = Fr29::add_csub(A, Bv);
        const Fr29 n1 = Fr29::mul(Fr29::sub_lazy(A, Bv), W);
        A = n0; Bv = n1;
      }
      r0 = A.to_fr();
      r1 = Bv.to_fr();
      break;
    }
    case FR29_MUL2: {   // a * (b * w), both factors in twiddle form
      const Fr29 W = Fr29::mul(Fr29::twiddle_from_fr(y), Fr29::twiddle_from_fr(t));
      r0 = Fr29::mul(Fr29::from_fr(x), W).to_fr();
      break;
    }
    case FR29_SUB_REDUCE: {
      // operands first pushed to the top of the lazy range: (x + 0) via add_csub keeps them, so use doubled values
      const Fr29 A = Fr29::from_fr(x), Bv = Fr29::from_fr(y);
      r0 = Fr29::sub_reduce(Fr29::add_csub(A, A), Fr29::add_csub(Bv, Bv)).to_fr();
      break;
    }
  }
  st_fr(out.o0, r0);
  st_fr(out.o1, r1);
}

// ---- fp_safegcd.cuh: Bernstein-Yang inversions; a and r are 12 words, the Fr instances use the first 8 ------------------
enum : uint32_t { GCD_FP28 = 0, GCD_FP28_LAZY, GCD_FR29_TW, GCD_FR_MONT, GCD_CG_INV };
struct SafegcdIn { uint32_t op, a[12]; };
struct SafegcdOut { uint32_t r[12]; };
HD void case_safegcd(const SafegcdIn& in, SafegcdOut& out) {
#pragma unroll
  for (int i = 0; i < 12; ++i) out.r[i] = 0;
  switch (in.op) {
    case GCD_FP28:   // Fp (R = 2^384 Montgomery) -> its inverse in the same form, through Fp28
      st_fp(out.r, fp28_inv_gcd(Fp28::from_fp(ld_fp(in.a))).to_fp());
      break;
    case GCD_FP28_LAZY: {   // same input scaled lazily (value 5x + 3x = 8x as unreduced limbs < 64p): the inverse of 8x
      const Fp28 A = Fp28::from_fp(ld_fp(in.a));
      const Fp28 A8 = Fp28::add(Fp28::add(A.dbl().dbl(), A), Fp28::add(A.dbl(), A));
      st_fp(out.r, fp28_inv_gcd(A8).to_fp());
      break;
    }
    case GCD_FR29_TW: {   // Fr (R = 2^256) -> inverse, through twiddle form
      const Fr29 inv_t = fr29_inv_gcd_tw(Fr29::twiddle_from_fr(ld_fr(in.a)));   // x^-1 * 2^261
      st_fr(out.r, Fr29::mul(inv_t, Fr29::from_fr(Fr::one())).to_fr());        // * R / 2^261 = x^-1 R
      break;
    }
    case GCD_FR_MONT:   // the Montgomery-in / Montgomery-out Fr inverse the host driver uses per proof
      st_fr(out.r, fr_inv_gcd(ld_fr(in.a)));
      break;
    case GCD_CG_INV:    // the same through the composer's out-of-line call (an Fr by value)
      st_fr(out.r, cg_inv(ld_fr(in.a)));
      break;
  }
}

// ---- g1codec.cuh: G1Affine::from_bytes on a 48-byte compressed encoding -------------------------------------------------
struct DecompressIn { uint8_t enc[48]; };
struct DecompressOut { uint32_t rc, p[24]; };
HD void case_decompress(const DecompressIn& in, DecompressOut& out) {
  uint8_t enc[48];
#pragma unroll
  for (int i = 0; i < 48; ++i) enc[i] = in.enc[i];
  G1Affine a;
  a.x = Fp::zero();
  a.y = Fp::zero();
  out.rc = (uint32_t)g1_decompress48(enc, &a);
  st_aff(out.p, a);
}

// ---- msm_recode.cuh: canonical scalar -> d[4 j .. 4 j + 3] = slot, row, bucket, sign; n = the number of digits ------------
// mode 0: signed windows; 1: width-17 NAF from registers; 2: the same from the kernels' strided LDS-parked form;
// 21: width-21 NAF; 120 / 116: even-position digits of width 20 / 16 (parked form)
struct RecodeIn { uint32_t mode, s[8]; };
struct RecodeOut { uint32_t n, d[4 * MSM_DIGITS]; };
HD void case_recode(const RecodeIn& in, RecodeOut& out) {
  Big<8> s;
#pragma unroll
  for (int k = 0; k < 8; ++k) s.l[k] = in.s[k];
  uint32_t* d = out.d;
  for (int j = 0; j < 4 * MSM_DIGITS; ++j) d[j] = 0;
  uint32_t n = 0;
  auto emit = [&](int slot, uint32_t row, uint32_t bucket, uint32_t sign) {
    if (n < (uint32_t)MSM_DIGITS) { d[4 * n] = (uint32_t)slot; d[4 * n + 1] = row; d[4 * n + 2] = bucket; d[4 * n + 3] = sign; }
    ++n;
  };
  uint32_t park[9 * 3];
  for (int j = 0; j < 9; ++j) { park[3 * j] = 0xdeadbeefu; park[3 * j + 1] = j < 8 ? s.l[j] : 0u; park[3 * j + 2] = 0x12345678u; }
  const uint32_t mode = in.mode;
  if (mode == 120) for_each_digit_even<20>(StridedLimbs{park + 1, 3}, emit);
  else if (mode == 116) for_each_digit_even<16>(StridedLimbs{park + 1, 3}, emit);
  else if (mode == 21) for_each_digit_naf<21>(s, emit);
  else if (mode == 2) for_each_digit_bitpos(StridedLimbs{park + 1, 3}, emit);
  else for_each_digit(s, mode ? MSM_ROWS_BITPOS : MSM_ROWS_WINDOW, emit);
  out.n = n;
}

// ---- transcript.hpp: Merlin's published test protocol (equivalence_simple) ------------------------------------------------
struct MerlinIn { uint32_t unused; };
struct MerlinOut { uint8_t challenge[32]; };
HD void case_merlin(const MerlinIn&, MerlinOut& out) {
  Transcript t((const uint8_t*)"test protocol", 13);
  t.append_message("some label", (const uint8_t*)"some data", 9);
  uint8_t c[32];
  t.challenge_bytes("challenge", c, 32);
  for (int i = 0; i < 32; ++i) out.challenge[i] = c[i];
}

// ---- the pairing tower over Fp28 (pairing28.cuh) ------------------------------------------------------------------------
// Raw limbs in and out: 14 words per coordinate (Montgomery, R = 2^392), 2 coordinates per Fp2, 6 per Fp6, 12 per Fp12 in
// the order of the structs.  Compiled only into the PAIRING object of the device twin (the group is named on its command
// line) and into the host twin: the header brings hostpairing.hpp with it, which the other objects need not parse.
#if !defined(ARITH_GROUP) || defined(ARITH_GROUP_PAIRING)
}  // namespace arith
#include "../../plonk_amd/csrc/pairing28.cuh"
namespace arith {
#define ARITH_HAS_PAIRING 1

// The one shared read-only buffer of the families that read the tables (Frobenius constants, prepared lines of x_h and
// h): filled once by <prefix>shared_tables of the harness; the case bodies find it here, so that every family keeps the
// two-argument body the runners expand.
static const PairingTables28* h_pairing_tables = nullptr;
#if defined(__HIPCC__)
static __device__ const PairingTables28* d_pairing_tables = nullptr;
#endif
HD const PairingTables28* pairing_tables() {
#if defined(__HIP_DEVICE_COMPILE__)
  return d_pairing_tables;
#else
  return h_pairing_tables;
#endif
}

HD F2r ld_f2r(const uint32_t* w) { return {ld_fp28(w), ld_fp28(w + 14)}; }
HD void st_f2r(uint32_t* w, const F2r& x) {
  st_fp28(w, x.a);
  st_fp28(w + 14, x.b);
}
// n Fp2 coefficients of an Fp6 (3) or Fp12 (6), which the structs hold back to back
HD void ld_f2rs(F2r* c, const uint32_t* w, int n) {
  for (int i = 0; i < n; ++i) c[i] = ld_f2r(w + 28 * i);
}
HD void st_f2rs(uint32_t* w, const F2r* c, int n) {
  for (int i = 0; i < n; ++i) st_f2r(w + 28 * i, c[i]);
}
HD void zero_words(uint32_t* w, int n) {
  for (int i = 0; i < n; ++i) w[i] = 0;
}

enum : uint32_t { P28_RED = 0, P28_ADD, P28_SUB, P28_NEG };
struct P28RedIn { uint32_t op, a[14], b[14]; };
struct P28RedOut { uint32_t r[14]; };
HD void case_p28_red(const P28RedIn& in, P28RedOut& out) {
  const Fp28 a = ld_fp28(in.a), b = ld_fp28(in.b);
  Fp28 r = Fp28::zero();
  switch (in.op) {
    case P28_RED: r = p28_red(a); break;
    case P28_ADD: r = p28_add(a, b); break;
    case P28_SUB: r = p28_sub(a, b); break;
    case P28_NEG: r = p28_neg(a); break;
  }
  st_fp28(out.r, r);
}

enum : uint32_t { F2R_ADD = 0, F2R_SUB, F2R_NEG, F2R_CONJ, F2R_MUL_XI, F2R_MUL, F2R_SQR, F2R_MUL_FP, F2R_INV };
struct F2rIn { uint32_t op, x[28], y[28], k[14]; };
struct F2rOut { uint32_t r[28]; };
HD void case_f2r(const F2rIn& in, F2rOut& out) {
  const F2r x = ld_f2r(in.x), y = ld_f2r(in.y);
  F2r r = f2r_zero();
  switch (in.op) {
    case F2R_ADD: r = f2r_add(x, y); break;
    case F2R_SUB: r = f2r_sub(x, y); break;
    case F2R_NEG: r = f2r_neg(x); break;
    case F2R_CONJ: r = f2r_conj(x); break;
    case F2R_MUL_XI: r = f2r_mul_xi(x); break;
    case F2R_MUL: r = f2r_mul(x, y); break;
    case F2R_SQR: r = f2r_sqr(x); break;
    case F2R_MUL_FP: r = f2r_mul_fp(x, ld_fp28(in.k)); break;
    case F2R_INV: r = f2r_inv(x); break;
  }
  st_f2r(out.r, r);
}

// alias: 0 = the result in an object of its own, 1 = r == x, 2 = r == y (the aliasing the header's comments allow)
enum : uint32_t { F6R_ADD = 0, F6R_SUB, F6R_NEG, F6R_MUL_V, F6R_MUL, F6R_INV, F6R_MUL_01, F6R_MUL_1 };
struct F6rIn { uint32_t op, alias, x[84], y[84], a0[28], a1[28]; };
struct F6rOut { uint32_t r[84]; };
HD void case_f6r(const F6rIn& in, F6rOut& out) {
  F6r x, y, sep;
  ld_f2rs(&x.c0, in.x, 3);
  ld_f2rs(&y.c0, in.y, 3);
  ld_f2rs(&sep.c0, in.x, 3);
  const F2r a0 = ld_f2r(in.a0), a1 = ld_f2r(in.a1);
  F6r* r = in.alias == 1 ? &x : in.alias == 2 ? &y : &sep;
  switch (in.op) {
    case F6R_ADD: f6r_add(r, &x, &y); break;
    case F6R_SUB: f6r_sub(r, &x, &y); break;
    case F6R_NEG: f6r_neg(r, &x); break;
    case F6R_MUL_V: f6r_mul_v(r, &x); break;
    case F6R_MUL: f6r_mul(r, &x, &y); break;
    case F6R_INV: f6r_inv(r, &x); break;
    case F6R_MUL_01: f6r_mul_01(r, &x, &a0, &a1); break;
    case F6R_MUL_1: f6r_mul_1(r, &x, &a1); break;
  }
  st_f2rs(out.r, &r->c0, 3);
}

// l = three Fp2 coefficients: (a0, a1, b1) of f12r_mul_014, (c0, c1, c2) of a line; flag = f12r_is_one, put = f12r_put
enum : uint32_t { F12R_MUL = 0, F12R_SQR, F12R_CONJ, F12R_INV, F12R_MUL_014, F12R_MUL_LINE, F12R_MUL_LINE_GENERIC, F12R_IS_ONE, F12R_PUT };
struct F12rIn { uint32_t op, alias, x[168], y[168], l[84], px[14], py[14]; };
struct F12rOut { uint32_t flag, r[168], put[144]; };
HD void case_f12r(const F12rIn& in, F12rOut& out) {
  F12r x, y, sep;
  ld_f2rs(&x.c0.c0, in.x, 6);
  ld_f2rs(&y.c0.c0, in.y, 6);
  ld_f2rs(&sep.c0.c0, in.x, 6);
  Line28 l;
  ld_f2rs(&l.c0, in.l, 3);
  const Fp28 px = ld_fp28(in.px), py = ld_fp28(in.py);
  F12r* r = in.alias == 1 ? &x : in.alias == 2 ? &y : &sep;
  out.flag = 0;
  zero_words(out.put, 144);
  switch (in.op) {
    case F12R_MUL: f12r_mul(r, &x, &y); break;
    case F12R_SQR: f12r_sqr(r, &x); break;
    case F12R_CONJ: f12r_conj(r, &x); break;
    case F12R_INV: f12r_inv(r, &x); break;
    case F12R_MUL_014: f12r_mul_014(r, &x, &l.c0, &l.c1, &l.c2); break;
    case F12R_MUL_LINE: r = &x; f12r_mul_line(r, &l, &px, &py); break;                    // in place by its signature
    case F12R_MUL_LINE_GENERIC: r = &x; f12r_mul_line_generic(r, &l, &px, &py); break;
    case F12R_IS_ONE: r = &x; out.flag = f12r_is_one(&x) ? 1u : 0u; break;
    case F12R_PUT: {
      uint64_t w[72];
      r = &x;
      f12r_put(&x, w);
      for (int i = 0; i < 72; ++i) {
        out.put[2 * i] = (uint32_t)w[i];
        out.put[2 * i + 1] = (uint32_t)(w[i] >> 32);
      }
      break;
    }
  }
  st_f2rs(out.r, &r->c0.c0, 6);
}

struct F12rFrobIn { uint32_t k, alias, x[168]; };
struct F12rFrobOut { uint32_t r[168]; };
HD void case_f12r_frob(const F12rFrobIn& in, F12rFrobOut& out) {
  F12r x, sep;
  ld_f2rs(&x.c0.c0, in.x, 6);
  ld_f2rs(&sep.c0.c0, in.x, 6);
  F12r* r = in.alias == 1 ? &x : &sep;
  f12r_frob(r, &x, (int)in.k, pairing_tables());
  st_f2rs(out.r, &r->c0.c0, 6);
}

// F4_SQR: x holds a, b (56 words), r gets c0, c1; the other two take an element of the cyclotomic subgroup
enum : uint32_t { CYC_F4_SQR = 0, CYC_SQR, CYC_POW_X };
struct F12rCycIn { uint32_t op, alias, x[168]; };
struct F12rCycOut { uint32_t r[168]; };
HD void case_f12r_cyc(const F12rCycIn& in, F12rCycOut& out) {
  F12r x, sep;
  ld_f2rs(&x.c0.c0, in.x, 6);
  ld_f2rs(&sep.c0.c0, in.x, 6);
  F12r* r = in.alias == 1 ? &x : &sep;
  switch (in.op) {
    case CYC_F4_SQR: {
      F2r c0, c1;
      f4r_sqr(x.c0.c0, x.c0.c1, &c0, &c1);
      r = &sep;
      f12r_set_one(r);
      r->c0.c0 = c0;
      r->c0.c1 = c1;
      break;
    }
    case CYC_SQR: f12r_cyc_sqr(r, &x); break;
    case CYC_POW_X: r = &sep; cyc_pow_x_28(r, &x); break;   // r must not be f
  }
  st_f2rs(out.r, &r->c0.c0, 6);
}

// AFF: g1 = X, Y, ZZ, ZZZ (4 x 12 words, R = 2^384) -> inf, r[0..27] = x, y; MILLER: the affine points a, b (x, y, inf)
// -> r = miller2_28; FINAL_EXP: x -> r (alias 1: in place)
enum : uint32_t { STAGE_AFF = 0, STAGE_MILLER, STAGE_FINAL_EXP };
struct PairingStagesIn { uint32_t op, alias, g1[48], a[28], a_inf, b[28], b_inf, x[168]; };
struct PairingStagesOut { uint32_t inf, r[168]; };
HD void case_pairing_stages(const PairingStagesIn& in, PairingStagesOut& out) {
  F12r x, sep;
  f12r_set_one(&sep);
  F12r* r = &sep;
  out.inf = 0;
  switch (in.op) {
    case STAGE_AFF: {
      G1 p;
      p.X = ld_fp(in.g1);
      p.Y = ld_fp(in.g1 + 12);
      p.ZZ = ld_fp(in.g1 + 24);
      p.ZZZ = ld_fp(in.g1 + 36);
      const G1Aff28 a = g1aff28_of_g1(p);
      out.inf = a.inf;
      sep.c0.c0 = F2r{a.x, a.y};
      break;
    }
    case STAGE_MILLER: {
      G1Aff28 a, b;
      a.x = ld_fp28(in.a);
      a.y = ld_fp28(in.a + 14);
      a.inf = in.a_inf;
      b.x = ld_fp28(in.b);
      b.y = ld_fp28(in.b + 14);
      b.inf = in.b_inf;
      miller2_28(r, pairing_tables(), &a, &b);
      break;
    }
    case STAGE_FINAL_EXP:
      ld_f2rs(&x.c0.c0, in.x, 6);
      if (in.alias == 1) r = &x;
      final_exponentiation_28(r, &x, pairing_tables());
      break;
  }
  st_f2rs(out.r, &r->c0.c0, 6);
}
#endif   // the pairing tower

}  // namespace arith

// Every family, once: X(name, input record, output record).  Both back ends expand this list into their runners
// (h_case_<name>, d_case_<name>) and their record sizes, so neither can run a family the other does not.  The groups are
// the units the device twin is compiled in (one object each, side by side).
#define ARITH_FAMILIES_FIELD(X)      \
  X(fr, FrIn, FrOut)                 \
  X(fp, FpIn, FpOut)                 \
  X(fp28, Fp28In, Fp28Out)           \
  X(fp28_raw, Fp28RawIn, Fp28RawOut) \
  X(fr29, Fr29In, Fr29Out)
#define ARITH_FAMILIES_G1(X) \
  X(g1, G1In, G1Out)
#define ARITH_FAMILIES_G1_FULL(X) \
  X(g1_full, G1FullIn, G1FullOut)
#define ARITH_FAMILIES_G1R(X) \
  X(g1r, G1rIn, G1rOut)
#define ARITH_FAMILIES_GLV(X) \
  X(glv, GlvIn, GlvOut)
#define ARITH_FAMILIES_INVERSE(X) \
  X(safegcd, SafegcdIn, SafegcdOut)
#define ARITH_FAMILIES_CODEC(X)              \
  X(decompress, DecompressIn, DecompressOut) \
  X(recode, RecodeIn, RecodeOut)             \
  X(merlin, MerlinIn, MerlinOut)
#define ARITH_FAMILIES_PAIRING(X)         \
  X(p28_red, P28RedIn, P28RedOut)         \
  X(f2r, F2rIn, F2rOut)                   \
  X(f6r, F6rIn, F6rOut)                   \
  X(f12r, F12rIn, F12rOut)                \
  X(f12r_frob, F12rFrobIn, F12rFrobOut)   \
  X(f12r_cyc, F12rCycIn, F12rCycOut)      \
  X(pairing_stages, PairingStagesIn, PairingStagesOut)
#define ARITH_FAMILIES(X)   \
  ARITH_FAMILIES_FIELD(X)   \
  ARITH_FAMILIES_G1(X)      \
  ARITH_FAMILIES_G1_FULL(X) \
  ARITH_FAMILIES_G1R(X)     \
  ARITH_FAMILIES_GLV(X)     \
  ARITH_FAMILIES_INVERSE(X) \
  ARITH_FAMILIES_CODEC(X)   \
  ARITH_FAMILIES_PAIRING(X)
