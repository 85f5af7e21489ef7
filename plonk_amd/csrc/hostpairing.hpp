// Host-side optimal-ate pairing of BLS12-381 for proof verification (no HIP): the Fp6 / Fp12 tower over hostg2.hpp's F2,
// the decoding of a compressed G2 point, the Miller loop with precomputed line coefficients (the reference's G2Prepared,
// dusk-bls12_381 pairings.rs) over any number of pairs, and one final exponentiation.
//
//   Fp6  = Fp2[v] / (v^3 - xi),  xi = 1 + u;      Fp12 = Fp6[w] / (w^2 - v)   (so w^6 = xi)
//   x = -0xd201000000010000; M-type twist E': y^2 = x^3 + 4 xi, untwisted by (x', y') -> (x' / w^2, y' / w^3).
//
// A batch verification needs two Miller loops and one final exponentiation ("Proof verification"): not worth a
// kernel.  The hard part of the final exponentiation is the x-chain of 3 (p^4 - p^2 + 1) / r (Hayashida, Hayasaka, Teruya
// 2020), so pairing() returns e(P, Q)^3: a non-degenerate bilinear map all the same (gcd(3, r) = 1), and the product of
// pairings is 1 exactly when it is 1 for the plain reduced pairing.  tests/pairing_ref.py computes the same value
// independently (affine lines over Fp[w] / (w^12 - 2 w^6 + 2), square-and-multiply final exponentiation).
#pragma once
#include <vector>

#include "hostg2.hpp"

namespace plonk {

static inline F2 f2_neg(const F2& x) {
  Fp64 z;
  memset(&z, 0, sizeof z);
  return {fp64_sub(z, x.a), fp64_sub(z, x.b)};
}
static inline F2 f2_conj(const F2& x) { return {x.a, f2_neg(x).b}; }
static inline F2 f2_mul_xi(const F2& x) { return {fp64_sub(x.a, x.b), fp64_add(x.a, x.b)}; }   // (a + b u)(1 + u)
static inline F2 f2_mul_fp(const F2& x, const Fp64& k) { return {fp64_mul(x.a, k), fp64_mul(x.b, k)}; }
static inline F2 f2_zero() { F2 z; memset(&z, 0, sizeof z); return z; }
static F2 f2_inv(const F2& x) {   // (a - b u) / (a^2 + b^2)
  const Fp64 n = fp64_inv(fp64_add(fp64_mul(x.a, x.a), fp64_mul(x.b, x.b)));
  return f2_mul_fp(f2_conj(x), n);
}

struct F6 {
  F2 c0, c1, c2;
};
static inline F6 f6_add(const F6& x, const F6& y) { return {f2_add(x.c0, y.c0), f2_add(x.c1, y.c1), f2_add(x.c2, y.c2)}; }
static inline F6 f6_sub(const F6& x, const F6& y) { return {f2_sub(x.c0, y.c0), f2_sub(x.c1, y.c1), f2_sub(x.c2, y.c2)}; }
static inline F6 f6_neg(const F6& x) { return {f2_neg(x.c0), f2_neg(x.c1), f2_neg(x.c2)}; }
static inline F6 f6_mul_v(const F6& x) { return {f2_mul_xi(x.c2), x.c0, x.c1}; }
static F6 f6_mul(const F6& x, const F6& y) {   // Karatsuba over the three coefficients
  const F2 t0 = f2_mul(x.c0, y.c0), t1 = f2_mul(x.c1, y.c1), t2 = f2_mul(x.c2, y.c2);
  const F2 c0 = f2_add(t0, f2_mul_xi(f2_sub(f2_sub(f2_mul(f2_add(x.c1, x.c2), f2_add(y.c1, y.c2)), t1), t2)));
  const F2 c1 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(x.c0, x.c1), f2_add(y.c0, y.c1)), t0), t1), f2_mul_xi(t2));
  const F2 c2 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(x.c0, x.c2), f2_add(y.c0, y.c2)), t0), t2), t1);
  return {c0, c1, c2};
}
static F6 f6_inv(const F6& x) {
  const F2 A = f2_sub(f2_sqr(x.c0), f2_mul_xi(f2_mul(x.c1, x.c2)));
  const F2 B = f2_sub(f2_mul_xi(f2_sqr(x.c2)), f2_mul(x.c0, x.c1));
  const F2 C = f2_sub(f2_sqr(x.c1), f2_mul(x.c0, x.c2));
  const F2 n = f2_add(f2_mul(x.c0, A), f2_mul_xi(f2_add(f2_mul(x.c2, B), f2_mul(x.c1, C))));
  const F2 ni = f2_inv(n);
  return {f2_mul(A, ni), f2_mul(B, ni), f2_mul(C, ni)};
}

struct F12 {
  F6 c0, c1;
};
static F12 f12_one() {
  F12 r;
  memset(&r, 0, sizeof r);
  r.c0.c0 = f2_one();
  return r;
}
static F12 f12_mul(const F12& x, const F12& y) {
  const F6 t0 = f6_mul(x.c0, y.c0), t1 = f6_mul(x.c1, y.c1);
  const F6 c1 = f6_sub(f6_sub(f6_mul(f6_add(x.c0, x.c1), f6_add(y.c0, y.c1)), t0), t1);
  return {f6_add(t0, f6_mul_v(t1)), c1};
}
static F12 f12_sqr(const F12& x) { return f12_mul(x, x); }
static F12 f12_conj(const F12& x) { return {x.c0, f6_neg(x.c1)}; }   // x^(p^6): the inverse on the cyclotomic subgroup
static F12 f12_inv(const F12& x) {                                       // (c0 - c1 w) / (c0^2 - v c1^2)
  const F6 ni = f6_inv(f6_sub(f6_mul(x.c0, x.c0), f6_mul_v(f6_mul(x.c1, x.c1))));
  return {f6_mul(x.c0, ni), f6_neg(f6_mul(x.c1, ni))};
}
static bool f12_is_one(const F12& x) {
  const F12 o = f12_one();
  const F2* a = &x.c0.c0;
  const F2* b = &o.c0.c0;
  for (int i = 0; i < 6; ++i)
    if (!f2_eq(a[i], b[i])) return false;
  return true;
}
// x^(p^k): every coefficient is a w^j (j = 2 i + h for c_h.c_i), and (a w^j)^p = conj(a) w^j xi^(j (p - 1) / 6)
struct FrobConsts {
  F2 g[3][6];   // g[k-1][j] = xi^(j (p^k - 1) / 6) for k = 1, 2, 3 (built as powers of the k = 1 constants)
};
static const FrobConsts& frob_consts() {
  static const FrobConsts fc = [] {
    FrobConsts r;
    Fp64 e = fp64_mod();   // (p - 1) / 6
    e.l[0] -= 1;
    uint64_t rem = 0;
    for (int i = 5; i >= 0; --i) {
      const unsigned __int128 cur = ((unsigned __int128)rem << 64) | e.l[i];
      e.l[i] = (uint64_t)(cur / 6);
      rem = (uint64_t)(cur % 6);
    }
    const F2 g1 = f2_pow(F2{to64(Fp::one()), to64(Fp::one())}, e);
    F2 gj = f2_one();
    for (int j = 0; j < 6; ++j) { r.g[0][j] = gj; gj = f2_mul(gj, g1); }
    // xi^(j (p^2 - 1) / 6) = g1_j^p * g1_j = conj(g1_j) g1_j; p^3 likewise from p^2
    for (int j = 0; j < 6; ++j) r.g[1][j] = f2_mul(f2_conj(r.g[0][j]), r.g[0][j]);
    for (int j = 0; j < 6; ++j) r.g[2][j] = f2_mul(r.g[0][j], r.g[1][j]);   // (p^3 - 1) = p^2 (p - 1) + (p^2 - 1): conj^2 = id
    return r;
  }();
  return fc;
}
static F12 f12_frob(const F12& x, int k) {   // k = 1, 2, 3
  const FrobConsts& fc = frob_consts();
  F12 r;
  const F6* in[2] = {&x.c0, &x.c1};
  F6* out[2] = {&r.c0, &r.c1};
  for (int h = 0; h < 2; ++h) {
    const F2* a = &in[h]->c0;
    F2* o = &out[h]->c0;
    for (int i = 0; i < 3; ++i) {
      const F2 c = (k & 1) ? f2_conj(a[i]) : a[i];
      o[i] = f2_mul(c, fc.g[k - 1][2 * i + h]);
    }
  }
  return r;
}

// ---- G2: decoding and the prepared line coefficients ------------------------------------------------------------------
struct G2Aff {
  F2 x, y;
  bool inf;
};
// G2Affine::from_bytes after g2_compressed_valid accepted the encoding: the root whose sign matches flag 0x20 (y
// lexicographically largest: compare y.c1, then y.c0, against its negation as integers)
static Fp64 fp64_canon(const Fp64& m) {
  Fp64 one;
  memset(&one, 0, sizeof one);
  one.l[0] = 1;
  return fp64_mul(m, one);
}
static bool fp64_gt(const Fp64& a, const Fp64& b) {
  for (int i = 5; i >= 0; --i)
    if (a.l[i] != b.l[i]) return a.l[i] > b.l[i];
  return false;
}
static G2Aff g2_decode_valid(const uint8_t in[96]) {
  G2Aff P;
  memset(&P, 0, sizeof P);
  if (in[0] & 0x40) { P.inf = true; return P; }
  Fp64 c1, c0;
  fp64_from_be48(in, true, &c1);
  fp64_from_be48(in + 48, false, &c0);
  Fp r2;
  for (int i = 0; i < 12; ++i) r2.l[i] = FpP::R2[i];
  P.x = {fp64_mul(c0, to64(r2)), fp64_mul(c1, to64(r2))};
  const Fp64 four = to64(Fp::from_u64(4));
  f2_sqrt(f2_add(f2_mul(f2_sqr(P.x), P.x), F2{four, four}), &P.y);
  const F2 ny = f2_neg(P.y);
  const Fp64 y1 = fp64_canon(P.y.b), n1 = fp64_canon(ny.b), y0 = fp64_canon(P.y.a), n0 = fp64_canon(ny.a);
  const bool largest = fp64_is_zero(y1) ? fp64_gt(y0, n0) : fp64_gt(y1, n1);
  if (largest != ((in[0] & 0x20) != 0)) P.y = ny;
  return P;
}

static constexpr uint64_t BLS_X = 0xd201000000010000ull;   // |x|; x is negative

// one line per step: l(P) = c0 + (c1 * P.x) w^2 + (c2 * P.y) w^3 up to a factor in Fp4 (killed by the final exponentiation)
struct LineCoeffs {
  F2 c0, c1, c2;
};
struct G2Prepared {
  std::vector<LineCoeffs> lines;
  bool inf = true;
};
// Costello, Lange, Naehrig (eprint 2010/354) algorithms 26 / 27 in homogeneous projective coordinates (X, Y, Z) over Fp2
static LineCoeffs line_dbl(F2& X, F2& Y, F2& Z) {
  const F2 t0 = f2_sqr(X), t1 = f2_sqr(Y), t2 = f2_sqr(t1);
  F2 t3 = f2_sub(f2_sub(f2_sqr(f2_add(t1, X)), t0), t2);
  t3 = f2_dbl(t3);
  const F2 t4 = f2_add(f2_dbl(t0), t0);
  F2 t6 = f2_add(X, t4);
  const F2 t5 = f2_sqr(t4), zz = f2_sqr(Z);
  X = f2_sub(f2_sub(t5, t3), t3);
  Z = f2_sub(f2_sub(f2_sqr(f2_add(Z, Y)), t1), zz);
  Y = f2_sub(f2_mul(f2_sub(t3, X), t4), f2_dbl(f2_dbl(f2_dbl(t2))));
  const F2 a = f2_neg(f2_dbl(f2_mul(t4, zz)));
  t6 = f2_sub(f2_sub(f2_sub(f2_sqr(t6), t0), t5), f2_dbl(f2_dbl(t1)));
  const F2 b = f2_dbl(f2_mul(Z, zz));
  return {t6, a, b};
}
static LineCoeffs line_add(F2& X, F2& Y, F2& Z, const G2Aff& q) {
  const F2 zz = f2_sqr(Z), yy = f2_sqr(q.y);
  const F2 t0 = f2_mul(zz, q.x);
  const F2 t1 = f2_mul(f2_sub(f2_sub(f2_sqr(f2_add(q.y, Z)), yy), zz), zz);
  const F2 t2 = f2_sub(t0, X), t3 = f2_sqr(t2);
  const F2 t4 = f2_dbl(f2_dbl(t3)), t5 = f2_mul(t4, t2);
  const F2 t6 = f2_sub(f2_sub(t1, Y), Y);
  F2 t9 = f2_mul(t6, q.x);
  const F2 t7 = f2_mul(t4, X);
  X = f2_sub(f2_sub(f2_sub(f2_sqr(t6), t5), t7), t7);
  Z = f2_sub(f2_sub(f2_sqr(f2_add(Z, t2)), zz), t3);
  F2 t10 = f2_add(q.y, Z);
  const F2 t8 = f2_mul(f2_sub(t7, X), t6);
  Y = f2_sub(t8, f2_dbl(f2_mul(Y, t5)));
  t10 = f2_sub(f2_sub(f2_sqr(t10), yy), f2_sqr(Z));
  t9 = f2_sub(f2_dbl(t9), t10);
  return {t9, f2_dbl(f2_neg(t6)), f2_dbl(Z)};
}
static G2Prepared g2_prepare(const G2Aff& q) {
  G2Prepared r;
  r.inf = q.inf;
  if (q.inf) return r;
  F2 X = q.x, Y = q.y, Z = f2_one();
  bool found = false;
  for (int b = 63; b >= 0; --b) {
    const bool bit = ((BLS_X >> 1) >> b) & 1;
    if (!found) { found = bit; continue; }
    r.lines.push_back(line_dbl(X, Y, Z));
    if (bit) r.lines.push_back(line_add(X, Y, Z, q));
  }
  r.lines.push_back(line_dbl(X, Y, Z));
  return r;
}

// affine G1 point in Montgomery form (Fp64), inf = identity
struct G1Aff64 {
  Fp64 x, y;
  bool inf;
};
// f * (c0 + c1 w^2 + c4 w^3): c0, c1 at Fp12.c0.{c0, c1}, c4 at Fp12.c1.c1
static F12 f12_mul_line(const F12& f, const LineCoeffs& l, const G1Aff64& p) {
  F12 s;
  memset(&s, 0, sizeof s);
  s.c0.c0 = l.c0;
  s.c0.c1 = f2_mul_fp(l.c1, p.x);
  s.c1.c1 = f2_mul_fp(l.c2, p.y);
  return f12_mul(f, s);
}
// prod_i f_{x, Q_i}(P_i), pairs with an identity on either side skipped (their pairing is 1)
static F12 multi_miller_loop(const G1Aff64* ps, const G2Prepared* const* qs, int n) {
  F12 f = f12_one();
  size_t idx = 0;
  bool found = false;
  auto step = [&](void) {
    for (int i = 0; i < n; ++i)
      if (!ps[i].inf && !qs[i]->inf) f = f12_mul_line(f, qs[i]->lines[idx], ps[i]);
    ++idx;
  };
  for (int b = 63; b >= 0; --b) {
    const bool bit = ((BLS_X >> 1) >> b) & 1;
    if (!found) { found = bit; continue; }
    step();
    if (bit) step();
    f = f12_sqr(f);
  }
  step();
  return f12_conj(f);   // x < 0
}
static F12 cyc_pow_x(const F12& f) {   // f^x for f in the cyclotomic subgroup: f^|x| conjugated
  F12 acc = f;
  for (int b = 62; b >= 0; --b) {
    acc = f12_sqr(acc);
    if ((BLS_X >> b) & 1) acc = f12_mul(acc, f);
  }
  return f12_conj(acc);
}
// f^(3 (p^12 - 1) / r):  easy part f^((p^6 - 1)(p^2 + 1)), then 3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3
static F12 final_exponentiation(const F12& f) {
  F12 m = f12_mul(f12_conj(f), f12_inv(f));
  m = f12_mul(f12_frob(m, 2), m);
  F12 a = f12_mul(cyc_pow_x(m), f12_conj(m));            // m^(x - 1)
  a = f12_mul(cyc_pow_x(a), f12_conj(a));                // m^((x - 1)^2)
  const F12 b = f12_mul(cyc_pow_x(a), f12_frob(a, 1));   // a^(x + p)
  const F12 c = f12_mul(f12_mul(cyc_pow_x(cyc_pow_x(b)), f12_frob(b, 2)), f12_conj(b));   // b^(x^2 + p^2 - 1)
  return f12_mul(c, f12_mul(f12_sqr(m), m));
}
static F12 pairing(const G1Aff64& p, const G2Prepared& q) {
  const G2Prepared* qs[1] = {&q};
  return final_exponentiation(multi_miller_loop(&p, qs, 1));
}

}  // namespace plonk
