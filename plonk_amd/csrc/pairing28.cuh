// The optimal-ate pairing check of hostpairing.hpp restated over the device field Fp28 (fp28.cuh), __host__ __device__ in
// place (the HD convention of field.cuh): pairing.hip runs it in one lane per check, tests/csrc/host_pairing28.cpp compiles
// the same code with g++ and compares it with hostpairing.hpp bit for bit.
//
// Same tower (Fp2 = Fp[u] / (u^2 + 1), Fp6 = Fp2[v] / (v^3 - xi), Fp12 = Fp6[w] / (w^2 - v)), same Frobenius constants
// (converted from the host's, not recomputed), same Miller loop over PREPARED line coefficients, same final exponentiation
// (the e^3 map).  Three routines are specialised, each equal to the generic f12r_mul on every input it is used for (they
// change the cost, never the value; tests/csrc/host_pairing28.cpp compares them): the sparse line product (a line has three
// non-zero Fp2 coefficients of twelve: 13 Fp2 products for 18), the complex-method f12r_sqr (two Fp6 products for three) and
// the Granger-Scott squaring on the cyclotomic subgroup (nine Fp2 squarings) for cyc_pow_x_28.
//
// Bounds.  Every coordinate that is stored is normalised (limbs < 2^28) and below 2p: products come out of Fp28::mul /
// mul2 that way, and sums and differences pass p28_red, a subtraction of floor(top limb / (p's top limb + 1)) * p — one
// short multiply-and-carry chain, about a tenth of a product.  Inside an Fp2 product the lazy forms of fp28.cuh are used
// where their documented limits allow (annotated per line).
//
// Registers.  An Fp12 is 168 limbs and cannot sit in registers next to a product, so Fp6 / Fp12 values live in private
// memory and their routines are out of line (P28_NOINLINE) with pointer arguments; Fp2 operations are inline and stay in
// registers.  No array in here is indexed by a run-time value unless it is already in memory.
#pragma once
#include "curve28.cuh"
#include "hostpairing.hpp"

#if defined(__HIPCC__)
#define P28_NOINLINE __host__ __device__ __attribute__((noinline)) inline
#else
#define P28_NOINLINE inline
#endif

namespace plonk {

// v normalised with value < 64p  ->  the same residue, normalised and < 2p
HD Fp28 p28_red(const Fp28& v) {
  // q = floor(top / (ptop + 1)) never exceeds floor(v / p), and v - q p < 2^364 (ptop + 65) < 2p for top < 64 (ptop + 1)
  const uint32_t q = v.l[Fp28::N - 1] / (Fp28::mod(Fp28::N - 1) + 1u);
  Fp28 r;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) {
    const int64_t d = (int64_t)v.l[i] - (int64_t)((uint64_t)q * Fp28::mod(i)) + c;
    if (i < Fp28::N - 1) {
      r.l[i] = (uint32_t)d & Fp28::MASK;
      c = d >> Fp28::B;
    } else {
      r.l[i] = (uint32_t)d;
    }
  }
  return r;
}
HD Fp28 p28_add(const Fp28& a, const Fp28& b) { return p28_red(Fp28::add(a, b)); }        // < 4p
HD Fp28 p28_sub(const Fp28& a, const Fp28& b) { return p28_red(Fp28::sub<4>(a, b)); }     // < 6p
HD Fp28 p28_neg(const Fp28& a) { return p28_red(Fp28::neg_lazy<4>(a).normalized()); }    // <= 4p

struct F2r {   // a + b u
  Fp28 a, b;
};
HD F2r f2r_zero() { return {Fp28::zero(), Fp28::zero()}; }
HD F2r f2r_one() { return {Fp28::one(), Fp28::zero()}; }
HD F2r f2r_add(const F2r& x, const F2r& y) { return {p28_add(x.a, y.a), p28_add(x.b, y.b)}; }
HD F2r f2r_sub(const F2r& x, const F2r& y) { return {p28_sub(x.a, y.a), p28_sub(x.b, y.b)}; }
HD F2r f2r_neg(const F2r& x) { return {p28_neg(x.a), p28_neg(x.b)}; }
HD F2r f2r_conj(const F2r& x) { return {x.a, p28_neg(x.b)}; }
HD F2r f2r_mul_xi(const F2r& x) { return {p28_sub(x.a, x.b), p28_add(x.a, x.b)}; }   // (a + b u)(1 + u)
// two fused two-product reductions: the cost of Karatsuba's three products (6 x 196 mads) with results below 2p at once
HD F2r f2r_mul(const F2r& x, const F2r& y) {
  F2r r;
  r.a = Fp28::mul2(x.a, y.a, x.b, Fp28::neg_lazy<4>(y.b));   // 2*2 + 2*4 = 12; the lazy operand meets a normalised one
  r.b = Fp28::mul2(x.a, y.b, x.b, y.a);                      // 2*2 + 2*2 = 8
  return r;
}
HD F2r f2r_sqr(const F2r& x) {
  F2r r;
  r.a = Fp28::mul(Fp28::add_lazy(x.a, x.b), Fp28::sub_lazy<4>(x.a, x.b));   // 4 * 6 = 24; mul takes two lazy operands
  r.b = Fp28::mul(Fp28::add_lazy(x.a, x.a), x.b);                           // 4 * 2
  return r;
}
HD F2r f2r_mul_fp(const F2r& x, const Fp28& k) { return {Fp28::mul(x.a, k), Fp28::mul(x.b, k)}; }
HD F2r f2r_inv(const F2r& x) {   // (a - b u) / (a^2 + b^2)
  const Fp28 n = fp28_inv_gcd(Fp28::mul2(x.a, x.a, x.b, x.b));
  return {Fp28::mul(x.a, n), Fp28::mul(p28_neg(x.b), n)};
}
HD bool p28_is_one(const Fp28& v) {
  const Fp28 c = v.canon(), o = Fp28::one();
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) acc |= c.l[i] ^ o.l[i];
  return acc == 0;
}

struct F6r {
  F2r c0, c1, c2;
};
struct F12r {
  F6r c0, c1;
};

P28_NOINLINE void f6r_add(F6r* r, const F6r* x, const F6r* y) {
  r->c0 = f2r_add(x->c0, y->c0);
  r->c1 = f2r_add(x->c1, y->c1);
  r->c2 = f2r_add(x->c2, y->c2);
}
P28_NOINLINE void f6r_sub(F6r* r, const F6r* x, const F6r* y) {
  r->c0 = f2r_sub(x->c0, y->c0);
  r->c1 = f2r_sub(x->c1, y->c1);
  r->c2 = f2r_sub(x->c2, y->c2);
}
P28_NOINLINE void f6r_neg(F6r* r, const F6r* x) {
  r->c0 = f2r_neg(x->c0);
  r->c1 = f2r_neg(x->c1);
  r->c2 = f2r_neg(x->c2);
}
P28_NOINLINE void f6r_mul_v(F6r* r, const F6r* x) {   // r may be x
  const F2r t = f2r_mul_xi(x->c2);
  r->c2 = x->c1;
  r->c1 = x->c0;
  r->c0 = t;
}
// Karatsuba over the three coefficients, as f6_mul; r may be x or y (every read of x and y precedes the stores)
P28_NOINLINE void f6r_mul(F6r* r, const F6r* x, const F6r* y) {
  const F2r t0 = f2r_mul(x->c0, y->c0), t1 = f2r_mul(x->c1, y->c1), t2 = f2r_mul(x->c2, y->c2);
  const F2r c0 = f2r_add(t0, f2r_mul_xi(f2r_sub(f2r_sub(f2r_mul(f2r_add(x->c1, x->c2), f2r_add(y->c1, y->c2)), t1), t2)));
  const F2r c1 = f2r_add(f2r_sub(f2r_sub(f2r_mul(f2r_add(x->c0, x->c1), f2r_add(y->c0, y->c1)), t0), t1), f2r_mul_xi(t2));
  const F2r c2 = f2r_add(f2r_sub(f2r_sub(f2r_mul(f2r_add(x->c0, x->c2), f2r_add(y->c0, y->c2)), t0), t2), t1);
  r->c0 = c0;
  r->c1 = c1;
  r->c2 = c2;
}
P28_NOINLINE void f6r_inv(F6r* r, const F6r* x) {
  const F2r A = f2r_sub(f2r_sqr(x->c0), f2r_mul_xi(f2r_mul(x->c1, x->c2)));
  const F2r B = f2r_sub(f2r_mul_xi(f2r_sqr(x->c2)), f2r_mul(x->c0, x->c1));
  const F2r C = f2r_sub(f2r_sqr(x->c1), f2r_mul(x->c0, x->c2));
  const F2r n = f2r_add(f2r_mul(x->c0, A), f2r_mul_xi(f2r_add(f2r_mul(x->c2, B), f2r_mul(x->c1, C))));
  const F2r ni = f2r_inv(n);
  r->c0 = f2r_mul(A, ni);
  r->c1 = f2r_mul(B, ni);
  r->c2 = f2r_mul(C, ni);
}

P28_NOINLINE void f12r_set_one(F12r* r) {
  r->c0.c0 = f2r_one();
  r->c0.c1 = f2r_zero();
  r->c0.c2 = f2r_zero();
  r->c1.c0 = f2r_zero();
  r->c1.c1 = f2r_zero();
  r->c1.c2 = f2r_zero();
}
// r may be x or y
P28_NOINLINE void f12r_mul(F12r* r, const F12r* x, const F12r* y) {
  F6r t0, t1, s, u;
  f6r_mul(&t0, &x->c0, &y->c0);
  f6r_mul(&t1, &x->c1, &y->c1);
  f6r_add(&s, &x->c0, &x->c1);
  f6r_add(&u, &y->c0, &y->c1);
  f6r_mul(&s, &s, &u);
  f6r_sub(&s, &s, &t0);
  f6r_sub(&r->c1, &s, &t1);
  f6r_mul_v(&t1, &t1);
  f6r_add(&r->c0, &t0, &t1);
}
// x^2 by the complex method: c0' = (c0 + c1)(c0 + v c1) - c0 c1 - v c0 c1, c1' = 2 c0 c1; r may be x
P28_NOINLINE void f12r_sqr(F12r* r, const F12r* x) {
  F6r ab, s, t;
  f6r_mul(&ab, &x->c0, &x->c1);
  f6r_add(&s, &x->c0, &x->c1);
  f6r_mul_v(&t, &x->c1);
  f6r_add(&t, &t, &x->c0);
  f6r_mul(&s, &s, &t);
  f6r_sub(&s, &s, &ab);
  f6r_add(&r->c1, &ab, &ab);
  f6r_mul_v(&ab, &ab);
  f6r_sub(&r->c0, &s, &ab);
}
// x * (a0 + a1 v): five Fp2 products; r may be x
P28_NOINLINE void f6r_mul_01(F6r* r, const F6r* x, const F2r* a0, const F2r* a1) {
  const F2r t0 = f2r_mul(x->c0, *a0), t1 = f2r_mul(x->c1, *a1);
  const F2r c0 = f2r_add(t0, f2r_mul_xi(f2r_mul(x->c2, *a1)));
  const F2r c1 = f2r_sub(f2r_sub(f2r_mul(f2r_add(x->c0, x->c1), f2r_add(*a0, *a1)), t0), t1);
  const F2r c2 = f2r_add(t1, f2r_mul(x->c2, *a0));
  r->c0 = c0;
  r->c1 = c1;
  r->c2 = c2;
}
// x * (b1 v): three Fp2 products; r may be x
P28_NOINLINE void f6r_mul_1(F6r* r, const F6r* x, const F2r* b1) {
  const F2r c0 = f2r_mul_xi(f2r_mul(x->c2, *b1)), c1 = f2r_mul(x->c0, *b1), c2 = f2r_mul(x->c1, *b1);
  r->c0 = c0;
  r->c1 = c1;
  r->c2 = c2;
}
// x * ((a0 + a1 v) + (b1 v) w), the shape of a line: Karatsuba over w with the two sparse Fp6 products; r may be x
P28_NOINLINE void f12r_mul_014(F12r* r, const F12r* x, const F2r* a0, const F2r* a1, const F2r* b1) {
  F6r t0, t1, s;
  const F2r ab = f2r_add(*a1, *b1);
  f6r_mul_01(&t0, &x->c0, a0, a1);
  f6r_mul_1(&t1, &x->c1, b1);
  f6r_add(&s, &x->c0, &x->c1);
  f6r_mul_01(&s, &s, a0, &ab);
  f6r_sub(&s, &s, &t0);
  f6r_sub(&r->c1, &s, &t1);
  f6r_mul_v(&t1, &t1);
  f6r_add(&r->c0, &t0, &t1);
}
// (a + b s)^2 in Fp4 = Fp2[s] / (s^2 - xi): three Fp2 squarings
HD void f4r_sqr(const F2r& a, const F2r& b, F2r* c0, F2r* c1) {
  const F2r t0 = f2r_sqr(a), t1 = f2r_sqr(b);
  *c0 = f2r_add(f2r_mul_xi(t1), t0);
  *c1 = f2r_sub(f2r_sub(f2r_sqr(f2r_add(a, b)), t0), t1);
}
// x^2 for x in the cyclotomic subgroup (Granger, Scott: "Faster squaring in the cyclotomic subgroup of sixth degree
// extensions", PKC 2010): the three Fp4 squarings of (c0.c0, c1.c1), (c1.c0, c0.c2), (c0.c1, c1.c2); r may be x
P28_NOINLINE void f12r_cyc_sqr(F12r* r, const F12r* x) {
  const F2r z0 = x->c0.c0, z4 = x->c0.c1, z3 = x->c0.c2, z2 = x->c1.c0, z1 = x->c1.c1, z5 = x->c1.c2;
  F2r t0, t1, t2, t3, d;
  f4r_sqr(z0, z1, &t0, &t1);
  d = f2r_sub(t0, z0);
  r->c0.c0 = f2r_add(f2r_add(d, d), t0);    // 3 t0 - 2 z0
  d = f2r_add(t1, z1);
  r->c1.c1 = f2r_add(f2r_add(d, d), t1);    // 3 t1 + 2 z1
  f4r_sqr(z2, z3, &t0, &t1);
  f4r_sqr(z4, z5, &t2, &t3);
  d = f2r_sub(t0, z4);
  r->c0.c1 = f2r_add(f2r_add(d, d), t0);
  d = f2r_add(t1, z5);
  r->c1.c2 = f2r_add(f2r_add(d, d), t1);
  t0 = f2r_mul_xi(t3);
  d = f2r_add(t0, z2);
  r->c1.c0 = f2r_add(f2r_add(d, d), t0);
  d = f2r_sub(t2, z3);
  r->c0.c2 = f2r_add(f2r_add(d, d), t2);
}
P28_NOINLINE void f12r_conj(F12r* r, const F12r* x) {   // x^(p^6); r may be x
  r->c0 = x->c0;
  f6r_neg(&r->c1, &x->c1);
}
P28_NOINLINE void f12r_inv(F12r* r, const F12r* x) {   // (c0 - c1 w) / (c0^2 - v c1^2); r may be x
  F6r a, b;
  f6r_mul(&a, &x->c0, &x->c0);
  f6r_mul(&b, &x->c1, &x->c1);
  f6r_mul_v(&b, &b);
  f6r_sub(&a, &a, &b);
  f6r_inv(&a, &a);
  f6r_mul(&b, &x->c1, &a);
  f6r_mul(&r->c0, &x->c0, &a);
  f6r_neg(&r->c1, &b);
}
P28_NOINLINE bool f12r_is_one(const F12r* x) {
  bool ok = p28_is_one(x->c0.c0.a) && x->c0.c0.b.is_zero_mod();
  ok = ok && x->c0.c1.a.is_zero_mod() && x->c0.c1.b.is_zero_mod() && x->c0.c2.a.is_zero_mod() && x->c0.c2.b.is_zero_mod();
  ok = ok && x->c1.c0.a.is_zero_mod() && x->c1.c0.b.is_zero_mod() && x->c1.c1.a.is_zero_mod() && x->c1.c1.b.is_zero_mod();
  return ok && x->c1.c2.a.is_zero_mod() && x->c1.c2.b.is_zero_mod();
}

// ---- what a check reads from memory: the Frobenius constants and the prepared lines of x_h and h ------------------------
struct Line28 {
  F2r c0, c1, c2;
};
static constexpr int PAIRING_LINES = 68;   // 62 doublings + 5 additions + the last doubling of |x| / 2
struct PairingTables28 {
  F2r frob[3][6];   // FrobConsts::g
  Line28 xh[PAIRING_LINES], h[PAIRING_LINES];
  uint32_t xh_inf, h_inf;
};

// x^(p^k), k = 1, 2, 3: coefficient 3 h + i of the tower order is a w^(2 i + h); r may be x
P28_NOINLINE void f12r_frob(F12r* r, const F12r* x, int k, const PairingTables28* T) {
  const F2r* in = &x->c0.c0;
  F2r* out = &r->c0.c0;
  for (int h = 0; h < 2; ++h)
    for (int i = 0; i < 3; ++i) {
      const F2r a = in[3 * h + i];
      out[3 * h + i] = f2r_mul((k & 1) ? f2r_conj(a) : a, T->frob[k - 1][2 * i + h]);
    }
}

// f * (c0 + (c1 px) w^2 + (c2 py) w^3), the value of f12_mul_line: w^2 = v, w^3 = v w, so the line is (c0 + (c1 px) v) + ((c2 py) v) w
P28_NOINLINE void f12r_mul_line(F12r* f, const Line28* l, const Fp28* px, const Fp28* py) {
  const F2r a1 = f2r_mul_fp(l->c1, *px), b1 = f2r_mul_fp(l->c2, *py);
  f12r_mul_014(f, f, &l->c0, &a1, &b1);
}
// the same through the generic product (what the sparse form is tested against)
P28_NOINLINE void f12r_mul_line_generic(F12r* f, const Line28* l, const Fp28* px, const Fp28* py) {
  F12r s;
  s.c0.c0 = l->c0;
  s.c0.c1 = f2r_mul_fp(l->c1, *px);
  s.c0.c2 = f2r_zero();
  s.c1.c0 = f2r_zero();
  s.c1.c1 = f2r_mul_fp(l->c2, *py);
  s.c1.c2 = f2r_zero();
  f12r_mul(f, f, &s);
}

struct G1Aff28 {   // affine, coordinates < 2p; inf = identity
  Fp28 x, y;
  uint32_t inf;
};

// multi_miller_loop for the two pairs (a, x_h), (b, h); a pair with an identity on either side is skipped
P28_NOINLINE void miller2_28(F12r* f, const PairingTables28* T, const G1Aff28* a, const G1Aff28* b) {
  const bool use_a = !a->inf && !T->xh_inf, use_b = !b->inf && !T->h_inf;
  f12r_set_one(f);
  int idx = 0;
  bool found = false;
  for (int bit_i = 63; bit_i >= 0; --bit_i) {
    const bool bit = ((BLS_X >> 1) >> bit_i) & 1;
    if (!found) { found = bit; continue; }
    for (int s = 0; s < (bit ? 2 : 1); ++s) {
      if (use_a) f12r_mul_line(f, &T->xh[idx], &a->x, &a->y);
      if (use_b) f12r_mul_line(f, &T->h[idx], &b->x, &b->y);
      ++idx;
    }
    f12r_sqr(f, f);
  }
  if (use_a) f12r_mul_line(f, &T->xh[idx], &a->x, &a->y);
  if (use_b) f12r_mul_line(f, &T->h[idx], &b->x, &b->y);
  f12r_conj(f, f);   // x < 0
}

P28_NOINLINE void cyc_pow_x_28(F12r* r, const F12r* f) {   // f^x on the cyclotomic subgroup; r must not be f
  *r = *f;
  for (int b = 62; b >= 0; --b) {
    f12r_cyc_sqr(r, r);
    if ((BLS_X >> b) & 1) f12r_mul(r, r, f);
  }
  f12r_conj(r, r);
}

// f^(3 (p^12 - 1) / r), the steps of final_exponentiation; r may be f
P28_NOINLINE void final_exponentiation_28(F12r* r, const F12r* f, const PairingTables28* T) {
  F12r m, a, b, t, u;
  f12r_conj(&t, f);
  f12r_inv(&u, f);
  f12r_mul(&m, &t, &u);
  f12r_frob(&t, &m, 2, T);
  f12r_mul(&m, &t, &m);
  cyc_pow_x_28(&t, &m);
  f12r_conj(&u, &m);
  f12r_mul(&a, &t, &u);            // m^(x - 1)
  cyc_pow_x_28(&t, &a);
  f12r_conj(&u, &a);
  f12r_mul(&a, &t, &u);            // m^((x - 1)^2)
  cyc_pow_x_28(&t, &a);
  f12r_frob(&u, &a, 1, T);
  f12r_mul(&b, &t, &u);            // a^(x + p)
  cyc_pow_x_28(&t, &b);
  cyc_pow_x_28(&u, &t);
  f12r_frob(&t, &b, 2, T);
  f12r_mul(&u, &u, &t);
  f12r_conj(&t, &b);
  f12r_mul(&u, &u, &t);            // c = b^(x^2 + p^2 - 1)
  f12r_cyc_sqr(&t, &m);
  f12r_mul(&t, &t, &m);
  f12r_mul(r, &u, &t);
}

// an XYZZ point in the 12 x 32-bit form (what the sum kernels write; ZZ == 0 marks the identity) -> affine over Fp28
HD G1Aff28 g1aff28_of_g1(const G1& p) {
  G1Aff28 r;
  r.inf = p.is_identity() ? 1u : 0u;
  if (r.inf) {
    r.x = Fp28::zero();
    r.y = Fp28::zero();
    return r;
  }
  const Fp28 zz = Fp28::from_fp(p.ZZ), zzz = Fp28::from_fp(p.ZZZ);
  const Fp28 inv = fp28_inv_gcd(Fp28::mul(zz, zzz));
  r.x = Fp28::mul(Fp28::from_fp(p.X), Fp28::mul(inv, zzz));
  r.y = Fp28::mul(Fp28::from_fp(p.Y), Fp28::mul(inv, zz));
  return r;
}

// e(-A, x_h) e(B, h) raised by the final exponentiation: one two-pair Miller loop, one final exponentiation
P28_NOINLINE void pairing_check_value_28(F12r* out, const PairingTables28* T, const G1& A, const G1& B) {
  G1Aff28 a = g1aff28_of_g1(A);
  const G1Aff28 b = g1aff28_of_g1(B);
  if (!a.inf) a.y = p28_neg(a.y);
  miller2_28(out, T, &a, &b);
  final_exponentiation_28(out, out, T);
}

// the value as 12 canonical integers (6 x 64-bit words each) in tower order: put_f12 of tests/csrc/host_verify.cpp
HD void p28_put_canonical(const Fp28& v, uint64_t* out6) {
  Fp28 one_int = Fp28::zero();
  one_int.l[0] = 1;
  const Fp28 c = Fp28::mul(v, one_int).canon();   // x R' / R'
  uint32_t w[12];
  c.reslice_to32(w);
#pragma unroll
  for (int i = 0; i < 6; ++i) out6[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}
P28_NOINLINE void f12r_put(const F12r* f, uint64_t* out72) {
  const F2r* c = &f->c0.c0;
  for (int i = 0; i < 6; ++i) {
    p28_put_canonical(c[i].a, out72 + 12 * i);
    p28_put_canonical(c[i].b, out72 + 12 * i + 6);
  }
}

// ---- host: the tables from the host's prepared points ---------------------------------------------------------------------
static inline Fp28 p28_of_fp64(const Fp64& x) { return Fp28::from_fp(from64(x)); }
static inline Fp64 fp64_of_p28(const Fp28& x) { return to64(x.to_fp()); }
static inline F2r f2r_of_f2(const F2& x) { return {p28_of_fp64(x.a), p28_of_fp64(x.b)}; }
static inline F2 f2_of_f2r(const F2r& x) { return {fp64_of_p28(x.a), fp64_of_p28(x.b)}; }
// false when a prepared point does not have the PAIRING_LINES lines of a finite point (or none, for the identity)
static bool pairing_tables_fill(const G2Prepared& x_h, const G2Prepared& h, PairingTables28* T) {
  memset(T, 0, sizeof *T);
  const FrobConsts& fc = frob_consts();
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 6; ++j) T->frob[k][j] = f2r_of_f2(fc.g[k][j]);
  const G2Prepared* src[2] = {&x_h, &h};
  Line28* dst[2] = {T->xh, T->h};
  for (int s = 0; s < 2; ++s) {
    if (src[s]->inf) continue;
    if (src[s]->lines.size() != (size_t)PAIRING_LINES) return false;
    for (int i = 0; i < PAIRING_LINES; ++i) {
      const LineCoeffs& l = src[s]->lines[i];
      dst[s][i] = Line28{f2r_of_f2(l.c0), f2r_of_f2(l.c1), f2r_of_f2(l.c2)};
    }
  }
  T->xh_inf = x_h.inf ? 1u : 0u;
  T->h_inf = h.inf ? 1u : 0u;
  return true;
}

}  // namespace plonk
