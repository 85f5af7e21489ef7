// Witness diagnosis, the part that compiles for the host as well as for the device (no HIP): the 17 gate identities of one
// row, each tested for zero ON ITS OWN (never folded with a separation challenge, so the answer is exact), and the decoding
// of a sigma evaluation K_col * omega^row back into the wire position (col, row).  Included by diagnose.hip (value type: the
// reduced-radix twiddle form of fr29.cuh) and by the CPU test harness tests/csrc/host_diagnose.cpp (value type: Fr).
//
// The formulas are the ones widgets.hpp / poly.hip's quotient_kernel evaluate; the ORDER of the 17 values is the one the
// reference's debugger reports (src/debugger.rs:121-179):
//   0      arithmetic   (q_m a b + q_l a + q_r b + q_o c + q_f d + q_c) q_arith + PI
//   1-4    range        the quad deltas of c/d, b/c, a/b and next-row d / a, each times q_range
//   5-9    logic        the quad deltas of a, b, d, the product term, the xor/and relation, each times q_logic
//   10-13  fixed base   bit consistency, xy consistency, x accumulator, y accumulator, each times q_fixed_group_add
//   14-16  variable base addition: xy consistency, x3, y3, each times q_variable_group_add
// A field has no zero divisors, so "identity * selector != 0" is "selector != 0 and identity != 0": a family is only
// evaluated on rows whose selector value is non-zero, and the product with the selector is never formed.
//
// The value type T needs operator+ - * and an overload of diag_nonzero(const T&) that is exact whatever lazy range T keeps.
#pragma once
#include "field.cuh"
#include "permutation.hpp"

namespace plonk {

static constexpr int DIAG_FAMILIES = 17;           // gate identities; bit 17 of the per-family counts is "a copy constraint fails"
static constexpr uint32_t DIAG_POS_NONE = 0xFFFFFFFFu;   // never a packed position (permutation.hpp: n < 2^30)
// selector ids in plonk_prover_desc.polys order (poly.hpp's QS_* and widgets.hpp's WQS_* name the same numbers)
enum { DQ_M = 0, DQ_L, DQ_R, DQ_O, DQ_F, DQ_C, DQ_ARITH, DQ_RANGE, DQ_LOGIC, DQ_FIXED, DQ_VAR, DQ_COUNT };

HD bool diag_nonzero(const Fr& x) { return !x.is_zero(); }

template <class T>
struct DiagConsts {
  T one, two, three, c9, c18, c81, c83, ed;   // small constants and the Edwards d of the embedded curve
};

template <class T> HD T diag_x4(const T& x) { const T d = x + x; return d + d; }
template <class T> HD T diag_delta(const T& f, const DiagConsts<T>& k) {   // f (f-1)(f-2)(f-3)
  return f * (f - k.one) * (f - k.two) * (f - k.three);
}

// A row is read through a loader L:
//   T wire(col), T wire_next(col)   the value on wire col (0..3 = a, b, c, d) of this row / of row i + 1 mod n
//   bool sel_nonzero(id)            selector id is non-zero on this row
//   T sel(id)                       its value (zero when the selector polynomial is identically zero)
//   T pi()                          the public-input value of the row
template <class T, class L>
HD uint32_t diag_row_families(const L& ld, const DiagConsts<T>& k, bool widgets) {
  uint32_t m = 0;
  const T a = ld.wire(0), b = ld.wire(1), c = ld.wire(2), d = ld.wire(3);
  {
    T v = ld.pi();
    if (ld.sel_nonzero(DQ_ARITH))
      v = (ld.sel(DQ_M) * a * b + ld.sel(DQ_L) * a + ld.sel(DQ_R) * b + ld.sel(DQ_O) * c + ld.sel(DQ_F) * d + ld.sel(DQ_C)) *
              ld.sel(DQ_ARITH) + v;
    if (diag_nonzero(v)) m |= 1u;
  }
  if (!widgets) return m;
  if (ld.sel_nonzero(DQ_RANGE)) {
    const T d_w = ld.wire_next(3);
    if (diag_nonzero(diag_delta(c - diag_x4(d), k))) m |= 1u << 1;
    if (diag_nonzero(diag_delta(b - diag_x4(c), k))) m |= 1u << 2;
    if (diag_nonzero(diag_delta(a - diag_x4(b), k))) m |= 1u << 3;
    if (diag_nonzero(diag_delta(d_w - diag_x4(a), k))) m |= 1u << 4;
  }
  if (ld.sel_nonzero(DQ_LOGIC)) {
    const T la = ld.wire_next(0) - diag_x4(a), lb = ld.wire_next(1) - diag_x4(b), lo = ld.wire_next(3) - diag_x4(d);
    const T& w = c;
    if (diag_nonzero(diag_delta(la, k))) m |= 1u << 5;
    if (diag_nonzero(diag_delta(lb, k))) m |= 1u << 6;
    if (diag_nonzero(diag_delta(lo, k))) m |= 1u << 7;
    if (diag_nonzero(w - la * lb)) m |= 1u << 8;
    const T ab = la + lb;
    const T F = w * (w * (diag_x4(w) - k.c18 * ab + k.c81) + k.c18 * (la * la + lb * lb) - k.c81 * ab + k.c83);
    const T Ee = k.three * (ab + lo) - (F + F);
    const T Bb = ld.sel(DQ_C) * (k.c9 * lo - k.three * ab);
    if (diag_nonzero(Bb + Ee)) m |= 1u << 9;
  }
  if (ld.sel_nonzero(DQ_FIXED)) {
    const T a_w = ld.wire_next(0), b_w = ld.wire_next(1), d_w = ld.wire_next(3);
    const T bit = d_w - d - d;
    if (diag_nonzero(bit * (bit - k.one) * (bit + k.one))) m |= 1u << 10;
    if (diag_nonzero(bit * ld.sel(DQ_C) - c)) m |= 1u << 11;
    const T y_alpha = bit * bit * (ld.sel(DQ_R) - k.one) + k.one;
    const T x_alpha = ld.sel(DQ_L) * bit;
    const T cab = c * a * b * k.ed;
    if (diag_nonzero((a_w + a_w * cab) - (a * y_alpha + b * x_alpha))) m |= 1u << 12;
    if (diag_nonzero((b_w - b_w * cab) - (b * y_alpha + a * x_alpha))) m |= 1u << 13;
  }
  if (ld.sel_nonzero(DQ_VAR)) {
    const T a_w = ld.wire_next(0), b_w = ld.wire_next(1), x1y2 = ld.wire_next(3);
    const T y1x2 = b * c;
    const T dxy = k.ed * x1y2 * y1x2;
    if (diag_nonzero(a * d - x1y2)) m |= 1u << 14;
    if (diag_nonzero((x1y2 + y1x2) - (a_w + a_w * dxy))) m |= 1u << 15;
    if (diag_nonzero((b * d + a * c) - (b_w - b_w * dxy))) m |= 1u << 16;
  }
  return m;
}

// ---- sigma decoding ---------------------------------------------------------------------------------------------------
// s = K_col * omega^row with K = 1, 7, 13, 17 and omega of order n = 2^logn.  s^n = K_col^n names the column (the four
// values are pairwise distinct for every logn <= 28); s / K_col then lies in the cyclic group of order 2^logn and its
// discrete logarithm comes out bit by bit, lowest first (Pohlig-Hellman): t^(2^(logn-1-j)) is -1 exactly when bit j of
// what is left of the exponent is set, and multiplying by omega^(-2^j) clears it.  About logn^2 / 2 squarings.
static constexpr int DIAG_MAX_LOG = 28;
template <class T>
struct SigmaDecodeConsts {
  T one;
  T kn[4];      // K_col^n
  T kinv[4];    // 1 / K_col
  T winv[DIAG_MAX_LOG];   // omega^(-2^j)
  uint32_t logn;
};
template <class T>
HD uint32_t sigma_decode(const T& s, const SigmaDecodeConsts<T>& k) {
  T p = s;
  for (uint32_t j = 0; j < k.logn; ++j) p = p * p;
  uint32_t col = 4;
  for (uint32_t cc = 0; cc < 4; ++cc)
    if (!diag_nonzero(p - k.kn[cc])) col = cc;
  if (col == 4) return DIAG_POS_NONE;
  T t = s * k.kinv[col];
  uint32_t row = 0;
  for (uint32_t j = 0; j < k.logn; ++j) {
    T u = t;
    for (uint32_t i = j + 1; i < k.logn; ++i) u = u * u;
    if (diag_nonzero(u - k.one)) {
      row |= 1u << j;
      t = t * k.winv[j];
    }
  }
  if (diag_nonzero(t - k.one)) return DIAG_POS_NONE;
  return (col << SIGMA_ROW_BITS) | row;   // sigma_pack (permutation.hpp)
}

// ---- host-side constants over Fr (diagnose.hip converts them to its own value type) ------------------------------------
inline DiagConsts<Fr> diag_consts_fr() {
  DiagConsts<Fr> k;
  k.one = Fr::one();
  k.two = Fr::from_u64(2);
  k.three = Fr::from_u64(3);
  k.c9 = Fr::from_u64(9);
  k.c18 = Fr::from_u64(18);
  k.c81 = Fr::from_u64(81);
  k.c83 = Fr::from_u64(83);
  k.ed = (Fr::from_u64(10240) * Fr::from_u64(10241).inv()).neg();   // dusk_jubjub::EDWARDS_D
  return k;
}
inline SigmaDecodeConsts<Fr> sigma_decode_consts_fr(uint32_t logn) {
  SigmaDecodeConsts<Fr> k;
  k.one = Fr::one();
  k.logn = logn;
  const uint64_t ks[4] = {1, 7, 13, 17};   // src/composer/permutation/constants.rs
  for (int cc = 0; cc < 4; ++cc) {
    const Fr kc = Fr::from_u64(ks[cc]);
    k.kn[cc] = kc.pow_u64(1ull << logn);
    k.kinv[cc] = kc.inv();
  }
  Fr wi = fr_domain_root(logn).inv();
  for (int j = 0; j < DIAG_MAX_LOG; ++j) { k.winv[j] = wi; wi = wi.sqr(); }
  return k;
}

}  // namespace plonk
