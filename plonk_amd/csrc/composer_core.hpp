// The gadget composer, the part that compiles for the host as well as for the device (no HIP): every gadget of the
// reference's composer stated ONCE, as a template over a backend B, giving both the gates it emits and how the value of
// every witness it allocates follows from its inputs.  Two kinds of backend walk the same statement:
//   a recorder (B::EXEC == false; composer_host.hpp): alloc() hands out the next witness index, emit() appends a gate;
//     values are never looked at
//   an executor (B::EXEC == true; composer.hip's lanes, composer_host.hpp's one-thread host executor): alloc(v) stores v
//     in the next slot of the witness table, get() reads a slot, emit() is empty
// so a gadget's witness order is the same for both by construction, and a record of the witness program (ComposerOp) only
// has to say which gadget, which width, which inputs and where its contiguous outputs begin.
//
// Restated from the reference (cited per gadget): src/composer.rs, src/composer/{bits,range,logic,select,truncate,point,
// fixed_base}.rs.  Gate layouts are pinned by the reference's own gate_digest literals (tests/golden/composer_layouts.json).
//
// No runtime-indexed local array anywhere: bits are taken off a 256-bit integer by shifting it, signed digits live in two
// 256-bit masks, and the intermediates of the whole-gadget scalar multiplications (Z coordinates, prefix products of the
// one batch inversion) are parked in the gadget's own output slots until the inverse is known.
#pragma once
#include "field.cuh"
#include "fp_safegcd.cuh"   // fr_inv_gcd

namespace plonk {

// kinds of a witness-program record (the public enum plonk_gadget names the gadgets; several of those are a few records)
enum : uint32_t {
  CK_CONST = 0,    // out = pool[cst]                                         (append_constant, the witnesses of Composer::initialized)
  CK_GATE,         // out = (q_m a b + q_l a + q_r b + q_f d + q_c) * ninv    (append_evaluated_output; pool: q_m q_l q_r q_f q_c -1/q_o)
  CK_SELECT,       // component_select: 4 outputs
  CK_SELECT_ONE,   // component_select_one
  CK_DECOMP,       // component_decomposition<width>: 2 * width outputs
  CK_RANGE,        // range_check(width): the quad accumulators (+ 3 for an odd width)
  CK_TRUNCATE,     // component_truncate<width>
  CK_SPLIT,        // bind_truncation_split(input, low, width)
  CK_CANONICAL,    // assert_canonical_truncation(high, low, width)
  CK_JJ_SCALAR,    // assert_canonical_jubjub_scalar
  CK_LOGIC_AND,    // append_logic_and<width>  (width = bit pairs)
  CK_LOGIC_XOR,
  CK_ADD_POINT,    // add_point_gates: x1 y2, x3, y3
  CK_TORSION,      // assert_torsion_free_point: 14 outputs, one inversion
  CK_MUL_GEN,      // component_mul_generator: 1280 outputs, one inversion (pool: the 256 multiples of the generator)
  CK_MUL_POINT,    // component_mul_point: 2520 outputs, one inversion
  CK_COUNT
};

struct ComposerOp {
  uint32_t kind, width;
  uint32_t in[4];       // input witness indices (unused: 0)
  uint32_t out0, nout;  // the contiguous witness slots the gadget allocated
  uint32_t cst;         // first constant of the record in the Fr constant pool
  uint32_t level;       // 1 + the highest level among the producers of its inputs (inputs and constants: 0)
  uint32_t id;          // index of the record in allocation order (what the error word reports)
};
struct ComposerPiRow {  // a public-input row: PI = -(q_m a b + q_l a + q_r b + q_o c + q_f d + q_c) under the filled witnesses
  uint32_t row, w[4];
  uint32_t cst;         // pool: q_m q_l q_r q_o q_f q_c
};
static constexpr uint32_t COMPOSER_NO_ERROR = 0xFFFFFFFFu;

// one gate: the 11 selectors in plonk_prover_desc.polys order and the four wires
struct ComposerRow {
  Fr q[11];
  uint32_t w[4];
  bool pi;
};
enum { CQ_M = 0, CQ_L, CQ_R, CQ_O, CQ_F, CQ_C, CQ_ARITH, CQ_RANGE, CQ_LOGIC, CQ_FIXED, CQ_VAR };

HD ComposerRow crow(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  ComposerRow r;
#pragma unroll
  for (int i = 0; i < 11; ++i) r.q[i] = Fr::zero();
  r.w[0] = a; r.w[1] = b; r.w[2] = c; r.w[3] = d;
  r.pi = false;
  return r;
}
// Constraint::arithmetic (constraint.rs:203): the six external selectors + q_arith = 1
HD ComposerRow crow_arith(const Fr& qm, const Fr& ql, const Fr& qr, const Fr& qo, const Fr& qf, const Fr& qc, uint32_t a, uint32_t b,
                          uint32_t c, uint32_t d) {
  ComposerRow r = crow(a, b, c, d);
  r.q[CQ_M] = qm; r.q[CQ_L] = ql; r.q[CQ_R] = qr; r.q[CQ_O] = qo; r.q[CQ_F] = qf; r.q[CQ_C] = qc;
  r.q[CQ_ARITH] = Fr::one();
  return r;
}

// The inversion is the one primitive that is CALLED rather than inlined on the device: a gadget lane inverts at most once or
// twice, and a dozen inlined copies of the safegcd loop are most of what the executor kernel would otherwise compile.
// By value: a reference would pin the operand to memory.
#if defined(__HIPCC__)
__host__ __device__ __noinline__ inline Fr cg_inv(Fr a) { return fr_inv_gcd(a); }
#else
inline Fr cg_inv(Fr a) { return fr_inv_gcd(a); }
#endif

// ---- 256-bit integers (canonical values), static indexing only ----------------------------------------------------------
struct U256 {
  uint32_t l[8];
};
HD U256 u256_zero() { U256 r; for (int i = 0; i < 8; ++i) r.l[i] = 0; return r; }
HD U256 u256_of(const Fr& x) {   // the canonical integer of a Montgomery value
  const Fr c = x.from_mont();
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = c.l[i];
  return r;
}
HD Fr u256_fr(const U256& x) {   // any integer below 2^256, reduced
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = x.l[i];
  return r.to_mont();
}
HD U256 u256_shl(const U256& x, uint32_t s) {   // s < 256; a barrel shifter: words by 4, 2, 1, then bits
  U256 r = x;
  if (s & 128) {
#pragma unroll
    for (int i = 7; i >= 0; --i) r.l[i] = i >= 4 ? r.l[i - 4] : 0;
  }
  if (s & 64) {
#pragma unroll
    for (int i = 7; i >= 0; --i) r.l[i] = i >= 2 ? r.l[i - 2] : 0;
  }
  if (s & 32) {
#pragma unroll
    for (int i = 7; i >= 0; --i) r.l[i] = i >= 1 ? r.l[i - 1] : 0;
  }
  const uint32_t b = s & 31;
  if (b) {
#pragma unroll
    for (int i = 7; i >= 0; --i) r.l[i] = (r.l[i] << b) | (i ? r.l[i - 1] >> (32 - b) : 0);
  }
  return r;
}
HD U256 u256_shr(const U256& x, uint32_t s) {   // s < 256
  U256 r = x;
  if (s & 128) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = i + 4 < 8 ? r.l[i + 4] : 0;
  }
  if (s & 64) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = i + 2 < 8 ? r.l[i + 2] : 0;
  }
  if (s & 32) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = i + 1 < 8 ? r.l[i + 1] : 0;
  }
  const uint32_t b = s & 31;
  if (b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = (r.l[i] >> b) | (i < 7 ? r.l[i + 1] << (32 - b) : 0);
  }
  return r;
}
HD U256 u256_low(const U256& x, uint32_t bits) {   // x mod 2^bits, bits <= 256
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t lo = 32u * i;
    r.l[i] = bits >= lo + 32 ? x.l[i] : (bits > lo ? x.l[i] & ((1u << (bits - lo)) - 1u) : 0u);
  }
  return r;
}
HD U256 u256_bits(const U256& x, uint32_t start, uint32_t end) {   // recompose_bits (bits.rs:18-32): bits [start, end), end <= 256
  if (start >= 256) return u256_zero();
  return u256_low(u256_shr(x, start), end - start);
}
HD bool u256_geq(const U256& a, const uint32_t (&m)[8]) {
  bool ge = true;   // equal so far
#pragma unroll
  for (int i = 0; i < 8; ++i) ge = a.l[i] > m[i] || (a.l[i] == m[i] && ge);
  return ge;
}
HD Fr fr_pow2(uint32_t k) {   // BlsScalar::pow_of_2(k), k < 256
  U256 o = u256_zero();
  o.l[0] = 1;
  return u256_fr(u256_shl(o, k));
}
HD Fr fr_limbs(const uint32_t (&v)[8]) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = v[i];
  return r;
}

// ---- the embedded curve: -x^2 + y^2 = 1 + d x^2 y^2 over Fr ---------------------------------------------------------------
HD Fr jj_d() {   // dusk_jubjub::EDWARDS_D = -(10240 / 10241), Montgomery limbs
  constexpr uint32_t v[8] = {0xb974f6b0u, 0x2a522455u, 0x0d9acab3u, 0xfc6cc9efu, 0xc27628d1u, 0x7a08fb94u, 0xfe0e262eu, 0x57f8f6a8u};
  return fr_limbs(v);
}
// order of the prime-order subgroup, and 8^-1 modulo it (point.rs:22-27), canonical limbs
#define JJ_ORDER_LIMBS {0xd6f72cb7u, 0xd0970e5eu, 0xccc81082u, 0xa6682093u, 0x01343b00u, 0x06673b01u, 0x6533afa9u, 0x0e7db4eau}
#define JJ_EIGHT_INV_LIMBS {0xdadee597u, 0x5a12e1cbu, 0x79990210u, 0x14cd0412u, 0x20268760u, 0x20cce760u, 0x4ca675f5u, 0x01cfb69du}
#define FR_MODULUS_MINUS_ONE_LIMBS {0x00000000u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}

struct JJ {   // projective (X : Y : Z), x = X / Z
  Fr X, Y, Z;
};
HD JJ jj_identity() { return JJ{Fr::zero(), Fr::one(), Fr::one()}; }
// complete addition (a = -1 a square, d a non-square): add-2008-bbjlp
HD JJ jj_add(const JJ& p, const JJ& q) {
  const Fr A = p.Z * q.Z, B = A * A, C = p.X * q.X, D = p.Y * q.Y, E = jj_d() * C * D, F = B - E, G = B + E;
  JJ r;
  r.X = A * F * ((p.X + p.Y) * (q.X + q.Y) - C - D);
  r.Y = A * G * (D + C);
  r.Z = F * G;
  return r;
}
HD JJ jj_add_affine(const JJ& p, const Fr& x2, const Fr& y2) {   // Z2 = 1
  const Fr B = p.Z * p.Z, C = p.X * x2, D = p.Y * y2, E = jj_d() * C * D, F = B - E, G = B + E;
  JJ r;
  r.X = p.Z * F * ((p.X + p.Y) * (x2 + y2) - C - D);
  r.Y = p.Z * G * (D + C);
  r.Z = F * G;
  return r;
}
HD bool jj_on_curve(const Fr& x, const Fr& y) {
  const Fr x2 = x * x, y2 = y * y;
  return (y2 - x2) == (Fr::one() + jj_d() * x2 * y2);
}
// [k] (x, y) for a canonical 256-bit k, most significant bit first
HD JJ jj_mul(const Fr& x, const Fr& y, U256 k) {
  JJ r = jj_identity();
  for (int i = 0; i < 256; ++i) {
    r = jj_add(r, r);
    if (k.l[7] >> 31) r = jj_add_affine(r, x, y);
    k = u256_shl(k, 1);
  }
  return r;
}

// ---- composer basics (composer.rs) ---------------------------------------------------------------------------------------
// witnesses 0 and 1 are the constants zero and one of Composer::initialized (composer.rs:177-189)
static constexpr uint32_t CW_ZERO = 0, CW_ONE = 1;

// gate_add / gate_mul (composer.rs:423-439): q_o = -1, c = q_m a b + q_l a + q_r b + q_f d + q_c, one arithmetic gate
template <class B>
HD uint32_t cg_eval(B& b, const Fr& qm, const Fr& ql, const Fr& qr, const Fr& qc, uint32_t a, uint32_t bb) {
  Fr v = Fr::zero();
  if constexpr (B::EXEC) {
    const Fr av = b.get(a), bv = b.get(bb);
    v = qm * av * bv + ql * av + qr * bv + qc;
  }
  const uint32_t c = b.alloc(v);
  b.emit(crow_arith(qm, ql, qr, Fr::one().neg(), Fr::zero(), qc, a, bb, c, CW_ZERO));
  return c;
}
template <class B> HD uint32_t cg_mul(B& b, uint32_t a, uint32_t bb) { return cg_eval(b, Fr::one(), Fr::zero(), Fr::zero(), Fr::zero(), a, bb); }
// assert_equal (composer.rs:392-397)
template <class B> HD void cg_assert_equal(B& b, uint32_t a, uint32_t bb) {
  b.emit(crow_arith(Fr::zero(), Fr::one(), Fr::one().neg(), Fr::zero(), Fr::zero(), Fr::zero(), a, bb, CW_ZERO, CW_ZERO));
}
// assert_equal_constant (composer.rs:402-417): -a + constant + PI = 0
template <class B> HD void cg_assert_equal_constant(B& b, uint32_t a, const Fr& constant, bool pub) {
  ComposerRow r = crow_arith(Fr::zero(), Fr::one().neg(), Fr::zero(), Fr::zero(), Fr::zero(), constant, a, CW_ZERO, CW_ZERO, CW_ZERO);
  r.pi = pub;
  b.emit(r);
}
// component_boolean (bits.rs:43-54): a a - a = 0
template <class B> HD void cg_boolean(B& b, uint32_t a) {
  b.emit(crow_arith(Fr::one(), Fr::zero(), Fr::zero(), Fr::one().neg(), Fr::zero(), Fr::zero(), a, a, a, CW_ZERO));
}

// ---- selection (select.rs) ---------------------------------------------------------------------------------------------
// component_select (select.rs:24-50): bit a, 1 - bit, (1 - bit) b, their sum; the last output is the result
template <class B> HD uint32_t cg_select(B& b, uint32_t bit, uint32_t a, uint32_t bb) {
  const Fr one = Fr::one(), zero = Fr::zero();
  const uint32_t bit_a = cg_mul(b, bit, a);
  const uint32_t one_min = cg_eval(b, zero, one.neg(), zero, one, bit, CW_ZERO);
  const uint32_t omb_b = cg_mul(b, one_min, bb);
  return cg_eval(b, zero, one, one, zero, omb_b, bit_a);
}
// component_select_one (select.rs:59-82): 1 - bit + bit value
template <class B> HD uint32_t cg_select_one(B& b, uint32_t bit, uint32_t value) {
  const Fr one = Fr::one();
  Fr v = Fr::zero();
  if constexpr (B::EXEC) {
    const Fr bv = b.get(bit);
    v = one - bv + bv * b.get(value);
  }
  const uint32_t f = b.alloc(v);
  b.emit(crow_arith(one, one.neg(), Fr::zero(), one.neg(), Fr::zero(), one, bit, value, f, CW_ZERO));
  return f;
}

// ---- range (range.rs) --------------------------------------------------------------------------------------------------
// range_check_even (range.rs:122-203): the base-4 accumulators of the low num_bits bits, most significant quad first, four
// to a q_range gate on wires d, c, b, a; a closing selector-free gate carrying the last accumulator on d; assert_equal.
// Allocates num_bits / 2 witnesses.
template <class B> HD void cg_range_even(B& b, uint32_t w, uint32_t num_bits) {
  if (num_bits == 0) {
    b.emit(crow_arith(Fr::zero(), Fr::one(), Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero(), w, CW_ZERO, CW_ZERO, CW_ZERO));
    return;
  }
  const uint32_t num_gates = (num_bits + 7) >> 3, num_quads = num_gates * 4;
  const uint32_t pad = 1 + (((num_quads << 1) - num_bits) >> 1), cnt = num_bits >> 1;
  const uint32_t base = b.mark();
  if constexpr (B::EXEC) {
    U256 t = u256_shl(u256_of(b.get(w)), 256 - num_bits);
    const Fr one = Fr::one(), two = one + one;
    Fr acc = Fr::zero();
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint32_t quad = t.l[7] >> 30;
      acc = acc.dbl().dbl();
      if (quad & 1) acc = acc + one;
      if (quad & 2) acc = acc + two;
      b.alloc(acc);
      t = u256_shl(t, 2);
    }
  } else {
    for (uint32_t i = 0; i < cnt; ++i) b.alloc(Fr::zero());
    // accumulator of step i (pad <= i <= num_quads) sits on wire [d, c, b, a][i % 4] of gate i / 4
    auto at = [&](uint32_t i) { return i >= pad && i <= num_quads ? base + (i - pad) : CW_ZERO; };
    for (uint32_t g = 0; g < num_gates; ++g) {
      ComposerRow r = crow(at(4 * g + 3), at(4 * g + 2), at(4 * g + 1), at(4 * g));
      r.q[CQ_RANGE] = Fr::one();
      b.emit(r);
    }
    b.emit(crow(CW_ZERO, CW_ZERO, CW_ZERO, base + cnt - 1));
  }
  cg_assert_equal(b, base + cnt - 1, w);
}
// range_check (range.rs:88-116): an odd width peels the top bit off as a boolean
template <class B> HD void cg_range(B& b, uint32_t w, uint32_t num_bits) {
  const bool odd = (num_bits & 1) != 0;
  const uint32_t top = num_bits - 1;
  uint32_t target = w, lower = CW_ZERO;
  Fr tb = Fr::zero();
  if (odd) {
    Fr lo = Fr::zero();
    if constexpr (B::EXEC) {
      const U256 v = u256_of(b.get(w));
      lo = u256_fr(u256_low(v, top));
      tb = u256_fr(u256_bits(v, top, top + 1));
    }
    target = lower = b.alloc(lo);
  }
  cg_range_even(b, target, odd ? top : num_bits);   // the one call site: both parities share the code
  if (odd) {
    const uint32_t top_bit = b.alloc(tb);
    cg_boolean(b, top_bit);
    const uint32_t rec = cg_eval(b, Fr::zero(), Fr::one(), fr_pow2(top), Fr::zero(), lower, top_bit);
    cg_assert_equal(b, rec, w);
  }
}
HD uint32_t cg_range_outputs(uint32_t num_bits) { return (num_bits & 1) ? (num_bits - 1) / 2 + 3 : num_bits / 2; }

// ---- bits (bits.rs) ----------------------------------------------------------------------------------------------------
// component_decomposition<N> (bits.rs:66-98): per bit i the bit (boolean) and the running sum 2^i bit + acc; bit i is output
// 2 i, the closing assert_equal ties the last sum to the scalar.  2 N witnesses, 2 N + 1 gates.
template <class B> HD void cg_decomposition(B& b, uint32_t scalar, uint32_t n) {
  U256 t = u256_zero();
  if constexpr (B::EXEC) t = u256_of(b.get(scalar));
  Fr pow = Fr::one(), accv = Fr::zero();
  uint32_t acc = CW_ZERO;
  for (uint32_t i = 0; i < n; ++i) {
    Fr bv = Fr::zero();
    if constexpr (B::EXEC) {
      if (t.l[0] & 1) { bv = Fr::one(); accv = accv + pow; }
      t = u256_shr(t, 1);
    }
    const uint32_t bit = b.alloc(bv);
    cg_boolean(b, bit);
    const uint32_t sum = b.alloc(accv);
    b.emit(crow_arith(Fr::zero(), pow, Fr::one(), Fr::one().neg(), Fr::zero(), Fr::zero(), bit, acc, sum, CW_ZERO));
    acc = sum;
    pow = pow.dbl();
  }
  cg_assert_equal(b, acc, scalar);
}

// ---- truncation (truncate.rs) --------------------------------------------------------------------------------------------
// assert_canonical_truncation (truncate.rs:121-182): (high, low) <= (r_high, r_low) lexicographically, r - 1 split at num_bits
template <class B> HD void cg_canonical_truncation(B& b, uint32_t high, uint32_t low, uint32_t num_bits) {
  const uint32_t high_bits = 255 - num_bits;
  const Fr one = Fr::one(), zero = Fr::zero();
  constexpr uint32_t qm1[8] = FR_MODULUS_MINUS_ONE_LIMBS;
  U256 m;
#pragma unroll
  for (int i = 0; i < 8; ++i) m.l[i] = qm1[i];
  const Fr r_low = u256_fr(u256_low(m, num_bits)), r_high = u256_fr(u256_bits(m, num_bits, 256));
  const uint32_t diff = cg_eval(b, zero, one.neg(), zero, r_high, high, CW_ZERO);
  cg_range(b, diff, high_bits);
  Fr iv = zero;
  if constexpr (B::EXEC) iv = cg_inv(b.get(diff));   // 0 -> 0
  const uint32_t inverse = b.alloc(iv);
  const uint32_t product = cg_mul(b, diff, inverse);
  const uint32_t is_top = cg_eval(b, zero, one.neg(), zero, one, product, CW_ZERO);
  b.emit(crow_arith(one, zero, zero, zero, zero, zero, diff, is_top, CW_ZERO, CW_ZERO));
  const uint32_t rlml = cg_eval(b, zero, one.neg(), zero, r_low, low, CW_ZERO);
  const uint32_t guard = cg_mul(b, is_top, rlml);
  cg_range(b, guard, num_bits);
}
// bind_truncation_split (truncate.rs:27-56): input = high 2^num_bits + low with high range-checked and the split canonical
template <class B> HD void cg_truncation_split(B& b, uint32_t input, uint32_t low, uint32_t num_bits) {
  Fr hv = Fr::zero();
  if constexpr (B::EXEC) hv = u256_fr(u256_bits(u256_of(b.get(input)), num_bits, 256));
  const uint32_t high = b.alloc(hv);
  cg_range(b, high, 255 - num_bits);
  const uint32_t rec = cg_eval(b, Fr::zero(), fr_pow2(num_bits), Fr::one(), Fr::zero(), high, low);
  cg_assert_equal(b, rec, input);
  cg_canonical_truncation(b, high, low, num_bits);
}
// component_truncate<N> (truncate.rs:86-109), N <= 254: the low part and its range check, then the split; the first output
// is the result.  make_low = false is bind_truncation_split on a low part the caller supplies — one statement, and one copy
// of the split's code in the executor kernel, for both records (CK_TRUNCATE / CK_SPLIT).
template <class B> HD uint32_t cg_truncate(B& b, uint32_t w, uint32_t n, bool make_low = true, uint32_t low = CW_ZERO) {
  if (make_low) {
    Fr lv = Fr::zero();
    if constexpr (B::EXEC) lv = u256_fr(u256_low(u256_of(b.get(w)), n));
    low = b.alloc(lv);
    cg_range(b, low, n);
  }
  cg_truncation_split(b, w, low, n);
  return low;
}

// ---- logic (logic.rs) --------------------------------------------------------------------------------------------------
// append_logic_component<BIT_PAIRS> (logic.rs:42-173): per quad, most significant first, the accumulators of a, b, the quad
// product and the accumulator of the result; gate i carries the PREVIOUS accumulators on a, b, d and product i on c; a
// closing selector-free gate carries the last ones; then both inputs are bound (logic.rs:181-212).  The result is witness
// out0 + 4 (BIT_PAIRS - 1) + 3, or the constant zero for no bit pairs.
template <class B> HD uint32_t cg_logic(B& b, uint32_t wa, uint32_t wb, uint32_t pairs, bool is_xor) {
  const Fr one = Fr::one(), two = one + one;
  U256 ta = u256_zero(), tb = u256_zero();
  if constexpr (B::EXEC) {
    if (pairs) {
      ta = u256_shl(u256_of(b.get(wa)), 256 - 2 * pairs);
      tb = u256_shl(u256_of(b.get(wb)), 256 - 2 * pairs);
    }
  }
  Fr la = Fr::zero(), ra = Fr::zero(), oa = Fr::zero();
  uint32_t pa = CW_ZERO, pb = CW_ZERO, pd = CW_ZERO;
  const Fr sel = is_xor ? one.neg() : one;
  for (uint32_t i = 0; i < pairs; ++i) {
    Fr prod = Fr::zero();
    if constexpr (B::EXEC) {
      const uint32_t lq = ta.l[7] >> 30, rq = tb.l[7] >> 30, oq = is_xor ? lq ^ rq : lq & rq;
      la = la.dbl().dbl(); ra = ra.dbl().dbl(); oa = oa.dbl().dbl();
      if (lq & 1) la = la + one;
      if (lq & 2) la = la + two;
      if (rq & 1) ra = ra + one;
      if (rq & 2) ra = ra + two;
      if (oq & 1) oa = oa + one;
      if (oq & 2) oa = oa + two;
      prod = Fr::from_u64((uint64_t)lq * rq);
      ta = u256_shl(ta, 2);
      tb = u256_shl(tb, 2);
    }
    const uint32_t xa = b.alloc(la), xb = b.alloc(ra), xc = b.alloc(prod), xd = b.alloc(oa);
    ComposerRow r = crow(pa, pb, xc, pd);
    r.q[CQ_C] = sel;
    r.q[CQ_LOGIC] = sel;
    b.emit(r);
    pa = xa; pb = xb; pd = xd;
  }
  b.emit(crow(pa, pb, CW_ZERO, pd));
  if (pairs) {
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
    for (int side = 0; side < 2; ++side) cg_truncation_split(b, side ? wb : wa, side ? pb : pa, 2 * pairs);
  }
  return pd;
}

// ---- points (point.rs) ---------------------------------------------------------------------------------------------------
// add_point_gates (point.rs:357-405): witnesses x1 y2, x3, y3; a q_variable_group_add gate on (x1, y1, x2, y2) and the row
// after it carrying (x3, y3, -, x1 y2).  A sum without an affine image falls back to the identity (point.rs:379-383).
template <class B> HD void cg_add_point_rows(B& b, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2, uint32_t base) {
  ComposerRow r = crow(x1, y1, x2, y2);
  r.q[CQ_VAR] = Fr::one();
  b.emit(r);
  b.emit(crow(base + 1, base + 2, CW_ZERO, base));
}
template <class B> HD void cg_add_point(B& b, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2) {
  Fr v0 = Fr::zero(), v1 = Fr::zero(), v2 = Fr::zero();
  if constexpr (B::EXEC) {
    const Fr X1 = b.get(x1), Y1 = b.get(y1), X2 = b.get(x2), Y2 = b.get(y2), one = Fr::one();
    const Fr x1y2 = X1 * Y2, y1x2 = Y1 * X2, t = jj_d() * x1y2 * y1x2, dx = one + t, dy = one - t;
    const Fr inv = cg_inv(dx * dy);
    v0 = x1y2;
    if (inv.is_zero()) { v1 = Fr::zero(); v2 = one; }
    else { v1 = (x1y2 + y1x2) * dy * inv; v2 = (Y1 * Y2 + X1 * X2) * dx * inv; }
  }
  const uint32_t base = b.alloc(v0);
  b.alloc(v1);
  b.alloc(v2);
  cg_add_point_rows(b, x1, y1, x2, y2, base);
}

// assert_torsion_free_point (point.rs:239-296): Q = [8^-1] P (the identity for an off-curve P), Q on the curve, P = [8] Q by
// three constrained doublings.  14 witnesses: Q (2), u^2, v^2, u^2 v^2, then (x1 y2, x3, y3) per doubling.  The lane works
// in projective coordinates and inverts once, for the four Z of Q, 2Q, 4Q, 8Q together.
template <class B> HD void cg_torsion_free(B& b, uint32_t px, uint32_t py) {
  const uint32_t base = b.mark();
  if constexpr (B::EXEC) {
    const Fr x = b.get(px), y = b.get(py);
    constexpr uint32_t e8[8] = JJ_EIGHT_INV_LIMBS;
    U256 k;
#pragma unroll
    for (int i = 0; i < 8; ++i) k.l[i] = e8[i];
    JJ q1 = jj_on_curve(x, y) ? jj_mul(x, y, k) : jj_identity();
    JJ q2 = jj_add(q1, q1), q4 = jj_add(q2, q2), q8 = jj_add(q4, q4);
    const Fr p2 = q1.Z * q2.Z, p3 = p2 * q4.Z, p4 = p3 * q8.Z;
    Fr inv = cg_inv(p4);
    const Fr i8 = inv * p3;
    inv = inv * q8.Z;
    const Fr i4 = inv * p2;
    inv = inv * q4.Z;
    const Fr i2 = inv * q1.Z, i1 = inv * q2.Z;
    const Fr u = q1.X * i1, v = q1.Y * i1, u2 = u * u, v2 = v * v;
    const Fr x2 = q2.X * i2, y2 = q2.Y * i2, x4 = q4.X * i4, y4 = q4.Y * i4;
    b.alloc(u); b.alloc(v); b.alloc(u2); b.alloc(v2); b.alloc(u2 * v2);
    b.alloc(u * v); b.alloc(x2); b.alloc(y2);
    b.alloc(x2 * y2); b.alloc(x4); b.alloc(y4);
    b.alloc(x4 * y4); b.alloc(q8.X * i8); b.alloc(q8.Y * i8);
  } else {
    const Fr one = Fr::one();
    const uint32_t qu = b.alloc(one), qv = b.alloc(one);
    const uint32_t u2 = cg_mul(b, qu, qu), v2 = cg_mul(b, qv, qv), u2v2 = cg_mul(b, u2, v2);
    b.emit(crow_arith(Fr::zero(), one.neg(), one, jj_d().neg(), Fr::zero(), one.neg(), u2, v2, u2v2, CW_ZERO));
    uint32_t x = qu, y = qv;
    for (int k = 0; k < 3; ++k) {
      const uint32_t s = b.alloc(one);
      b.alloc(one); b.alloc(one);
      cg_add_point_rows(b, x, y, x, y, s);
      x = s + 1; y = s + 2;
    }
    cg_assert_equal(b, px, x);
    cg_assert_equal(b, py, y);
  }
  (void)base;
}

// component_mul_point (point.rs:454-475): decomposition<252> of the scalar, then per bit from the top: double the running
// point, select P or the identity (select_zero / select_one without the boolean gate), add.  504 + 252 * 8 witnesses; per
// bit the slots are  dbl: x1 y2, x3, y3;  select: x, y;  add: x1 y2, x3, y3.
// Values: pass 1 walks the chain in projective coordinates and parks X, Y in the x3 / y3 slots, Z in the x1 y2 slot and the
// running product of the Z in the select slot that follows (dbl) / precedes (add); ONE inversion; pass 2 walks back turning
// the parked coordinates into affine ones; pass 3 fills the products and selections from the affine values.
static constexpr uint32_t MUL_POINT_BITS = 252;
template <class B> HD void cg_mul_point(B& b, uint32_t scalar, uint32_t px, uint32_t py) {
  const uint32_t bits0 = b.mark();
  cg_decomposition(b, scalar, MUL_POINT_BITS);
  const uint32_t s0 = b.mark();
  if constexpr (B::EXEC) {
    const Fr X = b.get(px), Y = b.get(py), one = Fr::one();
    JJ r = jj_identity();
    Fr run = one;
    for (uint32_t k = 0; k < MUL_POINT_BITS; ++k) {
      const uint32_t s = s0 + 8 * k;
      r = jj_add(r, r);
      b.put(s + 1, r.X); b.put(s + 2, r.Y); b.put(s, r.Z);
      run = run * r.Z;
      b.put(s + 4, run);
      if (!b.get(bits0 + 2 * (MUL_POINT_BITS - 1 - k)).is_zero()) r = jj_add_affine(r, X, Y);
      b.put(s + 6, r.X); b.put(s + 7, r.Y); b.put(s + 5, r.Z);
      run = run * r.Z;
      b.put(s + 3, run);
    }
    Fr inv = cg_inv(run);
    for (uint32_t k = MUL_POINT_BITS; k-- > 0;) {
      const uint32_t s = s0 + 8 * k;
      Fr zi = inv * b.get(s + 4);
      inv = inv * b.get(s + 5);
      b.put(s + 6, b.get(s + 6) * zi); b.put(s + 7, b.get(s + 7) * zi);
      zi = k ? inv * b.get(s - 8 + 3) : inv;
      inv = inv * b.get(s);
      b.put(s + 1, b.get(s + 1) * zi); b.put(s + 2, b.get(s + 2) * zi);
    }
    Fr rx = Fr::zero(), ry = one;
    for (uint32_t k = 0; k < MUL_POINT_BITS; ++k) {
      const uint32_t s = s0 + 8 * k;
      b.put(s, rx * ry);
      rx = b.get(s + 1);
      const Fr bit = b.get(bits0 + 2 * (MUL_POINT_BITS - 1 - k));
      const Fr sy = one - bit + bit * Y;
      b.put(s + 3, bit * X); b.put(s + 4, sy);
      b.put(s + 5, rx * sy);
      rx = b.get(s + 6); ry = b.get(s + 7);
    }
    b.skip(8 * MUL_POINT_BITS);
  } else {
    const Fr one = Fr::one();
    uint32_t rx = CW_ZERO, ry = CW_ONE;   // Composer::IDENTITY
    for (uint32_t k = 0; k < MUL_POINT_BITS; ++k) {
      const uint32_t bit = bits0 + 2 * (MUL_POINT_BITS - 1 - k);
      uint32_t s = b.alloc(one);
      b.alloc(one); b.alloc(one);
      cg_add_point_rows(b, rx, ry, rx, ry, s);
      rx = s + 1; ry = s + 2;
      const uint32_t sx = cg_mul(b, bit, px), sy = cg_select_one(b, bit, py);
      s = b.alloc(one);
      b.alloc(one); b.alloc(one);
      cg_add_point_rows(b, rx, ry, sx, sy, s);
      rx = s + 1; ry = s + 2;
    }
  }
}
HD uint32_t cg_mul_point_result(uint32_t out0) { return out0 + 2 * MUL_POINT_BITS + 8 * (MUL_POINT_BITS - 1) + 6; }   // x; y follows

// ---- fixed base (fixed_base.rs) ------------------------------------------------------------------------------------------
// assert_canonical_jubjub_scalar (fixed_base.rs:317-328): scalar < 2^252 and (r - 1) - scalar < 2^252
static constexpr uint32_t JJ_SCALAR_BITS = 252, FIXED_ROUNDS = 256, FIXED_LEADING_ZERO = 3;
HD Fr jj_order_minus_one() {   // BlsScalar::from(-JubJubScalar::one()), Montgomery limbs
  constexpr uint32_t v[8] = {0x00ded6e7u, 0xc65dbb50u, 0xc2254e45u, 0x10d8a660u, 0xbd1de2f1u, 0x45cfd3d0u, 0x0977974eu, 0x731b5c58u};
  return fr_limbs(v);
}
template <class B> HD void cg_canonical_jubjub_scalar(B& b, uint32_t scalar) {
  uint32_t w = scalar;
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
  for (int pass = 0; pass < 2; ++pass) {
    cg_range(b, w, JJ_SCALAR_BITS);
    if (pass == 0) w = cg_eval(b, Fr::zero(), Fr::one().neg(), Fr::zero(), jj_order_minus_one(), scalar, CW_ZERO);
  }
}
// component_mul_generator (fixed_base.rs:114-307).  tab(2 i), tab(2 i + 1): x and y of [2^(255 - i)] G, the multiple round i
// adds (the recorder computes the 256 multiples once per generator and keeps them in the constant pool).
// Signed digits: the width-2 NAF, d = 2 - (k mod 4) for odd k, else 0, k = (k - d) / 2; 256 of them, consumed from the top.
// Witnesses: the two range checks and the distance (253), then per round acc_x, acc_y, accumulated_bit, xy_alpha, then the
// closing acc_x, acc_y, accumulated_bit.  Values: as cg_mul_point — pass 1 parks X, Y in the acc_x / acc_y slots of row
// i + 1, Z in its accumulated_bit slot and the running product in the xy_alpha slot of row i; one inversion; pass 2 back;
// pass 3 fills the scalar accumulators and xy_alpha.
// Returns false when the scalar is not below the subgroup order (Error::JubJubScalarMalformed, fixed_base.rs:132-136).
template <class B, class Tab> HD bool cg_mul_generator(B& b, uint32_t scalar, const Tab& tab) {
  cg_canonical_jubjub_scalar(b, scalar);
  const uint32_t r0 = b.mark();
  const Fr one = Fr::one(), zero = Fr::zero();
  if constexpr (B::EXEC) {
    U256 k = u256_of(b.get(scalar));
    constexpr uint32_t order[8] = JJ_ORDER_LIMBS;
    if (u256_geq(k, order)) return false;
    U256 nz = u256_zero(), ng = u256_zero();   // bit j: digit j is non-zero / negative
    for (uint32_t j = 0; j < FIXED_ROUNDS; ++j) {
      nz = u256_shr(nz, 1);
      ng = u256_shr(ng, 1);
      if (k.l[0] & 1) {
        nz.l[7] |= 0x80000000u;
        if (k.l[0] & 2) {   // k mod 4 == 3: digit -1, k + 1
          ng.l[7] |= 0x80000000u;
          uint32_t c = 1;
#pragma unroll
          for (int i = 0; i < 8; ++i) { const uint32_t s = k.l[i] + c; c = s < c ? 1u : 0u; k.l[i] = s; }
        } else {
          k.l[0] &= ~1u;
        }
      }
      k = u256_shr(k, 1);
    }
    JJ acc = jj_identity();
    Fr run = one;
    U256 tz = nz, tg = ng;
    b.put(r0, zero); b.put(r0 + 1, one);
    for (uint32_t i = 0; i < FIXED_ROUNDS; ++i) {
      if (tz.l[7] >> 31) {
        const Fr xb = tab(2 * i);
        acc = jj_add_affine(acc, (tg.l[7] >> 31) ? xb.neg() : xb, tab(2 * i + 1));
      }
      tz = u256_shl(tz, 1); tg = u256_shl(tg, 1);
      const uint32_t s = r0 + 4 * (i + 1);
      b.put(s, acc.X); b.put(s + 1, acc.Y); b.put(s + 2, acc.Z);
      run = run * acc.Z;
      b.put(s - 4 + 3, run);
    }
    Fr inv = cg_inv(run);
    for (uint32_t i = FIXED_ROUNDS; i >= 1; --i) {
      const uint32_t s = r0 + 4 * i;
      const Fr zi = i >= 2 ? inv * b.get(s - 8 + 3) : inv;
      inv = inv * b.get(s + 2);
      b.put(s, b.get(s) * zi); b.put(s + 1, b.get(s + 1) * zi);
    }
    Fr sacc = zero;
    tz = nz; tg = ng;
    for (uint32_t i = 0; i < FIXED_ROUNDS; ++i) {
      const uint32_t s = r0 + 4 * i;
      b.put(s + 2, sacc);
      Fr xy = zero;
      sacc = sacc.dbl();
      if (tz.l[7] >> 31) {
        xy = tab(2 * i) * tab(2 * i + 1);
        if (tg.l[7] >> 31) { xy = xy.neg(); sacc = sacc - one; } else { sacc = sacc + one; }
      }
      b.put(s + 3, xy);
      tz = u256_shl(tz, 1); tg = u256_shl(tg, 1);
    }
    b.put(r0 + 4 * FIXED_ROUNDS + 2, sacc);
    b.skip(4 * FIXED_ROUNDS + 3);
  } else {
    uint32_t leading = CW_ZERO;
    for (uint32_t i = 0; i < FIXED_ROUNDS; ++i) {
      const uint32_t ax = b.alloc(one), ay = b.alloc(one), ab = b.alloc(one);
      if (i == FIXED_LEADING_ZERO) leading = ab;
      if (i == 0) {
        cg_assert_equal_constant(b, ax, zero, false);
        cg_assert_equal_constant(b, ay, one, false);
        cg_assert_equal_constant(b, ab, zero, false);
      }
      const uint32_t xy = b.alloc(one);
      const Fr xb = tab(2 * i), yb = tab(2 * i + 1);
      ComposerRow r = crow(ax, ay, xy, ab);
      r.q[CQ_L] = xb; r.q[CQ_R] = yb; r.q[CQ_C] = xb * yb;
      r.q[CQ_FIXED] = one;
      b.emit(r);
    }
    const uint32_t ax = b.alloc(one), ay = b.alloc(one), last = b.alloc(one);
    b.emit(crow_arith(zero, zero, zero, zero, zero, zero, ax, ay, CW_ZERO, last));   // the shifted-wire anchor (fixed_base.rs:286-288)
    cg_assert_equal_constant(b, leading, zero, false);
    cg_assert_equal(b, last, scalar);
  }
  return true;
}
static constexpr uint32_t MUL_GEN_OUTPUTS = 2 * (JJ_SCALAR_BITS / 2) + 1 + 4 * FIXED_ROUNDS + 3;
HD uint32_t cg_mul_generator_result(uint32_t out0) { return out0 + 2 * (JJ_SCALAR_BITS / 2) + 1 + 4 * FIXED_ROUNDS; }   // x; y follows

// ---- one record -----------------------------------------------------------------------------------------------------------
// Runs the gadget of record op on backend b (the recorder calls the cg_* functions directly while it records; executors
// come through here).  b.next is op.out0 on entry; pool(i): constant i of the program.  Returns false for a malformed
// JubJub scalar (the only error a fill can report).
template <class B, class Pool> HD bool composer_exec(B& b, const ComposerOp& op, const Pool& pool) {
  switch (op.kind) {
    case CK_CONST:
      b.alloc(pool(op.cst));
      break;
    case CK_GATE: {
      const Fr a = b.get(op.in[0]), bb = b.get(op.in[1]), d = b.get(op.in[2]);
      b.alloc((pool(op.cst) * a * bb + pool(op.cst + 1) * a + pool(op.cst + 2) * bb + pool(op.cst + 3) * d + pool(op.cst + 4)) * pool(op.cst + 5));
      break;
    }
    case CK_SELECT: cg_select(b, op.in[0], op.in[1], op.in[2]); break;
    case CK_SELECT_ONE: cg_select_one(b, op.in[0], op.in[1]); break;
    case CK_DECOMP: cg_decomposition(b, op.in[0], op.width); break;
    case CK_RANGE: cg_range(b, op.in[0], op.width); break;
    case CK_TRUNCATE:
    case CK_SPLIT: cg_truncate(b, op.in[0], op.width, op.kind == CK_TRUNCATE, op.in[1]); break;
    case CK_CANONICAL: cg_canonical_truncation(b, op.in[0], op.in[1], op.width); break;
    case CK_JJ_SCALAR: cg_canonical_jubjub_scalar(b, op.in[0]); break;
    case CK_LOGIC_AND:
    case CK_LOGIC_XOR: cg_logic(b, op.in[0], op.in[1], op.width, op.kind == CK_LOGIC_XOR); break;
    case CK_ADD_POINT: cg_add_point(b, op.in[0], op.in[1], op.in[2], op.in[3]); break;
    case CK_TORSION: cg_torsion_free(b, op.in[0], op.in[1]); break;
    case CK_MUL_GEN: {
      const uint32_t cst = op.cst;
      return cg_mul_generator(b, op.in[0], [&](uint32_t i) { return pool(cst + i); });
    }
    case CK_MUL_POINT: cg_mul_point(b, op.in[0], op.in[1], op.in[2]); break;
    default: break;
  }
  return true;
}
// the public-input value of a flagged row: whatever satisfies the row under the filled witnesses
template <class B, class Pool> HD Fr composer_pi_value(const B& b, const ComposerPiRow& r, const Pool& pool) {
  const Fr a = b.get(r.w[0]), bb = b.get(r.w[1]), c = b.get(r.w[2]), d = b.get(r.w[3]);
  return (pool(r.cst) * a * bb + pool(r.cst + 1) * a + pool(r.cst + 2) * bb + pool(r.cst + 3) * c + pool(r.cst + 4) * d + pool(r.cst + 5)).neg();
}

}  // namespace plonk
