// The gadget composer, host part (no HIP): the recorder behind plonk_composer_* and the one-thread host executor of the
// witness program.  Included by composer.hip and by the CPU test harness tests/csrc/host_composer.cpp.
//
// A Composer records gadget calls.  It yields
//   (a) the layout plonk_compile takes: 11 selector columns, 4 wire-index columns, the witness count, the public-input rows;
//   (b) a witness program: ComposerOp records (composer_core.hpp) in allocation order + an Fr constant pool.  A record's
//       outputs are the contiguous witness slots its gadget allocated; records without outputs (assertions) are not kept.
// Every record gets a level — one more than the highest level among the producers of its inputs; input witnesses and
// constants are level 0 — and schedule() sorts the records by (level, kind): a level only reads slots that lower levels
// wrote, and the lanes of a level's launch are grouped by kind.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/plonk_hip.h"
#include "composer_core.hpp"

namespace plonk {

struct ComposerSchedule {
  std::vector<ComposerOp> ops;          // sorted by (level, kind), allocation order within
  std::vector<uint32_t> level_off;      // records of level l: [level_off[l], level_off[l + 1])
  uint32_t widest = 0;
};

class Composer {
 public:
  std::vector<Fr> sel[11];
  std::vector<uint32_t> wires[4];
  std::vector<uint32_t> wlevel;         // per witness: level of the record that produces it (0: input / constant)
  std::vector<uint32_t> inputs;         // witness slot of input i, in allocation order
  std::vector<ComposerPiRow> pi_rows;
  std::vector<ComposerOp> ops;          // allocation order
  std::vector<Fr> pool;
  struct GenTable { Fr x, y; uint32_t cst; };
  std::vector<GenTable> gens;           // the multiples of a generator are kept once per generator

  // ---- recorder backend of composer_core.hpp
  static constexpr bool EXEC = false;
  uint32_t alloc(const Fr&) { wlevel.push_back(cur_level); return (uint32_t)wlevel.size() - 1; }
  uint32_t mark() const { return (uint32_t)wlevel.size(); }
  void emit(const ComposerRow& r) {
    const uint32_t row = (uint32_t)wires[0].size();
    for (int k = 0; k < 11; ++k) sel[k].push_back(r.q[k]);
    for (int w = 0; w < 4; ++w) wires[w].push_back(r.w[w]);
    if (r.pi) {
      ComposerPiRow p;
      p.row = row;
      for (int w = 0; w < 4; ++w) p.w[w] = r.w[w];
      p.cst = (uint32_t)pool.size();
      for (int k = 0; k < 6; ++k) pool.push_back(r.q[k]);
      pi_rows.push_back(p);
    }
  }

  Composer() {   // Composer::initialized (composer.rs:177-240)
    const Fr one = Fr::one();
    const uint32_t zero_w = constant_witness(Fr::zero()), one_w = constant_witness(one);
    cg_assert_equal_constant(*this, zero_w, Fr::zero(), false);
    cg_assert_equal_constant(*this, one_w, one, false);
    const uint32_t six = constant_witness(Fr::from_u64(6)), one2 = constant_witness(one), seven = constant_witness(Fr::from_u64(7)),
                   m20 = constant_witness(Fr::from_u64(20).neg());
    emit(crow_arith(one, Fr::from_u64(2), Fr::from_u64(3), Fr::from_u64(4), one, Fr::from_u64(4), six, seven, m20, one2));
    emit(crow_arith(one, one, one, one, Fr::zero(), Fr::from_u64(127), m20, six, seven, CW_ZERO));
  }

  uint64_t constraints() const { return wires[0].size(); }
  uint64_t witnesses() const { return wlevel.size(); }
  bool known(uint32_t w) const { return w < wlevel.size(); }

  uint32_t input() {   // append_witness: a value the caller supplies per proof
    cur_level = 0;
    const uint32_t w = alloc(Fr::zero());
    inputs.push_back(w);
    return w;
  }
  // a witness whose value is a constant of the circuit, WITHOUT the gate that pins it (append_constant adds that)
  uint32_t constant_witness(const Fr& v) {
    const uint32_t in[4] = {0, 0, 0, 0};
    const uint32_t cst = (uint32_t)pool.size();
    pool.push_back(v);
    const uint32_t out0 = mark();
    record(CK_CONST, 0, in, 0, cst, [&] { alloc(v); });
    return out0;
  }
  // one record: body() runs the gadget on this recorder; returns the first output slot
  template <class F> uint32_t record(uint32_t kind, uint32_t width, const uint32_t* in, int nin, uint32_t cst, F&& body) {
    ComposerOp op{};
    op.kind = kind;
    op.width = width;
    uint32_t lvl = 0;
    for (int i = 0; i < nin; ++i) {
      op.in[i] = in[i];
      lvl = std::max(lvl, wlevel[in[i]]);
    }
    op.level = kind == CK_CONST ? 0 : lvl + 1;
    op.cst = cst;
    op.out0 = mark();
    op.id = (uint32_t)ops.size();
    cur_level = op.level;
    body();
    cur_level = 0;
    op.nout = mark() - op.out0;
    if (op.nout) {
      ops.push_back(op);
      sched_valid = false;
    }
    return op.out0;
  }

  const ComposerSchedule& schedule() const {
    if (!sched_valid) {
      sched.ops = ops;
      std::stable_sort(sched.ops.begin(), sched.ops.end(), [](const ComposerOp& a, const ComposerOp& b) {
        return a.level != b.level ? a.level < b.level : a.kind < b.kind;
      });
      uint32_t levels = 0;
      for (const ComposerOp& o : sched.ops) levels = std::max(levels, o.level + 1);
      sched.level_off.assign(levels + 1, 0);
      for (const ComposerOp& o : sched.ops) ++sched.level_off[o.level + 1];
      sched.widest = 0;
      for (uint32_t l = 0; l < levels; ++l) {
        sched.widest = std::max(sched.widest, sched.level_off[l + 1]);
        sched.level_off[l + 1] += sched.level_off[l];
      }
      sched_valid = true;
    }
    return sched;
  }

  // the 256 multiples of a generator, [2^(255 - i)] G at pool[cst + 2 i], pool[cst + 2 i + 1] (fixed_base.rs:170-183)
  uint32_t generator_table(const Fr& gx, const Fr& gy) {
    for (const GenTable& g : gens)
      if (g.x == gx && g.y == gy) return g.cst;
    const uint32_t cst = (uint32_t)pool.size();
    pool.resize(pool.size() + 2 * FIXED_ROUNDS);
    JJ p{gx, gy, Fr::one()};
    for (uint32_t i = 0; i < FIXED_ROUNDS; ++i) {
      const Fr zi = fr_inv_gcd(p.Z);
      pool[cst + 2 * (FIXED_ROUNDS - 1 - i)] = p.X * zi;
      pool[cst + 2 * (FIXED_ROUNDS - 1 - i) + 1] = p.Y * zi;
      p = jj_add(p, p);
    }
    gens.push_back(GenTable{gx, gy, cst});
    return cst;
  }

 private:
  uint32_t cur_level = 0;
  mutable ComposerSchedule sched;
  mutable bool sched_valid = false;
};

// ---- constant points, validated as the reference validates them -----------------------------------------------------------
inline bool jj_torsion_free(const Fr& x, const Fr& y) {   // on the curve and [r] P = identity
  if (!jj_on_curve(x, y)) return false;
  constexpr uint32_t order[8] = JJ_ORDER_LIMBS;
  U256 k;
  for (int i = 0; i < 8; ++i) k.l[i] = order[i];
  const JJ p = jj_mul(x, y, k);
  return p.X.is_zero() && p.Y == p.Z;
}
inline bool jj_prime_order(const Fr& x, const Fr& y) { return jj_torsion_free(x, y) && !(x.is_zero() && y == Fr::one()); }

inline Fr fr_of_words(const uint64_t* v) {
  Fr r;
  memcpy(r.l, v, 32);
  return r;
}

// ---- the recording calls behind the C ABI (composer.hip wraps them with the error text; the test harness calls them as
// they are).  *why: a static text for PLONK_ERR_ARG / PLONK_ERR_POINT -------------------------------------------------------
inline int composer_api_gate(Composer& c, const uint64_t* selectors, const uint32_t wires[4], uint32_t flags, uint32_t* out,
                             const char** why) {
  Fr q[6];
  for (int k = 0; k < 6; ++k) q[k] = fr_of_words(selectors + 4 * k);
  const bool solve = (flags & 2u) && !q[CQ_O].is_zero();   // with q_o = 0 nothing can be solved for: the caller's c wire stays (composer.rs:352-356)
  for (int w = 0; w < 4; ++w)
    if (!c.known(wires[w]) && !(solve && w == 2)) return (*why = "wire names a witness that was not allocated", PLONK_ERR_ARG);
  uint32_t cw = wires[2];
  if (out) *out = 0xFFFFFFFFu;
  if (solve) {   // append_evaluated_output (composer.rs:307-359): solve the row for c
    const uint32_t in[4] = {wires[0], wires[1], wires[3], 0};
    const uint32_t cst = (uint32_t)c.pool.size();
    c.pool.push_back(q[CQ_M]); c.pool.push_back(q[CQ_L]); c.pool.push_back(q[CQ_R]); c.pool.push_back(q[CQ_F]); c.pool.push_back(q[CQ_C]);
    c.pool.push_back(q[CQ_O] == Fr::one().neg() ? Fr::one() : fr_inv_gcd(q[CQ_O]).neg());
    cw = c.record(CK_GATE, 0, in, 3, cst, [&] { c.alloc(Fr::zero()); });
    if (out) *out = cw;
  }
  ComposerRow r = crow_arith(q[CQ_M], q[CQ_L], q[CQ_R], q[CQ_O], q[CQ_F], q[CQ_C], wires[0], wires[1], cw, wires[3]);
  r.pi = (flags & 1u) != 0;
  c.emit(r);
  return PLONK_OK;
}

inline int composer_api_gadget(Composer& c, int kind, uint32_t width, const uint32_t* in, uint32_t nin, const uint64_t* consts,
                               uint32_t nconsts, uint32_t* out, uint32_t out_cap, uint32_t* nout, const char** why) {
  auto need = [&](uint32_t ni, uint32_t nc, uint32_t no) -> bool {
    if (nin != ni || nconsts != nc || (ni && !in) || (nc && !consts)) { *why = "wrong number of inputs or constants for this gadget"; return false; }
    for (uint32_t i = 0; i < ni; ++i)
      if (!c.known(in[i])) { *why = "input names a witness that was not allocated"; return false; }
    if (no > out_cap || (no && !out)) { *why = "out_cap is below the gadget's output count"; return false; }
    if (nout) *nout = no;
    return true;
  };
  auto bad_width = [&]() { *why = "width outside the gadget's range"; return PLONK_ERR_ARG; };
  const Fr zero = Fr::zero(), one = Fr::one();
  uint32_t i4[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < nin && i < 4; ++i) i4[i] = in[i];
  switch (kind) {
    case PLONK_G_CONSTANT: {   // append_constant (composer.rs:363-373)
      if (!need(0, 1, 1)) return PLONK_ERR_ARG;
      const Fr v = fr_of_words(consts);
      out[0] = c.constant_witness(v);
      cg_assert_equal_constant(c, out[0], v, false);
      return PLONK_OK;
    }
    case PLONK_G_PUBLIC: {   // append_public (composer.rs:378-389): an input and a public row -a + PI = 0
      if (!need(0, 0, 1)) return PLONK_ERR_ARG;
      out[0] = c.input();
      cg_assert_equal_constant(c, out[0], zero, true);
      return PLONK_OK;
    }
    case PLONK_G_ASSERT_EQUAL:
      if (!need(2, 0, 0)) return PLONK_ERR_ARG;
      cg_assert_equal(c, in[0], in[1]);
      return PLONK_OK;
    case PLONK_G_ASSERT_EQUAL_CONSTANT:   // width bit 0: the row is public as well (assert_equal_constant's `public`)
      if (!need(1, 1, 0)) return PLONK_ERR_ARG;
      cg_assert_equal_constant(c, in[0], fr_of_words(consts), (width & 1u) != 0);
      return PLONK_OK;
    case PLONK_G_BOOLEAN:
      if (!need(1, 0, 0)) return PLONK_ERR_ARG;
      cg_boolean(c, in[0]);
      return PLONK_OK;
    case PLONK_G_SELECT:
      if (!need(3, 0, 1)) return PLONK_ERR_ARG;
      out[0] = c.record(CK_SELECT, 0, i4, 3, 0, [&] { cg_select(c, in[0], in[1], in[2]); }) + 3;
      return PLONK_OK;
    case PLONK_G_SELECT_ONE:
      if (!need(2, 0, 1)) return PLONK_ERR_ARG;
      out[0] = c.record(CK_SELECT_ONE, 0, i4, 2, 0, [&] { cg_select_one(c, in[0], in[1]); });
      return PLONK_OK;
    case PLONK_G_SELECT_ZERO: {   // component_select_zero (select.rs:91-99): gate_mul
      if (!need(2, 0, 1)) return PLONK_ERR_ARG;
      Fr s[6] = {one, zero, zero, one.neg(), zero, zero};
      uint64_t qs[24];
      memcpy(qs, s, sizeof qs);
      const uint32_t w[4] = {in[0], in[1], 0, 0};
      return composer_api_gate(c, qs, w, 2u, &out[0], why);
    }
    case PLONK_G_DECOMPOSITION: {
      if (width < 1 || width > 256) return bad_width();
      if (!need(1, 0, width)) return PLONK_ERR_ARG;
      const uint32_t o = c.record(CK_DECOMP, width, i4, 1, 0, [&] { cg_decomposition(c, in[0], width); });
      for (uint32_t i = 0; i < width; ++i) out[i] = o + 2 * i;
      return PLONK_OK;
    }
    case PLONK_G_RANGE_BITS:
    case PLONK_G_RANGE: {   // component_range<BIT_PAIRS> = the even check on min(2 BIT_PAIRS, 256) bits (range.rs:68-77)
      const uint32_t bits = kind == PLONK_G_RANGE ? (width > 128 ? 256 : 2 * width) : width;
      if (bits > 256) return bad_width();
      if (!need(1, 0, 0)) return PLONK_ERR_ARG;
      c.record(CK_RANGE, bits, i4, 1, 0, [&] { cg_range(c, in[0], bits); });
      return PLONK_OK;
    }
    case PLONK_G_TRUNCATE:
      if (width > 254) return bad_width();
      if (!need(1, 0, 1)) return PLONK_ERR_ARG;
      out[0] = c.record(CK_TRUNCATE, width, i4, 1, 0, [&] { cg_truncate(c, in[0], width); });
      return PLONK_OK;
    case PLONK_G_BIND_TRUNCATION_SPLIT:
      if (width > 254) return bad_width();
      if (!need(2, 0, 0)) return PLONK_ERR_ARG;
      c.record(CK_SPLIT, width, i4, 2, 0, [&] { cg_truncate(c, in[0], width, false, in[1]); });
      return PLONK_OK;
    case PLONK_G_CANONICAL_TRUNCATION:
      if (width > 254) return bad_width();
      if (!need(2, 0, 0)) return PLONK_ERR_ARG;
      c.record(CK_CANONICAL, width, i4, 2, 0, [&] { cg_canonical_truncation(c, in[0], in[1], width); });
      return PLONK_OK;
    case PLONK_G_LOGIC_AND:
    case PLONK_G_LOGIC_XOR: {
      if (width > 127) return bad_width();
      if (!need(2, 0, 1)) return PLONK_ERR_ARG;
      const bool x = kind == PLONK_G_LOGIC_XOR;
      uint32_t res = CW_ZERO;
      c.record(x ? CK_LOGIC_XOR : CK_LOGIC_AND, width, i4, 2, 0, [&] { res = cg_logic(c, in[0], in[1], width, x); });
      out[0] = res;
      return PLONK_OK;
    }
    case PLONK_G_POINT:   // append_point (point.rs:60-82): two inputs
      if (!need(0, 0, 2)) return PLONK_ERR_ARG;
      out[0] = c.input();
      out[1] = c.input();
      return PLONK_OK;
    case PLONK_G_CONSTANT_POINT: {   // append_constant_point (point.rs:100-125)
      if (!need(0, 2, 2)) return PLONK_ERR_ARG;
      const Fr x = fr_of_words(consts), y = fr_of_words(consts + 4);
      if (!jj_torsion_free(x, y)) return (*why = "constant point is not an on-curve member of the prime-order subgroup (Error::JubJubPointNotTorsionFree)", PLONK_ERR_POINT);
      out[0] = c.constant_witness(x);
      cg_assert_equal_constant(c, out[0], x, false);
      out[1] = c.constant_witness(y);
      cg_assert_equal_constant(c, out[1], y, false);
      return PLONK_OK;
    }
    case PLONK_G_PUBLIC_POINT:   // append_public_point (point.rs:142-165)
      if (!need(0, 0, 2)) return PLONK_ERR_ARG;
      out[0] = c.input();
      out[1] = c.input();
      cg_assert_equal_constant(c, out[0], zero, true);
      cg_assert_equal_constant(c, out[1], zero, true);
      return PLONK_OK;
    case PLONK_G_ASSERT_EQUAL_POINT:
      if (!need(4, 0, 0)) return PLONK_ERR_ARG;
      cg_assert_equal(c, in[0], in[2]);
      cg_assert_equal(c, in[1], in[3]);
      return PLONK_OK;
    case PLONK_G_ASSERT_EQUAL_PUBLIC_POINT:
      if (!need(2, 0, 0)) return PLONK_ERR_ARG;
      cg_assert_equal_constant(c, in[0], zero, true);
      cg_assert_equal_constant(c, in[1], zero, true);
      return PLONK_OK;
    case PLONK_G_NEG_POINT:
    case PLONK_G_SUB_POINT:
    case PLONK_G_ADD_POINT: {
      const bool neg = kind != PLONK_G_ADD_POINT, add = kind != PLONK_G_NEG_POINT;
      if (!need(add ? 4 : 2, 0, 2)) return PLONK_ERR_ARG;
      uint32_t bx = in[add ? 2 : 0], by = in[add ? 3 : 1];
      if (neg) {   // component_neg_point (point.rs:302-315): gate_mul of left(-1) a(x)
        Fr s[6] = {zero, one.neg(), zero, one.neg(), zero, zero};
        uint64_t qs[24];
        memcpy(qs, s, sizeof qs);
        const uint32_t w[4] = {bx, 0, 0, 0};
        const int rc = composer_api_gate(c, qs, w, 2u, &bx, why);
        if (rc) return rc;
      }
      if (add) {
        const uint32_t p[4] = {in[0], in[1], bx, by};
        const uint32_t o = c.record(CK_ADD_POINT, 0, p, 4, 0, [&] { cg_add_point(c, p[0], p[1], p[2], p[3]); });
        out[0] = o + 1;
        out[1] = o + 2;
      } else {
        out[0] = bx;
        out[1] = by;
      }
      return PLONK_OK;
    }
    case PLONK_G_SELECT_IDENTITY: {   // component_select_identity (point.rs:418-444)
      if (!need(3, 0, 2)) return PLONK_ERR_ARG;
      cg_boolean(c, in[0]);
      Fr s[6] = {one, zero, zero, one.neg(), zero, zero};
      uint64_t qs[24];
      memcpy(qs, s, sizeof qs);
      const uint32_t w[4] = {in[0], in[1], 0, 0};
      const int rc = composer_api_gate(c, qs, w, 2u, &out[0], why);
      if (rc) return rc;
      const uint32_t p[4] = {in[0], in[2], 0, 0};
      out[1] = c.record(CK_SELECT_ONE, 0, p, 2, 0, [&] { cg_select_one(c, p[0], p[1]); });
      return PLONK_OK;
    }
    case PLONK_G_SELECT_POINT: {   // component_select_point (point.rs:490-500): two component_select
      if (!need(5, 0, 2)) return PLONK_ERR_ARG;
      const uint32_t px[4] = {in[0], in[1], in[3], 0}, py[4] = {in[0], in[2], in[4], 0};
      out[0] = c.record(CK_SELECT, 0, px, 3, 0, [&] { cg_select(c, px[0], px[1], px[2]); }) + 3;
      out[1] = c.record(CK_SELECT, 0, py, 3, 0, [&] { cg_select(c, py[0], py[1], py[2]); }) + 3;
      return PLONK_OK;
    }
    case PLONK_G_TORSION_FREE:
      if (!need(2, 0, 0)) return PLONK_ERR_ARG;
      c.record(CK_TORSION, 0, i4, 2, 0, [&] { cg_torsion_free(c, in[0], in[1]); });
      return PLONK_OK;
    case PLONK_G_CANONICAL_JUBJUB_SCALAR:
      if (!need(1, 0, 0)) return PLONK_ERR_ARG;
      c.record(CK_JJ_SCALAR, 0, i4, 1, 0, [&] { cg_canonical_jubjub_scalar(c, in[0]); });
      return PLONK_OK;
    case PLONK_G_MUL_GENERATOR: {
      if (!need(1, 2, 2)) return PLONK_ERR_ARG;
      const Fr x = fr_of_words(consts), y = fr_of_words(consts + 4);
      if (!jj_prime_order(x, y)) return (*why = "generator is not an on-curve point of exact prime order (Error::JubJubGeneratorNotPrimeOrder)", PLONK_ERR_POINT);
      const uint32_t cst = c.generator_table(x, y);
      const Fr* tab = c.pool.data() + cst;
      const uint32_t o = c.record(CK_MUL_GEN, 0, i4, 1, cst, [&] { cg_mul_generator(c, in[0], [&](uint32_t i) { return tab[i]; }); });
      out[0] = cg_mul_generator_result(o);
      out[1] = out[0] + 1;
      return PLONK_OK;
    }
    case PLONK_G_MUL_POINT: {
      if (!need(3, 0, 2)) return PLONK_ERR_ARG;
      const uint32_t o = c.record(CK_MUL_POINT, 0, i4, 3, 0, [&] { cg_mul_point(c, in[0], in[1], in[2]); });
      out[0] = cg_mul_point_result(o);
      out[1] = out[0] + 1;
      return PLONK_OK;
    }
    default:
      *why = "unknown gadget kind";
      return PLONK_ERR_ARG;
  }
}

inline void composer_api_info(const Composer& c, plonk_composer_summary* out) {
  const ComposerSchedule& s = c.schedule();
  out->constraints = c.constraints();
  out->witnesses = c.witnesses();
  out->inputs = c.inputs.size();
  out->public_rows = c.pi_rows.size();
  out->records = s.ops.size();
  out->levels = s.level_off.size() - 1;
  out->widest_level = s.widest;
}
inline void composer_api_layout(const Composer& c, uint64_t* const selectors[11], uint32_t* const wires[4], uint32_t* input_slots,
                                uint64_t* pi_rows) {
  const uint64_t n = c.constraints();
  if (selectors)
    for (int k = 0; k < 11; ++k)
      if (selectors[k] && n) memcpy(selectors[k], c.sel[k].data(), n * sizeof(Fr));
  if (wires)
    for (int w = 0; w < 4; ++w)
      if (wires[w] && n) memcpy(wires[w], c.wires[w].data(), n * sizeof(uint32_t));
  if (input_slots && !c.inputs.empty()) memcpy(input_slots, c.inputs.data(), c.inputs.size() * sizeof(uint32_t));
  if (pi_rows)
    for (size_t i = 0; i < c.pi_rows.size(); ++i) pi_rows[i] = c.pi_rows[i].row;
}

// ---- the one-thread host executor: the same composer_exec over the scheduled records -------------------------------------
struct HostExec {
  static constexpr bool EXEC = true;
  Fr* tab;
  uint32_t next;
  uint32_t lo, hi;    // the slots this record may write: its own outputs (every index is checked; a miss is counted, not done)
  uint64_t size;
  uint64_t* misses;
  bool readable(uint32_t i) const { return i < size || (++*misses, false); }
  bool writable(uint32_t i) const { return (i >= lo && i < hi) || (++*misses, false); }
  Fr get(uint32_t i) const { return readable(i) ? tab[i] : Fr::zero(); }
  void put(uint32_t i, const Fr& v) { if (writable(i)) tab[i] = v; }
  uint32_t alloc(const Fr& v) { put(next, v); return next++; }
  uint32_t mark() const { return next; }
  void skip(uint32_t n) { next += n; }
  void emit(const ComposerRow&) {}
};
// table: witnesses() values; pi_out: one value per public row (nullable); returns the lowest id of a record that reported a
// malformed JubJub scalar, COMPOSER_NO_ERROR when none did.  *misses (nullable): accesses outside the table or writes outside
// the running record's own output slots — the executor's indexing is the device lanes' indexing, so zero here is the bound
// check of the kernels
inline uint32_t composer_fill_host(const Composer& c, const Fr* inputs, Fr* table, Fr* pi_out, uint64_t* misses = nullptr) {
  uint64_t local = 0;
  if (!misses) misses = &local;
  for (size_t i = 0; i < c.inputs.size(); ++i) table[c.inputs[i]] = inputs[i];
  const Fr* pool = c.pool.data();
  auto pl = [pool](uint32_t i) { return pool[i]; };
  uint32_t err = COMPOSER_NO_ERROR;
  for (const ComposerOp& op : c.schedule().ops) {
    HostExec b{table, op.out0, op.out0, op.out0 + op.nout, c.witnesses(), misses};
    if (!composer_exec(b, op, pl)) err = std::min(err, op.id);
    else if (b.next != op.out0 + op.nout) ++*misses;
  }
  if (pi_out) {
    const HostExec b{table, 0, 0, 0, c.witnesses(), misses};
    for (size_t i = 0; i < c.pi_rows.size(); ++i) pi_out[i] = composer_pi_value(b, c.pi_rows[i], pl);
  }
  return err;
}

}  // namespace plonk
