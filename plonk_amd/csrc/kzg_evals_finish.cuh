// The chain of hostg1.hpp finish_bit_sums over the reduced-radix group law (curve28.cuh), for one commitment: what
// kze_finish_kernel (kzg_evals.hip) runs per lane before g1r_compress48_words (g1codec.cuh).  HD like the rest of the
// arithmetic: tests/csrc/host_kzg_evals_tables.cpp compiles it with g++ against the big-int model.
//
// Slots of a commitment (msm_bits_kernel): rows T_0 .. T_(rb-1) at [0, rb), columns T'_0 .. T'_6 at [rb, rb + 7), C_128 at
// rb + 7, S at rb + 8; rb = 8 (2^15 buckets) or 12 (2^19).  W = Horner over U_0 .. U_(6+rb) with U_j = T'_j (j < 7),
// U_7 = C_128 + T_0, U_(7+j) = T_j; bit-position rows: 2 W - S.  Every step is the complete law: identity slots, an
// accumulator equal or opposite to its addend occur (G1R::add doubles or cancels).  `ld(slot)` returns the slot as a G1R with
// canonical coordinates; the chain keeps ONE accumulator and ONE addend live, the addend read where it is used: no array of
// points, nothing indexed in registers.
#pragma once
#include "curve28.cuh"

namespace plonk {

HD G1R g1r_of_g1(const G1& q) {
  if (q.is_identity()) return G1R::identity();
  G1R r;
  r.X = Fp28::from_fp(q.X);
  r.Y = Fp28::from_fp(q.Y);
  r.ZZ = Fp28::from_fp(q.ZZ);
  r.ZZZ = Fp28::from_fp(q.ZZZ);
  return r;
}

template <class Load>
HD G1R kze_finish_chain(const Load& ld, int rb, bool bitpos) {
  G1R acc = ld(rb - 1);   // U_(6+rb) = T_(rb-1)
  for (int j = 5 + rb; j >= 0; --j) {
    G1R u = ld(j > 7 ? j - 7 : (j == 7 ? rb + 7 : rb + j));
    if (j == 7) u = u.add(ld(0));
    acc = acc.dbl().add(u);
  }
  if (bitpos) {
    G1R s = ld(rb + 8);
    if (!s.is_identity()) s.Y = Fp28::sub<16>(Fp28::zero(), s.Y).canon();   // -S: Y < p in
    acc = acc.dbl().add(s);
  }
  return acc;
}

}  // namespace plonk
