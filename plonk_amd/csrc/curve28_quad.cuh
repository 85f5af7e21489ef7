// The quad-cooperative point addition of the MSM's reduction tail (msm.hip), in a header of its own so that a test kernel
// can call it (tests/csrc/dev_msm_tail.hip).  Device only.  No namespace of its own: include it INSIDE namespace plonk (msm.hip
// does so inside its per-bucket-count namespace), after curve28.cuh.
#pragma once

// ---- quad-cooperative tail (round 3) -----------------------------------------------------------
// The row/column and bit-sum kernels are chains of DEPENDENT full additions (12 products + 2 squarings,
// ~7.6 k instructions each) on a chip that is mostly idle while they run.  The 14 products of an
// addition form four levels of mutually independent products:
//     U1 U2 S1 S2 | P^2 R^2 ZZ1*ZZ2 ZZZ1*ZZZ2 | P*PP U1*PP ZZ12*PP ZZZ12*P | R*(Q-X3) PPP*(-S1) T*PP
// so the four lanes of a quad hold the SAME two points, each lane computes ONE product per level, and the
// results are exchanged with DPP quad broadcasts (one v_mov_dpp per limb): 4 products + ~0.6 k
// instructions of selects / exchanges instead of 14 products per addition — the latency of an addition drops
// ~2.8x, at 1.6x the issue slots, which these kernels have to spare.  A "logical lane" is a quad; control flow is
// uniform inside a quad by construction (replicated operands), which the DPP reads rely on.
template <int K>
__device__ __forceinline__ Fp28 quad_get(const Fp28& v) {   // lane K of the quad -> all four lanes
  Fp28 r;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i)
    r.l[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.l[i], K * 0x55, 0xf, 0xf, true);
  return r;
}
__device__ __forceinline__ Fp28 quad_sel(uint32_t q, const Fp28& a0, const Fp28& a1, const Fp28& a2, const Fp28& a3) {
  // bit masks, not ?: — the compiler turns a four-way conditional over arrays into a pointer select with the
  // operands parked in scratch memory, which is the last thing a latency-bound chain needs.  Two levels of (m & x) | (~m & y),
  // which is ONE v_bfi_b32 each: 3 instructions per limb (round 6, second session; until then four ANDs and two ORs per
  // limb — 672 of the ~3.3 k instructions of a quad addition were these selects).
  const bool b0 = (q & 1u) != 0, b1 = (q & 2u) != 0;
  Fp28 r;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) {
    const uint32_t lo = b0 ? a1.l[i] : a0.l[i], hi = b0 ? a3.l[i] : a2.l[i];   // per-limb selects on two lane masks: v_cndmask_b32
    r.l[i] = b1 ? hi : lo;
  }
  return r;
}
// a + b, both replicated over the quad; q = lane & 3.  Same bounds as G1R::add (Y3 < 4p here: two reductions
// instead of the fused one, inside the Y < 8p contract).
__device__ __forceinline__ G1R g1r_add_quad(const G1R& a, const G1R& b, uint32_t q) {
  if (a.is_identity()) return b;
  if (b.is_identity()) return a;
  const Fp28 m1 = Fp28::mul(quad_sel(q, a.X, b.X, a.Y, b.Y), quad_sel(q, b.ZZ, a.ZZ, b.ZZZ, a.ZZZ));
  const Fp28 U1 = quad_get<0>(m1), U2 = quad_get<1>(m1), S1 = quad_get<2>(m1), S2 = quad_get<3>(m1);   // < 2p
  const Fp28 P_ = Fp28::sub_lazy<4>(U2, U1);                // < 6p, lazy limbs
  const Fp28 R_ = Fp28::sub<4>(S2, S1);                     // < 6p, normalised
  if (G1R::maybe_zero(P_) && P_.normalized().is_zero_mod()) {
    // equal or opposite points (never for independent bucket sums; small or repeated bases reach it): every lane of the
    // quad doubles on its own.  Inlined — an out-of-line call would pin both points in scratch memory on the hot path.
    return R_.is_zero_mod() ? a.dbl() : G1R::identity();
  }
  const Fp28 m2 = Fp28::mul(quad_sel(q, P_, R_, a.ZZ, a.ZZZ), quad_sel(q, P_, R_, b.ZZ, b.ZZZ));   // 6*6, 2*2 -> < 2p
  const Fp28 PP = quad_get<0>(m2), RR = quad_get<1>(m2), ZZ12 = quad_get<2>(m2), ZZZ12 = quad_get<3>(m2);
  const Fp28 m3 = Fp28::mul(quad_sel(q, P_, U1, ZZ12, ZZZ12), quad_sel(q, PP, PP, PP, P_));           // 6*2, 2*2 -> < 2p
  const Fp28 PPP = quad_get<0>(m3), Q_ = quad_get<1>(m3), T_ = quad_get<3>(m3);
  G1R r;
  r.ZZ = quad_get<2>(m3);
  r.X = Fp28::sub<8>(Fp28::sub_lazy<4>(RR, PPP), Fp28::add_lazy(Q_, Q_));                             // < 14p
  const Fp28 m4 = Fp28::mul(quad_sel(q, R_, PPP, T_, T_),                                              // 6*34, 2*4, 2*2 -> < 2p
                            quad_sel(q, Fp28::sub_lazy<32>(Q_, r.X), Fp28::neg_lazy<4>(S1), PP, PP));
  r.Y = Fp28::add(quad_get<0>(m4), quad_get<1>(m4));                                                   // < 4p
  r.ZZZ = quad_get<2>(m4);
  return r;
}
