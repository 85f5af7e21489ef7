// The schedule of one proof (prover.hip): the choices prover_prove and prover_prove_sharded make for a (size, prover state,
// configuration), in one place — both call prove_schedule once, before their first launch, and read nothing but the
// result afterwards.  Every threshold stands beside the measurement that set it.  No HIP here:
// tests/csrc/host_prove_schedule.cpp compiles this header with g++ and tests/test_prove_schedule_host.py compares it with
// the model tests/prove_schedule_model.py over every combination of its inputs.
#pragma once
#include <stdint.h>

namespace plonk {

struct ProveScheduleIn {
  uint32_t logn;
  bool lag_on;          // wire commitments over the Lagrange-basis key (Prover::lag_on)
  bool lag_z;           // ... whose table holds z's third blinding point (Prover::lag_z)
  bool wires_pending;   // host wire columns still arriving on the copy stream (plonk_prover_prove)
  uint32_t world;
  bool sharded;
  uint64_t n;           // 2^logn
  uint64_t rank_pts;    // sharded: coefficients this rank owns (hi - lo)
  // the switches, as Config holds them
  int wire_by_column;   // PLONK_WIRE_BY_COLUMN: -1 never, 0 by size, 1 / 2 at every size
  int wire_polys_side;  // PLONK_WIRE_POLYS_SIDE: -1 by size, 0, 1
  int side_defer;       // PLONK_SIDE_DEFER: -1 by size, 0, 1, 2 = round 1 only
  int z_commit_coeff;   // PLONK_Z_COMMIT: -1 evals at every size, 0 by size, 1 coeff
  int shard_side;       // plonk_gpu_config.shard_side_stream / PLONK_SHARD_SIDE: -1 off
  int shard_z;          // plonk_gpu_config.shard_grand_product / PLONK_SHARD_Z: -1 off, 0 by size, 1 on
};

struct ProveSchedule {
  bool by_column;        // round 1: the wire group is launched in parts, as the host columns arrive
  uint32_t wire_parts;   // ... in that many: 3 = a, b, c + d; 4 = one per column; 1 = one grouped launch; 0 = sharded (Prover::last_wire_launches keeps its value)
  bool polys_on_side;    // the wire inverse transforms + blinding run on the side stream, not in front of the wire commitments
  bool side_defer_r1;    // round 1 (a, b, c, d + PI): side work starts after the group's accumulation, not with the group
  bool side_defer_r2;    // round 2 (z): the same
  bool z_from_evals;     // round 2: z is committed from its evaluations over the Lagrange-basis key
  bool shard_z;          // sharded, round 2: the grand product is split over the ranks
};

static inline ProveSchedule prove_schedule(const ProveScheduleIn& in) {
  const uint32_t L = in.logn;
  ProveSchedule s{};
  if (!in.sharded) {
    // Host wire columns (plonk_prover_prove, round 6): column k lands over PCIe 32 n bytes after column k - 1 (0.65 ms apart at
    // 2^20 gates), and until round 5 the commitment group waited for all four before its grouped bucket sort — 2.1 ms of every
    // such proof with nothing but the four inverse transforms to hide in.  Now each column's transform is followed at once by
    // ITS bucket sort, accumulation and bucket sums (msm_batch_device phase 1 on column k: the throughput-bound 90 % of a
    // commitment), under the next columns' copies; the latency-bound reduction tail still runs once for the group (phase 2).
    // Same additions, same bucket sums, same bytes.  Resident columns (plonk_prover_prove_dev, what `value` times) keep the
    // grouped launch: four launches have four ramp-downs.
    // plonk_gpu_config has no field for it; PLONK_WIRE_BY_COLUMN: 0 = never, 1 / 2 = at EVERY size (a, b, c + d / one launch per
    // column: what the variant tests use to run the phased launches on small circuits), unset = from 2^19 gates on
    s.by_column = in.lag_on && in.wires_pending && in.world == 1 && in.wire_by_column >= 0 && (L > 18 || in.wire_by_column > 0);
    // Columns a and b each get a launch of their own as they land; c and d — both have arrived by the time b's accumulation
    // ends (0.65 ms per column over PCIe against ~1.5 ms of commitment work per column at 2^20 gates) — share one: a sort
    // launch set and an accumulation ramp-down less.  Measured and NOT adopted (profiles/r06/host_wires_ab.jsonl): column k's
    // work on a stream of its own (k & 1), gated only by its copy — no gain at 2^20 (gap 1.09-1.27 against 1.12 ms) and a
    // loss at 2^19 (0.38-0.54 against 0.24): the accumulations are VALU-bound, so overlapping them only interleaves them.
    // PLONK_WIRE_BY_COLUMN=2: one launch per column (A/B)
    s.wire_parts = s.by_column ? (in.wire_by_column == 2 ? 4 : 3) : 1;
    // Up to 2^19 gates the wire polynomials (needed from round 3 on) ride on the side stream under the commitment pipeline,
    // started after the group's accumulation (side_defer below): they fill its latency-bound reduction tail.  At 2^20 the
    // accumulation owns the VALU and its register file (two waves of 256 VGPRs per SIMD: no transform wave fits beside
    // them), the tails of the four groups are too short for the 6 ms of side transforms, and the inverse transforms keep
    // their place in front of the commitment (same-box A/B, profiles/r06b/polys_side_*.jsonl: 2^19 18.1-18.3 -> 17.4-17.7 ms
    // with both moved, 2^20 32.17 -> 32.07-32.44).  PLONK_WIRE_POLYS_SIDE=0/1 forces it.
    s.polys_on_side = in.lag_on && !s.by_column && (in.wire_polys_side >= 0 ? in.wire_polys_side == 1 : L <= 19);
    // Side transforms either start with the group (they then compete with its bandwidth-bound sort) or wait for the end of
    // its accumulation and fill the latency-bound tail.  Same-box A/B (r02e): waiting wins up to 2^18 gates (2^16: 5.19 vs
    // 5.33 ms) and on the widget workload (38.1 vs 38.5 ms) but loses on the dense 2^20 headline (37.2-37.4 vs 36.6-36.8 ms:
    // z's transform no longer fits between its commitment and the quotient), so it follows the size; round 6: 2^19 gates
    // wait too, together with the wire inverse transforms (above).  PLONK_SIDE_DEFER=0/1 forces it.
    const bool defer_size = L <= 18 || (L == 19 && !s.by_column);   // (host wire columns at 2^19 gates keep the phased launches' order)
    s.side_defer_r1 = in.side_defer >= 0 ? in.side_defer >= 1 : defer_size;
    s.side_defer_r2 = in.side_defer >= 0 ? in.side_defer == 1 : defer_size;   // ("2" = round 1 only)
    // z committed from its evaluations (round 6, second session; prover_prove, round 2, says what moves where): up to 2^17 gates
    // only: same-box A/B 2^12 2.04 -> 2.01 ms, 2^16 4.09 -> 4.03, 2^17 5.88 -> 5.86 (even in a later
    // five-repetition pair); at 2^18 the coefficient form is 1 % ahead (9.88 against 10.00 ms, mid_sizes_ab.jsonl), at 2^19 too, and
    // at 2^20 the transform that left the main stream competes with the commitment's sort on the side stream instead (32.2 against
    // 32.3), so larger circuits keep the coefficient form (profiles/r06b/zcommit_ab.jsonl).
    s.z_from_evals = in.lag_on && in.lag_z && (L <= 17 || in.z_commit_coeff < 0);
    return s;
  }
  // Round 4 (r04): the schedule of the single-GPU path for a RANK.  With the Lagrange-basis slice the wire commitments read
  // the wire VALUES, so the replicated wire polynomials (needed from round 3 on) ride on the side stream under the
  // commitment pipeline — a rank's MSM over 1/W of the points leaves most of the chip idle in its latency-bound sort and
  // reduction tail (W = 8 at 2^20: 1.4 of the rank's 7.7 ms were these transforms in front of the commitment).  The side
  // work starts after the group's accumulation (side_defer) while the rank's share is small; PLONK_SHARD_SIDE=0 restores
  // the round-3 order.
  const bool on = in.shard_side >= 0;   // plonk_gpu_config.shard_side_stream = -1 / PLONK_SHARD_SIDE=0 restores the round-3 order
  const bool small = in.rank_pts <= (1ull << 18) + 64;   // (2^19 points per rank: 19.2 -> 19.4 ms, the accumulation owns the VALU)
  s.polys_on_side = in.lag_on && on && small;
  s.side_defer_r1 = s.side_defer_r2 = on && small;
  // Round 4: the grand product (permutation.rs:213-294) split over the ranks from 2^19 gates and four ranks on.
  // PLONK_SHARD_Z=0 / 1 forces either (the multi-rank tests run small circuits through both).
  // rank alone, loop-back collectives (profiles/r04): W = 8 at 2^20 gates 7.41 -> 7.01 ms, at 2^22 21.9 -> 20.1; W = 2 at 2^20
  // 19.05 -> 19.27 (half of 0.5 ms of work against two more host round trips): from four ranks on
  const bool wanted = in.shard_z > 0 ? true : in.shard_z < 0 ? false : (L >= 19 && in.world >= 4);
  s.shard_z = wanted && in.n % in.world == 0 && in.n / in.world >= 2;
  return s;   // by_column, z_from_evals: single GPU only; wire_parts = 0
}

}  // namespace plonk
