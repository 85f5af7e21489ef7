// What the host and the device share of plonk_msm_points (msm_points.hip): the plan of a call — digit width, windows, slice
// length, which path — and the signed-digit recoding of a GLV half.  HD and HIP-free, so that the CPU test harness
// (tests/csrc/host_msm_points.cpp) runs exactly the code the kernels run and the GPU tests can compare the plan a call
// reports (plonk_ctx_last_msm_points) with the plan computed here.
//
// A scalar k < q is split by glv_split (curve28.cuh) into k = k1 + k2 LAMBDA with k1, k2 < 2^128.  Each half is written in
// signed digits of c bits, d_w in [-2^(c-1), 2^(c-1)]:  half = sum_w d_w 2^(c w).  Window w takes the c bits at position
// c w plus the carry of the window below; a value above 2^(c-1) becomes value - 2^c and carries one.  ceil(129 / c) windows
// always suffice: the top window holds at most c - 1 bits of the half (128 - c (W - 1) <= c - 1 because c W >= 129), so with
// a carry it reaches at most 2^(c-1) and never carries out.  |d_w| is the bucket, 1 .. 2^(c-1); zero digits have none.
#pragma once
#include <stdint.h>

#include "field.cuh"   // HD

namespace plonk {

constexpr uint32_t MP_C_MIN = 2, MP_C_MAX = 16;
constexpr uint32_t MP_HALF_BITS = 129;                 // 128 bits of a half + the bit a carry may reach
constexpr uint64_t MP_MAX_TERMS = 1ull << 24;          // term indices take 24 bits of an entry
constexpr uint32_t MP_SLICE_MIN = 4, MP_SLICE_MAX = 64;
// Below this many terms the call runs the per-term kernel of verify.hip: the crossover measured on an MI355X by
// tools/msm_points_bench.py.  64 is the SMALLEST size measured — the bucket path won there and at every
// larger size by more than the spread of the repetitions; nothing below 64 terms has been timed.
constexpr uint32_t MP_MIN_BUCKET_TERMS = 64;
// an entry of the sorted list: term index | half << 24 | negative << 25
constexpr uint32_t MP_ENTRY_TERM = 0x00ffffffu, MP_ENTRY_HALF = 1u << 24, MP_ENTRY_NEG = 1u << 25;

HD uint32_t mp_windows(uint32_t c) { return (MP_HALF_BITS + c - 1) / c; }
HD uint32_t mp_buckets(uint32_t c) { return 1u << (c - 1); }   // per window

// The digit width for m terms: the c that minimises  windows(c) * (2 m + 4 * 2^(c-1)).  Per window a term gives two entries
// (one per half, 1 - 2^-c of them non-zero) = two mixed additions, and a bucket costs about four general additions on its
// way to the window sum (two in the chunked running sums, the rest in the slice tree, the mul_u32 of a chunk and the trees).
// Ties go to the smaller c (fewer buckets to clear and scan).
HD uint32_t mp_choose_c(uint64_t m) {
  uint32_t best = MP_C_MIN;
  uint64_t best_cost = ~0ull;
  for (uint32_t c = MP_C_MIN; c <= MP_C_MAX; ++c) {
    const uint64_t cost = (uint64_t)mp_windows(c) * (2 * m + 4ull * mp_buckets(c));
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}
// The longest run of entries one lane accumulates serially: short enough that 2 m windows entries fill about 2^17 lanes
// (the device holds 2^16 lanes at one wave per SIMD), within [4, 64].
HD uint32_t mp_choose_slice(uint64_t m, uint32_t c) {
  const uint64_t s = (2 * m * mp_windows(c)) >> 17;
  return s < MP_SLICE_MIN ? MP_SLICE_MIN : s > MP_SLICE_MAX ? MP_SLICE_MAX : (uint32_t)s;
}

struct MpPlan {
  uint32_t path;            // 0 per-term kernel, 1 buckets
  uint32_t c, windows, slice_entries;
};
// force_c / force_slice / min_bucket_terms: plonk_msm_points_opts (0 = automatic)
HD MpPlan mp_plan(uint64_t m, uint32_t force_c, uint32_t force_slice, uint32_t min_bucket_terms) {
  MpPlan p;
  p.path = m >= (uint64_t)(min_bucket_terms ? min_bucket_terms : MP_MIN_BUCKET_TERMS) ? 1u : 0u;
  p.c = force_c ? force_c : mp_choose_c(m);
  p.windows = mp_windows(p.c);
  p.slice_entries = force_slice ? force_slice : mp_choose_slice(m, p.c);
  return p;
}

// Digit w of the half k (k[0] low word, k < 2^128); *carry is the carry into window w on entry and out of it on return.
// Call for w = 0, 1, ... in order, starting with *carry = 0.
HD int32_t mp_digit(const uint64_t k[2], uint32_t c, uint32_t w, uint32_t* carry) {
  const uint32_t bit = w * c;
  uint32_t raw = 0;
  if (bit < 128) {
    const uint32_t wi = bit >> 6, sh = bit & 63;
    uint64_t v = k[wi] >> sh;
    if (wi == 0 && sh) v |= k[1] << (64 - sh);
    raw = (uint32_t)v & ((1u << c) - 1u);
  }
  raw += *carry;
  if (raw > (1u << (c - 1))) {
    *carry = 1;
    return (int32_t)raw - (int32_t)(1u << c);
  }
  *carry = 0;
  return (int32_t)raw;
}

// f(half, window, bucket, negative) for every non-zero digit of both halves; bucket in [1, 2^(c-1)]
template <class F>
HD void mp_for_each_digit(const uint64_t k1[2], const uint64_t k2[2], uint32_t c, F&& f) {
  const uint32_t W = mp_windows(c);
  for (uint32_t h = 0; h < 2; ++h) {
    const uint64_t* k = h ? k2 : k1;
    if (!(k[0] | k[1])) continue;
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) {
      const int32_t d = mp_digit(k, c, w, &carry);
      if (d) f(h, w, (uint32_t)(d < 0 ? -d : d), d < 0);
    }
  }
}

HD uint32_t mp_count_digits(const uint64_t k1[2], const uint64_t k2[2], uint32_t c) {
  uint32_t n = 0;
  mp_for_each_digit(k1, k2, c, [&](uint32_t, uint32_t, uint32_t, bool) { ++n; });
  return n;
}

}  // namespace plonk
