// KZG10 commitments of many short vectors (kzg_many.hip): everything the host decides before a kernel runs — the window count
// W(c), the signed-digit recoding of a whole canonical scalar, the size and the indexing of the window tables, the automatic
// digit width and the plan a call reports.  HD and HIP-free like kzg_evals_core.hpp: the kernels and the handle call these
// functions, tests/csrc/host_kzg_many.cpp compiles them with g++ against the big-int model tests/kzg_many_model.py.
//
// A value s < q is written in signed digits of c bits, d_w in [-2^(c-1), 2^(c-1)]:  s = sum_(w < W) d_w 2^(c w)  — the
// convention of msm_points_core.hpp, here over the whole scalar.  Window w takes the c bits at position c w plus the carry of
// the window below; a value above 2^(c-1) becomes value - 2^c and carries one.  That carry chain is the carry chain of the
// addition s + H, H having the digit 2^(c-1) - 1 in every window below the top, so the top digit (s + H) >> c (W - 1) grows
// with s: W(c) is the smallest W for which q - 1 does not carry out of window W - 1, and then no scalar below q does.
//     c      2   3   4   5   6   7   8
//     W(c) 128  86  64  52  43  37  32          (c = 3, 5: 255 = c W exactly and the top bits of q exceed 2^(c-1): one more)
// The tables hold, for every Lagrange point L_i, window w < W and d in 1 .. 2^(c-1), the affine point [d 2^(c w)] L_i
// (G1AffineR, 128 bytes; 128 zero bytes when L_i is the identity) at entry (i W + w) 2^(c-1) + d - 1:
//     commitment = sum_i sum_w sign(d_(i,w)) T[i][w][|d_(i,w)|]        n W mixed additions at most, no doublings
#pragma once
#include <stdint.h>

#include "../../include/plonk_hip.h"
#include "field.cuh"

namespace plonk {

static constexpr uint32_t KZM_C_MIN = 2, KZM_C_MAX = 8;
static constexpr uint32_t KZM_LOG_N_MAX = 12;
static constexpr uint64_t KZM_MAX_COUNT = 1ull << 24;      // vectors of plonk_kzg_commit_many, segments of plonk_kzg_update_many
static constexpr uint64_t KZM_MAX_TERMS = 1ull << 28;      // offsets[count] of plonk_kzg_update_many
// terms of ONE segment at most: a segment is one wave's work (1024 terms per lane here, tens of milliseconds), and a shared
// device is not to be held by a single wave for minutes; 16 n for the largest domain
static constexpr uint64_t KZM_MAX_SEGMENT = 1ull << 16;
static constexpr uint64_t KZM_ENTRY_BYTES = 128;           // sizeof(G1AffineR)
static constexpr uint64_t KZM_SLOT_BYTES = 256;            // sizeof(G1RSlot): one partial sum
static constexpr uint32_t KZM_LANES = 64;                  // one wave per (vector, slice)
// Waves the device holds of kzm_accumulate_kernel: 256 CUs x 4 SIMDs x 2 (the kernel's registers allow two waves per SIMD,
// DESIGN.md section 22).  A call with fewer vectors than this cuts each vector into slices until it has that many waves.
static constexpr uint32_t KZM_RESIDENT_WAVES = 2048;
static constexpr uint64_t KZM_CHUNK_MAX = 1ull << 20;      // vectors per chunk at most (the grid)
static constexpr uint64_t KZM_TERM_BYTES = 36;             // a sparse term in the workspace: the delta (32) and its index (4)

// the bit pattern of q - 1 (FrP::MOD with the low bit cleared: q is odd)
HD void kzm_q_minus_1(uint32_t out[8]) {
  for (int k = 0; k < 8; ++k) out[k] = FrP::MOD[k];
  out[0] -= 1u;
}

// The next digit of the canonical scalar in s (8 x 32-bit limbs, s[0] low): takes the low c bits, shifts s right by c IN
// PLACE (every limb index is a constant: the kernel keeps s in registers) and applies the carry.  *carry is the carry into
// the window on entry and out of it on return.  Call W times, starting with *carry = 0.
HD int32_t kzm_next_digit(uint32_t s[8], uint32_t c, uint32_t* carry) {
  uint32_t raw = (s[0] & ((1u << c) - 1u)) + *carry;
#pragma unroll
  for (int k = 0; k < 7; ++k) s[k] = (s[k] >> c) | (s[k + 1] << (32 - c));
  s[7] >>= c;
  if (raw > (1u << (c - 1))) {
    *carry = 1;
    return (int32_t)raw - (int32_t)(1u << c);
  }
  *carry = 0;
  return (int32_t)raw;
}

// digits[w], w < windows; returns the carry out of the last window (0 for every s < q when windows >= kzm_windows(c))
HD uint32_t kzm_recode(const uint32_t s[8], uint32_t c, uint32_t windows, int32_t* digits) {
  uint32_t t[8], carry = 0;
  for (int k = 0; k < 8; ++k) t[k] = s[k];
  for (uint32_t w = 0; w < windows; ++w) digits[w] = kzm_next_digit(t, c, &carry);
  return carry;
}

// W(c): the smallest window count for which q - 1, and with it every scalar below q, does not carry out
HD uint32_t kzm_windows(uint32_t c) {
  uint32_t qm1[8];
  kzm_q_minus_1(qm1);
  for (uint32_t W = (255 + c - 1) / c;; ++W) {
    uint32_t t[8], carry = 0;
    for (int k = 0; k < 8; ++k) t[k] = qm1[k];
    for (uint32_t w = 0; w < W; ++w) (void)kzm_next_digit(t, c, &carry);
    if (!carry) return W;
  }
}

HD uint64_t kzm_table_entries(uint32_t log_n, uint32_t c) { return ((uint64_t)kzm_windows(c) << log_n) << (c - 1); }
HD uint64_t kzm_table_bytes(uint32_t log_n, uint32_t c) { return kzm_table_entries(log_n, c) * KZM_ENTRY_BYTES; }
// the entry of [d 2^(c w)] L_i, d in 1 .. 2^(c-1)
HD uint64_t kzm_entry(uint32_t c, uint32_t windows, uint64_t i, uint32_t w, uint32_t d) {
  return ((i * windows + w) << (c - 1)) + (d - 1);
}

// window_bits == 0: the widest c <= 8 whose tables fit `left` bytes of the context's table budget (0: none does).  The
// widest is also the fastest at every size measured: the additions fall as 1 / c.
HD uint32_t kzm_auto_width(uint32_t log_n, uint64_t left) {
  for (uint32_t c = KZM_C_MAX; c >= KZM_C_MIN; --c)
    if (kzm_table_bytes(log_n, c) <= left) return c;
  return 0;
}

// plonk_kzg_many_tables_build's argument check
HD int kzm_check_build(bool has_domain, uint32_t log_n, uint32_t window_bits) {
  if (!has_domain) return PLONK_ERR_ARG;
  if (log_n < 1 || log_n > KZM_LOG_N_MAX) return PLONK_ERR_ARG;
  if (window_bits && (window_bits < KZM_C_MIN || window_bits > KZM_C_MAX)) return PLONK_ERR_ARG;
  return PLONK_OK;
}

// ---- the plan of a call ---------------------------------------------------------------------------------------------------------
// One wave owns a (vector, slice): the n / slices values of the slice, each with its W digits.  A vector (or a forced slice)
// of fewer than 64 values spreads the windows of a value over 64 / values lanes, so a wave is full while values x W >= 64.
struct KzmPlan {
  uint32_t log_n, window_bits, windows;
  uint32_t slices;           // partial sums per vector (a power of two)
  uint64_t count;            // vectors (segments of the sparse form)
  uint64_t terms;            // values the call adds up: count x n (sparse: offsets[count])
  uint64_t chunk_vectors;    // vectors of a full chunk
  uint64_t chunks;
  uint64_t additions;        // the bound terms x W (zero digits are not counted on the device)
};

// slices: 1 once the call has a wave per resident wave slot; otherwise doubled until it has, but never below 64 values per
// slice: one value per lane.  Measured: at n = 2^8 four slices of 64 values are the fastest cut for
// every count up to 256 (0.61 .. 0.67 ms against 1.4 ms uncut), two for 1024; thinner slices, which spread the windows of a
// value over idle lanes, only add partial sums for the compression lane to chain (128 slices: 2.2 ms).
// force_slices (the door's test-only setter; a power of two) overrides the rule, up to one value per slice.
HD uint32_t kzm_slices(uint32_t log_n, uint64_t count, uint32_t force_slices) {
  const uint64_t n = 1ull << log_n;
  uint32_t s = 1;
  if (force_slices) {
    while ((uint64_t)s * 2 <= n && s * 2 <= force_slices) s *= 2;
    return s;
  }
  const uint64_t most = n / KZM_LANES;
  while (count * s < KZM_RESIDENT_WAVES && (uint64_t)s * 2 <= most) s *= 2;
  return s;
}

// bytes of workspace a vector of a chunk takes: its partial sums, its 48 output bytes and, in the host form, its values in
// both staging buffers
HD uint64_t kzm_vector_bytes(uint32_t log_n, uint32_t slices, bool host_form) {
  return KZM_SLOT_BYTES * slices + 48 + (host_form ? (64ull << log_n) : 0);
}

HD KzmPlan kzm_plan(uint32_t log_n, uint32_t c, uint64_t count, uint64_t ws_cap, bool host_form, uint32_t force_slices) {
  KzmPlan p;
  p.log_n = log_n;
  p.window_bits = c;
  p.windows = kzm_windows(c);
  p.slices = kzm_slices(log_n, count, force_slices);
  p.count = count;
  p.terms = count << log_n;
  uint64_t per = ws_cap / kzm_vector_bytes(log_n, p.slices, host_form);
  if (per < 1) per = 1;   // a chunk of one vector is always allowed
  if (per > KZM_CHUNK_MAX) per = KZM_CHUNK_MAX;
  if (per > count) per = count;
  p.chunk_vectors = per;
  p.chunks = count ? (count + per - 1) / per : 0;
  p.additions = p.terms * p.windows;
  return p;
}

// The sparse form (plonk_kzg_update_many): a wave per segment (slices = 1), chunks of consecutive segments cut greedily so
// that the terms and the partial sums of a chunk stay under the cap (a chunk of one segment is always allowed).  The decoded
// bases are resident for the whole call (148 bytes each) and are not part of the cut.
// The segments of the chunk that starts at `first`:
HD uint64_t kzm_sparse_chunk(const uint64_t* offsets, uint64_t count, uint64_t first, uint64_t ws_cap) {
  const uint64_t seg = KZM_SLOT_BYTES + 48;
  uint64_t bytes = 0, k = first;
  while (k < count && k - first < KZM_CHUNK_MAX) {
    const uint64_t add = seg + KZM_TERM_BYTES * (offsets[k + 1] - offsets[k]);
    if (k > first && bytes + add > ws_cap) break;
    bytes += add;
    ++k;
  }
  return k - first;
}
HD KzmPlan kzm_sparse_plan(uint32_t log_n, uint32_t c, const uint64_t* offsets, uint64_t count, uint64_t ws_cap) {
  KzmPlan p;
  p.log_n = log_n;
  p.window_bits = c;
  p.windows = kzm_windows(c);
  p.slices = 1;
  p.count = count;
  p.terms = count ? offsets[count] : 0;
  p.chunk_vectors = 0;
  p.chunks = 0;
  for (uint64_t first = 0; first < count;) {
    const uint64_t k = kzm_sparse_chunk(offsets, count, first, ws_cap);
    if (k > p.chunk_vectors) p.chunk_vectors = k;   // the largest chunk
    ++p.chunks;
    first += k;
  }
  p.additions = p.terms * p.windows;
  return p;
}

// plonk_kzg_commit_many's argument checks
HD int kzm_check_commit(bool has_domain, bool has_values, bool has_out, uint64_t count) {
  if (!has_domain) return PLONK_ERR_ARG;
  if (count > KZM_MAX_COUNT) return PLONK_ERR_ARG;
  if (count && (!has_values || !has_out)) return PLONK_ERR_ARG;
  return PLONK_OK;
}
// plonk_kzg_update_many's: the pointers, the caps (count, total, one segment), offsets that start at 0 and never decrease,
// every index below n
HD int kzm_check_update(bool has_domain, const uint64_t* offsets, const uint32_t* index, bool has_deltas, bool has_out, uint64_t count,
                        uint32_t log_n) {
  if (!has_domain) return PLONK_ERR_ARG;
  if (count > KZM_MAX_COUNT) return PLONK_ERR_ARG;
  if (!count) return PLONK_OK;
  if (!offsets || !has_out) return PLONK_ERR_ARG;
  if (offsets[0] != 0) return PLONK_ERR_ARG;
  for (uint64_t j = 0; j < count; ++j)
    if (offsets[j + 1] < offsets[j] || offsets[j + 1] - offsets[j] > KZM_MAX_SEGMENT) return PLONK_ERR_ARG;
  const uint64_t total = offsets[count];
  if (total > KZM_MAX_TERMS) return PLONK_ERR_ARG;
  if (total && (!index || !has_deltas)) return PLONK_ERR_ARG;
  for (uint64_t k = 0; k < total; ++k)
    if (index[k] >> log_n) return PLONK_ERR_ARG;
  return PLONK_OK;
}

}  // namespace plonk
