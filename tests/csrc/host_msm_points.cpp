// CPU test harness of plonk_msm_points: the shared header plonk_amd/csrc/msm_points_core.hpp (the plan of a call and the
// signed-digit recoding, exactly what the kernels of msm_points.hip run) and a plain host bucket pipeline over G1R that follows
// the device's stages — recode, group by (window, bucket), accumulate by slices with add_affine / add_affine_pair, slice sums
// to bucket sums, running sums per window, Horner over the windows.  Compiled with g++ and driven from
// tests/test_msm_points_host.py through ctypes; with -DHMP_MAIN it is a stand-alone program (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../plonk_amd/csrc/curve28.cuh"
#include "../../plonk_amd/csrc/g1codec.cuh"
#include "../../plonk_amd/csrc/msm_points_core.hpp"

using namespace plonk;

static void canonical_scalar(const uint8_t* mont32, uint32_t k[8]) {
  Fr s;
  memcpy(s.l, mont32, 32);
  const Fr c = s.from_mont();
  memcpy(k, c.l, 32);
}

extern "C" {

// out: path, c, windows, slice_entries
void hmp_plan(uint64_t m, uint32_t force_c, uint32_t force_slice, uint32_t min_bucket_terms, uint32_t out[4]) {
  const MpPlan p = mp_plan(m, force_c, force_slice, min_bucket_terms);
  out[0] = p.path; out[1] = p.c; out[2] = p.windows; out[3] = p.slice_entries;
}

// k: canonical scalar (8 words).  halves: k1 (2 x u64), k2 (2 x u64).  digits: windows of half 1, then windows of half 2.
// Returns the window count.
uint32_t hmp_recode(const uint32_t k[8], uint32_t c, uint64_t halves[4], int32_t* digits) {
  const GlvScalar g = glv_split(k);
  halves[0] = g.k1[0]; halves[1] = g.k1[1]; halves[2] = g.k2[0]; halves[3] = g.k2[1];
  const uint32_t W = mp_windows(c);
  for (uint32_t h = 0; h < 2; ++h) {
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) digits[h * W + w] = mp_digit(h ? g.k2 : g.k1, c, w, &carry);
    if (carry) return 0;   // a carry out of the top window: the recoding would be wrong
  }
  return W;
}

// the entries a call would sort: Montgomery scalars, finite[i] = 0 for an identity point
uint64_t hmp_count_digits(const uint8_t* scalars_mont, const uint8_t* finite, uint64_t m, uint32_t c) {
  uint64_t n = 0;
  for (uint64_t i = 0; i < m; ++i) {
    if (!finite[i]) continue;
    uint32_t k[8];
    canonical_scalar(scalars_mont + 32 * i, k);
    const GlvScalar g = glv_split(k);
    n += mp_count_digits(g.k1, g.k2, c);
  }
  return n;
}

// sum_i s_i P_i by the host bucket pipeline.  points: m x 96 bytes (96 zero bytes = identity); scalars: Montgomery.
// stats: entries, slices, longest bucket
int hmp_msm(const uint8_t* points96, const uint8_t* scalars_mont, uint64_t m, uint32_t c, uint32_t ksl, uint8_t out97[97],
            uint64_t stats[3]) {
  if (c < MP_C_MIN || c > MP_C_MAX || !ksl || m > MP_MAX_TERMS) return -1;
  const uint32_t W = mp_windows(c), nb = mp_buckets(c);
  std::vector<Fp28> xs(m), ys(m);
  std::vector<std::vector<uint32_t>> bucket((size_t)W * nb);
  for (uint64_t i = 0; i < m; ++i) {
    G1Affine a;
    memcpy(a.x.l, points96 + 96 * i, 48);
    memcpy(a.y.l, points96 + 96 * i + 48, 48);
    bool finite = false;
    for (int j = 0; j < 12; ++j) finite |= (a.x.l[j] | a.y.l[j]) != 0;
    if (!finite) continue;
    xs[i] = Fp28::from_fp(a.x);
    ys[i] = Fp28::from_fp(a.y);
    uint32_t k[8];
    canonical_scalar(scalars_mont + 32 * i, k);
    const GlvScalar g = glv_split(k);
    mp_for_each_digit(g.k1, g.k2, c, [&](uint32_t h, uint32_t w, uint32_t b, bool neg) {
      bucket[(size_t)w * nb + (b - 1)].push_back((uint32_t)i | (h ? MP_ENTRY_HALF : 0u) | (neg ? MP_ENTRY_NEG : 0u));
    });
  }
  auto entry_point = [&](uint32_t e, Fp28* x, Fp28* y) {
    const uint32_t t = e & MP_ENTRY_TERM;
    *x = (e & MP_ENTRY_HALF) ? Fp28::mul(xs[t], glv_beta()) : xs[t];
    *y = (e & MP_ENTRY_NEG) ? Fp28::neg_lazy<4>(ys[t]) : ys[t];
  };
  stats[0] = stats[1] = stats[2] = 0;
  std::vector<G1R> B((size_t)W * nb);
  for (size_t bi = 0; bi < bucket.size(); ++bi) {
    const std::vector<uint32_t>& ent = bucket[bi];
    stats[0] += ent.size();
    if (ent.size() > stats[2]) stats[2] = ent.size();
    G1R sum = G1R::identity();
    for (size_t beg = 0; beg < ent.size(); beg += ksl) {   // one slice, as one lane of mp_accumulate_kernel takes it
      const size_t end = beg + ksl < ent.size() ? beg + ksl : ent.size();
      ++stats[1];
      Fp28 x, y, x2, y2;
      entry_point(ent[beg], &x, &y);
      G1R acc;
      size_t k = beg + 1;
      if (k < end) {
        entry_point(ent[k++], &x2, &y2);
        if (G1R::pair_distinct(x, x2)) acc = G1R::add_affine_pair(x, y, x2, y2);
        else acc = G1R::from_affine(x, y.normalized()).add_affine(x2, y2);
      } else {
        acc = G1R::from_affine(x, y.normalized());
      }
      for (; k < end; ++k) {
        entry_point(ent[k], &x, &y);
        acc = acc.add_affine(x, y);
      }
      sum = sum.add(acc);
    }
    B[bi] = sum;
  }
  G1R total = G1R::identity();
  for (uint32_t w = W; w-- > 0;) {
    for (uint32_t d = 0; d < c; ++d) total = total.dbl();
    G1R run = G1R::identity(), T = G1R::identity();
    for (uint32_t i = nb; i-- > 0;) {
      run = run.add(B[(size_t)w * nb + i]);
      T = T.add(run);
    }
    total = total.add(T);
  }
  memset(out97, 0, 97);
  if (total.is_identity()) { out97[96] = 1; return 0; }
  Fp28 x, y;
  g1r_to_affine(total, &x, &y);
  const Fp xf = x.to_fp(), yf = y.to_fp();
  memcpy(out97, xf.l, 48);
  memcpy(out97 + 48, yf.l, 48);
  return 0;
}

}  // extern "C"

#ifdef HMP_MAIN
// Stand-alone run: every digit width on edge and pseudo-random scalars (the digits must rebuild the half, mod 2^128, with no
// carry out), and the pipeline at two widths and slice lengths on curve points with repeats, opposites and an identity — the
// two sums must agree (k1 P + k2 phi(P) is the same element whatever the digits are).
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
int main() {
  typedef unsigned __int128 u128;
  int bad = 0;
  for (uint32_t c = MP_C_MIN; c <= MP_C_MAX; ++c) {
    for (int it = 0; it < 64; ++it) {
      uint32_t k[8];
      for (int j = 0; j < 8; ++j) {   // 0, 1, 2^128 - 1, 2^254 - 1, then pseudo-random
        if (it == 0) k[j] = 0;
        else if (it == 1) k[j] = j == 0;
        else if (it == 2) k[j] = j < 4 ? 0xffffffffu : 0u;
        else if (it == 3) k[j] = 0xffffffffu;
        else k[j] = (uint32_t)rng();
      }
      k[7] &= 0x3fffffffu;   // below q
      uint64_t halves[4];
      std::vector<int32_t> d(2 * mp_windows(c));
      const uint32_t W = hmp_recode(k, c, halves, d.data());
      if (W != (129 + c - 1) / c) { ++bad; continue; }
      for (int h = 0; h < 2; ++h) {
        u128 acc = 0;
        for (uint32_t w = W; w-- > 0;) {
          acc = (acc << c) + (u128)(__int128)d[h * W + w];   // mod 2^128: a carry into bit 128 wraps away with what it repays
          if (d[h * W + w] > (1 << (c - 1)) || d[h * W + w] < -(1 << (c - 1))) ++bad;
        }
        const u128 want = ((u128)halves[2 * h + 1] << 64) | halves[2 * h];
        if (acc != want) ++bad;
      }
    }
  }
  // points: x = 1, 2, ... until 6 decode; then P0, P0, -P0, identity, P1 ... with scalars
  std::vector<G1Affine> pts;
  for (uint32_t x = 1; pts.size() < 6 && x < 200; ++x) {
    uint8_t comp[48] = {0};
    comp[0] = 0x80;
    comp[47] = (uint8_t)x;
    G1Affine a;
    if (g1_decompress48(comp, &a) == G1DEC_OK) pts.push_back(a);
  }
  const size_t m = 24;
  std::vector<uint8_t> p96(96 * m, 0), sc(32 * m, 0);
  for (size_t i = 0; i < m; ++i) {
    if (i % 7 != 3) {
      G1Affine a = pts[i % 3 == 0 ? 0 : i % pts.size()];
      if (i % 5 == 4) a.y = a.y.neg();
      memcpy(&p96[96 * i], a.x.l, 48);
      memcpy(&p96[96 * i + 48], a.y.l, 48);
    }
    for (int j = 0; j < 4; ++j) { const uint64_t v = i % 4 == 1 ? 5 * (j == 0) : rng(); memcpy(&sc[32 * i + 8 * j], &v, 8); }
    sc[32 * i + 31] &= 0x3f;
  }
  uint8_t o1[97], o2[97];
  uint64_t st[3];
  if (hmp_msm(p96.data(), sc.data(), m, 4, 2, o1, st) || hmp_msm(p96.data(), sc.data(), m, 13, 64, o2, st)) ++bad;
  if (memcmp(o1, o2, 97)) ++bad;
  printf("host_msm_points: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
