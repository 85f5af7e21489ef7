// Variable-base MSM over caller-supplied points: plonk_msm_points / plonk_msm_points_dev (the reference's
// msm_variable_base for points that are not the commit key).  A bucket method: no tables are precomputed, so unlike msm.hip
// the cost is all in the call.  DESIGN.md section 13.
//
//   mp_points_kernel     one lane per term: the point, decoded (g1_decompress48) or loaded, optionally checked
//                        (g1r_on_curve_in_subgroup), stored ONCE as a 128-byte G1AffineR entry; its kind (VDEC_*)
//   mp_recode_kernel     one lane per term: canonical scalar -> glv_split -> (k1, k2), kept for the scatter; the signed
//                        c-bit digits of both halves (msm_points_core.hpp) counted per (window, bucket)
//   mp_scan_kernel       one workgroup: exclusive scans of the bucket counts and of the slices per bucket (a bucket of n
//                        entries is cut into ceil(n / slice_entries) slices); totals and the longest bucket
//   mp_scatter_kernel    one lane per term: the digits again, each entry to its bucket's next free place
//   mp_accumulate_kernel one lane per slice: mixed additions of the slice's points (phi applied as x * beta when a half-2
//                        entry is read, the digit's sign on y); the first two through add_affine_pair when their x differ
//   mp_bucket_kernel     one lane per bucket: up to MP_LANE_SLICES slice sums added in the lane, longer buckets listed for
//   mp_heavy_kernel      one workgroup per listed bucket: lanes stride over its slices, then a tree in LDS
//   mp_window_kernel     one lane per run of MP_RUN buckets: sum B and sum (b - base) B by running sums, + [base] sum B
//                        (mul_u32), then a tree over the wave in LDS: one partial per 1024 buckets of a window
//   mp_wsum_kernel       one lane per window: its partials added, written as canonical XYZZ
// The host adds the windows (Horner, c doublings each, hostg1.hpp: a single lane would spend ~1 ms on 129 dependent
// doublings).  Every addition that can meet equal or opposite points or the identity is the general law (G1R::add_affine,
// G1R::add): duplicates, P and -P, phi(P) given explicitly and sums that pass through the identity need no special case.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "curve28.cuh"
#include "devmem.cuh"
#include "g1codec.cuh"
#include "hostg1.hpp"
#include "msm_points_core.hpp"

namespace plonk {

void prof_begin(Ctx* c, int slot);   // capi.hip
void prof_end(Ctx* c, int slot);

namespace {

constexpr uint32_t MP_BAD_DECODE = 1, MP_BAD_CHECK = 2;
struct MpMeta {            // what the host reads back after the scan
  uint32_t bad;            // MP_BAD_* of any term
  uint32_t entries;        // non-zero digits
  uint32_t slices;
  uint32_t longest;        // entries of the longest bucket
  uint32_t nheavy;         // buckets listed for mp_heavy_kernel
  uint32_t pad[3];
};

constexpr int MP_TERM_LANES = 64;
constexpr int MP_SCAN_LANES = 1024;
constexpr int MP_ACC_LANES = 128;
constexpr uint32_t MP_LANE_SLICES = 8;     // a bucket of at most this many slices is summed by its lane
constexpr int MP_HEAVY_LANES = 128;
constexpr uint32_t MP_HEAVY_BLOCKS = 1024;
constexpr uint32_t MP_RUN = 16;            // buckets per lane of the window sums
constexpr int MP_WIN_LANES = 64;           // one wave: 1024 buckets per workgroup
constexpr uint32_t MP_WIN_SPAN = MP_RUN * MP_WIN_LANES;

}  // namespace

__global__ void __launch_bounds__(MP_TERM_LANES) mp_points_kernel(MpInput in, uint32_t m, G1AffineR* __restrict__ aff,
                                                                  G1Affine* __restrict__ aff_fp, int32_t* __restrict__ kind,
                                                                  MpMeta* __restrict__ meta) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  G1Affine a;
  a.x = Fp::zero();
  a.y = Fp::zero();
  int st = VDEC_OK;
  uint32_t bad = 0;
  if (in.sc) {
    const uint32_t p = in.ids[t];
    st = in.kind[p];
    if (st == VDEC_OK) a = in.pts[p];
  } else if (in.flags & PLONK_POINTS_COMPRESSED) {
    const int rc = g1_decompress48(in.points + 48ull * t, &a);
    if (rc == G1DEC_IDENTITY) st = VDEC_IDENTITY;
    else if (rc != G1DEC_OK) { st = VDEC_BAD; bad = MP_BAD_DECODE; }
  } else {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(in.points + 96ull * t);
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) { a.x.l[i] = w[i]; a.y.l[i] = w[12 + i]; nz |= w[i] | w[12 + i]; }
    if (!nz) st = VDEC_IDENTITY;
  }
  Fp28 x = Fp28::zero(), y = Fp28::zero();
  if (st == VDEC_OK) {
    x = Fp28::from_fp(a.x);
    y = Fp28::from_fp(a.y);
    if (!in.sc && (in.flags & PLONK_POINTS_CHECK) && !g1r_on_curve_in_subgroup(x, y)) { st = VDEC_BAD; bad = MP_BAD_CHECK; }
  }
  if (st != VDEC_OK) {
    a.x = Fp::zero();
    a.y = Fp::zero();
    x = Fp28::zero();
    y = Fp28::zero();
  }
  if (bad) atomicOr(&meta->bad, bad);
  kind[t] = st;
  if (aff) { st_f28(&aff[t].x, x); st_f28(&aff[t].y, y); }
  if (aff_fp) aff_fp[t] = a;
}

// atomicAdd(&counter[key], 1) for every active lane, returning the lane's own old value.  When all active lanes of the wave
// hold the same key — every scalar equal puts whole waves on one counter, and same-address atomics serialise — the first
// lane adds the lane count once and the others take their rank; otherwise one atomic per lane.
__device__ __forceinline__ uint32_t mp_counter_next(uint32_t* __restrict__ counter, uint32_t key) {
  const uint64_t active = __ballot(1);
  const uint32_t first = __builtin_amdgcn_readfirstlane(key);
  if (__ballot(key == first) != active) return atomicAdd(&counter[key], 1u);
  const uint32_t rank = __popcll(active & ((1ull << __lane_id()) - 1ull));
  uint32_t base = 0;
  if (!rank) base = atomicAdd(&counter[key], (uint32_t)__popcll(active));
  return __builtin_amdgcn_readfirstlane(base) + rank;   // the first active lane is the one of rank 0
}

// the canonical scalar of term t (8 words); false when it is zero
__device__ __forceinline__ bool mp_scalar(const MpInput& in, uint32_t t, uint32_t k[8]) {
  uint32_t nz = 0;
  if (in.sc) {
#pragma unroll
    for (int w = 0; w < 8; ++w) { k[w] = in.sc[8ull * t + w]; nz |= k[w]; }
  } else {
    const Fr s = in.scalars[t].from_mont();
#pragma unroll
    for (int w = 0; w < 8; ++w) { k[w] = s.l[w]; nz |= k[w]; }
  }
  return nz != 0;
}

__global__ void __launch_bounds__(MP_TERM_LANES) mp_recode_kernel(MpInput in, uint32_t m, const int32_t* __restrict__ kind,
                                                                  uint32_t c, GlvScalar* __restrict__ glv,
                                                                  uint32_t* __restrict__ counts) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  GlvScalar g;
  g.k1[0] = g.k1[1] = g.k2[0] = g.k2[1] = 0;
  uint32_t k[8];
  if (mp_scalar(in, t, k) && kind[t] == VDEC_OK) g = glv_split(k);
  glv[t] = g;
  const uint32_t nb = mp_buckets(c);
  mp_for_each_digit(g.k1, g.k2, c, [&](uint32_t, uint32_t w, uint32_t b, bool) { (void)mp_counter_next(counts, w * nb + (b - 1)); });
}

// the per-term path: canonical scalars and ids for msm_run
__global__ void __launch_bounds__(MP_TERM_LANES) mp_pack_kernel(MpInput in, uint32_t m, uint32_t* __restrict__ sc,
                                                                uint32_t* __restrict__ ids) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  uint32_t k[8];
  (void)mp_scalar(in, t, k);
#pragma unroll
  for (int w = 0; w < 8; ++w) sc[8ull * t + w] = k[w];
  ids[t] = t;
}

// off[b] / cur[b] = entries before bucket b, slice_off[b] = slices before it (b <= nbt); meta: totals and the longest bucket
__global__ void __launch_bounds__(MP_SCAN_LANES) mp_scan_kernel(const uint32_t* __restrict__ counts, uint32_t nbt, uint32_t ksl,
                                                                uint32_t* __restrict__ off, uint32_t* __restrict__ cur,
                                                                uint32_t* __restrict__ slice_off, MpMeta* __restrict__ meta) {
  __shared__ uint32_t se[MP_SCAN_LANES], ss[MP_SCAN_LANES], longest;
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nbt + MP_SCAN_LANES - 1) / MP_SCAN_LANES;
  const uint32_t b0 = t * per < nbt ? t * per : nbt, b1 = b0 + per < nbt ? b0 + per : nbt;
  if (!t) longest = 0;
  uint32_t e = 0, s = 0, mx = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t n = counts[b];
    e += n;
    s += (n + ksl - 1) / ksl;
    mx = n > mx ? n : mx;
  }
  se[t] = e;
  ss[t] = s;
  __syncthreads();
  if (mx) atomicMax(&longest, mx);
  for (uint32_t d = 1; d < MP_SCAN_LANES; d <<= 1) {   // inclusive scan of the lanes' totals
    const uint32_t ve = t >= d ? se[t - d] : 0, vs = t >= d ? ss[t - d] : 0;
    __syncthreads();
    se[t] += ve;
    ss[t] += vs;
    __syncthreads();
  }
  uint32_t pe = se[t] - e, ps = ss[t] - s;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t n = counts[b];
    off[b] = pe;
    cur[b] = pe;
    slice_off[b] = ps;
    pe += n;
    ps += (n + ksl - 1) / ksl;
  }
  if (t == MP_SCAN_LANES - 1) {
    off[nbt] = se[t];
    slice_off[nbt] = ss[t];
    meta->entries = se[t];
    meta->slices = ss[t];
    meta->longest = longest;
  }
}

__global__ void __launch_bounds__(MP_TERM_LANES) mp_scatter_kernel(const GlvScalar* __restrict__ glv, uint32_t m, uint32_t c,
                                                                   uint32_t* __restrict__ cur, uint32_t* __restrict__ entries) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  const GlvScalar g = glv[t];
  const uint32_t nb = mp_buckets(c);
  mp_for_each_digit(g.k1, g.k2, c, [&](uint32_t h, uint32_t w, uint32_t b, bool neg) {
    const uint32_t pos = mp_counter_next(cur, w * nb + (b - 1));
    entries[pos] = t | (h ? MP_ENTRY_HALF : 0u) | (neg ? MP_ENTRY_NEG : 0u);
  });
}

// the point of an entry as add_affine takes it: x < 2p (times beta for a half-2 entry: phi(P) = (beta x, y)), y or 4p - y
__device__ __forceinline__ void mp_entry_point(const G1AffineR* __restrict__ aff, uint32_t e, Fp28* x, Fp28* y) {
  const G1AffineR* p = aff + (e & MP_ENTRY_TERM);
  const Fp28 x0 = ld_f28(&p->x), y0 = ld_f28(&p->y);
  const Fp28 one = Fp28::one(), beta = glv_beta();
  Fp28 f;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) f.l[i] = (e & MP_ENTRY_HALF) ? beta.l[i] : one.l[i];
  *x = Fp28::mul(x0, f);                                      // 2 * 1 -> < 2p
  const bool neg = (e & MP_ENTRY_NEG) != 0;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) y->l[i] = neg ? Fp28::pad<4>(i) - y0.l[i] : y0.l[i];   // lazy limbs: it only feeds products
}

__global__ void __launch_bounds__(MP_ACC_LANES) mp_accumulate_kernel(const G1AffineR* __restrict__ aff,
                                                                     const uint32_t* __restrict__ entries,
                                                                     const uint32_t* __restrict__ off,
                                                                     const uint32_t* __restrict__ slice_off, uint32_t nbt,
                                                                     uint32_t nslices, uint32_t ksl, G1RSlot* __restrict__ partial) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslices) return;
  uint32_t lo = 0, hi = nbt - 1;   // the slice's bucket: the largest b with slice_off[b] <= s (an empty bucket shares its offset with the next)
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (slice_off[mid] <= s) lo = mid; else hi = mid - 1;
  }
  const uint32_t b = lo;
  const uint32_t beg = off[b] + (s - slice_off[b]) * ksl;
  uint32_t end = beg + ksl;
  const uint32_t bend = off[b + 1];
  if (end > bend) end = bend;
  Fp28 x, y;
  mp_entry_point(aff, entries[beg], &x, &y);
  G1R acc;
  uint32_t k = beg + 1;
  if (k < end) {
    Fp28 x2, y2;
    mp_entry_point(aff, entries[k], &x2, &y2);
    ++k;
    if (G1R::pair_distinct(x, x2)) acc = G1R::add_affine_pair(x, y, x2, y2);
    else acc = G1R::from_affine(x, y.normalized()).add_affine(x2, y2);   // equal or opposite: the general law doubles or cancels
  } else {
    acc = G1R::from_affine(x, y.normalized());
  }
  for (; k < end; ++k) {
    mp_entry_point(aff, entries[k], &x, &y);
    acc = acc.add_affine(x, y);
  }
  st_g1r(partial + s, acc);
}

__global__ void __launch_bounds__(64) mp_bucket_kernel(const G1RSlot* __restrict__ partial, const uint32_t* __restrict__ slice_off,
                                                       uint32_t nbt, G1RSlot* __restrict__ buckets,
                                                       uint32_t* __restrict__ heavy, MpMeta* __restrict__ meta) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbt) return;
  const uint32_t s0 = slice_off[b], s1 = slice_off[b + 1];
  if (s1 - s0 > MP_LANE_SLICES) {
    heavy[atomicAdd(&meta->nheavy, 1u)] = b;
    return;
  }
  G1R acc = G1R::identity();
  if (s0 < s1) acc = ld_g1r(partial + s0);
  for (uint32_t s = s0 + 1; s < s1; ++s) acc = acc.add(ld_g1r(partial + s));
  st_g1r(buckets + b, acc);
}

__global__ void __launch_bounds__(MP_HEAVY_LANES) mp_heavy_kernel(const G1RSlot* __restrict__ partial,
                                                                  const uint32_t* __restrict__ slice_off,
                                                                  const uint32_t* __restrict__ heavy,
                                                                  const MpMeta* __restrict__ meta, G1RSlot* __restrict__ buckets) {
  __shared__ G1R sh[MP_HEAVY_LANES];
  const uint32_t lane = threadIdx.x, n = meta->nheavy;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {   // (i and n are the same in every lane: the barriers are uniform)
    const uint32_t b = heavy[i], s0 = slice_off[b], s1 = slice_off[b + 1];
    G1R acc = G1R::identity();
    for (uint32_t s = s0 + lane; s < s1; s += MP_HEAVY_LANES) acc = acc.add(ld_g1r(partial + s));
    sh[lane] = acc;
    __syncthreads();
    for (uint32_t d = MP_HEAVY_LANES / 2; d; d >>= 1) {
      if (lane < d) sh[lane] = sh[lane].add(sh[lane + d]);
      __syncthreads();
    }
    if (!lane) st_g1r(buckets + b, sh[0]);
    __syncthreads();
  }
}

// grid (ceil(nb / 1024), windows).  Lane g of a window owns buckets base + 1 .. base + MP_RUN, base = MP_RUN g (bucket b at
// index b - 1): running sums from the top give S = sum B_b and T = sum (b - base) B_b, the lane's share is T + [base] S.
__global__ void __launch_bounds__(MP_WIN_LANES) mp_window_kernel(const G1RSlot* __restrict__ buckets, uint32_t nb,
                                                                 G1RSlot* __restrict__ chunk) {
  __shared__ G1R sh[MP_WIN_LANES];
  const uint32_t lane = threadIdx.x, w = blockIdx.y;
  const uint32_t base = (blockIdx.x * MP_WIN_LANES + lane) * MP_RUN;
  const G1RSlot* B = buckets + (uint64_t)w * nb;
  G1R run = G1R::identity(), T = G1R::identity();
  for (uint32_t j = MP_RUN; j-- > 0;) {
    const uint32_t i = base + j;
    if (i >= nb) continue;
    run = run.add(ld_g1r(B + i));
    T = T.add(run);
  }
  if (base && !run.is_identity()) T = T.add(run.mul_u32(base));
  sh[lane] = T;
  __syncthreads();
  for (uint32_t d = MP_WIN_LANES / 2; d; d >>= 1) {
    if (lane < d) sh[lane] = sh[lane].add(sh[lane + d]);
    __syncthreads();
  }
  if (!lane) st_g1r(chunk + (uint64_t)w * gridDim.x + blockIdx.x, sh[0]);
}

__global__ void __launch_bounds__(64) mp_wsum_kernel(const G1RSlot* __restrict__ chunk, uint32_t windows, uint32_t per_window,
                                                     G1* __restrict__ wsum) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= windows) return;
  G1R acc = ld_g1r(chunk + (uint64_t)w * per_window);
  for (uint32_t i = 1; i < per_window; ++i) acc = acc.add(ld_g1r(chunk + (uint64_t)w * per_window + i));
  wsum[w] = acc.to_g1();
}

// ---- host side --------------------------------------------------------------------------------------------------------
namespace {

struct MpBufs {
  enum { POINTS, SCALARS, AFF, AFF_FP, KIND, GLV, COUNTS, OFF, CUR, SLICE_OFF, ENTRIES, PARTIAL, BUCKETS, HEAVY, CHUNK, WSUM,
         META, SC, IDS, PART, NBUF };
};
// the context's grow-only workspace (Ctx::points_ws); a request for 0 bytes allocates 16
struct MpWork : MpBufs, DevBufs<MpBufs::NBUF, 16> {};

MpWork& mp_work(Ctx* c) {
  if (!c->points_ws) c->points_ws = new MpWork();
  return *(MpWork*)c->points_ws;
}

int mp_bad_point(uint32_t bad) {
  set_last_error("plonk_msm_points", bad & MP_BAD_DECODE ? "not a valid compressed point of G1"
                                                         : "a point is off the curve or outside the prime-order subgroup (PLONK_POINTS_CHECK)",
                 __FILE__, __LINE__);
  return PLONK_ERR_POINT;
}

H1 h1_identity() {
  H1 h;
  memset(&h, 0, sizeof h);
  return h;
}
G1 g1_of_h1(const H1& h) {
  if (h.inf()) return G1::identity();
  G1 g;
  g.X = from64(h.X); g.Y = from64(h.Y); g.ZZ = from64(h.ZZ); g.ZZZ = from64(h.ZZZ);
  return g;
}

inline dim3 term_grid(uint64_t m) { return dim3((uint32_t)((m + MP_TERM_LANES - 1) / MP_TERM_LANES)); }

// below opts.min_bucket_terms: the terms packed for msm_run, verify.hip's per-term kernel
int mp_run_per_term(Ctx* c, MpWork& w, const MpInput& in, uint64_t m, G1* sum) {
  const hipStream_t st = c->stream;
  H1 sums[2];
  PTRY(w.need(MpWork::PART, sizeof(G1) * 2 * VERIFY_MSM_MAX_BLOCKS));
  if (in.sc) {
    PTRY(msm_run(c, in.sc, in.ids, m, 0, in.pts, in.kind, w.at<G1>(MpWork::PART), sums));
    *sum = g1_of_h1(sums[0]);
    return PLONK_OK;
  }
  PTRY(w.need(MpWork::AFF_FP, sizeof(G1Affine) * m));
  PTRY(w.need(MpWork::KIND, 4 * m));
  PTRY(w.need(MpWork::SC, 32 * m));
  PTRY(w.need(MpWork::IDS, 4 * m));
  PTRY(w.need(MpWork::META, sizeof(MpMeta)));
  MpMeta* meta = w.at<MpMeta>(MpWork::META);
  HIP_TRY(hipMemsetAsync(meta, 0, sizeof(MpMeta), st));
  hipLaunchKernelGGL(mp_points_kernel, term_grid(m), dim3(MP_TERM_LANES), 0, st, in, (uint32_t)m, (G1AffineR*)nullptr,
                     w.at<G1Affine>(MpWork::AFF_FP), w.at<int32_t>(MpWork::KIND), meta);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mp_pack_kernel, term_grid(m), dim3(MP_TERM_LANES), 0, st, in, (uint32_t)m, w.at<uint32_t>(MpWork::SC),
                     w.at<uint32_t>(MpWork::IDS));
  HIP_TRY(hipGetLastError());
  MpMeta mh;
  HIP_TRY(hipMemcpyAsync(&mh, meta, sizeof mh, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (mh.bad) return mp_bad_point(mh.bad);
  PTRY(msm_run(c, w.at<uint32_t>(MpWork::SC), w.at<uint32_t>(MpWork::IDS), m, 0, w.at<G1Affine>(MpWork::AFF_FP),
                 w.at<int32_t>(MpWork::KIND), w.at<G1>(MpWork::PART), sums));
  *sum = g1_of_h1(sums[0]);
  return PLONK_OK;
}

int mp_run_buckets(Ctx* c, MpWork& w, const MpInput& in, uint64_t m, const MpPlan& plan, plonk_msm_points_info* info, G1* sum) {
  const hipStream_t st = c->stream;
  const uint32_t cb = plan.c, W = plan.windows, nb = mp_buckets(cb), nbt = W * nb, ksl = plan.slice_entries;
  PTRY(w.need(MpWork::AFF, sizeof(G1AffineR) * m));
  PTRY(w.need(MpWork::KIND, 4 * m));
  PTRY(w.need(MpWork::GLV, sizeof(GlvScalar) * m));
  PTRY(w.need(MpWork::COUNTS, 4ull * nbt));
  PTRY(w.need(MpWork::OFF, 4ull * (nbt + 1)));
  PTRY(w.need(MpWork::CUR, 4ull * nbt));
  PTRY(w.need(MpWork::SLICE_OFF, 4ull * (nbt + 1)));
  PTRY(w.need(MpWork::BUCKETS, sizeof(G1RSlot) * (uint64_t)nbt));
  PTRY(w.need(MpWork::HEAVY, 4ull * nbt));
  const uint32_t per_window = (nb + MP_WIN_SPAN - 1) / MP_WIN_SPAN;
  PTRY(w.need(MpWork::CHUNK, sizeof(G1RSlot) * (uint64_t)W * per_window));
  PTRY(w.need(MpWork::WSUM, sizeof(G1) * W));
  PTRY(w.need(MpWork::META, sizeof(MpMeta)));
  MpMeta* meta = w.at<MpMeta>(MpWork::META);
  uint32_t* counts = w.at<uint32_t>(MpWork::COUNTS);
  uint32_t* off = w.at<uint32_t>(MpWork::OFF);
  uint32_t* slice_off = w.at<uint32_t>(MpWork::SLICE_OFF);
  // 1. load and recode
  prof_begin(c, 15);
  HIP_TRY(hipMemsetAsync(meta, 0, sizeof(MpMeta), st));
  HIP_TRY(hipMemsetAsync(counts, 0, 4ull * nbt, st));
  hipLaunchKernelGGL(mp_points_kernel, term_grid(m), dim3(MP_TERM_LANES), 0, st, in, (uint32_t)m, w.at<G1AffineR>(MpWork::AFF),
                     (G1Affine*)nullptr, w.at<int32_t>(MpWork::KIND), meta);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mp_recode_kernel, term_grid(m), dim3(MP_TERM_LANES), 0, st, in, (uint32_t)m, w.at<const int32_t>(MpWork::KIND),
                     cb, w.at<GlvScalar>(MpWork::GLV), counts);
  HIP_TRY(hipGetLastError());
  prof_end(c, 15);
  // 2. group by (window, bucket): the scan, then the sizes come back (entries, slices, a bad point), then the scatter
  prof_begin(c, 22);
  hipLaunchKernelGGL(mp_scan_kernel, dim3(1), dim3(MP_SCAN_LANES), 0, st, counts, nbt, ksl, off, w.at<uint32_t>(MpWork::CUR),
                     slice_off, meta);
  HIP_TRY(hipGetLastError());
  MpMeta mh;
  HIP_TRY(hipMemcpyAsync(&mh, meta, sizeof mh, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (mh.bad) { prof_end(c, 22); return mp_bad_point(mh.bad); }
  info->nonzero_digits = mh.entries;
  info->slices = mh.slices;
  info->longest_bucket = mh.longest;
  if (!mh.entries) {   // every scalar zero or every point the identity
    prof_end(c, 22);
    *sum = G1::identity();
    return PLONK_OK;
  }
  PTRY(w.need(MpWork::ENTRIES, 4ull * mh.entries));
  PTRY(w.need(MpWork::PARTIAL, sizeof(G1RSlot) * (uint64_t)mh.slices));
  hipLaunchKernelGGL(mp_scatter_kernel, term_grid(m), dim3(MP_TERM_LANES), 0, st, w.at<const GlvScalar>(MpWork::GLV), (uint32_t)m, cb,
                     w.at<uint32_t>(MpWork::CUR), w.at<uint32_t>(MpWork::ENTRIES));
  HIP_TRY(hipGetLastError());
  prof_end(c, 22);
  // 3. accumulate the slices
  prof_begin(c, 23);
  hipLaunchKernelGGL(mp_accumulate_kernel, dim3((mh.slices + MP_ACC_LANES - 1) / MP_ACC_LANES), dim3(MP_ACC_LANES), 0, st,
                     w.at<const G1AffineR>(MpWork::AFF), w.at<const uint32_t>(MpWork::ENTRIES), off, slice_off, nbt, mh.slices, ksl,
                     w.at<G1RSlot>(MpWork::PARTIAL));
  HIP_TRY(hipGetLastError());
  prof_end(c, 23);
  // 4. slice sums -> bucket sums
  prof_begin(c, 30);
  hipLaunchKernelGGL(mp_bucket_kernel, dim3((nbt + 63) / 64), dim3(64), 0, st, w.at<const G1RSlot>(MpWork::PARTIAL), slice_off, nbt,
                     w.at<G1RSlot>(MpWork::BUCKETS), w.at<uint32_t>(MpWork::HEAVY), meta);
  HIP_TRY(hipGetLastError());
  if (mh.longest > (uint64_t)MP_LANE_SLICES * ksl) {   // some bucket has more than MP_LANE_SLICES slices
    const uint32_t blocks = nbt < MP_HEAVY_BLOCKS ? nbt : MP_HEAVY_BLOCKS;
    hipLaunchKernelGGL(mp_heavy_kernel, dim3(blocks), dim3(MP_HEAVY_LANES), 0, st, w.at<const G1RSlot>(MpWork::PARTIAL), slice_off,
                       w.at<const uint32_t>(MpWork::HEAVY), meta, w.at<G1RSlot>(MpWork::BUCKETS));
    HIP_TRY(hipGetLastError());
  }
  prof_end(c, 30);
  // 5. window sums
  prof_begin(c, 31);
  hipLaunchKernelGGL(mp_window_kernel, dim3(per_window, W), dim3(MP_WIN_LANES), 0, st, w.at<const G1RSlot>(MpWork::BUCKETS), nb,
                     w.at<G1RSlot>(MpWork::CHUNK));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mp_wsum_kernel, dim3((W + 63) / 64), dim3(64), 0, st, w.at<const G1RSlot>(MpWork::CHUNK), W, per_window,
                     w.at<G1>(MpWork::WSUM));
  HIP_TRY(hipGetLastError());
  prof_end(c, 31);
  // 6. the windows: Horner on the host
  std::vector<G1> ws(W);
  HIP_TRY(hipMemcpyAsync(ws.data(), w.p[MpWork::WSUM], sizeof(G1) * W, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  H1 acc = h1_identity();
  for (uint32_t k = W; k-- > 0;) {
    if (!acc.inf())
      for (uint32_t d = 0; d < cb; ++d) acc = h1_dbl(acc);
    acc = h1_add(acc, h1_of_g1(ws[k]));
  }
  *sum = g1_of_h1(acc);
  return PLONK_OK;
}

}  // namespace

void msm_points_ws_release(Ctx* c) {
  delete (MpWork*)c->points_ws;
  c->points_ws = nullptr;
}

int msm_points_run(Ctx* c, const MpInput& in, uint64_t m, const plonk_msm_points_opts* opts, G1* sum) {
  plonk_msm_points_opts o = {};
  if (opts) o = *opts;
  const MpPlan plan = mp_plan(m, o.window_bits, o.slice_entries, o.min_bucket_terms);
  plonk_msm_points_info info = {};
  info.path = plan.path;
  info.window_bits = plan.c;
  info.windows = plan.windows;
  info.slice_entries = plan.slice_entries;
  info.terms = m;
  int rc = PLONK_OK;
  if (!m) *sum = G1::identity();
  else if (plan.path) rc = mp_run_buckets(c, mp_work(c), in, m, plan, &info, sum);
  else rc = mp_run_per_term(c, mp_work(c), in, m, sum);
  if (rc == PLONK_OK) {
    c->last_points = info;
    c->last_points_valid = true;
  }
  return rc;
}

namespace {

int mp_check_args(const char* api_fn, plonk_ctx* ctx, const void* points, const void* scalars, uint64_t m,
                  const plonk_msm_points_opts* opts, const void* out) {
  const char* msg = nullptr;
  if (!ctx || !out || (m && (!points || !scalars))) msg = "invalid argument: a required pointer is NULL";
  else if (m > MP_MAX_TERMS) msg = "invalid argument: at most 2^24 terms per call";
  else if (opts) {
    if (opts->struct_size < sizeof(plonk_msm_points_opts)) msg = "invalid argument: opts.struct_size is smaller than plonk_msm_points_opts";
    else if (opts->flags & ~(uint32_t)(PLONK_POINTS_COMPRESSED | PLONK_POINTS_CHECK)) msg = "invalid argument: unknown bit in opts.flags";
    else if (opts->window_bits && (opts->window_bits < MP_C_MIN || opts->window_bits > MP_C_MAX)) msg = "invalid argument: opts.window_bits must be 0 or in 2..16";
    else if (opts->slice_entries > (1u << 20)) msg = "invalid argument: opts.slice_entries must be at most 2^20";
  }
  if (!msg) return PLONK_OK;
  set_last_error(api_fn, msg, __FILE__, __LINE__);
  return PLONK_ERR_ARG;
}

}  // namespace
}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_msm_points(plonk_ctx* ctx, const uint8_t* points, const uint64_t* scalars, uint64_t m, const plonk_msm_points_opts* opts,
                     uint8_t out_xy_inf[97]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  PTRY(mp_check_args(api_fn, ctx, points, scalars, m, opts, out_xy_inf));
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  MpWork& w = mp_work(&c);
  MpInput in;
  in.flags = opts ? opts->flags : 0;
  if (m) {
    const uint64_t pbytes = (in.flags & PLONK_POINTS_COMPRESSED ? 48ull : 96ull) * m;
    PTRY(w.need(MpWork::POINTS, pbytes));
    PTRY(w.need(MpWork::SCALARS, 32 * m));
    HIP_TRY(hipMemcpyAsync(w.p[MpWork::POINTS], points, pbytes, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipMemcpyAsync(w.p[MpWork::SCALARS], scalars, 32 * m, hipMemcpyHostToDevice, c.stream));
    in.points = w.at<const uint8_t>(MpWork::POINTS);
    in.scalars = w.at<const Fr>(MpWork::SCALARS);
  }
  G1 sum;
  PTRY(msm_points_run(&c, in, m, opts, &sum));
  batch_xyzz_to_affine97(&sum, 1, reinterpret_cast<uint8_t (*)[97]>(out_xy_inf));
  return PLONK_OK;
  });
}

int plonk_msm_points_dev(plonk_ctx* ctx, const void* points_dev, const void* scalars_dev, uint64_t m,
                         const plonk_msm_points_opts* opts, void* out97_dev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  PTRY(mp_check_args(api_fn, ctx, points_dev, scalars_dev, m, opts, out97_dev));
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  MpInput in;
  in.flags = opts ? opts->flags : 0;
  in.points = (const uint8_t*)points_dev;
  in.scalars = (const Fr*)scalars_dev;
  G1 sum;
  PTRY(msm_points_run(&c, in, m, opts, &sum));
  uint8_t out[1][97];
  batch_xyzz_to_affine97(&sum, 1, out);
  HIP_TRY(hipMemcpyAsync(out97_dev, out[0], 97, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  return PLONK_OK;
  });
}

int plonk_ctx_last_msm_points(plonk_ctx* ctx, plonk_msm_points_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out) return (set_last_error(api_fn, "invalid argument", __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  if (!ctx->c.last_points_valid) return (set_last_error(api_fn, "no plonk_msm_points call has run on this context", __FILE__, __LINE__), PLONK_ERR_STATE);
  *out = ctx->c.last_points;
  return PLONK_OK;
  });
}

}  // extern "C"
