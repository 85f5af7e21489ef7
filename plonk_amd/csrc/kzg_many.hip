// KZG10 commitments of many short vectors over window tables of a plonk_kzg_domain's Lagrange points.  The recoding, the
// table indexing and the plan are in kzg_many_core.hpp; DESIGN.md section 22 has the resources and the measurements.
//
//   kzm_bases_kernel       table build, one lane per Lagrange point: 2^(c w) L_i for every window as XYZZ slots, by c
//                          doublings from the window below
//   kzm_entries_kernel     table build, one lane per ENTRY: [d] base by a double-and-add of at most c - 1 steps, one safegcd
//                          inverse, x || y < 2p.  An inverse per lane and no shared batch inversion: an entry is then its own
//                          lane from the base on, the build runs device-wide with no pass over a scratch array of ZZ / ZZZ
//                          products, and it happens once per handle (DESIGN.md section 22 has its time).
//   kzm_scan_kernel        resident values: the canonical-form check
//   kzm_accumulate_kernel  one wave per (vector, slice): a lane takes its values out of Montgomery form, recodes them and
//                          adds one table entry per non-zero digit (the first two by G1R::add_affine_pair where
//                          pair_distinct holds, every later one by G1R::add_affine; the sign as 4p - y, lazily); the 64 lane
//                          sums meet in a tree of G1R::add over cross-lane moves; lane 0 writes one XYZZ slot
//   kzm_sparse_kernel      the same lane function behind the loader of plonk_kzg_update_many: the terms of a segment dealt
//                          round-robin to the lanes, the index read beside the delta
//   kzm_compress_kernel    one lane per commitment: the slices' partial sums, the decoded base if there is one,
//                          g1r_compress48_words (g1codec.cuh)
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "devmem.cuh"
#include "g1codec.cuh"
#include "kzg_core.hpp"
#include "kzg_handle.hpp"
#include "kzg_evals.hpp"
#include "kzg_many.hpp"

namespace plonk {

static_assert(sizeof(G1AffineR) == KZM_ENTRY_BYTES, "entry size");
static_assert(sizeof(G1RSlot) == KZM_SLOT_BYTES, "slot size");

// ---- the table build --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KZM_LANES) kzm_bases_kernel(const G1Affine* __restrict__ lag, uint64_t n, uint32_t c, uint32_t W,
                                                              G1RSlot* __restrict__ bases) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Affine a = ld_aff(lag + i);
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) any |= a.x.l[k] | a.y.l[k];
  G1R b = any ? G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)) : G1R::identity();
  for (uint32_t w = 0; w < W; ++w) {
    st_g1r(bases + i * W + w, b);
    for (uint32_t k = 0; k < c; ++k) b = b.dbl();
  }
}

__global__ void __launch_bounds__(KZM_LANES) kzm_entries_kernel(const G1RSlot* __restrict__ bases, uint64_t entries, uint32_t c,
                                                                G1AffineR* __restrict__ table) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const uint32_t d = (uint32_t)(e & ((1u << (c - 1)) - 1u)) + 1u;
  const G1R b = ld_g1r(bases + (e >> (c - 1)));
  Fp28 x = Fp28::zero(), y = Fp28::zero();   // the identity's mark: 128 zero bytes
  if (!b.is_identity()) g1r_to_affine(b.mul_u32(d), &x, &y);   // (d < q: a finite base has finite multiples)
  st_f28(&table[e].x, x);
  st_f28(&table[e].y, y);
}

__global__ void __launch_bounds__(256) kzm_scan_kernel(const Fr* __restrict__ values, uint64_t total, unsigned long long* __restrict__ bad) {
  unsigned long long b = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const Fr x = ld_fr(values + i);
    bool lt = false;
    for (int k = 7; k >= 0; --k)
      if (x.l[k] != FrP::MOD[k]) { lt = x.l[k] < FrP::MOD[k]; break; }
    if (!lt) b = 1;
  }
  if (b) atomicOr(bad, b);
}

// ---- the accumulation -------------------------------------------------------------------------------------------------------
namespace {

// The sum of a wave over nv terms; ld(t, &value, &point) gives term t < nv.  vpl = min(64, nv rounded up to a power of two)
// lanes share the terms of a pass, 64 / vpl lanes share the windows of a term: lane = part * vpl + k owns the terms k, k + vpl,
// ... and of each the windows w = part mod (64 / vpl).  A lane holds ONE accumulator and, before its second entry, the first
// one as an affine pair; the recoding shifts the scalar in place (constant limb indices, no array indexed at run time).
template <class Load>
__device__ __forceinline__ G1R kzm_wave_sum(const KzmTables& tb, uint32_t nv, const Load& ld) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t vlog = 0;
  while (vlog < 6 && (1u << vlog) < nv) ++vlog;
  const uint32_t vpl = 1u << vlog, lpv_mask = (64u >> vlog) - 1u;
  const uint32_t k = lane & (vpl - 1u), part = lane >> vlog;
  const uint32_t c = tb.window_bits, W = tb.windows;
  G1R acc = G1R::identity();
  Fp28 px = Fp28::zero(), py = Fp28::zero();
  uint32_t state = 0;   // 0: nothing yet, 1: one entry waits in (px, py), 2: acc holds the sum
  for (uint32_t t = k; t < nv; t += vpl) {
    Fr v;
    uint32_t point;
    ld(t, &v, &point);
    Fr s = v.from_mont();
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) {
      const int32_t d = kzm_next_digit(s.l, c, &carry);
      if (!d || (w & lpv_mask) != part) continue;
      const G1AffineR* e = tb.entries + kzm_entry(c, W, point, w, (uint32_t)(d < 0 ? -d : d));
      const Fp28 x = ld_f28(&e->x), y = ld_f28(&e->y);
      if (y.is_zero_limbs()) continue;   // an identity Lagrange point
      // -y as 4p - y without carry propagation (lazy limbs): it only feeds a product
      Fp28 y2;
#pragma unroll
      for (int i = 0; i < Fp28::N; ++i) y2.l[i] = d < 0 ? Fp28::pad<4>(i) - y.l[i] : y.l[i];
      if (state == 0) {
        px = x;
        py = y2;
        state = 1;
        continue;
      }
      if (state == 1) {
        state = 2;
        if (G1R::pair_distinct(px, x)) {
          acc = G1R::add_affine_pair(px, py, x, y2);
          continue;
        }
        acc = G1R::from_affine(px, py.normalized());   // equal or opposite points: the general path doubles or cancels
      }
      acc = acc.add_affine(x, y2);
    }
  }
  if (state == 1) acc = G1R::from_affine(px, py.normalized());
  // the 64 lane sums: a tree of G1R::add over cross-lane moves (56 words per point and level)
#pragma unroll 1
  for (int off = 32; off; off >>= 1) {
    G1R o;
#pragma unroll
    for (int i = 0; i < Fp28::N; ++i) {
      o.X.l[i] = __shfl_down(acc.X.l[i], off, 64);
      o.Y.l[i] = __shfl_down(acc.Y.l[i], off, 64);
      o.ZZ.l[i] = __shfl_down(acc.ZZ.l[i], off, 64);
      o.ZZZ.l[i] = __shfl_down(acc.ZZZ.l[i], off, 64);
    }
    acc = acc.add(o);
  }
  return acc;
}

struct KzmDenseLoad {
  const Fr* v;      // the slice's first value
  uint32_t first;   // its index in the vector
  __device__ __forceinline__ void operator()(uint32_t t, Fr* value, uint32_t* point) const {
    *value = ld_fr(v + t);
    *point = first + t;
  }
};
struct KzmSparseLoad {
  const Fr* d;
  const uint32_t* idx;
  __device__ __forceinline__ void operator()(uint32_t t, Fr* value, uint32_t* point) const {
    *value = ld_fr(d + t);
    *point = idx[t];
  }
};

}  // namespace

__global__ void __launch_bounds__(KZM_LANES) kzm_accumulate_kernel(KzmTables tb, const Fr* __restrict__ values, uint32_t slice_log,
                                                                   G1RSlot* __restrict__ partial) {
  const uint64_t j = (uint64_t)blockIdx.x >> slice_log;
  const uint32_t s = blockIdx.x & ((1u << slice_log) - 1u);
  const uint32_t nv = 1u << (tb.log_n - slice_log);
  const KzmDenseLoad ld = {values + (j << tb.log_n) + (uint64_t)s * nv, s * nv};
  const G1R sum = kzm_wave_sum(tb, nv, ld);
  if (!(threadIdx.x & 63u)) st_g1r(partial + blockIdx.x, sum);
}

__global__ void __launch_bounds__(KZM_LANES) kzm_sparse_kernel(KzmTables tb, const uint64_t* __restrict__ offsets,
                                                               const uint32_t* __restrict__ index, const Fr* __restrict__ deltas,
                                                               G1RSlot* __restrict__ partial) {
  const uint64_t a = offsets[blockIdx.x], b = offsets[blockIdx.x + 1];
  const KzmSparseLoad ld = {deltas + a, index + a};
  const G1R sum = kzm_wave_sum(tb, (uint32_t)(b - a), ld);
  if (!(threadIdx.x & 63u)) st_g1r(partial + blockIdx.x, sum);
}

__global__ void __launch_bounds__(KZM_LANES) kzm_compress_kernel(const G1RSlot* __restrict__ partial, uint32_t slices,
                                                                 const G1Affine* __restrict__ base, const int32_t* __restrict__ kind,
                                                                 uint64_t count, uint32_t* __restrict__ out48) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  G1R acc = ld_g1r(partial + j * slices);
  for (uint32_t s = 1; s < slices; ++s) acc = acc.add(ld_g1r(partial + j * slices + s));
  if (base && kind[j] == VDEC_OK) {
    const G1Affine a = ld_aff(base + j);
    acc = acc.add(G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)));
  }
  uint32_t w[12];
  g1r_compress48_words(acc, w);
#pragma unroll
  for (int k = 0; k < 12; ++k) out48[12 * j + k] = w[k];
}

// ---- launchers (kzg_many.hpp) -------------------------------------------------------------------------------------------------
int kzm_tables_fill(Ctx* c, const G1Affine* lag, uint32_t log_n, uint32_t window_bits, G1AffineR* table) {
  if (!lag || !table || kzm_check_build(true, log_n, window_bits) != PLONK_OK || !window_bits) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  const uint64_t n = 1ull << log_n, entries = kzm_table_entries(log_n, window_bits);
  const uint32_t W = kzm_windows(window_bits);
  G1RSlot* bases = nullptr;
  HIP_TRY(hipMalloc((void**)&bases, sizeof(G1RSlot) * n * W));
  hipLaunchKernelGGL(kzm_bases_kernel, dim3((uint32_t)((n + KZM_LANES - 1) / KZM_LANES)), dim3(KZM_LANES), 0, c->stream, lag, n, window_bits, W, bases);
  hipLaunchKernelGGL(kzm_entries_kernel, dim3((uint32_t)((entries + KZM_LANES - 1) / KZM_LANES)), dim3(KZM_LANES), 0, c->stream,
                     (const G1RSlot*)bases, entries, window_bits, table);
  int rc = hipGetLastError() == hipSuccess ? PLONK_OK : PLONK_ERR_HIP;
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = PLONK_ERR_HIP;
  (void)hipFree(bases);
  if (rc == PLONK_ERR_HIP) set_last_error("kzm_tables_fill", "a launch of the window-table build failed", __FILE__, __LINE__);
  return rc;
}

int kzm_scan(Ctx* c, const Fr* values, uint64_t total, unsigned long long* bad) {
  if (!total) return PLONK_OK;
  const uint32_t blocks = (uint32_t)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(kzm_scan_kernel, dim3(blocks), dim3(256), 0, c->stream, values, total, bad);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzm_accumulate(Ctx* c, const KzmTables& t, const Fr* values, uint64_t count, uint32_t slices, G1RSlot* partial) {
  uint32_t slice_log = 0;
  while ((1u << slice_log) < slices) ++slice_log;
  if (!count || !slices || (1u << slice_log) != slices || slice_log > t.log_n || count * slices > 0x7fffffffull)
    return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kzm_accumulate_kernel, dim3((uint32_t)(count * slices)), dim3(KZM_LANES), 0, c->stream, t, values, slice_log, partial);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzm_accumulate_sparse(Ctx* c, const KzmTables& t, const uint64_t* offsets, const uint32_t* index, const Fr* deltas, uint64_t count,
                          G1RSlot* partial) {
  if (!count || count > 0x7fffffffull) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kzm_sparse_kernel, dim3((uint32_t)count), dim3(KZM_LANES), 0, c->stream, t, offsets, index, deltas, partial);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzm_compress(Ctx* c, const G1RSlot* partial, uint32_t slices, const G1Affine* base, const int32_t* kind, uint64_t count, uint8_t* out48) {
  if (!count || !slices || ((uintptr_t)out48 & 3u) || (base && !kind)) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kzm_compress_kernel, dim3((uint32_t)((count + KZM_LANES - 1) / KZM_LANES)), dim3(KZM_LANES), 0, c->stream, partial, slices,
                     base, kind, count, (uint32_t*)out48);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the state a handle holds for these calls ------------------------------------------------------------------------------
struct KzmBufs {
  enum { PARTIAL, OUT48, META, OFFS, INDEX, DELTAS, BCOMP, BPTS, BKIND, NBUF };   // grow-only
};
struct KzgMany : KzmBufs, DevBufs<KzmBufs::NBUF> {
  Ctx* tab_ctx = nullptr;
  G1AffineR* table = nullptr;     // held against the context's table budget
  uint64_t table_bytes = 0;
  uint32_t window_bits = 0, windows = 0, built = 0;
  uint32_t force_slices = 0;      // test-only (kzm_test_force_slices)
  KzmPlan last = {};
  void drop_tables() {
    if (!table) return;
    (void)hipStreamSynchronize(tab_ctx->stream);
    (void)hipFree(table);
    tab_ctx->table_bytes -= table_bytes < tab_ctx->table_bytes ? table_bytes : tab_ctx->table_bytes;
    table = nullptr;
    table_bytes = 0;
    window_bits = windows = built = 0;
    last = {};
  }
  ~KzgMany() { drop_tables(); }
};

void kzm_release(KzgMany* many) { delete many; }
void kzm_test_force_slices(KzgDomain* d, uint32_t slices) { kzd_state(d->many)->force_slices = slices; }
bool kzm_handle_tables(const KzgDomain* d, KzmTables* out) {
  const KzgMany* m = d->many;
  if (!m || !m->table) return false;
  *out = KzmTables{m->table, d->log_n, m->window_bits, m->windows};
  return true;
}

namespace {

KzmTables tables_of(const KzgDomain* d, const KzgMany* m) { return KzmTables{m->table, d->log_n, m->window_bits, m->windows}; }

int tables_build_body(const char* api_fn, KzgDomain* d, KzgMany* m, uint32_t window_bits) {
  Ctx& c = *d->c;
  if (m->table && window_bits == m->window_bits) {
    m->built = 0;
    return PLONK_OK;
  }
  // `after`: what is left of the budget once the tables this build replaces are given back — the automatic width is chosen for
  // it.  `left`: what is left while the handle still holds them — the new tables are built BESIDE the old ones (a failed build
  // keeps them), so this is what they have to fit: the context never holds more than its budget, not even for a moment.
  const uint64_t left = c.cfg.table_budget > c.table_bytes ? c.cfg.table_budget - c.table_bytes : 0;
  const uint64_t after = left + m->table_bytes;
  if (!window_bits) {
    window_bits = kzm_auto_width(d->log_n, after);
    if (!window_bits) API_FAIL(PLONK_ERR_ARG, "invalid argument: no window width's tables fit what is left of the context's table budget");
    if (m->table && window_bits == m->window_bits) {
      m->built = 0;
      return PLONK_OK;
    }
  }
  const uint64_t bytes = kzm_table_bytes(d->log_n, window_bits);
  if (bytes > left) API_FAIL(PLONK_ERR_ARG, m->table && bytes <= after ? "invalid argument: no room in the context's table budget for the new window tables beside the ones they replace (drop those first)"
                                                                        : "invalid argument: the window tables do not fit what is left of the context's table budget");
  uint32_t built_points = 0;
  PTRY(kze_points_ready(d, &built_points));
  G1AffineR* t = nullptr;
  HIP_TRY(hipMalloc((void**)&t, bytes));
  const int rc = kzm_tables_fill(&c, kze_points(d), d->log_n, window_bits, t);
  if (rc != PLONK_OK) {
    (void)hipFree(t);
    return rc;
  }
  m->drop_tables();   // a build with another width replaces the tables
  m->tab_ctx = &c;
  m->table = t;
  m->table_bytes = bytes;
  m->window_bits = window_bits;
  m->windows = kzm_windows(window_bits);
  m->built = 1;
  c.table_bytes += bytes;
  return PLONK_OK;
}

int commit_body(KzgDomain* d, KzgMany* m, const void* values, uint64_t count, bool resident, void* out48, const KzmPlan& plan) {
  Ctx& c = *d->c;
  const uint64_t n = 1ull << d->log_n, per = plan.chunk_vectors;
  const KzmTables tb = tables_of(d, m);
  PTRY(m->need(KzgMany::PARTIAL, sizeof(G1RSlot) * per * plan.slices));
  if (resident) {
    for (uint64_t first = 0; first < count; first += per) {
      const uint64_t cnt = count - first < per ? count - first : per;
      PTRY(kzm_accumulate(&c, tb, (const Fr*)values + first * n, cnt, plan.slices, m->at<G1RSlot>(KzgMany::PARTIAL)));
      PTRY(kzm_compress(&c, m->at<G1RSlot>(KzgMany::PARTIAL), plan.slices, nullptr, nullptr, cnt, (uint8_t*)out48 + 48 * first));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    return PLONK_OK;
  }
  // the host form: chunk g + 1 is uploaded (copy stream) under the kernels of chunk g (main stream)
  PTRY(m->need(KzgMany::OUT48, 48 * per));
  Fr* stage[2];
  hipEvent_t up[2], done[2];
  PTRY(kzg_stage_reserve(&c, per * n, stage, up, done));
  HIP_TRY(hipStreamSynchronize(c.stream));   // the copy stream is not ordered behind what the main stream still runs
  uint64_t g = 0;
  for (uint64_t first = 0; first < count; first += per, ++g) {
    const int b = (int)(g & 1);
    const uint64_t cnt = count - first < per ? count - first : per;
    if (g >= 2) HIP_TRY(hipStreamWaitEvent(c.copy_stream, done[b], 0));
    HIP_TRY(hipMemcpyAsync(stage[b], (const uint64_t*)values + 4 * first * n, sizeof(Fr) * cnt * n, hipMemcpyHostToDevice, c.copy_stream));
    HIP_TRY(hipEventRecord(up[b], c.copy_stream));
    HIP_TRY(hipStreamWaitEvent(c.stream, up[b], 0));
    PTRY(kzm_accumulate(&c, tb, stage[b], cnt, plan.slices, m->at<G1RSlot>(KzgMany::PARTIAL)));
    HIP_TRY(hipEventRecord(done[b], c.stream));
    PTRY(kzm_compress(&c, m->at<G1RSlot>(KzgMany::PARTIAL), plan.slices, nullptr, nullptr, cnt, m->at<uint8_t>(KzgMany::OUT48)));
    HIP_TRY(hipMemcpyAsync((uint8_t*)out48 + 48 * first, m->p[KzgMany::OUT48], 48 * cnt, hipMemcpyDeviceToHost, c.stream));
  }
  HIP_TRY(hipStreamSynchronize(c.stream));
  return PLONK_OK;
}

// *bad != 0: one of the resident values is not a canonical residue; returns with the stream synchronised
int scan_resident(Ctx* c, KzgMany* m, const Fr* values, uint64_t total, unsigned long long* bad) {
  PTRY(m->need(KzgMany::META, 8));
  *bad = 0;
  HIP_TRY(hipMemcpyAsync(m->p[KzgMany::META], bad, 8, hipMemcpyHostToDevice, c->stream));
  PTRY(kzm_scan(c, values, total, m->at<unsigned long long>(KzgMany::META)));
  HIP_TRY(hipMemcpyAsync(bad, m->p[KzgMany::META], 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PLONK_OK;
}

int commit_impl(const char* api_fn, plonk_kzg_domain* dom, const void* values, uint64_t count, bool resident, void* out48) {
  if (kzm_check_commit(dom != nullptr, values != nullptr, out48 != nullptr, count) != PLONK_OK)
    API_FAIL(PLONK_ERR_ARG, count > KZM_MAX_COUNT ? "invalid argument: at most 2^24 vectors per call" : "invalid argument: a required pointer is NULL");
  if (resident && count && (((uintptr_t)values & 15u) || ((uintptr_t)out48 & 3u))) API_FAIL(PLONK_ERR_ARG, "invalid argument: values_dev must be 16-byte and commitments48_dev 4-byte aligned");
  KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_WORK);
  KzgMany* m = d->many;
  if (!m || !m->table) API_FAIL(PLONK_ERR_STATE, "the handle holds no many-vector tables (plonk_kzg_many_tables_build)");
  const uint64_t n = 1ull << d->log_n;
  const KzmPlan plan = kzm_plan(d->log_n, m->window_bits, count, d->ws_cap, !resident, m->force_slices);
  if (!count) {
    m->last = plan;
    return PLONK_OK;
  }
  // before anything is queued for the result or written
  if (!resident) {
    Fr t;
    for (uint64_t k = 0; k < count * n; ++k)
      if (!kzg_fr_load((const uint64_t*)values + 4 * k, &t)) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
  } else {
    unsigned long long bad = 0;
    PTRY(kzd_drained(d->c, scan_resident(d->c, m, (const Fr*)values, count * n, &bad)));
    if (bad) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
  }
  PTRY(kzd_drained(d->c, commit_body(d, m, values, count, resident, out48, plan)));
  m->last = plan;
  return PLONK_OK;
}

int update_body(KzgDomain* d, KzgMany* m, const uint8_t* base48, const uint64_t* offsets, const uint32_t* index, const uint64_t* deltas,
                uint64_t count, uint8_t* out48, const KzmPlan& plan, const char* api_fn) {
  Ctx& c = *d->c;
  const KzmTables tb = tables_of(d, m);
  // the bases, decoded and subgroup-checked once and resident for the call: a bad one refuses before anything is written
  if (base48) {
    PTRY(m->need(KzgMany::BCOMP, 48 * count));
    PTRY(m->need(KzgMany::BPTS, sizeof(G1Affine) * count));
    PTRY(m->need(KzgMany::BKIND, 4 * count));
    std::vector<int32_t> st;
    for (uint64_t first = 0; first < count; first += 1u << 16) {
      const uint32_t cnt = (uint32_t)(count - first < (1u << 16) ? count - first : (1u << 16));
      PTRY(decode_points(&c, base48 + 48 * first, cnt, m->at<uint8_t>(KzgMany::BCOMP) + 48 * first, m->at<G1Affine>(KzgMany::BPTS) + first,
                         m->at<int32_t>(KzgMany::BKIND) + first, &st));
      for (uint32_t k = 0; k < cnt; ++k)
        if (st[k] == VDEC_BAD) API_FAIL(PLONK_ERR_POINT, "a base is not a valid compressed point of G1");
    }
  }
  uint64_t most_terms = 0;
  for (uint64_t first = 0; first < count;) {
    const uint64_t k = kzm_sparse_chunk(offsets, count, first, d->ws_cap);
    if (offsets[first + k] - offsets[first] > most_terms) most_terms = offsets[first + k] - offsets[first];
    first += k;
  }
  PTRY(m->need(KzgMany::PARTIAL, sizeof(G1RSlot) * plan.chunk_vectors));
  PTRY(m->need(KzgMany::OUT48, 48 * plan.chunk_vectors));
  PTRY(m->need(KzgMany::OFFS, 8 * (plan.chunk_vectors + 1)));
  PTRY(m->need(KzgMany::INDEX, 4 * most_terms));
  PTRY(m->need(KzgMany::DELTAS, sizeof(Fr) * most_terms));
  std::vector<uint64_t> rel;
  for (uint64_t first = 0; first < count;) {
    const uint64_t k = kzm_sparse_chunk(offsets, count, first, d->ws_cap);
    const uint64_t t0 = offsets[first], terms = offsets[first + k] - t0;
    rel.resize(k + 1);
    for (uint64_t j = 0; j <= k; ++j) rel[j] = offsets[first + j] - t0;
    HIP_TRY(hipMemcpyAsync(m->p[KzgMany::OFFS], rel.data(), 8 * (k + 1), hipMemcpyHostToDevice, c.stream));
    if (terms) {
      HIP_TRY(hipMemcpyAsync(m->p[KzgMany::INDEX], index + t0, 4 * terms, hipMemcpyHostToDevice, c.stream));
      HIP_TRY(hipMemcpyAsync(m->p[KzgMany::DELTAS], deltas + 4 * t0, sizeof(Fr) * terms, hipMemcpyHostToDevice, c.stream));
    }
    PTRY(kzm_accumulate_sparse(&c, tb, m->at<uint64_t>(KzgMany::OFFS), m->at<uint32_t>(KzgMany::INDEX), m->at<Fr>(KzgMany::DELTAS), k,
                               m->at<G1RSlot>(KzgMany::PARTIAL)));
    PTRY(kzm_compress(&c, m->at<G1RSlot>(KzgMany::PARTIAL), 1, base48 ? m->at<G1Affine>(KzgMany::BPTS) + first : nullptr,
                      base48 ? m->at<int32_t>(KzgMany::BKIND) + first : nullptr, k, m->at<uint8_t>(KzgMany::OUT48)));
    HIP_TRY(hipMemcpyAsync(out48 + 48 * first, m->p[KzgMany::OUT48], 48 * k, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));   // `rel` and the workspace are reused by the next chunk
    first += k;
  }
  return PLONK_OK;
}

}  // namespace

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_kzg_many_tables_build(plonk_kzg_domain* dom, uint32_t window_bits) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  if (kzm_check_build(true, d->log_n, window_bits) != PLONK_OK)
    API_FAIL(PLONK_ERR_ARG, d->log_n > KZM_LOG_N_MAX ? "invalid argument: many-vector tables are for domains of at most 2^12 values"
                                                      : "invalid argument: window_bits must be 0 or 2 .. 8");
  KZD_ENTER(d, api_fn, KZD_WORK);
  return kzd_drained(d->c, tables_build_body(api_fn, d, kzd_state(d->many), window_bits));
  });
}

int plonk_kzg_many_tables_drop(plonk_kzg_domain* dom) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_SET_DEVICE);
  if (d->many) d->many->drop_tables();
  return PLONK_OK;
  });
}

int plonk_kzg_commit_many(plonk_kzg_domain* dom, const uint64_t* values, uint64_t count, uint8_t* commitments48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int { return plonk::commit_impl(api_fn, dom, values, count, false, commitments48); });
}

int plonk_kzg_commit_many_dev(plonk_kzg_domain* dom, const void* values_dev, uint64_t count, void* commitments48_dev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int { return plonk::commit_impl(api_fn, dom, values_dev, count, true, commitments48_dev); });
}

int plonk_kzg_update_many(plonk_kzg_domain* dom, const uint8_t* base48, const uint64_t* offsets, const uint32_t* index, const uint64_t* deltas,
                          uint64_t count, uint8_t* commitments48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  if (kzm_check_update(true, offsets, index, deltas != nullptr, commitments48 != nullptr, count, d->log_n) != PLONK_OK)
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a NULL pointer, a count or total above its cap, offsets that do not start at 0 or decrease, or an index >= n");
  if (count) {
    Fr t;
    for (uint64_t k = 0; k < offsets[count]; ++k)
      if (!kzg_fr_load(deltas + 4 * k, &t)) API_FAIL(PLONK_ERR_DATA, "a delta is not a canonical residue");
  }
  KZD_ENTER(d, api_fn, KZD_WORK);
  KzgMany* m = d->many;
  if (!m || !m->table) API_FAIL(PLONK_ERR_STATE, "the handle holds no many-vector tables (plonk_kzg_many_tables_build)");
  const KzmPlan plan = kzm_sparse_plan(d->log_n, m->window_bits, offsets, count, d->ws_cap);
  if (count) PTRY(kzd_drained(d->c, update_body(d, m, base48, offsets, index, deltas, count, commitments48, plan, api_fn)));
  m->last = plan;
  return PLONK_OK;
  });
}

int plonk_kzg_many_last(plonk_kzg_domain* dom, plonk_kzg_many_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, 0);
  const KzgMany* m = d->many;
  plonk_kzg_many_info info = {};
  info.log_n = d->log_n;
  if (m && m->table) {
    info.window_bits = m->window_bits;
    info.windows = m->windows;
    info.built = m->built;
    info.table_bytes = m->table_bytes;
    if (m->last.window_bits) {
      info.count = m->last.count;
      info.terms = m->last.terms;
      info.chunks = m->last.chunks;
      info.chunk_vectors = m->last.chunk_vectors;
      info.slices = m->last.slices;
      info.additions = m->last.additions;
    }
  }
  *out = info;
  return PLONK_OK;
  });
}

}  // extern "C"
