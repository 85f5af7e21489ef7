// KZG10 cell proofs: a polynomial opened on every coset of its domain, one 48-byte proof per cell of l values
// (Feist-Khovratovich section 3).  The derivation, the index maps and the plan are in kzg_cells_core.hpp; DESIGN.md section 16
// has the resources and the measurements.  The group transforms, the extraction and the finishing kernel are those of
// kzg_domain.hip at size 2r and r; new here:
//
//   kzc_load_kernel       once per (handle, cell size): a^(u)_v = s_(u + l v) from row 0 of the commit-key tables, l x 2r slots
//   kzc_gather_kernel     g^(u)_t = f_(u + l (r-1-t)): the scalar side
//   kzc_ntt_kernel        G^(u) = NTT_2r(g^(u)) for 2r <= 2048: one workgroup per (u, polynomial), the vector in LDS, so that the
//                         l transforms of a polynomial are ONE launch (larger sizes go through ntt_device, one call per u)
//   kzc_transpose_kernel  the cell-major order of the ordinary size-n forward transform
//   kzc_mulacc_kernel     lane (p, s): the l / S terms [G^(u)_rev(p) / 2r] A^(u)_p of slice s, one after the other through the
//                         split double-and-add, added into an accumulator that stays in registers; ONE partial stored
//   kzc_reduce_kernel     the S partials of a position, added into the slot the inverse transform reads
// Every addition is the complete law (G1R::add).  A zero scalar or an identity operand multiplies nothing.  One wave per
// workgroup; a wave's 64 lanes are 64 consecutive positions p, so its loads of A^(u) and its stores of the partials touch 64
// consecutive 256-byte slots.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "kzg_core.hpp"
#include "kzg_handle.hpp"
#include "kzg_cells.hpp"
#include "devmem.cuh"

namespace plonk {

__global__ void __launch_bounds__(KZD_LANES) kzc_load_kernel(const G1AffineR* __restrict__ row0, uint32_t log_cell, uint32_t log_r,
                                                             G1RSlot* __restrict__ table) {
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (2ull << (log_cell + log_r))) return;
  const uint64_t u = idx >> (log_r + 1), v = idx & ((2ull << log_r) - 1);
  const uint64_t src = kzc_a_src(log_cell, 1ull << log_r, u, v);
  st_g1r(table + idx, src == KZD_NONE ? G1R::identity() : G1R::from_affine(ld_f28(&row0[src].x), ld_f28(&row0[src].y)));
}

__global__ void kzc_gather_kernel(const Fr* __restrict__ f, uint32_t log_cell, uint32_t log_r, Fr* __restrict__ g) {
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = 1ull << (log_cell + log_r);
  if (idx >= 2 * n) return;
  const uint64_t u = idx >> (log_r + 1), t = idx & ((2ull << log_r) - 1);
  const uint64_t src = kzc_g_src(log_cell, 1ull << log_r, u, t);
  st_fr(g + (uint64_t)blockIdx.y * 2 * n + idx, src == KZD_NONE ? Fr::zero() : ld_fr(f + (uint64_t)blockIdx.y * n + src));
}

// decimation in time on the bit-reversed vector: natural order out, as ntt_device leaves it.  tw[e] = w^e, e < size / 2, w the
// generator of the size-2^log_size domain; dynamic LDS: 32 B per element
__global__ void __launch_bounds__(KZC_NTT_LANES) kzc_ntt_kernel(Fr* __restrict__ g, uint32_t log_size, const Fr* __restrict__ tw) {
  extern __shared__ uint4 kzc_ntt_lds[];
  Fr* sh = reinterpret_cast<Fr*>(kzc_ntt_lds);
  const uint32_t size = 1u << log_size;
  Fr* v = g + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * size;
  for (uint32_t i = threadIdx.x; i < size; i += KZC_NTT_LANES) sh[kzd_rev(i, log_size)] = ld_fr(v + i);
  __syncthreads();
  for (uint32_t s = 0; s < log_size; ++s) {
    const uint32_t half = 1u << s;
    for (uint32_t t = threadIdx.x; t < size / 2; t += KZC_NTT_LANES) {
      const uint32_t j = t & (half - 1), lo = ((t - j) << 1) + j, hi = lo + half;
      Fr b = sh[hi];
      if (j) b = b * ld_fr(tw + ((uint64_t)j << (log_size - 1 - s)));
      const Fr a = sh[lo];
      sh[lo] = a + b;
      sh[hi] = a - b;
    }
    __syncthreads();
  }
  for (uint32_t i = threadIdx.x; i < size; i += KZC_NTT_LANES) st_fr(v + i, sh[i]);
}

__global__ void kzc_transpose_kernel(const Fr* __restrict__ evals, uint32_t log_n, uint32_t log_cell, Fr* __restrict__ cells) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> log_n) return;
  const uint64_t base = (uint64_t)blockIdx.y << log_n;
  st_fr(cells + base + kzc_cell_dst(log_n, log_cell, i), ld_fr(evals + base + i));
}

// grid = (2r / 64, S, polynomial); `terms` = l / S consecutive u per lane
__global__ void __launch_bounds__(KZD_LANES) kzc_mulacc_kernel(const G1RSlot* __restrict__ table, const Fr* __restrict__ G, uint64_t g_stride,
                                                               G1RSlot* __restrict__ ws, uint64_t stride, uint32_t log_r, uint64_t terms,
                                                               Fr scale) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t size = 2ull << log_r;
  if (p >= size) return;
  const uint64_t first = (uint64_t)blockIdx.y * terms;
  const Fr* g = G + (uint64_t)blockIdx.z * g_stride + first * size + kzd_rev(p, log_r + 1);
  const G1RSlot* a = table + first * size + p;
  G1R acc = G1R::identity();
  for (uint64_t k = 0; k < terms; ++k, g += size, a += size) {
    const Fr s = (ld_fr(g) * scale).from_mont();
    if (s.is_zero()) continue;
    const G1R t = kzd_mul_split(ld_g1r(a), glv_split(s.l));
    if (!t.is_identity()) acc = acc.add(t);
  }
  st_g1r(ws + (uint64_t)blockIdx.z * stride + kzc_partial_slot(1ull << log_r, blockIdx.y, p), acc);
}

__global__ void __launch_bounds__(KZD_LANES) kzc_reduce_kernel(G1RSlot* __restrict__ ws, uint64_t stride, uint32_t log_r, uint64_t slices) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t r = 1ull << log_r;
  if (p >= 2 * r) return;
  G1RSlot* base = ws + (uint64_t)blockIdx.y * stride;
  G1R acc = ld_g1r(base + p);
  for (uint64_t s = 1; s < slices; ++s) acc = acc.add(ld_g1r(base + kzc_partial_slot(r, s, p)));
  st_g1r(base + p, acc);
}

// ---- launchers (kzg_cells.hpp) ---------------------------------------------------------------------------------------------
static dim3 kzc_grid(uint64_t lanes, uint32_t y, uint32_t z = 1) { return dim3((uint32_t)((lanes + KZD_LANES - 1) / KZD_LANES), y, z); }

int kzc_table_build(Ctx* c, uint32_t log_n, uint32_t log_cell, const GlvScalar* tw, uint32_t tw_log, void* table) {
  if (kzc_check_cell(log_n, log_cell) || !c->srs_table || c->srs_n < (1ull << log_n)) return PLONK_ERR_ARG;
  const uint32_t log_r = log_n - log_cell;
  const uint64_t l = 1ull << log_cell, size = 2ull << log_r;
  hipLaunchKernelGGL(kzc_load_kernel, kzc_grid(2ull << log_n, 1), dim3(KZD_LANES), 0, c->stream, (const G1AffineR*)c->srs_table, log_cell,
                     log_r, (G1RSlot*)table);
  HIP_TRY(hipGetLastError());
  for (uint64_t u = 0; u < l; u += KZD_MAX_CHUNK) {   // grid.y of the batched transform
    const uint32_t cnt = (uint32_t)(l - u < KZD_MAX_CHUNK ? l - u : KZD_MAX_CHUNK);
    PTRY(kzd_transform(c, (G1RSlot*)table + u * size, size, log_r + 1, cnt, false, tw, tw_log, nullptr, nullptr));
  }
  return PLONK_OK;
}

int kzc_gather(Ctx* c, const Fr* f, uint32_t log_n, uint32_t log_cell, uint32_t batch, Fr* g) {
  if (kzc_check_cell(log_n, log_cell) || !batch || batch > KZD_MAX_CHUNK) return PLONK_ERR_ARG;
  hipLaunchKernelGGL(kzc_gather_kernel, dim3((uint32_t)(((2ull << log_n) + 255) / 256), batch), dim3(256), 0, c->stream, f, log_cell,
                     log_n - log_cell, g);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzc_ntt(Ctx* c, Fr* g, uint32_t log_size, uint64_t vectors, uint32_t batch, const Fr* tw) {
  if (log_size < 1 || log_size > KZC_NTT_MAX_LOG || !vectors || vectors > (1ull << KZD_MAX_LOG) || !batch || batch > KZD_MAX_CHUNK) return PLONK_ERR_ARG;
  hipLaunchKernelGGL(kzc_ntt_kernel, dim3((uint32_t)vectors, batch), dim3(KZC_NTT_LANES), sizeof(Fr) << log_size, c->stream, g, log_size, tw);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzc_transpose(Ctx* c, const Fr* evals, uint32_t log_n, uint32_t log_cell, uint32_t batch, Fr* cells) {
  if (kzc_check_cell(log_n, log_cell) || !batch || batch > KZD_MAX_CHUNK) return PLONK_ERR_ARG;
  hipLaunchKernelGGL(kzc_transpose_kernel, dim3((uint32_t)(((1ull << log_n) + 255) / 256), batch), dim3(256), 0, c->stream, evals, log_n,
                     log_cell, cells);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzc_mulacc(Ctx* c, const void* table, const Fr* G, uint64_t g_stride, void* ws, uint64_t stride, uint32_t log_n, uint32_t log_cell,
               uint64_t slices, uint32_t batch, const Fr& scale) {
  const uint64_t l = 1ull << log_cell;
  if (kzc_check_cell(log_n, log_cell) || !batch || batch > KZD_MAX_CHUNK || !slices || slices > l || (slices & (slices - 1)) ||
      slices > 65535 || stride < slices * (2ull << (log_n - log_cell)))
    return PLONK_ERR_ARG;
  const uint32_t log_r = log_n - log_cell;
  hipLaunchKernelGGL(kzc_mulacc_kernel, kzc_grid(2ull << log_r, (uint32_t)slices, batch), dim3(KZD_LANES), 0, c->stream,
                     (const G1RSlot*)table, G, g_stride, (G1RSlot*)ws, stride, log_r, l / slices, scale);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzc_reduce(Ctx* c, void* ws, uint64_t stride, uint32_t log_r, uint64_t slices, uint32_t batch) {
  if (!batch || batch > KZD_MAX_CHUNK || !slices || stride < slices * (2ull << log_r)) return PLONK_ERR_ARG;
  if (slices == 1) return PLONK_OK;   // the partial of slice 0 is the sum
  hipLaunchKernelGGL(kzc_reduce_kernel, kzc_grid(2ull << log_r, batch), dim3(KZD_LANES), 0, c->stream, (G1RSlot*)ws, stride, log_r, slices);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the state a handle holds for these calls ------------------------------------------------------------------------------
struct KzcBufs {
  enum { WS, F, G, EVALS, CELLS, TMP, OUT48, DESC, META, NBUF };   // grow-only
};
struct KzgCells : KzcBufs, DevBufs<KzcBufs::NBUF> {
  G1RSlot* table[KZD_MAX_LOG + 1] = {};   // by log_cell: built by the first call with that cell size
  Fr* ntt_tw[KZD_MAX_LOG + 1] = {};       // by log_cell: w_(2r)^e, e < r, where kzc_ntt_kernel takes the size
  uint64_t table_bytes = 0;
  uint64_t forced_slices = 0;
  plonk_kzg_cells_info last = {};
  ~KzgCells() {
    for (G1RSlot* t : table) (void)hipFree(t);
    for (Fr* t : ntt_tw) (void)hipFree(t);
  }
};

void kzc_release(KzgCells* cells) { delete cells; }

namespace {

int table_ready(const KzgDomain* d, KzgCells* e, uint32_t log_cell, uint32_t* built) {
  if (e->table[log_cell]) return PLONK_OK;
  const uint64_t bytes = (2ull << d->log_n) * KZD_SLOT_BYTES;
  const uint32_t log_size = d->log_n - log_cell + 1;
  if (log_size <= KZC_NTT_MAX_LOG && !e->ntt_tw[log_cell]) {   // the powers the scalar transform reads: at most 32 KiB
    std::vector<Fr> pw(1ull << (log_size - 1));
    const Fr w = fr_domain_root(log_size);
    Fr x = Fr::one();
    for (Fr& y : pw) {
      y = x;
      x = x * w;
    }
    Fr* tw_dev = nullptr;
    HIP_TRY(hipMalloc((void**)&tw_dev, sizeof(Fr) * pw.size()));
    if (hipMemcpy(tw_dev, pw.data(), sizeof(Fr) * pw.size(), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(tw_dev);
      return PLONK_ERR_HIP;
    }
    e->ntt_tw[log_cell] = tw_dev;
  }
  G1RSlot* t = nullptr;
  HIP_TRY(hipMalloc((void**)&t, bytes));
  int rc = kzc_table_build(d->c, d->log_n, log_cell, d->tw, d->log_n + 1, t);
  if (hipStreamSynchronize(d->c->stream) != hipSuccess && rc == PLONK_OK) rc = PLONK_ERR_HIP;
  if (rc != PLONK_OK) {
    (void)hipFree(t);
    return rc;
  }
  e->table[log_cell] = t;
  e->table_bytes += bytes;
  *built = 1;
  return PLONK_OK;
}

int cells_body(const KzgDomain* d, KzgCells* e, uint32_t log_cell, const void* const* polys, const uint64_t* trimmed, uint64_t count,
               void* cells, void* proofs48, void* commitments48) {
  Ctx& c = *d->c;
  const uint32_t L = d->log_n, log_r = L - log_cell;
  const uint64_t n = 1ull << L, l = 1ull << log_cell, r = 1ull << log_r, size = 2 * r;
  const KzcPlan plan = kzc_plan(L, log_cell, count, d->ws_cap, e->forced_slices);
  const uint64_t chunk = plan.chunk_polys, stride = plan.slices * size;
  plonk_kzg_cells_info info = {};
  info.log_n = L;
  info.log_cell = log_cell;
  info.count = count;
  info.slices = plan.slices;
  info.chunk_polys = chunk;
  info.workspace_bytes = plan.ws_bytes;
  PTRY(table_ready(d, e, log_cell, &info.built_table));
  PTRY(e->need(KzgCells::WS, plan.ws_bytes));
  PTRY(e->need(KzgCells::F, sizeof(Fr) * n * chunk));
  PTRY(e->need(KzgCells::G, sizeof(Fr) * 2 * n * chunk));
  PTRY(e->need(KzgCells::EVALS, sizeof(Fr) * n * chunk));
  PTRY(e->need(KzgCells::CELLS, sizeof(Fr) * n * chunk));
  PTRY(e->need(KzgCells::TMP, sizeof(Fr) * 2 * n));
  PTRY(e->need(KzgCells::OUT48, 48 * r * chunk));
  if (commitments48) PTRY(msm_reserve(&c, n));
  G1RSlot* ws = e->at<G1RSlot>(KzgCells::WS);
  Fr* f = e->at<Fr>(KzgCells::F);
  Fr* g = e->at<Fr>(KzgCells::G);
  Fr* ev = e->at<Fr>(KzgCells::EVALS);
  Fr* cl = e->at<Fr>(KzgCells::CELLS);
  Fr* tmp = e->at<Fr>(KzgCells::TMP);
  uint8_t* out48 = e->at<uint8_t>(KzgCells::OUT48);
  const Fr size_inv = Fr::from_u64(size).inv();
  std::vector<uint8_t> comm;
  for (uint64_t first = 0; first < count; first += chunk) {
    const uint32_t cnt = (uint32_t)(count - first < chunk ? count - first : chunk);
    PTRY(kzd_stage(&c, f, n, polys + first, trimmed + first, cnt));
    // cell values: the ordinary forward transform in cell-major order; G^(u) = NTT_2r of the gathered coefficients
    PTRY(kzc_gather(&c, f, L, log_cell, cnt, g));
    for (uint32_t b = 0; b < cnt; ++b) {
      PTRY(ntt_device(&c, f + (uint64_t)b * n, ev + (uint64_t)b * n, tmp, L, false, false, n));
      for (uint64_t u = 0; u < l && log_r + 1 > KZC_NTT_MAX_LOG; ++u) {
        Fr* gu = g + (uint64_t)b * 2 * n + u * size;
        PTRY(ntt_device(&c, gu, gu, tmp, log_r + 1, false, false, size));
      }
    }
    if (log_r + 1 <= KZC_NTT_MAX_LOG) PTRY(kzc_ntt(&c, g, log_r + 1, l, cnt, e->ntt_tw[log_cell]));
    PTRY(kzc_transpose(&c, ev, L, log_cell, cnt, cl));
    PTRY(kzc_mulacc(&c, e->table[log_cell], g, 2 * n, ws, stride, L, log_cell, plan.slices, cnt, size_inv));
    info.scalar_muls += 2 * n * cnt;
    PTRY(kzc_reduce(&c, ws, stride, log_r, plan.slices, cnt));
    PTRY(kzd_witnesses(&c, ws, stride, log_r, cnt, d->tw, L + 1, &info.stage_launches, &info.scalar_muls, out48));
    if (cells) HIP_TRY(hipMemcpyAsync((uint8_t*)cells + sizeof(Fr) * n * first, cl, sizeof(Fr) * n * cnt, hipMemcpyDefault, c.stream));
    HIP_TRY(hipMemcpyAsync((uint8_t*)proofs48 + 48 * r * first, out48, 48 * r * cnt, hipMemcpyDefault, c.stream));
    if (commitments48) PTRY(kzd_commit(&c, f, n, trimmed + first, cnt, comm, (uint8_t*)commitments48 + 48 * first));
    HIP_TRY(hipStreamSynchronize(c.stream));   // the chunk's buffers are reused by the next one
    ++info.chunks;
  }
  info.table_bytes = e->table_bytes;
  e->last = info;
  return PLONK_OK;
}

int cells_impl(const char* api_fn, plonk_kzg_domain* dom, uint32_t log_cell, const void* const* polys, const uint64_t* lens, uint64_t count,
               void* cells, void* proofs48, void* commitments48, bool resident) {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  if (kzc_check_cell(d->log_n, log_cell)) API_FAIL(PLONK_ERR_ARG, "invalid argument: log_cell must be in [1, log_n - 1]");
  if (count > KZD_MAX_COUNT) API_FAIL(PLONK_ERR_ARG, "invalid argument: at most 65536 polynomials per call");
  if (count && (!polys || !lens || !cells || !proofs48)) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  for (uint64_t i = 0; i < count; ++i)
    if (lens[i] && !polys[i]) API_FAIL(PLONK_ERR_ARG, "invalid argument: polys[i] is NULL with lens[i] > 0");
  KZD_ENTER(d, api_fn, KZD_WORK);
  if (!count) return PLONK_OK;
  KzgCells* e = kzd_state(d->cells);
  std::vector<uint64_t> trimmed(count);
  PTRY(kzd_lengths_on(api_fn, d->c, e, d->log_n, polys, lens, count, resident, trimmed.data()));
  return kzd_drained(d->c, cells_body(d, e, log_cell, polys, trimmed.data(), count, cells, proofs48, commitments48));
}

}  // namespace

int kzc_open_resident(KzgDomain* d, uint32_t log_cell, const void* const* polys_dev, const uint64_t* trimmed, uint64_t count, void* cells,
                      void* proofs48, void* commitments48, uint32_t* built_table) {
  KzgCells* e = kzd_state(d->cells);
  PTRY(cells_body(d, e, log_cell, polys_dev, trimmed, count, cells, proofs48, commitments48));
  if (e->last.built_table) *built_table = 1;
  return PLONK_OK;
}

void kzc_set_slices(plonk_kzg_domain* dom, uint64_t slices) {
  std::lock_guard<std::mutex> lk(dom->d->c->mu);
  kzd_state(dom->d->cells)->forced_slices = slices;
}

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_kzg_open_cells(plonk_kzg_domain* dom, uint32_t log_cell, const uint64_t* const* polys, const uint64_t* lens, uint64_t count,
                         uint64_t* cells, uint8_t* proofs48, uint8_t* commitments48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::cells_impl(api_fn, dom, log_cell, (const void* const*)polys, lens, count, cells, proofs48, commitments48, false);
  });
}

int plonk_kzg_open_cells_dev(plonk_kzg_domain* dom, uint32_t log_cell, const void* const* polys_dev, const uint64_t* lens, uint64_t count,
                             void* cells_dev, void* proofs48_dev, void* commitments48_dev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::cells_impl(api_fn, dom, log_cell, polys_dev, lens, count, cells_dev, proofs48_dev, commitments48_dev, true);
  });
}

int plonk_kzg_cell_points(plonk_kzg_domain* dom, uint32_t log_cell, uint64_t* x, uint64_t* shift) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !x) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgDomain* d = dom->d;
  if (kzc_check_cell(d->log_n, log_cell)) API_FAIL(PLONK_ERR_ARG, "invalid argument: log_cell must be in [1, log_n - 1]");
  KZD_ENTER(d, api_fn, KZD_KEY);
  const Fr w = fr_domain_root(d->log_n), phi = fr_domain_root(d->log_n - log_cell);
  Fr a = Fr::one(), b = Fr::one();
  for (uint64_t k = 0; k < (1ull << (d->log_n - log_cell)); ++k) {
    memcpy(x + 4 * k, a.l, 32);
    if (shift) memcpy(shift + 4 * k, b.l, 32);
    a = a * phi;
    b = b * w;
  }
  return PLONK_OK;
  });
}

int plonk_kzg_cells_last(plonk_kzg_domain* dom, plonk_kzg_cells_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_KEY);
  const KzgCells* e = d->cells;
  plonk_kzg_cells_info info = {};
  if (e) {
    info = e->last;
    info.table_bytes = e->table_bytes;
  }
  info.log_n = d->log_n;
  *out = info;
  return PLONK_OK;
  });
}

}  // extern "C"
