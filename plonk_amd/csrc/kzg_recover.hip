// KZG10 cell recovery: the coefficients of a polynomial, all of its cells and their proofs from a subset of the cells.  The
// mathematics, the index maps, the checks and the plan are in kzg_recover_core.hpp; DESIGN.md section 18 has the resources
// and the measurements.  The transforms are ntt_device's (inverse; forward on the coset of 7; inverse there; forward), the
// inversion of the r coset values of Z_r is poly_batch_inverse, the cell-major order is kzc_transpose, proofs and commitments
// come through the body of plonk_kzg_open_cells (kzc_open_resident); new here:
//
//   kzr_vanish_kernel    one wave per point p < 2r — phi^p (p < r) or 7^l phi^(p - r): the product over the missing cells of
//                        (point - phi^m), 64 slices of every 64th factor combined in LDS: Zdom[r] (zero at the missing cells)
//                        and Zcoset[r].  (One lane per point with the whole chain was built first and measured: 0.72 ms at
//                        512 factors, 4.4 times the four transforms of a 2^16 polynomial)
//   kzr_scatter_kernel   position k + r j of the natural-order array = values[slot(k)][j] * Zdom[k], zero for a missing cell:
//                        un-transpose, scaling and zero fill in one pass, every value read once
//   kzr_divide_kernel    element i times Zcoset^-1[i mod r]
//   kzr_tail_kernel      per polynomial: is any coefficient in [max_len, n) non-zero?  Lanes that find one store 1 into the
//                        polynomial's flag (the same value from every lane); nothing is added up, no atomics
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "poly.hpp"
#include "devmem.cuh"
#include "kzg_core.hpp"
#include "kzg_handle.hpp"
#include "kzg_cells.hpp"
#include "kzg_recover.hpp"

namespace plonk {

static constexpr uint32_t KZR_LANES = 256;
static constexpr uint32_t KZR_TAIL_BLOCKS = 1024;

// one wave per point (grid = 2r): lane s multiplies the factors m = s, s + 64, ... of its slice, the 64 partial products are
// multiplied pairwise in LDS.  Field products are exact, so the grouping does not show in the bytes.
__global__ void __launch_bounds__(KZR_VANISH_SLICES) kzr_vanish_kernel(const Fr* __restrict__ pw, const uint32_t* __restrict__ miss,
                                                                       uint32_t nmiss, uint32_t log_r, Fr shift, Fr* __restrict__ zdom,
                                                                       Fr* __restrict__ zcoset) {
  __shared__ Fr sh[KZR_VANISH_SLICES];
  const uint64_t p = blockIdx.x;
  const uint32_t s = threadIdx.x;
  const uint64_t e = kzr_point_exp(log_r, p);
  const bool coset = kzr_point_on_coset(log_r, p);
  Fr pt = ld_fr(pw + e);
  if (coset) pt = pt * shift;
  Fr acc = Fr::one();
  for (uint32_t m = kzr_vanish_first(s); m < nmiss; m += KZR_VANISH_SLICES) acc = acc * (pt - ld_fr(pw + miss[m]));
  sh[s] = acc;
  __syncthreads();
  for (uint32_t h = KZR_VANISH_SLICES / 2; h; h >>= 1) {
    if (s < h) sh[s] = sh[s] * sh[s + h];
    __syncthreads();
  }
  if (!s) st_fr((coset ? zcoset : zdom) + e, sh[0]);
}

__global__ void __launch_bounds__(KZR_LANES) kzr_scatter_kernel(const Fr* const* __restrict__ vecs, const int32_t* __restrict__ slot,
                                                                const Fr* __restrict__ zdom, uint32_t log_n, uint32_t log_cell,
                                                                Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> log_n) return;
  const uint64_t src = kzr_scatter_src(log_n, log_cell, i, slot);
  Fr v = Fr::zero();
  if (src != KZD_NONE) v = ld_fr(vecs[blockIdx.y] + src) * ld_fr(zdom + kzr_period(log_n, log_cell, i));
  st_fr(out + ((uint64_t)blockIdx.y << log_n) + i, v);
}

__global__ void __launch_bounds__(KZR_LANES) kzr_divide_kernel(Fr* __restrict__ v, const Fr* __restrict__ zinv, uint32_t log_n,
                                                               uint32_t log_cell) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> log_n) return;
  Fr* p = v + ((uint64_t)blockIdx.y << log_n) + i;
  st_fr(p, ld_fr(p) * ld_fr(zinv + kzr_period(log_n, log_cell, i)));
}

__global__ void __launch_bounds__(KZR_LANES) kzr_tail_kernel(const Fr* __restrict__ coeffs, uint32_t log_n, uint64_t first,
                                                             int32_t* __restrict__ flags) {
  const uint64_t n = 1ull << log_n;
  const Fr* p = coeffs + ((uint64_t)blockIdx.y << log_n);
  uint32_t nz = 0;
  for (uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const Fr x = ld_fr(p + i);
#pragma unroll
    for (int k = 0; k < 8; ++k) nz |= x.l[k];
  }
  if (nz) flags[blockIdx.y] = 1;
}

// ---- launchers (kzg_recover.hpp) -------------------------------------------------------------------------------------------
static int kzr_check_shape(uint32_t log_n, uint32_t log_cell, uint32_t batch) {
  if (kzc_check_cell(log_n, log_cell) || log_n > KZD_MAX_LOG || log_n - log_cell > KZR_MAX_LOG_R || !batch || batch > KZD_MAX_CHUNK)
    return PLONK_ERR_ARG;
  return PLONK_OK;
}

int kzr_vanish(Ctx* c, const Fr* pw, const uint32_t* miss, uint32_t nmiss, uint32_t log_n, uint32_t log_cell, Fr* zdom, Fr* zcoset) {
  PTRY(kzr_check_shape(log_n, log_cell, 1));
  const uint32_t log_r = log_n - log_cell;
  if (nmiss > (1u << log_r) || (nmiss && !miss)) return PLONK_ERR_ARG;
  const Fr shift = fr_generator().pow_u64(1ull << log_cell);
  hipLaunchKernelGGL(kzr_vanish_kernel, dim3(2u << log_r), dim3(KZR_VANISH_SLICES), 0, c->stream, pw, miss, nmiss, log_r, shift, zdom, zcoset);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzr_scatter(Ctx* c, const Fr* const* vecs, const int32_t* slot, const Fr* zdom, uint32_t log_n, uint32_t log_cell, uint32_t batch, Fr* out) {
  PTRY(kzr_check_shape(log_n, log_cell, batch));
  hipLaunchKernelGGL(kzr_scatter_kernel, dim3((uint32_t)(((1ull << log_n) + KZR_LANES - 1) / KZR_LANES), batch), dim3(KZR_LANES), 0, c->stream,
                     vecs, slot, zdom, log_n, log_cell, out);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzr_divide(Ctx* c, Fr* v, const Fr* zinv, uint32_t log_n, uint32_t log_cell, uint32_t batch) {
  PTRY(kzr_check_shape(log_n, log_cell, batch));
  hipLaunchKernelGGL(kzr_divide_kernel, dim3((uint32_t)(((1ull << log_n) + KZR_LANES - 1) / KZR_LANES), batch), dim3(KZR_LANES), 0, c->stream,
                     v, zinv, log_n, log_cell);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzr_tail(Ctx* c, const Fr* coeffs, uint32_t log_n, uint64_t max_len, uint32_t batch, int32_t* flags) {
  const uint64_t n = 1ull << log_n;
  if (log_n < 1 || log_n > KZD_MAX_LOG || !batch || batch > KZD_MAX_CHUNK || max_len > n) return PLONK_ERR_ARG;
  HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * batch, c->stream));
  const uint64_t first = kzr_tail_first(max_len);
  if (first == n) return PLONK_OK;
  const uint64_t blocks = (n - first + KZR_LANES - 1) / KZR_LANES;
  hipLaunchKernelGGL(kzr_tail_kernel, dim3((uint32_t)(blocks < KZR_TAIL_BLOCKS ? blocks : KZR_TAIL_BLOCKS), batch), dim3(KZR_LANES), 0,
                     c->stream, coeffs, log_n, first, flags);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the state a handle holds for these calls ------------------------------------------------------------------------------
struct KzrBufs {
  enum { A, IO, CL, TMP, PW, ZDOM, ZCOSET, SLOT, MISS, VECS, FLAGS, LEN, DESC, META, NBUF };   // grow-only
};
struct KzgRecover : KzrBufs, DevBufs<KzrBufs::NBUF> {
  plonk_kzg_recover_info last = {};
};

void kzr_release(KzgRecover* recover) { delete recover; }

namespace {

struct RecoverCall {
  uint32_t log_cell;
  const uint32_t* cell_ids;
  uint64_t available;
  const void* const* values;
  uint64_t count, max_len;
  void *coeffs, *cells, *proofs48, *commitments48;
  int32_t* status;
  bool resident;
};

// steps 1 to 3 of the mathematics for polynomials [first, first + cnt): their coefficients in A
int recover_chunk(const KzgDomain* d, KzgRecover* e, const RecoverCall& a, uint64_t first, uint32_t cnt) {
  Ctx& c = *d->c;
  const uint32_t L = d->log_n;
  const uint64_t n = 1ull << L, packed = a.available << a.log_cell;
  Fr* A = e->at<Fr>(KzgRecover::A);
  Fr* tmp = e->at<Fr>(KzgRecover::TMP);
  if (!a.resident)
    for (uint32_t b = 0; b < cnt; ++b)
      HIP_TRY(hipMemcpyAsync(e->at<Fr>(KzgRecover::IO) + (uint64_t)b * packed, a.values[first + b], sizeof(Fr) * packed, hipMemcpyHostToDevice,
                             c.stream));
  PTRY(kzr_scatter(&c, e->at<const Fr*>(KzgRecover::VECS) + first, e->at<int32_t>(KzgRecover::SLOT), e->at<Fr>(KzgRecover::ZDOM), L, a.log_cell,
                   cnt, A));
  for (uint32_t b = 0; b < cnt; ++b) {
    Fr* p = A + (uint64_t)b * n;
    PTRY(ntt_device(&c, p, p, tmp, L, true, false, n));    // P = f Z
    PTRY(ntt_device(&c, p, p, tmp, L, false, true, n));    // P on the coset of 7
  }
  PTRY(kzr_divide(&c, A, e->at<Fr>(KzgRecover::ZCOSET), L, a.log_cell, cnt));
  for (uint32_t b = 0; b < cnt; ++b) {
    Fr* p = A + (uint64_t)b * n;
    PTRY(ntt_device(&c, p, p, tmp, L, true, true, n));     // f
  }
  return PLONK_OK;
}

// the trimmed lengths of the chunk's coefficients (returns with the stream synchronised)
int chunk_lengths(Ctx& c, KzgRecover* e, uint64_t n, uint32_t cnt, uint64_t* trimmed) {
  unsigned long long* len = e->at<unsigned long long>(KzgRecover::LEN);
  for (uint32_t b = 0; b < cnt; ++b) PTRY(poly_trimmed_len(&c, e->at<Fr>(KzgRecover::A) + (uint64_t)b * n, n, len + b));
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "length words");
  HIP_TRY(hipMemcpyAsync(trimmed, len, sizeof(uint64_t) * cnt, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  return PLONK_OK;
}

int recover_body(const char* api_fn, KzgDomain* d, KzgRecover* e, const RecoverCall& a) {
  Ctx& c = *d->c;
  const uint32_t L = d->log_n, log_r = L - a.log_cell;
  const uint64_t n = 1ull << L, r = 1ull << log_r, count = a.count, packed = a.available << a.log_cell;
  const bool own_values = a.cells && !a.proofs48;   // with proofs the body of plonk_kzg_open_cells makes the cell values
  const KzrPlan plan = kzr_plan(L, a.log_cell, count, a.available, d->ws_cap, a.cells || a.proofs48);
  const uint64_t chunk = plan.chunk_polys;
  plonk_kzg_recover_info info = {};
  info.log_n = L;
  info.log_cell = a.log_cell;
  info.chunks = (uint32_t)plan.chunks;
  info.count = count;
  info.available = a.available;
  info.missing = plan.missing;
  info.max_len = a.max_len;
  info.chunk_polys = chunk;
  info.transforms = plan.transforms;
  info.vanish_muls = plan.vanish_muls;
  info.workspace_bytes = plan.ws_bytes;
  PTRY(e->need(KzgRecover::A, sizeof(Fr) * n * chunk));
  if (!a.resident || own_values) PTRY(e->need(KzgRecover::IO, sizeof(Fr) * n * chunk));
  if (own_values) PTRY(e->need(KzgRecover::CL, sizeof(Fr) * n * chunk));
  PTRY(e->need(KzgRecover::TMP, sizeof(Fr) * n));
  PTRY(e->need(KzgRecover::PW, sizeof(Fr) * r));
  PTRY(e->need(KzgRecover::ZDOM, sizeof(Fr) * r));
  PTRY(e->need(KzgRecover::ZCOSET, sizeof(Fr) * r));
  PTRY(e->need(KzgRecover::SLOT, sizeof(int32_t) * r));
  PTRY(e->need(KzgRecover::MISS, sizeof(uint32_t) * r));
  PTRY(e->need(KzgRecover::VECS, sizeof(Fr*) * count));
  PTRY(e->need(KzgRecover::FLAGS, sizeof(int32_t) * count));
  PTRY(e->need(KzgRecover::LEN, sizeof(uint64_t) * chunk));
  if (a.commitments48) PTRY(msm_reserve(&c, n));
  // the slot table, the missing list, the table of the polynomials' device addresses: alive until the call's last copy has run
  std::vector<int32_t> slot(r, KZR_MISSING);
  for (uint64_t i = 0; i < a.available; ++i) slot[a.cell_ids[i]] = (int32_t)i;
  std::vector<uint32_t> miss;
  for (uint64_t k = 0; k < r; ++k)
    if (slot[k] == KZR_MISSING) miss.push_back((uint32_t)k);
  std::vector<const Fr*> vecs(count);
  for (uint64_t b = 0; b < count; ++b)
    vecs[b] = a.resident ? (const Fr*)a.values[b] : e->at<Fr>(KzgRecover::IO) + (b % chunk) * packed;
  HIP_TRY(hipMemcpyAsync(e->p[KzgRecover::SLOT], slot.data(), sizeof(int32_t) * r, hipMemcpyHostToDevice, c.stream));
  if (!miss.empty()) HIP_TRY(hipMemcpyAsync(e->p[KzgRecover::MISS], miss.data(), sizeof(uint32_t) * miss.size(), hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(e->p[KzgRecover::VECS], vecs.data(), sizeof(Fr*) * count, hipMemcpyHostToDevice, c.stream));
  // Z_r at phi^k and at 7^l phi^k, the latter inverted: once per call
  PTRY(poly_power_array(&c, e->at<Fr>(KzgRecover::PW), r, fr_domain_root(log_r)));
  PTRY(kzr_vanish(&c, e->at<Fr>(KzgRecover::PW), e->at<uint32_t>(KzgRecover::MISS), (uint32_t)miss.size(), L, a.log_cell,
                  e->at<Fr>(KzgRecover::ZDOM), e->at<Fr>(KzgRecover::ZCOSET)));
  PTRY(poly_batch_inverse(&c, e->at<Fr>(KzgRecover::ZCOSET), r));
  // ---- the verdict of every polynomial, before anything is written ----
  for (uint64_t first = 0; first < count; first += chunk) {
    const uint32_t cnt = (uint32_t)(count - first < chunk ? count - first : chunk);
    PTRY(recover_chunk(d, e, a, first, cnt));
    PTRY(kzr_tail(&c, e->at<Fr>(KzgRecover::A), L, a.max_len, cnt, e->at<int32_t>(KzgRecover::FLAGS) + first));
  }
  std::vector<int32_t> flags(count);
  HIP_TRY(hipMemcpyAsync(flags.data(), e->p[KzgRecover::FLAGS], sizeof(int32_t) * count, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  for (uint64_t b = 0; b < count; ++b) info.inconsistent += flags[b] ? 1 : 0;
  if (a.status)
    for (uint64_t b = 0; b < count; ++b) a.status[b] = flags[b] ? PLONK_ERR_VERIFY : PLONK_OK;
  if (info.inconsistent) {
    e->last = info;
    API_FAIL(PLONK_ERR_VERIFY, "the values of a polynomial fit no polynomial of max_len coefficients");
  }
  // ---- from here on the call writes ----
  std::vector<uint64_t> trimmed(chunk);
  std::vector<const void*> ptrs(chunk);
  std::vector<uint8_t> comm;
  Fr* A = e->at<Fr>(KzgRecover::A);
  for (uint64_t first = 0; first < count; first += chunk) {
    const uint32_t cnt = (uint32_t)(count - first < chunk ? count - first : chunk);
    if (plan.passes > 1) PTRY(recover_chunk(d, e, a, first, cnt));   // (a single chunk still holds its coefficients)
    if (a.coeffs) HIP_TRY(hipMemcpyAsync((uint8_t*)a.coeffs + sizeof(Fr) * n * first, A, sizeof(Fr) * n * cnt, hipMemcpyDefault, c.stream));
    if (own_values) {
      Fr* ev = e->at<Fr>(KzgRecover::IO);
      Fr* cl = e->at<Fr>(KzgRecover::CL);
      for (uint32_t b = 0; b < cnt; ++b)
        PTRY(ntt_device(&c, A + (uint64_t)b * n, ev + (uint64_t)b * n, e->at<Fr>(KzgRecover::TMP), L, false, false, n));
      PTRY(kzc_transpose(&c, ev, L, a.log_cell, cnt, cl));
      HIP_TRY(hipMemcpyAsync((uint8_t*)a.cells + sizeof(Fr) * n * first, cl, sizeof(Fr) * n * cnt, hipMemcpyDefault, c.stream));
    }
    if (a.proofs48 || a.commitments48) PTRY(chunk_lengths(c, e, n, cnt, trimmed.data()));
    if (a.proofs48) {
      for (uint32_t b = 0; b < cnt; ++b) ptrs[b] = A + (uint64_t)b * n;
      PTRY(kzc_open_resident(d, a.log_cell, ptrs.data(), trimmed.data(), cnt, a.cells ? (uint8_t*)a.cells + sizeof(Fr) * n * first : nullptr,
                             (uint8_t*)a.proofs48 + 48 * r * first, a.commitments48 ? (uint8_t*)a.commitments48 + 48 * first : nullptr,
                             &info.built_table));
    } else if (a.commitments48) {
      PTRY(kzd_commit(&c, A, n, trimmed.data(), cnt, comm, (uint8_t*)a.commitments48 + 48 * first));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));   // the chunk's buffers are reused by the next one
  }
  e->last = info;
  return PLONK_OK;
}

int recover_impl(const char* api_fn, plonk_kzg_domain* dom, const RecoverCall& a) {
  if (!dom) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = dom->d;
  bool all_set = a.values != nullptr;
  for (uint64_t b = 0; all_set && b < a.count && a.count <= KZD_MAX_COUNT; ++b) all_set = a.values[b] != nullptr;
  if (kzr_check_args(true, d->log_n, a.log_cell, a.count, a.cell_ids, a.available, a.values != nullptr, all_set, a.max_len,
                     a.coeffs || a.cells || a.proofs48 || a.commitments48))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a NULL pointer, log_cell outside [1, log_n - 1], more than 2048 cells, count > 65536, "
                            "a cell index out of range or repeated, max_len outside [1, n], or no output at all");
  KZD_ENTER(d, api_fn, KZD_WORK);
  if (!a.count) return PLONK_OK;
  if (kzr_check_degree(a.log_cell, a.available, a.max_len)) API_FAIL(PLONK_ERR_DEGREE, "max_len exceeds the values given: too few cells");
  KzgRecover* e = kzd_state(d->recover);
  // canonical values, as plonk_kzg_open_cells checks its coefficients: on the host, or by a scan of the resident arrays
  std::vector<uint64_t> lens(a.count, a.available << a.log_cell), trimmed(a.count);
  PTRY(kzd_lengths_on(api_fn, d->c, e, d->log_n, a.values, lens.data(), a.count, a.resident, trimmed.data()));
  return kzd_drained(d->c, recover_body(api_fn, d, e, a));
}

}  // namespace

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_kzg_recover_cells(plonk_kzg_domain* dom, uint32_t log_cell, const uint32_t* cell_ids, uint64_t available, const uint64_t* const* values,
                            uint64_t count, uint64_t max_len, uint64_t* coeffs, uint64_t* cells, uint8_t* proofs48, uint8_t* commitments48,
                            int32_t* status) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::recover_impl(api_fn, dom, plonk::RecoverCall{log_cell, cell_ids, available, (const void* const*)values, count, max_len, coeffs,
                                                               cells, proofs48, commitments48, status, false});
  });
}

int plonk_kzg_recover_cells_dev(plonk_kzg_domain* dom, uint32_t log_cell, const uint32_t* cell_ids, uint64_t available,
                                const void* const* values_dev, uint64_t count, uint64_t max_len, void* coeffs_dev, void* cells_dev,
                                void* proofs48_dev, void* commitments48_dev, int32_t* status) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::recover_impl(api_fn, dom, plonk::RecoverCall{log_cell, cell_ids, available, values_dev, count, max_len, coeffs_dev, cells_dev,
                                                               proofs48_dev, commitments48_dev, status, true});
  });
}

int plonk_kzg_recover_last(plonk_kzg_domain* dom, plonk_kzg_recover_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgDomain* d = dom->d;
  KZD_ENTER(d, api_fn, KZD_KEY);
  const KzgRecover* e = d->recover;
  plonk_kzg_recover_info info = {};
  if (e) info = e->last;
  info.log_n = d->log_n;
  *out = info;
  return PLONK_OK;
  });
}

}  // extern "C"
