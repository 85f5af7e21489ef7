// Witness diagnosis on the device: which rows of a wire assignment fail which gate identity, and which wire cells break a
// copy constraint (plonk_prover_diagnose*, prover.hip).  Exact, row by row — nothing is folded with a challenge.
//
//   diag_row_kernel      one lane per row: the 17 identities of diagnose_core.hpp in the reduced-radix arithmetic of
//                        fr29.cuh (values in twiddle form x * 2^261, closed under Fr29::mul), the four copy checks
//                        through the decoded sigma positions, the row's mask, the workgroup's count of failing rows and
//                        the per-family counts
//   diag_scan_kernel     exclusive scan of the workgroup counts (one workgroup)
//   diag_scatter_kernel  the failing rows, ascending, into at most `cap` records
//   sigma_decode_kernel  one lane per (wire, row): K_col * omega^row -> packed position, once per prover
// Only vector stores and ordinary atomics (integer adds of exact counts).
#include "diagnose.hpp"
#include "devmem.cuh"

namespace plonk {

namespace {

// A value in twiddle form.  Range discipline (fr29.cuh; the lazy ranges poly.hip's widget path describes): every sum is
// add_csub'd and every difference sub_reduce'd to [0, 2q + eps), normalised, so both operands of every product are inside
// what Fr29::mul accepts and no lazily reduced value (sub_lazy: up to 6q, limbs above 2^29) ever reaches a zero test.
// The zero test itself is exact: to_fr() is canonical for anything below 4q.
struct T29 {
  Fr29 v;
};
__device__ __forceinline__ T29 operator+(const T29& a, const T29& b) { return T29{Fr29::add_csub(a.v, b.v)}; }
__device__ __forceinline__ T29 operator-(const T29& a, const T29& b) { return T29{Fr29::sub_reduce(a.v, b.v)}; }
__device__ __forceinline__ T29 operator*(const T29& a, const T29& b) { return T29{Fr29::mul(a.v, b.v)}; }
__device__ __forceinline__ bool diag_nonzero(const T29& x) { return !x.v.to_fr().is_zero(); }
__device__ __forceinline__ T29 t29_load(const Fr* p) { return T29{Fr29::twiddle_from_fr(ld_fr(p))}; }
__device__ __forceinline__ T29 t29_zero() { return T29{Fr29::zero()}; }

T29 t29_of(const Fr& x) { return T29{Fr29::twiddle_from_fr(x)}; }   // host

struct RowLoader {
  const DiagArgs& a;
  uint64_t i, iw;
  __device__ __forceinline__ T29 wire(int col) const { return t29_load(a.wires + (uint64_t)col * a.n + i); }
  __device__ __forceinline__ T29 wire_next(int col) const { return t29_load(a.wires + (uint64_t)col * a.n + iw); }
  __device__ __forceinline__ bool sel_nonzero(int id) const { return a.sel[id] && !ld_fr(a.sel[id] + i).is_zero(); }
  __device__ __forceinline__ T29 sel(int id) const { return a.sel[id] ? t29_load(a.sel[id] + i) : t29_zero(); }
  __device__ __forceinline__ T29 pi() const { return a.pi ? t29_load(a.pi + i) : t29_zero(); }
};

// WIDGETS = false: circuits whose range / logic / group-addition selector polynomials are all identically zero
template <bool WIDGETS>
__global__ void __launch_bounds__(DIAG_T) diag_row_kernel(DiagArgs a, DiagConsts<T29> k) {
  __shared__ uint32_t wave_cnt[DIAG_T / 64];
  const uint64_t i = (uint64_t)blockIdx.x * DIAG_T + threadIdx.x;
  uint32_t mask = 0;
  if (i < a.n) {
    const RowLoader ld{a, i, (i + 1) & (a.n - 1)};
    mask = diag_row_families<T29>(ld, k, WIDGETS);
    // copy constraints: the cell must equal the cell sigma maps it to (values are canonical: plain comparison)
    for (uint32_t col = 0; col < 4; ++col) {
      const uint32_t to = a.pos[(uint64_t)col * a.n + i];
      bool bad = to == DIAG_POS_NONE;
      if (!bad) {
        const uint64_t at = (uint64_t)(to >> SIGMA_ROW_BITS) * a.n + (to & ((1u << SIGMA_ROW_BITS) - 1));
        if (at != (uint64_t)col * a.n + i) bad = !(ld_fr(a.wires + (uint64_t)col * a.n + i) == ld_fr(a.wires + at));
      }
      if (bad) mask |= 1u << (DIAG_COPY_SHIFT + col);
    }
    a.mask[i] = mask;
  }
  // counts: failing rows of this workgroup (for the ordered compaction) and rows per family (exact integer atomics)
  const unsigned long long fail = __ballot(mask != 0);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (fail) {
    const uint32_t fams = mask & ((1u << DIAG_FAMILIES) - 1);
    for (int f = 0; f <= DIAG_FAMILIES; ++f) {
      const unsigned long long b = __ballot(f < DIAG_FAMILIES ? ((fams >> f) & 1u) != 0 : (mask >> DIAG_COPY_SHIFT) != 0);
      if (lane == 0 && b) atomicAdd(&a.ctr->family[f], (unsigned long long)__popcll(b));
    }
  }
  if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(fail);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < DIAG_T / 64; ++w) s += wave_cnt[w];
    a.block_cnt[blockIdx.x] = s;
  }
}

// exclusive scan of nb workgroup counts by ONE workgroup: lane t owns a contiguous chunk
static constexpr uint32_t SCAN_T = 1024;
__global__ void __launch_bounds__(SCAN_T) diag_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off, uint64_t nb,
                                                           DiagCounters* ctr) {
  __shared__ uint32_t sh[SCAN_T];
  const uint32_t t = threadIdx.x;
  const uint64_t per = (nb + SCAN_T - 1) / SCAN_T;
  const uint64_t lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
  uint32_t s = 0;
  for (uint64_t j = lo; j < hi; ++j) s += cnt[j];
  sh[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < SCAN_T; d <<= 1) {   // Hillis-Steele, inclusive
    const uint32_t v = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  uint32_t run = sh[t] - s;
  for (uint64_t j = lo; j < hi; ++j) { off[j] = run; run += cnt[j]; }
  if (t == SCAN_T - 1) ctr->failing = sh[t];
}

__global__ void __launch_bounds__(DIAG_T) diag_scatter_kernel(DiagArgs a) {
  __shared__ uint32_t wave_cnt[DIAG_T / 64];
  if (a.block_cnt[blockIdx.x] == 0) return;   // uniform over the workgroup
  const uint64_t i = (uint64_t)blockIdx.x * DIAG_T + threadIdx.x;
  const uint32_t mask = i < a.n ? a.mask[i] : 0;
  const unsigned long long fail = __ballot(mask != 0);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(fail);
  __syncthreads();
  if (!mask) return;
  uint64_t rank = a.block_off[blockIdx.x] + (uint32_t)__popcll(fail & ((1ull << lane) - 1));
  for (uint32_t w = 0; w < wave; ++w) rank += wave_cnt[w];
  const uint32_t fams = mask & ((1u << DIAG_FAMILIES) - 1), copy = mask >> DIAG_COPY_SHIFT;
  if (rank == 0) {
    a.ctr->first_row = i;
    a.ctr->first_families = fams;
    a.ctr->first_copy = copy;
  }
  if (rank < a.cap) {
    plonk_unsat_row r;
    r.row = i;
    r.families = fams;
    r.copy_wires = copy;
    a.out[rank] = r;
  }
}

__global__ void __launch_bounds__(256) sigma_decode_kernel(const Fr* __restrict__ sigma_n, uint32_t* __restrict__ pos, uint64_t total,
                                                           SigmaDecodeConsts<T29> k) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) pos[i] = sigma_decode<T29>(t29_load(sigma_n + i), k);
}

inline dim3 grid_of(uint64_t n, uint32_t t) { return dim3((unsigned)((n + t - 1) / t)); }

}  // namespace

int diag_sigma_decode(Ctx* c, const Fr* sigma_n, uint32_t* pos, uint64_t n, uint32_t logn) {
  if (logn > (uint32_t)DIAG_MAX_LOG) return (set_last_error("invalid argument", "diagnose: domain above 2^28", __FILE__, __LINE__), PLONK_ERR_ARG);
  const SigmaDecodeConsts<Fr> f = sigma_decode_consts_fr(logn);
  SigmaDecodeConsts<T29> k;
  k.one = t29_of(f.one);
  for (int i = 0; i < 4; ++i) { k.kn[i] = t29_of(f.kn[i]); k.kinv[i] = t29_of(f.kinv[i]); }
  for (int j = 0; j < DIAG_MAX_LOG; ++j) k.winv[j] = t29_of(f.winv[j]);
  k.logn = logn;
  hipLaunchKernelGGL(sigma_decode_kernel, grid_of(4 * n, 256), dim3(256), 0, c->stream, sigma_n, pos, 4 * n, k);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int diag_report(Ctx* c, const DiagArgs& a) {
  static const DiagConsts<T29> k = [] {
    const DiagConsts<Fr> f = diag_consts_fr();
    return DiagConsts<T29>{t29_of(f.one), t29_of(f.two), t29_of(f.three), t29_of(f.c9), t29_of(f.c18), t29_of(f.c81), t29_of(f.c83), t29_of(f.ed)};
  }();
  HIP_TRY(hipMemsetAsync(a.ctr, 0, sizeof(DiagCounters), c->stream));
  const dim3 grid = grid_of(a.n, DIAG_T);
  const bool widgets = a.sel[DQ_RANGE] || a.sel[DQ_LOGIC] || a.sel[DQ_FIXED] || a.sel[DQ_VAR];
  if (widgets) hipLaunchKernelGGL(diag_row_kernel<true>, grid, dim3(DIAG_T), 0, c->stream, a, k);
  else hipLaunchKernelGGL(diag_row_kernel<false>, grid, dim3(DIAG_T), 0, c->stream, a, k);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(diag_scan_kernel, dim3(1), dim3(SCAN_T), 0, c->stream, a.block_cnt, a.block_off, diag_blocks(a.n), a.ctr);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(diag_scatter_kernel, grid, dim3(DIAG_T), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

}  // namespace plonk
