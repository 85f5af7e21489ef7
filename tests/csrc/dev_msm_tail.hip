// extern "C" doors to everything of plonk_amd/csrc/msm.hip that follows the bucket sort (msm_batch_device_v of both compiled
// bucket counts, one phase per call) and to the work buffers it reads and writes, for tests/test_gpu_msm_tail.py.  Every door
// takes the plonk_ctx* the Python binding holds (Context.handle), device pointers and plain host arguments, queues on the
// context's stream, waits for that stream and returns the product's code (PLONK_ERR_*, negative) or, when the product was
// content, the HIP error of the wait (positive).  ONE kernel here, dmt_quad_add_kernel: the test kernel around g1r_add_quad
// (curve28_quad.cuh); every other kernel that runs is libplonk_hip.so's own.  Test code only.
#include "plonk_internal.hpp"
#include "curve28.cuh"

using namespace plonk;

struct dmt_cfg_t {   // the Config switches msm_batch_device_v and msm_reserve read, as one call sees them
  int ksl, order, acc_lds, acc_wg, bsum_lane, tail_serial, rc_lane_tree, lps, rcwv;
};
struct dmt_report_t {   // what the product decided
  uint32_t ksl, heavy_thresh, ordered, wide;
  int last_rowbits;
};
struct dmt_work_t {   // MsmWork as the tests see it
  void* entries;
  void* offsets;
  void* slice_off;
  void* full_off;
  void* part_list;
  void* multi_list;
  void* nheavy;
  void* heavy_list;
  void* buckets;
  void* tmp_words;
  void* partial;
  void* seg_sum;
  void* chunk;
  uint64_t cap_m;
  uint64_t cap_slices;
  uint64_t cap_segs;
};

namespace {

int finish(Ctx& c, int rc) {
  const hipError_t e = hipStreamSynchronize(c.stream);
  if (rc) return rc;
  return (int)e;
}
struct Overrides {   // the switches of one call; nullptr: the context's own
  Ctx& c;
  Config saved;
  Overrides(Ctx& ctx, const dmt_cfg_t* o) : c(ctx), saved(ctx.cfg) {
    if (!o) return;
    c.cfg.ksl = o->ksl;
    c.cfg.order = o->order;
    c.cfg.acc_lds = o->acc_lds != 0;
    c.cfg.acc_wg = o->acc_wg;
    c.cfg.bsum_lane = o->bsum_lane != 0;
    c.cfg.tail_serial = o->tail_serial != 0;
    c.cfg.rc_lane_tree = o->rc_lane_tree != 0;
    c.cfg.lps = o->lps;
    c.cfg.rcwv = o->rcwv;
  }
  ~Overrides() { c.cfg = saved; }
};

}  // namespace

#define DOOR(H) \
  Ctx& c = (H)->c; \
  std::lock_guard<std::mutex> lk(c.mu)

// ---- the test kernel around g1r_add_quad ---------------------------------------------------------------------------------
namespace plonk {
namespace {
struct alignas(16) QSlot {   // G1RSlot of msm.hip: four coordinates of 16 words
  Fp28Slot X, Y, ZZ, ZZZ;
};
__device__ __forceinline__ Fp28 q_ld(const Fp28Slot* p) {
  Fp28 r;
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) r.l[i] = p->w[i];
  return r;
}
__device__ __forceinline__ void q_st(Fp28Slot* p, const Fp28& v) {
#pragma unroll
  for (int i = 0; i < Fp28::N; ++i) p->w[i] = v.l[i];
  p->w[14] = 0u;
  p->w[15] = 0u;
}
__device__ __forceinline__ G1R q_ld_pt(const QSlot* p) {
  G1R r;
  r.X = q_ld(&p->X); r.Y = q_ld(&p->Y); r.ZZ = q_ld(&p->ZZ); r.ZZZ = q_ld(&p->ZZZ);
  return r;
}
#include "curve28_quad.cuh"
}  // namespace

// quad i (lanes 4 i .. 4 i + 3) loads operand pair i, replicated, and every one of its lanes stores its own result in
// out[4 i + q].  op[i] (uniform per quad): 0  a + b;  1  dbl(a) + b;  2  a + dbl(b);  3  (a + b) + a;  4  (a + b) + (b + a)
// — 1 .. 4 feed results of dbl() and of earlier quad additions back in as operands
__global__ void __launch_bounds__(64) dmt_quad_add_kernel(const QSlot* __restrict__ a_all, const QSlot* __restrict__ b_all,
                                                          const uint32_t* __restrict__ op_all, QSlot* __restrict__ out, uint32_t npairs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 2, q = t & 3;
  if (i >= npairs) return;   // whole quads
  const G1R a = q_ld_pt(a_all + i), b = q_ld_pt(b_all + i);
  const uint32_t op = op_all[i];
  G1R r;
  if (op == 0) r = g1r_add_quad(a, b, q);
  else if (op == 1) r = g1r_add_quad(a.dbl(), b, q);
  else if (op == 2) r = g1r_add_quad(a, b.dbl(), q);
  else if (op == 3) r = g1r_add_quad(g1r_add_quad(a, b, q), a, q);
  else r = g1r_add_quad(g1r_add_quad(a, b, q), g1r_add_quad(b, a, q), q);
  QSlot* o = out + t;
  q_st(&o->X, r.X); q_st(&o->Y, r.Y); q_st(&o->ZZ, r.ZZ); q_st(&o->ZZZ, r.ZZZ);
}
}  // namespace plonk

extern "C" {

// a, b: npairs slots of 256 bytes; op: npairs words; out: 4 * npairs slots (every byte of them is written)
int dmt_quad_add(plonk_ctx* h, const void* a, const void* b, const void* op, void* out, uint32_t npairs) {
  DOOR(h);
  if (npairs == 0 || npairs > (1u << 20)) return PLONK_ERR_ARG;
  hipLaunchKernelGGL(dmt_quad_add_kernel, dim3((4 * npairs + 63) / 64), dim3(64), 0, c.stream, (const QSlot*)a, (const QSlot*)b,
                     (const uint32_t*)op, (QSlot*)out, npairs);
  return finish(c, (int)hipGetLastError());
}

// One msm_batch_device_v call of the variant with 2^bits buckets: phase 1 (sort, accumulation, bucket sums, heavy buckets of
// the commitments [kb0, kb0 + count) of a group of group_count) or phase 2 (the group's reduction tail; kb0 / count are not
// read).  The batch is filled as msm_batch_device fills it; the table is the caller's.  scalars / m / out have group_count
// entries; phase 2 reads none of the scalars.  The switches of `cfg` hold for the call — applied before the reservation, whose
// slice capacity depends on cfg.ksl — and are put back after it.  ksl and heavy_thresh are the product's own choice: reported.
int dmt_phase(plonk_ctx* h, int phase, int bits, uint32_t rows, const void* table, uint64_t table_n, int group_count, int kb0,
              int count, const Fr* const* scalars, const uint64_t* m, int bit_sums, G1* const* out, const dmt_cfg_t* cfg,
              dmt_report_t* rep) {
  DOOR(h);
  if ((bits != 15 && bits != 19) || (phase != 1 && phase != 2) || group_count < 1 || group_count > MSM_MAX_BATCH || kb0 < 0 ||
      count < 1 || kb0 + count > group_count || !table || !rep)
    return PLONK_ERR_ARG;
  uint64_t mmax = 0;
  for (int k = 0; k < group_count; ++k) {
    if (m[k] > table_n) return PLONK_ERR_DEGREE;
    mmax = m[k] > mmax ? m[k] : mmax;
  }
  if (mmax == 0) return PLONK_ERR_ARG;   // msm_batch_device never calls the variant for an empty group
  Overrides switches(c, cfg);
  int rc = msm_reserve(&c, mmax);
  if (rc) return finish(c, rc);
  MsmBatch bt{};
  bt.count = phase == 1 ? count : group_count;
  bt.kb0 = phase == 1 ? kb0 : 0;
  bt.group_count = group_count;
  bt.cap_m = c.msm.cap_m;
  bt.cap_slices = c.msm.cap_slices;
  bt.table = table;
  bt.table_n = table_n;
  bt.rows = rows;
  for (int k = 0; k < group_count; ++k) {
    bt.scalars[k] = scalars[k];
    bt.m[k] = m[k];
    bt.out[k] = out[k];
    bt.tail[k] = nullptr;
    bt.split[k] = ~0ull;
  }
  rc = bits == 15 ? nb15::msm_batch_device_v(&c, bt, mmax, bit_sums != 0, phase) : nbl::msm_batch_device_v(&c, bt, mmax, bit_sums != 0, phase);
  rep->ksl = bt.ksl;
  rep->heavy_thresh = bt.heavy_thresh;
  rep->ordered = bt.ordered;
  rep->wide = bt.wide;
  rep->last_rowbits = c.msm.last_rowbits;
  return finish(c, rc);
}

// the work buffers after a reservation for m terms under the switches of `cfg` (they move when a capacity grows: ask again
// after every larger m or shorter forced slice)
int dmt_work(plonk_ctx* h, uint64_t m, const dmt_cfg_t* cfg, dmt_work_t* out) {
  DOOR(h);
  Overrides switches(c, cfg);
  const int rc = msm_reserve(&c, m ? m : 1);
  if (rc) return finish(c, rc);
  const MsmWork& w = c.msm;
  out->entries = w.entries;
  out->offsets = w.offsets;
  out->slice_off = w.slice_off;
  out->full_off = w.full_off;
  out->part_list = w.part_list;
  out->multi_list = w.multi_list;
  out->nheavy = w.nheavy;
  out->heavy_list = w.heavy_list;
  out->buckets = w.buckets;
  out->tmp_words = w.tmp_words;
  out->partial = w.partial;
  out->seg_sum = w.seg_sum;
  out->chunk = w.chunk;
  out->cap_m = w.cap_m;
  out->cap_slices = w.cap_slices;
  out->cap_segs = w.cap_segs;
  return finish(c, PLONK_OK);
}

int dmt_fill(plonk_ctx* h, void* ptr, int byte, uint64_t bytes) {
  DOOR(h);
  const hipError_t e = hipMemsetAsync(ptr, byte, bytes, c.stream);
  return finish(c, (int)e);
}

// (either side of dmt_read / dmt_write may be device memory: a bucket array kept on the device is copied in place)
int dmt_read(plonk_ctx* h, const void* ptr, void* host, uint64_t bytes) {
  DOOR(h);
  const hipError_t e = hipMemcpyAsync(host, ptr, bytes, hipMemcpyDefault, c.stream);
  return finish(c, (int)e);
}

int dmt_write(plonk_ctx* h, void* ptr, const void* host, uint64_t bytes) {
  DOOR(h);
  const hipError_t e = hipMemcpyAsync(ptr, host, bytes, hipMemcpyDefault, c.stream);
  return finish(c, (int)e);
}

// table[index[i]] = entries[i] for i < n: 128-byte entries, host arrays; every index below table_entries
int dmt_scatter(plonk_ctx* h, void* table, uint64_t table_entries, const uint32_t* index, const void* entries, uint64_t n) {
  DOOR(h);
  for (uint64_t i = 0; i < n; ++i)
    if (index[i] >= table_entries) return PLONK_ERR_ARG;
  hipError_t e = hipSuccess;
  for (uint64_t i = 0; i < n && e == hipSuccess; ++i)
    e = hipMemcpyAsync((uint8_t*)table + sizeof(G1AffineR) * (uint64_t)index[i], (const uint8_t*)entries + sizeof(G1AffineR) * i,
                       sizeof(G1AffineR), hipMemcpyHostToDevice, c.stream);
  return finish(c, (int)e);
}

}  // extern "C"
