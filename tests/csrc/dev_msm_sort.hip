// extern "C" doors to the bucket sort of plonk_amd/csrc/msm_sort.hip (msm_group_sort of both compiled bucket counts) and
// to the work buffers it writes, for tests/test_gpu_msm_sort.py.  No kernels here: the code that runs is libplonk_hip.so's
// own.  Every door takes the plonk_ctx* the Python binding holds (Context.handle), device pointers and plain host arguments,
// queues on the context's stream, waits for that stream and returns the product's code (PLONK_ERR_*, negative) or, when
// the product was content, the HIP error of the wait (positive).  Test code only.
#include "plonk_internal.hpp"

using namespace plonk;

namespace {

int finish(Ctx& c, int rc) {
  const hipError_t e = hipStreamSynchronize(c.stream);
  if (rc) return rc;
  return (int)e;
}
struct Sort13 {   // the partition geometry of one call
  Ctx& c;
  int saved;
  Sort13(Ctx& ctx, int v) : c(ctx), saved(ctx.cfg.sort13) { c.cfg.sort13 = v; }
  ~Sort13() { c.cfg.sort13 = saved; }
};

}  // namespace

#define DOOR(H) \
  Ctx& c = (H)->c; \
  std::lock_guard<std::mutex> lk(c.mu)

struct dms_work_t {   // MsmWork as the tests see it: what the sort writes, the scratch it goes through, the capacities
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
  uint64_t cap_m;
  uint64_t cap_slices;
};

extern "C" {

// One msm_group_sort launch: the commitments [kb0, kb0 + count) of a group of group_count, over 2^bits buckets.  The four
// per-commitment arrays have group_count entries (device pointers, host integers); tail[k] may be null with split[k] >= m[k].
// The batch is filled as msm_batch_device fills it (capacities from the context's work buffers, reserved here for the
// largest m); the table is null — the sort never reads it — so table_n is free.  wide < 0: by msm_needs_wide_words.
int dms_group_sort(plonk_ctx* h, int bits, uint32_t rows, uint64_t table_n, int group_count, int kb0, int count,
                   const Fr* const* scalars, const uint64_t* m, const Fr* const* tail, const uint64_t* split, uint32_t ksl,
                   uint32_t heavy_thresh, uint32_t ordered, int wide, int sort13) {
  DOOR(h);
  if ((bits != 15 && bits != 19) || group_count < 1 || group_count > MSM_MAX_BATCH || kb0 < 0 || count < 1 || kb0 + count > group_count)
    return PLONK_ERR_ARG;
  if (ksl == 0 || (ksl & (ksl - 1)) != 0) return PLONK_ERR_ARG;   // the kernels shift by log2(ksl): no door for what the product never passes
  uint64_t mmax = 0;
  for (int k = 0; k < group_count; ++k) mmax = m[k] > mmax ? m[k] : mmax;
  int rc = msm_reserve(&c, mmax ? mmax : 1);
  if (rc) return finish(c, rc);
  Sort13 geometry(c, sort13);
  MsmBatch bt{};
  bt.count = count;
  bt.kb0 = kb0;
  bt.group_count = group_count;
  bt.cap_m = c.msm.cap_m;
  bt.cap_slices = c.msm.cap_slices;
  bt.table = nullptr;
  bt.table_n = table_n;
  bt.rows = rows;
  bt.ksl = ksl;
  bt.heavy_thresh = heavy_thresh;
  bt.ordered = ordered ? 1u : 0u;
  for (int k = 0; k < group_count; ++k) {
    bt.scalars[k] = scalars[k];
    bt.m[k] = m[k];
    bt.out[k] = nullptr;
    bt.tail[k] = tail[k];
    bt.split[k] = tail[k] ? split[k] : ~0ull;
  }
  if (bits == 15) {
    bt.wide = wide < 0 ? (nb15::msm_needs_wide_words(rows, table_n) ? 1u : 0u) : (wide ? 1u : 0u);
    rc = nb15::msm_group_sort(&c, bt, mmax);
  } else {
    bt.wide = wide < 0 ? (nbl::msm_needs_wide_words(rows, table_n) ? 1u : 0u) : (wide ? 1u : 0u);
    rc = nbl::msm_group_sort(&c, bt, mmax);
  }
  return finish(c, rc);
}

// the work buffers after a reservation for m terms (they move when the capacity grows: ask again after every larger m)
int dms_work(plonk_ctx* h, uint64_t m, dms_work_t* out) {
  DOOR(h);
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
  out->cap_m = w.cap_m;
  out->cap_slices = w.cap_slices;
  return finish(c, PLONK_OK);
}

int dms_fill(plonk_ctx* h, void* ptr, int byte, uint64_t bytes) {
  DOOR(h);
  const hipError_t e = hipMemsetAsync(ptr, byte, bytes, c.stream);
  return finish(c, (int)e);
}

int dms_read(plonk_ctx* h, const void* ptr, void* host, uint64_t bytes) {
  DOOR(h);
  const hipError_t e = hipMemcpyAsync(host, ptr, bytes, hipMemcpyDeviceToHost, c.stream);
  return finish(c, (int)e);
}

int dms_needs_wide(int bits, uint32_t rows, uint64_t table_n) {
  if (bits == 15) return nb15::msm_needs_wide_words(rows, table_n) ? 1 : 0;
  if (bits == 19) return nbl::msm_needs_wide_words(rows, table_n) ? 1 : 0;
  return PLONK_ERR_ARG;
}

}  // extern "C"
