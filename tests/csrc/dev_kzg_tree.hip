// extern "C" doors to the launchers of plonk_amd/csrc/kzg_tree.hip (kzg_tree.hpp) — the map h, the finish kernel and the delta
// kernel — for tests/test_gpu_kzg_tree.py.  No kernels here: the code that runs is libplonk_hip.so's own.  Every door takes the
// plonk_ctx* the Python binding holds (Context.handle), device pointers and plain host arguments, queues on the context's
// stream, waits for that stream and returns the product's code (PLONK_ERR_*, negative) or, when the product was content, the
// HIP error of the wait (positive).  Test code only.
#include "kzg_handle.hpp"
#include "kzg_tree.hpp"

using namespace plonk;

namespace {

int finish(Ctx& c, int rc) {
  const hipError_t e = hipStreamSynchronize(c.stream);
  if (rc) return rc;
  return (int)e;
}

}  // namespace

#define DOOR(H) \
  Ctx& c = (H)->c; \
  std::lock_guard<std::mutex> lk(c.mu)

extern "C" {

// comp48: records of 48 bytes; list: count node indices or NULL (record j); out: count Montgomery Fr
int dkt_map(plonk_ctx* h, const void* comp48, const void* list, uint64_t count, void* out) {
  DOOR(h);
  KztSeed seed;
  if (!kzt_map_seed(&seed)) return PLONK_ERR_STATE;
  return finish(c, kzt_map_run(&c, seed, (const uint8_t*)comp48, (const uint64_t*)list, count, (Fr*)out));
}

// partial: count x slices slots of 256 bytes; list: count node indices or NULL (node first + j); pts / kind / comp48: the
// stored arrays of a level (96 / 4 / 48 bytes per node)
int dkt_finish(plonk_ctx* h, const void* partial, uint32_t slices, const void* list, uint64_t first, uint64_t count, int with_base, void* pts,
               void* kind, void* comp48) {
  DOOR(h);
  return finish(c, kzt_finish_run(&c, (const G1RSlot*)partial, slices, (const uint64_t*)list, first, count, with_base != 0, (G1Affine*)pts,
                                  (int32_t*)kind, (uint8_t*)comp48));
}

// fresh: count Fr; flat: count indices into vals; deltas: count Fr out
int dkt_delta(plonk_ctx* h, const void* fresh, const void* flat, uint64_t count, void* vals, void* deltas) {
  DOOR(h);
  return finish(c, kzt_delta_run(&c, (const Fr*)fresh, (const uint64_t*)flat, count, (Fr*)vals, (Fr*)deltas));
}

}  // extern "C"
