// extern "C" door to kze_finish of plonk_amd/csrc/kzg_evals.hip (kzg_evals.hpp) — the kernel that finishes and compresses the
// commitments of a call on a domain handle with Lagrange-basis tables — for tests/test_gpu_kzg_evals_tables.py.  No kernels
// here: the code that runs is libplonk_hip.so's own.  The door takes the plonk_ctx* the Python binding holds (Context.handle)
// and device pointers, queues on the context's stream, waits for that stream and returns the product's code (PLONK_ERR_*,
// negative) or, when the product was content, the HIP error of the wait (positive).  Test code only.
#include "kzg_domain.hpp"
#include "kzg_evals.hpp"

using namespace plonk;

extern "C" {

// out48[48 i] = the compressed commitment of the MSM_BIT_SUMS slots at bits + i * MSM_BIT_SUMS * sizeof(G1), i < count
int dkt_finish(plonk_ctx* h, const void* bits, uint32_t count, int rb, int bitpos, void* out48) {
  Ctx& c = h->c;
  std::lock_guard<std::mutex> lk(c.mu);
  const int rc = kze_finish(&c, (const G1*)bits, count, rb, bitpos != 0, (uint8_t*)out48);
  const hipError_t e = hipStreamSynchronize(c.stream);
  return rc ? rc : (int)e;
}

uint64_t dkt_const(int which) {
  switch (which) {
    case 0: return MSM_BIT_SUMS;
    case 1: return sizeof(G1);
    case 2: return KZE_FINISH_CHUNK;
    case 3: return KZE_TABLE_GROUP;
    case 4: return KZE_FINISH_LANES;
    default: return 0;
  }
}

}  // extern "C"
