// CPU harness for what a KZG domain handle with Lagrange-basis tables adds: the plan of its grouped table launches
// (plonk_amd/csrc/kzg_evals_core.hpp kze_tables_plan) and the lane function of kze_finish_kernel — the finishing chain
// (kzg_evals_finish.cuh) and the 48-byte encoding (g1codec.cuh) — compiled with g++ by tests/test_kzg_evals_tables_host.py and
// checked against the big-int model tests/kzg_evals_tables_model.py.
#include <string.h>

#include "../../plonk_amd/csrc/g1codec.cuh"
#include "../../plonk_amd/csrc/kzg_evals_core.hpp"
#include "../../plonk_amd/csrc/kzg_evals_finish.cuh"

using namespace plonk;

namespace {
struct HostLoad {
  const G1* b;
  G1R operator()(int slot) const { return g1r_of_g1(b[slot]); }
};
}  // namespace

extern "C" {

void hkt_plan(uint64_t commitments, uint64_t group_vectors, uint64_t joined, uint64_t separate, uint64_t out[5]) {
  const KzeTablesPlan p = kze_tables_plan(commitments, group_vectors, joined, separate);
  out[0] = p.msms;
  out[1] = p.group_launches;
  out[2] = p.device_finished;
  out[3] = p.finish_launches;
  out[4] = p.last_chunk;
}
uint64_t hkt_const(int which) {
  switch (which) {
    case 0: return KZE_TABLE_GROUP;
    case 1: return KZE_FINISH_CHUNK;
    case 2: return KZE_FINISH_LANES;
    case 3: return sizeof(G1);
    default: return 0;
  }
}
// bits: count x slots G1 (192 bytes each); out48: count x 48
void hkt_finish(const uint8_t* bits, uint32_t count, uint32_t slots, int rb, int bitpos, uint8_t* out48) {
  for (uint32_t i = 0; i < count; ++i) {
    G1 b[32];
    memcpy(b, bits + (size_t)i * slots * sizeof(G1), (size_t)slots * sizeof(G1));
    const HostLoad ld = {b};
    const G1R acc = kze_finish_chain(ld, rb, bitpos != 0);
    uint32_t w[12];
    g1r_compress48_words(acc, w);
    memcpy(out48 + 48 * (size_t)i, w, 48);
  }
}

}  // extern "C"
