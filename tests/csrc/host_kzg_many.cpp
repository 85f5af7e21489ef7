// CPU harness for what the host decides of the many-vector commitments on a KZG domain handle
// (plonk_amd/csrc/kzg_many_core.hpp): the recoding the accumulation kernel runs per value, W(c), the table size and indexing,
// the automatic width, the plans and the argument checks — compiled with g++ by tests/test_kzg_many_host.py and checked
// against the big-int model tests/kzg_many_model.py.
#include <string.h>

#include "../../plonk_amd/csrc/kzg_many_core.hpp"

using namespace plonk;

namespace {
void put(const KzmPlan& p, uint64_t out[9]) {
  out[0] = p.log_n;
  out[1] = p.window_bits;
  out[2] = p.windows;
  out[3] = p.slices;
  out[4] = p.count;
  out[5] = p.terms;
  out[6] = p.chunk_vectors;
  out[7] = p.chunks;
  out[8] = p.additions;
}
}  // namespace

extern "C" {

uint32_t hkm_windows(uint32_t c) { return kzm_windows(c); }
// s: 8 x 32-bit limbs, canonical; returns the carry out of the last window
uint32_t hkm_recode(const uint32_t s[8], uint32_t c, uint32_t windows, int32_t* digits) { return kzm_recode(s, c, windows, digits); }
uint64_t hkm_table_bytes(uint32_t log_n, uint32_t c) { return kzm_table_bytes(log_n, c); }
uint64_t hkm_entry(uint32_t c, uint64_t i, uint32_t w, uint32_t d) { return kzm_entry(c, kzm_windows(c), i, w, d); }
uint32_t hkm_auto_width(uint32_t log_n, uint64_t left) { return kzm_auto_width(log_n, left); }
uint32_t hkm_slices(uint32_t log_n, uint64_t count, uint32_t force) { return kzm_slices(log_n, count, force); }
void hkm_plan(uint32_t log_n, uint32_t c, uint64_t count, uint64_t ws_cap, int host_form, uint32_t force_slices, uint64_t out[9]) {
  put(kzm_plan(log_n, c, count, ws_cap, host_form != 0, force_slices), out);
}
void hkm_sparse_plan(uint32_t log_n, uint32_t c, const uint64_t* offsets, uint64_t count, uint64_t ws_cap, uint64_t out[9]) {
  put(kzm_sparse_plan(log_n, c, offsets, count, ws_cap), out);
}
int hkm_check_build(int has_domain, uint32_t log_n, uint32_t window_bits) { return kzm_check_build(has_domain != 0, log_n, window_bits); }
int hkm_check_commit(int has_domain, int has_values, int has_out, uint64_t count) {
  return kzm_check_commit(has_domain != 0, has_values != 0, has_out != 0, count);
}
int hkm_check_update(int has_domain, const uint64_t* offsets, const uint32_t* index, int has_deltas, int has_out, uint64_t count, uint32_t log_n) {
  return kzm_check_update(has_domain != 0, offsets, index, has_deltas != 0, has_out != 0, count, log_n);
}
uint64_t hkm_const(int which) {
  switch (which) {
    case 0: return KZM_RESIDENT_WAVES;
    case 1: return KZM_ENTRY_BYTES;
    case 2: return KZM_SLOT_BYTES;
    case 3: return KZM_CHUNK_MAX;
    case 4: return KZM_TERM_BYTES;
    case 5: return KZM_MAX_COUNT;
    case 6: return KZM_MAX_TERMS;
    case 7: return KZM_LANES;
    case 8: return KZM_LOG_N_MAX;
    case 9: return KZM_MAX_SEGMENT;
    default: return 0;
  }
}

}  // extern "C"
