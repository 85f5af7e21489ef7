// CPU harness for plonk_amd/csrc/kzg_domain_core.hpp (the index maps, the twiddle of a butterfly, the chunk plan, the
// operation counts and the argument checks of the whole-domain KZG10 openings), compiled with g++ by
// tests/test_kzg_domain_model_host.py and checked against the big-int model tests/kzg_domain_model.py.
#include "../../plonk_amd/csrc/kzg_domain_core.hpp"

using namespace plonk;

extern "C" {

uint64_t hkd_const(int which) {
  switch (which) {
    case 0: return KZD_MIN_LOG;
    case 1: return KZD_MAX_LOG;
    case 2: return KZD_MAX_COUNT;
    case 3: return KZD_SLOT_BYTES;
    case 4: return KZD_WS_CAP_DEFAULT;
    case 5: return KZD_MAX_CHUNK;
    case 6: return KZD_NONE;
    default: return 0;
  }
}
uint64_t hkd_rev(uint64_t i, uint32_t bits) { return kzd_rev(i, bits); }
uint64_t hkd_g_src(uint64_t n, uint64_t t) { return kzd_g_src(n, t); }
uint64_t hkd_h_src(uint64_t n, uint64_t k) { return kzd_h_src(n, k); }
uint64_t hkd_twiddle(uint32_t size_log, uint64_t half, uint64_t j, uint32_t tw_log, int inverse, int* negate) {
  bool neg = false;
  const uint64_t e = kzd_twiddle(size_log, half, j, tw_log, inverse != 0, &neg);
  *negate = neg ? 1 : 0;
  return e;
}
uint64_t hkd_stage_muls(uint32_t size_log, uint64_t half) { return kzd_stage_muls(size_log, half); }
uint64_t hkd_transform_muls(uint32_t size_log) { return kzd_transform_muls(size_log); }
void hkd_plan(uint32_t log_n, uint64_t count, uint64_t cap_bytes, uint64_t out[5]) {
  const KzdPlan p = kzd_plan(log_n, count, cap_bytes);
  out[0] = p.chunk_polys;
  out[1] = p.chunks;
  out[2] = p.ws_bytes;
  out[3] = p.stage_launches;
  out[4] = p.scalar_muls;
}
int hkd_check_create(uint32_t log_n, int has_comm, int has_srs, uint64_t srs_n) {
  return kzd_check_create(log_n, has_comm != 0, has_srs != 0, srs_n);
}
int hkd_check_len(uint32_t log_n, uint64_t trimmed) { return kzd_check_len(log_n, trimmed); }

}  // extern "C"
