// CPU test harness of the quarter-density recoding: plonk_amd/csrc/msm_recode.cuh for_each_digit_quad<16> / <20> (exactly what
// msm_hist_kernel and msm_partition_kernel run for 64-row tables) compiled with g++ and driven from tests/test_msm_quad_host.py
// through ctypes.  A scalar goes through the recoding twice: held in "registers" (limb_select's select chain) and parked
// limb-major with a stride, as the kernels park it in LDS (StridedLimbs, nine limbs).
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "../../plonk_amd/csrc/msm_recode.cuh"

using namespace plonk;

namespace {

struct Emit {
  uint32_t* out;   // 4 words per digit: slot, row, bucket, sign
  uint32_t n;
  void operator()(int slot, uint32_t row, uint32_t bucket, uint32_t sign) {
    out[4 * n] = (uint32_t)slot; out[4 * n + 1] = row; out[4 * n + 2] = bucket; out[4 * n + 3] = sign;
    ++n;
  }
};

template <class S>
uint32_t run(const S& s, uint32_t w, uint32_t* out) {
  Emit e{out, 0};
  if (w == 16) for_each_digit_quad<16>(s, e);
  else if (w == 20) for_each_digit_quad<20>(s, e);
  else if (w == 0) {   // the run-time dispatch: 64 rows -> width 16 (register scalars only: the window recoding reads s.l)
    if constexpr (std::is_same<S, Fr>::value) for_each_digit(s, MSM_ROWS_QUARTERPOS, e);
    else return ~0u;
  } else return ~0u;
  return e.n;
}

}  // namespace

extern "C" {

// k: canonical scalar (8 words); strided = 1: through StridedLimbs.  out: room for 16 digits x 4 words.  Returns the digit count.
uint32_t hmq_digits(const uint32_t k[8], uint32_t w, uint32_t strided, uint32_t* out) {
  if (strided) {
    uint32_t park[3 * 9 + 1];          // stride 3, starting at word 1: neighbours hold a pattern the recoding must not read
    for (uint32_t i = 0; i < 3 * 9 + 1; ++i) park[i] = 0xa5a5a5a5u;
    for (uint32_t j = 0; j < 8; ++j) park[1 + 3 * j] = k[j];
    park[1 + 3 * 8] = 0;
    return run(StridedLimbs{park + 1, 3}, w, out);
  }
  Fr s;
  memcpy(s.l, k, 32);
  return run(s, w, out);
}

// digits of n canonical scalars (8 words each), summed: the mean digit count without a Python loop per digit
uint64_t hmq_count(const uint32_t* k, uint64_t n, uint32_t w) {
  uint64_t total = 0;
  uint32_t out[64];
  for (uint64_t i = 0; i < n; ++i) total += hmq_digits(k + 8 * i, w, 1, out);
  return total;
}

uint32_t hmq_rows() { return MSM_ROWS_QUARTERPOS; }

}  // extern "C"
