// CPU test harness of the host-callable half of witness diagnosis: diagnose_core.hpp (the 17 identities of a row over plain
// Fr, the sigma decoding) compiled with g++ and driven from tests/test_diagnose_host.py through ctypes.  The copy check
// below is the one diagnose.hip's row kernel runs: compare the cell with the cell its decoded position names.
#include <cstdint>
#include <cstring>

#include "../../plonk_amd/csrc/diagnose_core.hpp"

using namespace plonk;

namespace {
struct HostLoader {
  uint64_t n, i;
  const Fr* wires;
  const Fr* const* selv;
  const Fr* pis;
  Fr wire(int col) const { return wires[(uint64_t)col * n + i]; }
  Fr wire_next(int col) const { return wires[(uint64_t)col * n + ((i + 1) & (n - 1))]; }
  bool sel_nonzero(int id) const { return selv[id] && !selv[id][i].is_zero(); }
  Fr sel(int id) const { return selv[id] ? selv[id][i] : Fr::zero(); }
  Fr pi() const { return pis ? pis[i] : Fr::zero(); }
};
}  // namespace

extern "C" {

// pos[k] = decoded position of sigma value k (Montgomery limbs), 0xFFFFFFFF when it decodes to none
void hd_sigma_decode(uint32_t logn, uint64_t count, const uint32_t* s_mont, uint32_t* pos) {
  const SigmaDecodeConsts<Fr> k = sigma_decode_consts_fr(logn);
  for (uint64_t i = 0; i < count; ++i) {
    Fr s;
    memcpy(s.l, s_mont + 8 * i, 32);
    pos[i] = sigma_decode<Fr>(s, k);
  }
}

// families[i] / copy[i] of every row i < n = 2^logn.  wires: [4][n]; sel[id]: [n] selector values or NULL; pi: [n] dense or
// NULL — all Montgomery limbs; pos: [4][n] positions as hd_sigma_decode returns them for the sigma evaluations.
void hd_report(uint32_t logn, const uint32_t* wires_mont, const uint32_t* const* sel_mont, const uint32_t* pi_mont,
               const uint32_t* pos, uint32_t* families, uint32_t* copy) {
  const uint64_t n = 1ull << logn;
  const DiagConsts<Fr> k = diag_consts_fr();
  const Fr* wires = reinterpret_cast<const Fr*>(wires_mont);
  const Fr* selv[DQ_COUNT];
  bool widgets = false;
  for (int id = 0; id < DQ_COUNT; ++id) {
    selv[id] = reinterpret_cast<const Fr*>(sel_mont[id]);
    if (id >= DQ_RANGE && selv[id]) widgets = true;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const HostLoader ld{n, i, wires, selv, reinterpret_cast<const Fr*>(pi_mont)};
    families[i] = diag_row_families<Fr>(ld, k, widgets);
    uint32_t cp = 0;
    for (uint32_t col = 0; col < 4; ++col) {
      const uint32_t to = pos[(uint64_t)col * n + i];
      bool bad = to == DIAG_POS_NONE;
      if (!bad) bad = !(wires[(uint64_t)col * n + i] == wires[(uint64_t)(to >> SIGMA_ROW_BITS) * n + (to & ((1u << SIGMA_ROW_BITS) - 1))]);
      if (bad) cp |= 1u << col;
    }
    copy[i] = cp;
  }
}

}  // extern "C"
