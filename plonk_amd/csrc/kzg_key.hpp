// The opening key behind a plonk_kzg_key handle (kzg.hip creates and destroys it): shared with the cell verifier
// (kzg_cell_verify.hip), which reads its prepared G2 points, its decoded g and its device line tables, and the two small
// helpers the files of the check calls (kzg.hip, kzg_cell_verify.hip, kzg_multiproof.hip) have in common.
#pragma once
#include <chrono>

#include "plonk_internal.hpp"
#include "hostg1.hpp"
#include "hostpairing.hpp"
#include "verify_core.hpp"

namespace plonk { struct KzgKey; }
struct plonk_kzg_key {
  plonk::KzgKey* k;
  plonk_ctx* ctx;
};

namespace plonk {

struct KzgKey {
  Ctx* c = nullptr;
  uint8_t opening_key[OPENING_KEY_LEN];
  G2Prepared h, x_h;
  G1Affine g_aff;        // g as decoded on the device
  Fr last_u, last_r;     // the challenges of the last batch_check / srs_check (test hook)
  void* pair_tables = nullptr;   // device: the lines of x_h and h for the pairing kernel, made by the first per-item call
  void* multiproof = nullptr;    // the workspace of plonk_kzg_multiproof_check (kzg_multiproof.hip), made by its first call
  ~KzgKey();                     // kzg_multiproof.hip: frees both
};

// the phase times of a check call (plonk_verify_info)
inline double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// a launcher of the check calls' files refuses its arguments: `what` names it in the last-error text
inline int kzg_bad_args(const char* what) {
  set_last_error(what, "invalid argument", __FILE__, __LINE__);
  return PLONK_ERR_ARG;
}

}  // namespace plonk
