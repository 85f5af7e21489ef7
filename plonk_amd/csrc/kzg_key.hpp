// The opening key behind a plonk_kzg_key handle (kzg.hip creates and destroys it): shared with the cell verifier
// (kzg_cell_verify.hip), which reads its prepared G2 points, its decoded g and its device line tables.
#pragma once
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

}  // namespace plonk
