// Argument blocks + launchers of diagnose.hip (witness diagnosis: which rows fail which gate identity / copy constraint).
#pragma once
#include "plonk_internal.hpp"
#include "diagnose_core.hpp"

namespace plonk {

// what the compaction leaves on the device for the host to read (one small copy per call)
struct DiagCounters {
  unsigned long long failing;        // rows with a non-empty mask
  unsigned long long family[18];     // rows failing identity f (0..16); [17] = rows with a copy-constraint failure
  unsigned long long first_row;      // lowest failing row (valid when failing != 0)
  uint32_t first_families, first_copy;
};
struct DiagArgs {
  uint64_t n;
  const Fr* wires;               // [4][n] a | b | c | d over the whole domain
  const Fr* pi;                  // [n] dense public-input values, or nullptr (none)
  const Fr* sel[DQ_COUNT];       // selector values on the domain; nullptr = the polynomial is identically zero
  const uint32_t* pos;           // [4][n] sigma decoded into packed positions (permutation.hpp), DIAG_POS_NONE = undecodable
  uint32_t* mask;                // [n] families (bits 0..16) | copy_wires << DIAG_COPY_SHIFT
  uint32_t* block_cnt;           // [diag_blocks(n)] failing rows per workgroup, then their exclusive scan in block_off
  uint32_t* block_off;
  DiagCounters* ctr;
  plonk_unsat_row* out;          // [min(cap, n)] records, ascending
  uint64_t cap;
};
static constexpr uint32_t DIAG_COPY_SHIFT = 24;
static constexpr uint32_t DIAG_T = 256;   // rows per workgroup of the row and scatter kernels
inline uint64_t diag_blocks(uint64_t n) { return (n + DIAG_T - 1) / DIAG_T; }

int diag_sigma_decode(Ctx* c, const Fr* sigma_n, uint32_t* pos, uint64_t n, uint32_t logn);
int diag_report(Ctx* c, const DiagArgs& a);   // row kernel, scan, ordered scatter; all on c->stream, no synchronisation

}  // namespace plonk
