// A stand-alone driver of plonk_amd/csrc/kzg_tree_core.hpp for a build with -fsanitize=address,undefined: the index logic takes
// the caller's indices as they come, so it is run here, on the CPU, over the cases tests/test_kzg_tree_host.py writes to
// standard input — one per line: log_n depth ws_cap count idx_0 .. idx_(count-1) — and prints per case one line of results
// that the test compares with the model:   rc_sets rc_proof vectors items path_nodes touched terms chunks checksum
// (checksum: a running sum over every output entry, so that every entry is read).  Test code only; never loaded into Python.
#include <stdio.h>

#include <sstream>
#include <string>
#include <iostream>

#include "../../plonk_amd/csrc/kzg_tree_core.hpp"

using namespace plonk;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    uint32_t log_n = 0, depth = 0;
    uint64_t ws_cap = 0, count = 0;
    if (!(in >> log_n >> depth >> ws_cap >> count)) continue;
    std::vector<uint64_t> idx(count);
    for (uint64_t k = 0; k < count; ++k) in >> idx[k];
    KztSets s;
    const int rc = kzt_sets(log_n, depth, count ? idx.data() : nullptr, count, KZT_MAX_CLAIMS, &s);
    if (rc != PLONK_OK) {
      printf("%d 0 0 0 0 0 0 0 0\n", rc);
      continue;
    }
    uint64_t sum = 0;
    for (const std::vector<uint64_t>& level : s.T)
      for (uint64_t v : level) sum += v;
    for (uint64_t v : s.order) sum += 3 * v;
    KztProofPlan pp;
    const int rc_proof = kzt_proof_plan(s, &pp);
    if (rc_proof == PLONK_OK) {
      for (uint64_t k = 0; k < pp.items; ++k) sum += 5 * (uint64_t)pp.vector_index[k] + 7 * (uint64_t)pp.point_index[k];
      for (uint64_t v : pp.level_vector) sum += 11 * v;
    }
    KztUpdatePlan up;
    kzt_update_plan(s, &up);
    for (uint64_t v : up.node) sum += 13 * v;
    for (uint64_t v : up.offsets) sum += 17 * v;
    for (uint64_t v : up.flat) sum += 19 * v;
    for (uint32_t v : up.child) sum += 23 * (uint64_t)v;
    const uint64_t chunks = kzt_update_chunks(up, ws_cap);
    uint64_t nodes = 0;
    (void)kzt_proof_nodes(log_n, depth, idx.data(), count, &nodes);
    printf("%d %d %llu %llu %llu %llu %llu %llu %llu\n", rc, rc_proof, (unsigned long long)pp.vectors, (unsigned long long)pp.items,
           (unsigned long long)(rc_proof == PLONK_OK ? nodes : 0), (unsigned long long)up.touched, (unsigned long long)up.terms,
           (unsigned long long)chunks, (unsigned long long)sum);
  }
  return 0;
}
