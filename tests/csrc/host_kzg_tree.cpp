// plonk_amd/csrc/kzg_tree_core.hpp compiled with g++ for tests/test_kzg_tree_host.py: the level sets, the update plan, the
// canonical order of a proof, the chunk plans and the map h, behind plain C entry points.  The caller sizes every output for
// the worst case: (depth + 1) x count entries for the sets, depth x count for nodes / terms, depth x (count + 1) for offsets.
// Test code only.
#include "../../plonk_amd/csrc/kzg_tree_core.hpp"

using namespace plonk;

extern "C" {

int hkt_check_shape(uint32_t log_n, uint32_t depth) { return kzt_check_shape(log_n, depth); }
uint64_t hkt_data_bytes(uint32_t log_n, uint32_t depth) { return kzt_data_bytes(log_n, depth); }
uint64_t hkt_nodes(uint32_t log_n, uint32_t depth) { return kzt_nodes(log_n, depth); }

uint64_t hkt_const(int which) {
  switch (which) {
    case 0: return KZT_LOG_N_MAX;
    case 1: return KZT_MAX_BITS;
    case 2: return KZT_MAX_UPDATE;
    case 3: return KZT_MAX_PROOF_NODES;
    case 4: return KZT_MAX_CLAIMS;
    case 5: return KZT_MSG_POS;
    default: return 0;
  }
}

// sizes[l] = |T_l|, l <= depth; flat: T_0, T_1, .. one after the other; order[k]
int hkt_sets(uint32_t log_n, uint32_t depth, const uint64_t* idx, uint64_t count, uint64_t max_count, uint64_t* sizes, uint64_t* flat,
             uint64_t* order) {
  KztSets s;
  const int rc = kzt_sets(log_n, depth, idx, count, max_count, &s);
  if (rc != PLONK_OK) return rc;
  for (uint32_t l = 0; l <= depth; ++l) {
    sizes[l] = s.T[l].size();
    for (uint64_t v : s.T[l]) *flat++ = v;
  }
  for (uint64_t k = 0; k < count; ++k) order[k] = s.order[k];
  return PLONK_OK;
}

int hkt_proof_nodes(uint32_t log_n, uint32_t depth, const uint64_t* idx, uint64_t count, uint64_t* nodes) {
  return kzt_proof_nodes(log_n, depth, idx, count, nodes);
}

// counts: vectors, items, path_nodes; level_vector: depth + 1
int hkt_proof_plan(uint32_t log_n, uint32_t depth, const uint64_t* idx, uint64_t count, uint64_t* counts, uint64_t* level_vector,
                   uint32_t* vector_index, uint32_t* point_index) {
  KztSets s;
  KztProofPlan p;
  int rc = kzt_sets(log_n, depth, idx, count, KZT_MAX_CLAIMS, &s);
  if (rc == PLONK_OK) rc = kzt_proof_plan(s, &p);
  if (rc != PLONK_OK) return rc;
  counts[0] = p.vectors;
  counts[1] = p.items;
  counts[2] = p.path_nodes;
  for (uint32_t l = 0; l <= depth; ++l) level_vector[l] = p.level_vector[l];
  for (uint64_t k = 0; k < p.items; ++k) {
    vector_index[k] = p.vector_index[k];
    point_index[k] = p.point_index[k];
  }
  return PLONK_OK;
}

// levels: depth x (nodes, terms, node_at, offs_at, term_at), bottom up; totals: touched, terms, most_nodes, most_terms, chunks
int hkt_update_plan(uint32_t log_n, uint32_t depth, const uint64_t* idx, uint64_t count, uint64_t ws_cap, uint64_t* levels, uint64_t* node,
                    uint64_t* offsets, uint64_t* flat, uint32_t* child, uint64_t* totals) {
  KztSets s;
  const int rc = kzt_sets(log_n, depth, idx, count, KZT_MAX_UPDATE, &s);
  if (rc != PLONK_OK) return rc;
  KztUpdatePlan p;
  kzt_update_plan(s, &p);
  for (uint32_t k = 0; k < depth; ++k) {
    const KztUpdateLevel& lv = p.level[k];
    const uint64_t row[5] = {lv.nodes, lv.terms, lv.node_at, lv.offs_at, lv.term_at};
    for (int i = 0; i < 5; ++i) levels[5 * k + i] = row[i];
  }
  for (size_t i = 0; i < p.node.size(); ++i) node[i] = p.node[i];
  for (size_t i = 0; i < p.offsets.size(); ++i) offsets[i] = p.offsets[i];
  for (size_t i = 0; i < p.flat.size(); ++i) flat[i] = p.flat[i];
  for (size_t i = 0; i < p.child.size(); ++i) child[i] = p.child[i];
  totals[0] = p.touched;
  totals[1] = p.terms;
  totals[2] = p.most_nodes;
  totals[3] = p.most_terms;
  totals[4] = kzt_update_chunks(p, ws_cap);
  return PLONK_OK;
}

// out: nodes, chunks, most_partials
void hkt_build_plan(uint32_t log_n, uint32_t depth, uint32_t window_bits, uint64_t ws_cap, uint64_t* out) {
  const KztBuildPlan p = kzt_build_plan(log_n, depth, window_bits, ws_cap);
  out[0] = p.nodes;
  out[1] = p.chunks;
  out[2] = p.most_partials;
}

// h by the seeded route the map kernel runs (0: the seed could not be made) ...
int hkt_map(const uint8_t* c48, uint32_t* out8) {
  KztSeed seed;
  if (!kzt_map_seed(&seed)) return 0;
  const Fr v = kzt_map_bytes(seed, c48);
  for (int k = 0; k < 8; ++k) out8[k] = v.l[k];
  return 1;
}
// the same for `count` commitments in one call (tools/kzg_tree_bench.py: the host leg of the route a caller had before)
int hkt_map_many(const uint8_t* c48, uint64_t count, uint32_t* out8) {
  KztSeed seed;
  if (!kzt_map_seed(&seed)) return 0;
  for (uint64_t j = 0; j < count; ++j) {
    const Fr v = kzt_map_bytes(seed, c48 + 48 * j);
    for (int k = 0; k < 8; ++k) out8[8 * j + k] = v.l[k];
  }
  return 1;
}
// ... and by the transcript itself
void hkt_map_transcript(const uint8_t* c48, uint32_t* out8) {
  Transcript t((const uint8_t*)"kzg10-tree-v1", 13);
  t.append_message("node", c48, 48);
  const Fr v = t.challenge_scalar("node-scalar");
  for (int k = 0; k < 8; ++k) out8[k] = v.l[k];
}

}  // extern "C"
