// KZG10 vector-commitment trees (kzg_tree.hip): everything the host decides from the shape and from the leaf indices of a call
// — the level sets, the segments and child indices of an update, the canonical order of a proof and its node count, the chunk
// plan of a build — and the map h from a commitment to the scalar its parent commits to.  HD and HIP-free like
// kzg_many_core.hpp: the handle, plonk_kzg_tree_check and the map kernel call these functions, tests/csrc/host_kzg_tree.cpp
// compiles them with g++ against the big-int model tests/kzg_tree_model.py.  The indices are the caller's and are trusted for
// nothing: every function here that takes them checks them first.
//
// A tree over a domain of n = 2^log_n values with depth D is complete: level l (0 = the root) has n^l nodes, node (l, k)
// commits to vals[l][k n .. k n + n), vals[D-1] holds the N = n^D leaves and vals[l][j] = h(C[l+1][j]) above them.  The flat
// index j of a value of level l is also the index of its child node on level l + 1, so for a set of leaves T_D
//     T_l = { j >> log_n : j in T_(l+1) }          l = D-1 .. 0,   T_0 = { 0 }
// names both the touched nodes of level l and the touched values of vals[l-1].
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/plonk_hip.h"
#include "field.cuh"
#include "kzg_many_core.hpp"
#include "transcript.hpp"

namespace plonk {

static constexpr uint32_t KZT_LOG_N_MAX = KZM_LOG_N_MAX;
static constexpr uint32_t KZT_MAX_BITS = 26;                // depth x log_n at most: 2^26 leaves, 2 GiB of them
static constexpr uint64_t KZT_MAX_UPDATE = 1ull << 20;      // leaves of one plonk_kzg_tree_update
static constexpr uint64_t KZT_MAX_PROOF_NODES = 65536;      // distinct nodes of one proof: the vectors of the multiproof
static constexpr uint64_t KZT_MAX_CLAIMS = 1ull << 20;      // its items
static constexpr uint32_t KZT_LANES = 64;
static constexpr uint32_t KZT_MSG_POS = 53;                 // where the 48 bytes of a node meet the STROBE state (kzt_map_seed)
enum : uint32_t { KZT_NONE = 0, KZT_BUILD = 1, KZT_UPDATE = 2, KZT_PROVE = 3 };   // plonk_kzg_tree_info.kind

HD int kzt_check_shape(uint32_t log_n, uint32_t depth) {
  if (log_n < 1 || log_n > KZT_LOG_N_MAX || depth < 1 || depth > KZT_MAX_BITS) return PLONK_ERR_ARG;
  return depth * log_n <= KZT_MAX_BITS ? PLONK_OK : PLONK_ERR_ARG;
}
HD uint64_t kzt_level_nodes(uint32_t log_n, uint32_t level) { return 1ull << (log_n * level); }
HD uint64_t kzt_leaves(uint32_t log_n, uint32_t depth) { return 1ull << (log_n * depth); }
HD uint64_t kzt_nodes(uint32_t log_n, uint32_t depth) {
  uint64_t s = 0;
  for (uint32_t l = 0; l < depth; ++l) s += kzt_level_nodes(log_n, l);
  return s;
}
// what a tree holds per level: the values, and per node 48 + 96 + 4 bytes
HD uint64_t kzt_data_bytes(uint32_t log_n, uint32_t depth) {
  uint64_t s = 0;
  for (uint32_t l = 0; l < depth; ++l) s += 32 * kzt_level_nodes(log_n, l + 1) + 148 * kzt_level_nodes(log_n, l);
  return s;
}

// ---- the level sets -------------------------------------------------------------------------------------------------------------
struct KztSets {
  uint32_t log_n = 0, depth = 0;
  std::vector<std::vector<uint64_t>> T;   // T[l], l = 0 .. depth, each ascending
  std::vector<uint64_t> order;            // order[k]: where the caller's arrays hold the leaf T[depth][k]
  uint64_t nodes_from(uint32_t first, uint32_t last) const {   // |T_first| + .. + |T_last|
    uint64_t s = 0;
    for (uint32_t l = first; l <= last && l < T.size(); ++l) s += T[l].size();
    return s;
  }
};

// PLONK_ERR_ARG for a shape out of range, a NULL or empty list, more than max_count indices, an index >= N, a repeated index
inline int kzt_sets(uint32_t log_n, uint32_t depth, const uint64_t* leaf_index, uint64_t count, uint64_t max_count, KztSets* out) {
  if (kzt_check_shape(log_n, depth) != PLONK_OK || !leaf_index || !count || count > max_count) return PLONK_ERR_ARG;
  const uint64_t N = kzt_leaves(log_n, depth);
  if (count > N) return PLONK_ERR_ARG;   // (more indices than leaves: one repeats)
  std::vector<std::pair<uint64_t, uint64_t>> s(count);
  for (uint64_t k = 0; k < count; ++k) {
    if (leaf_index[k] >= N) return PLONK_ERR_ARG;
    s[k] = std::make_pair(leaf_index[k], k);
  }
  std::sort(s.begin(), s.end());
  for (uint64_t k = 1; k < count; ++k)
    if (s[k].first == s[k - 1].first) return PLONK_ERR_ARG;
  out->log_n = log_n;
  out->depth = depth;
  out->T.assign(depth + 1, std::vector<uint64_t>());
  out->order.resize(count);
  std::vector<uint64_t>& leaves = out->T[depth];
  leaves.resize(count);
  for (uint64_t k = 0; k < count; ++k) {
    leaves[k] = s[k].first;
    out->order[k] = s[k].second;
  }
  for (uint32_t l = depth; l > 0; --l) {
    const std::vector<uint64_t>& below = out->T[l];
    std::vector<uint64_t>& up = out->T[l - 1];
    for (uint64_t k = 0; k < below.size(); ++k) {
      const uint64_t parent = below[k] >> log_n;
      if (up.empty() || up.back() != parent) up.push_back(parent);
    }
  }
  return PLONK_OK;
}

// ---- the update plan ------------------------------------------------------------------------------------------------------------
// Per level l = depth-1 .. 0 (step s = depth-1 - l): the touched nodes T_l, one segment per node over the touched values
// T_(l+1) of vals[l], and of each value its child index j mod n.  Everything is a pure function of the indices: made once,
// uploaded once.
struct KztUpdateLevel {
  uint64_t nodes, terms;          // |T_l|, |T_(l+1)|
  uint64_t node_at, offs_at, term_at;   // where the level starts in node / offsets / (flat, child)
};
struct KztUpdatePlan {
  std::vector<KztUpdateLevel> level;   // [depth], bottom up
  std::vector<uint64_t> node;          // T_l
  std::vector<uint64_t> offsets;       // nodes + 1 per level, relative to the level's first term
  std::vector<uint64_t> flat;          // T_(l+1): the index into vals[l]
  std::vector<uint32_t> child;         // flat mod n
  uint64_t touched = 0, terms = 0, most_nodes = 0, most_terms = 0;
};

inline void kzt_update_plan(const KztSets& s, KztUpdatePlan* p) {
  const uint32_t D = s.depth, L = s.log_n;
  const uint64_t mask = (1ull << L) - 1;
  *p = KztUpdatePlan();
  p->level.resize(D);
  for (uint32_t step = 0; step < D; ++step) {
    const uint32_t l = D - 1 - step;
    const std::vector<uint64_t>&nodes = s.T[l], &vals = s.T[l + 1];
    KztUpdateLevel& lv = p->level[step];
    lv.nodes = nodes.size();
    lv.terms = vals.size();
    lv.node_at = p->node.size();
    lv.offs_at = p->offsets.size();
    lv.term_at = p->flat.size();
    uint64_t k = 0;
    for (uint64_t j = 0; j < nodes.size(); ++j) {
      p->node.push_back(nodes[j]);
      p->offsets.push_back(k);
      while (k < vals.size() && (vals[k] >> L) == nodes[j]) {
        p->flat.push_back(vals[k]);
        p->child.push_back((uint32_t)(vals[k] & mask));
        ++k;
      }
    }
    p->offsets.push_back(k);
    p->touched += lv.nodes;
    p->terms += lv.terms;
    if (lv.nodes > p->most_nodes) p->most_nodes = lv.nodes;
    if (lv.terms > p->most_terms) p->most_terms = lv.terms;
  }
}
// chunks of the sparse accumulation of one level under the workspace cap (kzm_sparse_chunk over the level's offsets)
inline uint64_t kzt_update_chunks(const KztUpdatePlan& p, uint64_t ws_cap) {
  uint64_t chunks = 0;
  for (const KztUpdateLevel& lv : p.level)
    for (uint64_t first = 0; first < lv.nodes; ++chunks) first += kzm_sparse_chunk(p.offsets.data() + lv.offs_at, lv.nodes, first, ws_cap);
  return chunks;
}

// ---- the canonical order of a proof --------------------------------------------------------------------------------------------------
// Vectors: the nodes of T_0, T_1, .., T_(D-1).  Items: per level l in that order the values T_(l+1) of vals[l], as (the vector of
// node j >> log_n, point j mod n).  Path commitments: the nodes of T_1 .. T_(D-1); the items of level l < D-1 are one to one with
// the path commitments of level l + 1, in the same order.
struct KztProofPlan {
  uint64_t vectors = 0, items = 0, path_nodes = 0;
  std::vector<uint64_t> level_vector;            // [depth + 1]: the first vector of level l
  std::vector<uint32_t> vector_index, point_index;
};
HD int kzt_check_proof_size(uint64_t vectors, uint64_t items) {
  return vectors <= KZT_MAX_PROOF_NODES && items <= KZT_MAX_CLAIMS ? PLONK_OK : PLONK_ERR_ARG;
}
inline int kzt_proof_plan(const KztSets& s, KztProofPlan* p) {
  const uint32_t D = s.depth, L = s.log_n;
  const uint64_t mask = (1ull << L) - 1;
  *p = KztProofPlan();
  p->vectors = s.nodes_from(0, D - 1);
  p->items = s.nodes_from(1, D);
  p->path_nodes = D > 1 ? s.nodes_from(1, D - 1) : 0;
  if (kzt_check_proof_size(p->vectors, p->items) != PLONK_OK) return PLONK_ERR_ARG;
  p->level_vector.resize(D + 1);
  p->vector_index.reserve(p->items);
  p->point_index.reserve(p->items);
  uint64_t base = 0;
  for (uint32_t l = 0; l < D; ++l) {
    p->level_vector[l] = base;
    const std::vector<uint64_t>&nodes = s.T[l], &vals = s.T[l + 1];
    uint64_t r = 0;
    for (uint64_t k = 0; k < vals.size(); ++k) {
      while (nodes[r] != (vals[k] >> L)) ++r;   // (both ascending, every parent present: r stays below nodes.size())
      p->vector_index.push_back((uint32_t)(base + r));
      p->point_index.push_back((uint32_t)(vals[k] & mask));
    }
    base += nodes.size();
  }
  p->level_vector[D] = base;
  return PLONK_OK;
}
// plonk_kzg_tree_proof_nodes
inline int kzt_proof_nodes(uint32_t log_n, uint32_t depth, const uint64_t* leaf_index, uint64_t count, uint64_t* nodes) {
  KztSets s;
  const int rc = kzt_sets(log_n, depth, leaf_index, count, KZT_MAX_CLAIMS, &s);
  if (rc != PLONK_OK) return rc;
  const uint64_t vectors = s.nodes_from(0, depth - 1), items = s.nodes_from(1, depth);
  if (kzt_check_proof_size(vectors, items) != PLONK_OK) return PLONK_ERR_ARG;
  *nodes = vectors - 1;
  return PLONK_OK;
}

// ---- the chunk plan of a build ----------------------------------------------------------------------------------------------------------
// level l = depth-1 .. 0 commits its n^l nodes as plonk_kzg_commit_many_dev would (kzm_plan, resident form, the plan's own slices)
struct KztBuildPlan {
  uint64_t nodes = 0, chunks = 0, most_partials = 0;   // the partial sums of the largest chunk
  KzmPlan level[KZT_MAX_BITS];                         // [depth], indexed by level
};
inline KztBuildPlan kzt_build_plan(uint32_t log_n, uint32_t depth, uint32_t window_bits, uint64_t ws_cap) {
  KztBuildPlan p;
  for (uint32_t l = 0; l < depth; ++l) {
    p.level[l] = kzm_plan(log_n, window_bits, kzt_level_nodes(log_n, l), ws_cap, false, 0);
    p.nodes += p.level[l].count;
    p.chunks += p.level[l].chunks;
    const uint64_t partials = p.level[l].chunk_vectors * p.level[l].slices;
    if (partials > p.most_partials) p.most_partials = partials;
  }
  return p;
}

// ---- h: a node's 48 bytes -> the scalar its parent commits to ---------------------------------------------------------------------------
//     Transcript::new("kzg10-tree-v1"); append_message("node", c48); challenge_scalar("node-scalar")
// Every length is a constant, so the transcript meets the 48 bytes at a fixed place: up to the one permutation that stands
// between them and the 64 challenge bytes, everything else XORed into the STROBE state — the prefix before the message and the
// challenge's own framing after it — is the same for every node.  kzt_map_seed makes that state once (the message left out);
// kzt_map XORs the message in at byte KZT_MSG_POS, permutes, and reduces bytes 0 .. 63 as fr_from_bytes_wide does.
struct KztSeed {
  uint64_t a[25];
};

inline bool kzt_map_seed(KztSeed* seed) {
  Transcript t((const uint8_t*)"kzg10-tree-v1", 13);
  const uint8_t zero[48] = {0};
  t.append_message("node", zero, 48);
  uint8_t st[200];
  memcpy(st, t.strobe().raw_state(), 200);
  unsigned pos = t.strobe().raw_pos(), begin = t.strobe().raw_pos_begin();
  if (pos != KZT_MSG_POS + 48) return false;
  // challenge_bytes("node-scalar", 64) up to its permutation: meta_ad(label), meta_ad(le32(64), more), prf's header, run_f's
  // padding.  No absorb here reaches the rate (166), so none permutes.
  const uint8_t label[] = "node-scalar", le[4] = {64, 0, 0, 0};
  const uint8_t meta[2] = {(uint8_t)begin, 0x12};   // FLAG_M | FLAG_A
  begin = pos + 1;
  for (int i = 0; i < 2; ++i) st[pos++] ^= meta[i];
  for (int i = 0; i < 11; ++i) st[pos++] ^= label[i];
  for (int i = 0; i < 4; ++i) st[pos++] ^= le[i];
  const uint8_t prf[2] = {(uint8_t)begin, 0x07};    // FLAG_I | FLAG_A | FLAG_C
  begin = pos + 1;
  for (int i = 0; i < 2; ++i) st[pos++] ^= prf[i];
  st[pos] ^= (uint8_t)begin;
  st[pos + 1] ^= 0x04;
  st[167] ^= 0x80;
  for (int i = 0; i < 25; ++i) {
    uint64_t v = 0;
    for (int b = 0; b < 8; ++b) v |= (uint64_t)st[8 * i + b] << (8 * b);
    seed->a[i] = v;
  }
  return true;
}

// Keccak-f[1600] over 25 lanes held by value: every index is a constant, so a kernel keeps the state in registers
HD void kzt_keccak(uint64_t a[25]) {
#pragma unroll 1
  for (int rnd = 0; rnd < 24; ++rnd) {
    uint64_t c[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
    }
#pragma unroll
    for (int x = 0; x < 5; ++x)
#pragma unroll
      for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(a[x + 5 * y], KeccakConst::ROT[x][y]);
#pragma unroll
    for (int x = 0; x < 5; ++x)
#pragma unroll
      for (int y = 0; y < 5; ++y) a[x + 5 * y] = b[x + 5 * y] ^ ((~b[(x + 1) % 5 + 5 * y]) & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= KeccakConst::RC[rnd];
  }
}

// w: the 48 bytes as 12 words in memory order (w[0]'s low byte is byte 0)
HD Fr kzt_map(const KztSeed& seed, const uint32_t w[12]) {
  constexpr int LANE = KZT_MSG_POS / 8, SH = 8 * (KZT_MSG_POS % 8);
  static_assert(SH != 0 && LANE + 7 <= 20, "the message straddles lanes and stays inside the rate");
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] = seed.a[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const uint64_t m = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    a[LANE + i] ^= m << SH;
    a[LANE + i + 1] ^= m >> (64 - SH);
  }
  kzt_keccak(a);
  Fr lo, hi;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lo.l[2 * i] = (uint32_t)a[i];
    lo.l[2 * i + 1] = (uint32_t)(a[i] >> 32);
    hi.l[2 * i] = (uint32_t)a[4 + i];
    hi.l[2 * i + 1] = (uint32_t)(a[4 + i] >> 32);
  }
  const Fr r2 = Fr::r2();   // fr_from_bytes_wide on the 64 bytes
  return lo * r2 + (hi * r2) * r2;
}
// the same from bytes, for the host callers
inline Fr kzt_map_bytes(const KztSeed& seed, const uint8_t c48[48]) {
  uint32_t w[12];
  for (int k = 0; k < 12; ++k) w[k] = (uint32_t)c48[4 * k] | ((uint32_t)c48[4 * k + 1] << 8) | ((uint32_t)c48[4 * k + 2] << 16) | ((uint32_t)c48[4 * k + 3] << 24);
  return kzt_map(seed, w);
}

}  // namespace plonk
