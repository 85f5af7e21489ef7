// KZG10 vector-commitment trees on a plonk_kzg_domain that holds many-vector tables: all levels resident, build / update /
// prove without leaving the device between levels.  The index logic, the plans and the map h are in kzg_tree_core.hpp; the
// accumulation is kzg_many.hip's, through its launchers; DESIGN.md section 23 has the resources and the measurements.
//
//   kzt_map_kernel      one lane per commitment: 48 bytes -> h as a Montgomery Fr.  The STROBE state before the one permutation
//                       that depends on the node comes in as a kernel argument (kzt_map_seed); the Keccak state is 25 named
//                       lanes, every index a constant
//   kzt_finish_kernel   one lane per node: the slices' partial sums, plus the stored point in an update; ONE safegcd inverse,
//                       then the affine point, its flag and the 48 bytes; dense in a build, through a node list in an update
//   kzt_delta_kernel    one lane per touched value: delta = new - old, the store of the new value
//   kzt_gather_kernel   one lane per word: the commitments of a proof's nodes into one run for the copy to the host
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "devmem.cuh"
#include "g1codec.cuh"
#include "kzg_core.hpp"
#include "kzg_handle.hpp"
#include "kzg_many.hpp"
#include "kzg_multiproof.hpp"
#include "kzg_tree.hpp"

namespace plonk {

__global__ void __launch_bounds__(KZT_LANES) kzt_map_kernel(KztSeed seed, const uint32_t* __restrict__ comp, const uint64_t* __restrict__ list,
                                                            uint64_t count, Fr* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const uint32_t* src = comp + 12 * (list ? list[j] : j);
  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = src[k];
  st_fr(out + j, kzt_map(seed, w));
}

__global__ void __launch_bounds__(KZT_LANES) kzt_finish_kernel(const G1RSlot* __restrict__ partial, uint32_t slices,
                                                               const uint64_t* __restrict__ list, uint64_t first, uint64_t count, int with_base,
                                                               G1Affine* pts, int32_t* kind, uint32_t* comp) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const uint64_t node = list ? list[j] : first + j;
  G1R acc = ld_g1r(partial + j * slices);
  for (uint32_t s = 1; s < slices; ++s) acc = acc.add(ld_g1r(partial + j * slices + s));
  if (with_base && kind[node] == VDEC_OK) {
    const G1Affine a = ld_aff(pts + node);
    acc = acc.add(G1R::from_affine(Fp28::from_fp(a.x), Fp28::from_fp(a.y)));   // (the general addition: doubles, cancels)
  }
  G1Affine o;
  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) o.x.l[k] = o.y.l[k] = w[k] = 0;
  int32_t kd = VDEC_IDENTITY;
  if (acc.is_identity()) {
    w[0] = 0xC0u;
  } else {
    kd = VDEC_OK;
    Fp28 x, y;
    g1r_to_affine(acc, &x, &y);
    o.x = x.to_fp();
    o.y = y.to_fp();
    // G1Affine::to_bytes as g1r_compress48_words writes it, from the coordinates this lane has already
    const Fp xc = o.x.from_mont(), yc = o.y.from_mont();
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k] = __builtin_bswap32(xc.l[11 - k]);
    bool larger = false;   // y > (p - 1) / 2 = p >> 1
    for (int k = 11; k >= 0; --k) {
      const uint32_t half = (FpP::MOD[k] >> 1) | (k < 11 ? FpP::MOD[k + 1] << 31 : 0u);
      if (yc.l[k] != half) { larger = yc.l[k] > half; break; }
    }
    w[0] |= 0x80u | (larger ? 0x20u : 0u);
  }
  st_aff(pts + node, o);
  kind[node] = kd;
#pragma unroll
  for (int k = 0; k < 12; ++k) comp[12 * node + k] = w[k];
}

__global__ void __launch_bounds__(256) kzt_delta_kernel(const Fr* __restrict__ fresh, const uint64_t* __restrict__ flat, uint64_t count,
                                                        Fr* vals, Fr* __restrict__ deltas) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const Fr v = ld_fr(fresh + k);
  Fr* slot = vals + flat[k];
  st_fr(deltas + k, v - ld_fr(slot));
  st_fr(slot, v);
}

__global__ void __launch_bounds__(256) kzt_gather_kernel(const uint32_t* __restrict__ comp, const uint64_t* __restrict__ list, uint64_t words,
                                                         uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) return;
  out[i] = comp[12 * list[i / 12] + i % 12];
}

// ---- launchers (kzg_tree.hpp) ---------------------------------------------------------------------------------------------------
namespace {
bool grid_of(uint64_t count, uint32_t lanes, uint32_t* blocks) {
  const uint64_t b = (count + lanes - 1) / lanes;
  *blocks = (uint32_t)b;
  return count && b <= 0x7fffffffull;
}
}  // namespace

int kzt_map_run(Ctx* c, const KztSeed& seed, const uint8_t* comp48, const uint64_t* list, uint64_t count, Fr* out) {
  uint32_t blocks;
  if (!count) return PLONK_OK;
  if (!grid_of(count, KZT_LANES, &blocks) || !comp48 || !out || ((uintptr_t)comp48 & 3u)) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kzt_map_kernel, dim3(blocks), dim3(KZT_LANES), 0, c->stream, seed, (const uint32_t*)comp48, list, count, out);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzt_finish_run(Ctx* c, const G1RSlot* partial, uint32_t slices, const uint64_t* list, uint64_t first, uint64_t count, bool with_base,
                   G1Affine* pts, int32_t* kind, uint8_t* comp48) {
  uint32_t blocks;
  if (!count) return PLONK_OK;
  if (!grid_of(count, KZT_LANES, &blocks) || !slices || !partial || !pts || !kind || !comp48 || ((uintptr_t)comp48 & 3u))
    return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kzt_finish_kernel, dim3(blocks), dim3(KZT_LANES), 0, c->stream, partial, slices, list, first, count, with_base ? 1 : 0, pts,
                     kind, (uint32_t*)comp48);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzt_delta_run(Ctx* c, const Fr* fresh, const uint64_t* flat, uint64_t count, Fr* vals, Fr* deltas) {
  uint32_t blocks;
  if (!count) return PLONK_OK;
  if (!grid_of(count, 256, &blocks) || !fresh || !flat || !vals || !deltas) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kzt_delta_kernel, dim3(blocks), dim3(256), 0, c->stream, fresh, flat, count, vals, deltas);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

int kzt_gather_run(Ctx* c, const uint8_t* comp48, const uint64_t* list, uint64_t count, uint8_t* out48) {
  uint32_t blocks;
  if (!count) return PLONK_OK;
  if (!grid_of(12 * count, 256, &blocks) || !comp48 || !list || !out48) return (set_last_error("invalid argument", __func__, __FILE__, __LINE__), PLONK_ERR_ARG);
  hipLaunchKernelGGL(kzt_gather_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint32_t*)comp48, list, 12 * count, (uint32_t*)out48);
  HIP_TRY(hipGetLastError());
  return PLONK_OK;
}

// ---- the tree -----------------------------------------------------------------------------------------------------------------------
struct KztBufs {
  enum { PARTIAL, PLAN, FRESH, DELTAS, OUT48, META, NBUF };   // grow-only
};
struct KzgTree : KztBufs, DevBufs<KztBufs::NBUF> {
  KzgDomain* d = nullptr;
  uint32_t log_n = 0, depth = 0;
  bool built = false;
  Fr* vals[KZT_MAX_BITS] = {};
  uint8_t* comp[KZT_MAX_BITS] = {};
  G1Affine* pts[KZT_MAX_BITS] = {};
  int32_t* kind[KZT_MAX_BITS] = {};
  uint64_t data_bytes = 0;
  KztSeed seed;
  plonk_kzg_tree_info last = {};
  ~KzgTree() {
    for (uint32_t l = 0; l < KZT_MAX_BITS; ++l) {
      (void)hipFree(vals[l]);
      (void)hipFree(comp[l]);
      (void)hipFree(pts[l]);
      (void)hipFree(kind[l]);
    }
  }
};

namespace {

int tree_alloc(KzgTree* t) {
  for (uint32_t l = 0; l < t->depth; ++l) {
    const uint64_t nodes = kzt_level_nodes(t->log_n, l);
    HIP_TRY(hipMalloc((void**)&t->vals[l], sizeof(Fr) * (nodes << t->log_n)));
    HIP_TRY(hipMalloc((void**)&t->comp[l], 48 * nodes));
    HIP_TRY(hipMalloc((void**)&t->pts[l], sizeof(G1Affine) * nodes));
    HIP_TRY(hipMalloc((void**)&t->kind[l], 4 * nodes));
  }
  t->data_bytes = kzt_data_bytes(t->log_n, t->depth);
  return PLONK_OK;
}

void note(KzgTree* t, uint32_t kind, uint64_t touched, uint64_t terms, uint64_t chunks, uint64_t items, uint64_t vectors) {
  t->last = {};
  t->last.kind = kind;
  t->last.touched_nodes = touched;
  t->last.sparse_terms = terms;
  t->last.chunks = chunks;
  t->last.items = items;
  t->last.vectors = vectors;
}

// the levels above the leaves already in vals[D-1]
int build_levels(KzgTree* t, const KzmTables& tb, const KztBuildPlan& plan) {
  Ctx& c = *t->d->c;
  const uint32_t L = t->log_n;
  PTRY(t->need(KzgTree::PARTIAL, sizeof(G1RSlot) * plan.most_partials));
  for (uint32_t l = t->depth; l-- > 0;) {
    const KzmPlan& p = plan.level[l];
    for (uint64_t first = 0; first < p.count; first += p.chunk_vectors) {
      const uint64_t cnt = p.count - first < p.chunk_vectors ? p.count - first : p.chunk_vectors;
      PTRY(kzm_accumulate(&c, tb, t->vals[l] + (first << L), cnt, p.slices, t->at<G1RSlot>(KzgTree::PARTIAL)));
      PTRY(kzt_finish_run(&c, t->at<G1RSlot>(KzgTree::PARTIAL), p.slices, nullptr, first, cnt, false, t->pts[l], t->kind[l], t->comp[l]));
    }
    if (l) PTRY(kzt_map_run(&c, t->seed, t->comp[l], nullptr, p.count, t->vals[l - 1]));
  }
  HIP_TRY(hipStreamSynchronize(c.stream));
  return PLONK_OK;
}

// the host form's leaves: chunk g + 1 is uploaded (copy stream) under the copy of chunk g into vals[D-1] (main stream)
int stage_leaves(KzgTree* t, const uint64_t* leaves) {
  Ctx& c = *t->d->c;
  const uint64_t N = kzt_leaves(t->log_n, t->depth);
  uint64_t per = t->d->ws_cap / (2 * sizeof(Fr));
  if (per < (1ull << t->log_n)) per = 1ull << t->log_n;
  if (per > N) per = N;
  Fr* stage[2];
  hipEvent_t up[2], done[2];
  PTRY(kzg_stage_reserve(&c, per, stage, up, done));
  HIP_TRY(hipStreamSynchronize(c.stream));   // the copy stream is not ordered behind what the main stream still runs
  Fr* dst = t->vals[t->depth - 1];
  uint64_t g = 0;
  for (uint64_t first = 0; first < N; first += per, ++g) {
    const int b = (int)(g & 1);
    const uint64_t cnt = N - first < per ? N - first : per;
    if (g >= 2) HIP_TRY(hipStreamWaitEvent(c.copy_stream, done[b], 0));
    HIP_TRY(hipMemcpyAsync(stage[b], leaves + 4 * first, sizeof(Fr) * cnt, hipMemcpyHostToDevice, c.copy_stream));
    HIP_TRY(hipEventRecord(up[b], c.copy_stream));
    HIP_TRY(hipStreamWaitEvent(c.stream, up[b], 0));
    HIP_TRY(hipMemcpyAsync(dst + first, stage[b], sizeof(Fr) * cnt, hipMemcpyDeviceToDevice, c.stream));
    HIP_TRY(hipEventRecord(done[b], c.stream));
  }
  return PLONK_OK;
}

int build_body(const char* api_fn, KzgTree* t, const void* leaves, bool resident) {
  KzgDomain* d = t->d;
  Ctx& c = *d->c;
  const uint64_t N = kzt_leaves(t->log_n, t->depth);
  KzmTables tb;
  if (!kzm_handle_tables(d, &tb)) API_FAIL(PLONK_ERR_STATE, "the domain holds no many-vector tables (plonk_kzg_many_tables_build)");
  if (resident) {
    unsigned long long bad = 0;
    PTRY(t->need(KzgTree::META, 8));
    HIP_TRY(hipMemcpyAsync(t->p[KzgTree::META], &bad, 8, hipMemcpyHostToDevice, c.stream));
    PTRY(kzm_scan(&c, (const Fr*)leaves, N, t->at<unsigned long long>(KzgTree::META)));
    HIP_TRY(hipMemcpyAsync(&bad, t->p[KzgTree::META], 8, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (bad) API_FAIL(PLONK_ERR_DATA, "a leaf is not a canonical residue");
    HIP_TRY(hipMemcpyAsync(t->vals[t->depth - 1], leaves, sizeof(Fr) * N, hipMemcpyDeviceToDevice, c.stream));
  } else {
    PTRY(stage_leaves(t, (const uint64_t*)leaves));
  }
  const KztBuildPlan plan = kzt_build_plan(t->log_n, t->depth, tb.window_bits, d->ws_cap);
  PTRY(build_levels(t, tb, plan));
  t->built = true;
  note(t, KZT_BUILD, plan.nodes, 0, plan.chunks, 0, 0);
  return PLONK_OK;
}

int update_body(KzgTree* t, const KzmTables& tb, const KztSets& sets, const KztUpdatePlan& plan, const uint64_t* values) {
  KzgDomain* d = t->d;
  Ctx& c = *d->c;
  const uint64_t count = sets.order.size();
  // one upload: [node | offsets | flat] as 64-bit words, then the child indices
  const uint64_t w_node = 0, w_offs = plan.node.size(), w_flat = w_offs + plan.offsets.size(), words = w_flat + plan.flat.size();
  std::vector<uint64_t> up(words + (plan.child.size() + 1) / 2);
  memcpy(up.data() + w_node, plan.node.data(), 8 * plan.node.size());
  memcpy(up.data() + w_offs, plan.offsets.data(), 8 * plan.offsets.size());
  memcpy(up.data() + w_flat, plan.flat.data(), 8 * plan.flat.size());
  memcpy(up.data() + words, plan.child.data(), 4 * plan.child.size());
  std::vector<uint64_t> fresh(4 * count);   // the new leaves in the order of T_D
  for (uint64_t k = 0; k < count; ++k) memcpy(&fresh[4 * k], values + 4 * sets.order[k], 32);
  uint64_t most_chunk = 0;
  for (const KztUpdateLevel& lv : plan.level)
    for (uint64_t first = 0; first < lv.nodes;) {
      const uint64_t k = kzm_sparse_chunk(plan.offsets.data() + lv.offs_at, lv.nodes, first, d->ws_cap);
      if (k > most_chunk) most_chunk = k;
      first += k;
    }
  PTRY(t->need(KzgTree::PLAN, 8 * up.size()));
  PTRY(t->need(KzgTree::FRESH, sizeof(Fr) * plan.most_terms));
  PTRY(t->need(KzgTree::DELTAS, sizeof(Fr) * plan.most_terms));
  PTRY(t->need(KzgTree::PARTIAL, sizeof(G1RSlot) * most_chunk));
  const uint64_t* dev = t->at<uint64_t>(KzgTree::PLAN);
  const uint32_t* dev_child = (const uint32_t*)(dev + words);
  HIP_TRY(hipMemcpyAsync(t->p[KzgTree::PLAN], up.data(), 8 * up.size(), hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(t->p[KzgTree::FRESH], fresh.data(), sizeof(Fr) * count, hipMemcpyHostToDevice, c.stream));
  uint64_t chunks = 0;
  for (uint32_t step = 0; step < t->depth; ++step) {
    const uint32_t l = t->depth - 1 - step;
    const KztUpdateLevel& lv = plan.level[step];
    const uint64_t* nodes = dev + w_node + lv.node_at;
    PTRY(kzt_delta_run(&c, t->at<Fr>(KzgTree::FRESH), dev + w_flat + lv.term_at, lv.terms, t->vals[l], t->at<Fr>(KzgTree::DELTAS)));
    for (uint64_t first = 0; first < lv.nodes; ++chunks) {
      const uint64_t k = kzm_sparse_chunk(plan.offsets.data() + lv.offs_at, lv.nodes, first, d->ws_cap);
      // (the offsets of a level are relative to its first term: a chunk reads them where they are)
      PTRY(kzm_accumulate_sparse(&c, tb, dev + w_offs + lv.offs_at + first, dev_child + lv.term_at, t->at<Fr>(KzgTree::DELTAS), k,
                                 t->at<G1RSlot>(KzgTree::PARTIAL)));
      PTRY(kzt_finish_run(&c, t->at<G1RSlot>(KzgTree::PARTIAL), 1, nodes + first, 0, k, true, t->pts[l], t->kind[l], t->comp[l]));
      first += k;
    }
    if (l) PTRY(kzt_map_run(&c, t->seed, t->comp[l], nodes, lv.nodes, t->at<Fr>(KzgTree::FRESH)));
  }
  HIP_TRY(hipStreamSynchronize(c.stream));   // `up` and `fresh` are the call's
  note(t, KZT_UPDATE, plan.touched, plan.terms, chunks, 0, 0);
  return PLONK_OK;
}

int prove_body(const char* api_fn, KzgTree* t, const KztSets& sets, const KztProofPlan& plan, const uint8_t* label, uint64_t label_len,
               const uint64_t* challenges_override, uint64_t* values, uint8_t* path48, uint8_t* proof96) {
  KzgDomain* d = t->d;
  Ctx& c = *d->c;
  const uint64_t n = 1ull << t->log_n, M = plan.vectors, K = plan.items, count = sets.order.size();
  // the commitments of the proof's nodes, level by level, into one run
  std::vector<uint64_t> list;
  list.reserve(M);
  for (uint32_t l = 0; l < t->depth; ++l) list.insert(list.end(), sets.T[l].begin(), sets.T[l].end());
  std::vector<const void*> vecs(M);
  for (uint32_t l = 0; l < t->depth; ++l)
    for (uint64_t k = 0; k < sets.T[l].size(); ++k) vecs[plan.level_vector[l] + k] = t->vals[l] + sets.T[l][k] * n;
  std::vector<uint8_t> cm(48 * M);
  PTRY(t->need(KzgTree::PLAN, 8 * M));
  PTRY(t->need(KzgTree::OUT48, 48 * M));
  HIP_TRY(hipMemcpyAsync(t->p[KzgTree::PLAN], list.data(), 8 * M, hipMemcpyHostToDevice, c.stream));
  for (uint32_t l = 0; l < t->depth; ++l)
    PTRY(kzt_gather_run(&c, t->comp[l], t->at<uint64_t>(KzgTree::PLAN) + plan.level_vector[l], sets.T[l].size(),
                        t->at<uint8_t>(KzgTree::OUT48) + 48 * plan.level_vector[l]));
  HIP_TRY(hipMemcpyAsync(cm.data(), t->p[KzgTree::OUT48], 48 * M, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  std::vector<uint64_t> yk(4 * K);
  uint8_t proof[96];
  PTRY(kmp_open_entered(api_fn, d, vecs.data(), M, cm.data(), plan.vector_index.data(), plan.point_index.data(), K, label, label_len,
                        challenges_override, yk.data(), proof));
  for (uint64_t k = 0; k < count; ++k) memcpy(values + 4 * sets.order[k], &yk[4 * (K - count + k)], 32);
  if (plan.path_nodes) memcpy(path48, cm.data() + 48, 48 * plan.path_nodes);
  memcpy(proof96, proof, 96);
  note(t, KZT_PROVE, M, 0, 0, K, M);
  return PLONK_OK;
}

}  // namespace

}  // namespace plonk

using namespace plonk;

struct plonk_kzg_tree {
  plonk::KzgTree* t;
  plonk_kzg_domain* dom;
};

#define KZT_EMPTY_MSG "the tree is empty (plonk_kzg_tree_build)"

extern "C" {

int plonk_kzg_tree_create(plonk_kzg_domain* dom, uint32_t depth, plonk_kzg_tree** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!dom || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  *out = nullptr;
  KzgDomain* d = dom->d;
  if (kzt_check_shape(d->log_n, depth) != PLONK_OK) API_FAIL(PLONK_ERR_ARG, "invalid argument: log_n must be in [1, 12], depth >= 1 and depth * log_n <= 26");
  KZD_ENTER(d, api_fn, KZD_WORK);
  std::unique_ptr<KzgTree> t(new KzgTree());
  t->d = d;
  t->log_n = d->log_n;
  t->depth = depth;
  if (!kzt_map_seed(&t->seed)) API_FAIL(PLONK_ERR_STATE, "the transcript does not meet a node's bytes where the map kernel expects them");
  PTRY(tree_alloc(t.get()));
  *out = new plonk_kzg_tree{t.release(), dom};
  return PLONK_OK;
  });
}

void plonk_kzg_tree_destroy(plonk_kzg_tree* tree) {
  if (!tree) return;
  (void)plonk::api_guard(__func__, [&]() -> int {
    Ctx& c = *tree->t->d->c;
    std::lock_guard<std::mutex> lk(c.mu);
    if (!c.comm_poisoned) {
      (void)hipSetDevice(c.device);
      (void)hipStreamSynchronize(c.stream);
    }
    delete tree->t;
    return PLONK_OK;
  });
  delete tree;
}

static int tree_build(const char* api_fn, plonk_kzg_tree* tree, const void* leaves, bool resident) {
  if (!tree) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgTree* t = tree->t;
  KzgDomain* d = t->d;
  KZD_ENTER(d, api_fn, KZD_SET_DEVICE);
  t->built = false;   // whatever happens from here on: only a build that ends well fills the tree
  t->last = {};
  if (!leaves) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (resident && ((uintptr_t)leaves & 15u)) API_FAIL(PLONK_ERR_ARG, "invalid argument: leaves_dev must be 16-byte aligned");
  if (!resident) {
    Fr x;
    const uint64_t N = kzt_leaves(t->log_n, t->depth);
    for (uint64_t k = 0; k < N; ++k)
      if (!kzg_fr_load((const uint64_t*)leaves + 4 * k, &x)) API_FAIL(PLONK_ERR_DATA, "a leaf is not a canonical residue");
  }
  PTRY(kzd_enter_checks(api_fn, d, KZD_KEY | KZD_WHOLE_KEY));
  return kzd_drained(d->c, build_body(api_fn, t, leaves, resident));
}

int plonk_kzg_tree_build(plonk_kzg_tree* tree, const uint64_t* leaves) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int { return tree_build(api_fn, tree, leaves, false); });
}

int plonk_kzg_tree_build_dev(plonk_kzg_tree* tree, const void* leaves_dev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int { return tree_build(api_fn, tree, leaves_dev, true); });
}

int plonk_kzg_tree_nodes(plonk_kzg_tree* tree, uint32_t level, uint64_t first, uint64_t count, uint8_t* out48) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!tree || (count && !out48)) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgTree* t = tree->t;
  if (level >= t->depth) API_FAIL(PLONK_ERR_ARG, "invalid argument: the tree has no such level");
  const uint64_t nodes = kzt_level_nodes(t->log_n, level);
  if (first > nodes || count > nodes - first) API_FAIL(PLONK_ERR_ARG, "invalid argument: first + count exceeds the nodes of the level");
  KzgDomain* d = t->d;
  KZD_ENTER(d, api_fn, KZD_WORK);
  if (!t->built) API_FAIL(PLONK_ERR_STATE, KZT_EMPTY_MSG);
  if (!count) return PLONK_OK;
  Ctx& c = *d->c;
  HIP_TRY(hipMemcpyAsync(out48, t->comp[level] + 48 * first, 48 * count, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  return PLONK_OK;
  });
}

int plonk_kzg_tree_root(plonk_kzg_tree* tree, uint8_t out48[48]) {
  return plonk_kzg_tree_nodes(tree, 0, 0, 1, out48);
}

int plonk_kzg_tree_update(plonk_kzg_tree* tree, const uint64_t* leaf_index, const uint64_t* values, uint64_t count) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!tree || !leaf_index || !values) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgTree* t = tree->t;
  KztSets sets;
  if (kzt_sets(t->log_n, t->depth, leaf_index, count, KZT_MAX_UPDATE, &sets) != PLONK_OK)
    API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 2^20], every index below the number of leaves and none repeated");
  Fr x;
  for (uint64_t k = 0; k < count; ++k)
    if (!kzg_fr_load(values + 4 * k, &x)) API_FAIL(PLONK_ERR_DATA, "a value is not a canonical residue");
  KzgDomain* d = t->d;
  KZD_ENTER(d, api_fn, KZD_WORK);
  if (!t->built) API_FAIL(PLONK_ERR_STATE, KZT_EMPTY_MSG);
  KzmTables tb;
  if (!kzm_handle_tables(d, &tb)) API_FAIL(PLONK_ERR_STATE, "the domain holds no many-vector tables (plonk_kzg_many_tables_build)");
  KztUpdatePlan plan;
  kzt_update_plan(sets, &plan);
  const int rc = kzd_drained(d->c, update_body(t, tb, sets, plan, values));
  if (rc != PLONK_OK) t->built = false;   // a device failure mid-way: the levels no longer agree
  return rc;
  });
}

int plonk_kzg_tree_proof_nodes(uint32_t log_n, uint32_t depth, const uint64_t* leaf_index, uint64_t count, uint64_t* nodes) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!nodes) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (kzt_proof_nodes(log_n, depth, leaf_index, count, nodes) != PLONK_OK)
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a shape out of range, no index, an index that is repeated or out of range, or a proof above 65536 nodes or 2^20 items");
  return PLONK_OK;
  });
}

int plonk_kzg_tree_prove(plonk_kzg_tree* tree, const uint64_t* leaf_index, uint64_t count, const uint8_t* label, uint64_t label_len,
                         const uint64_t* challenges_override, uint64_t* values, uint8_t* path48, uint8_t proof96[96]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!tree || !leaf_index || !values || !proof96 || (label_len && !label)) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgTree* t = tree->t;
  KztSets sets;
  KztProofPlan plan;
  if (kzt_sets(t->log_n, t->depth, leaf_index, count, KZT_MAX_CLAIMS, &sets) != PLONK_OK || kzt_proof_plan(sets, &plan) != PLONK_OK)
    API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be at least 1, every index below the number of leaves and none repeated, at most 65536 distinct nodes and 2^20 items");
  if (plan.path_nodes && !path48) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgDomain* d = t->d;
  KZD_ENTER(d, api_fn, KZD_WORK);
  if (!t->built) API_FAIL(PLONK_ERR_STATE, KZT_EMPTY_MSG);
  return kzd_drained(d->c, prove_body(api_fn, t, sets, plan, label, label_len, challenges_override, values, path48, proof96));
  });
}

int plonk_kzg_tree_check(plonk_kzg_key* key, uint32_t log_n, uint32_t depth, const uint8_t root48[48], const uint64_t* leaf_index,
                         const uint64_t* values, uint64_t count, const uint8_t* path48, uint64_t nodes, const uint8_t proof96[96],
                         const uint8_t* label, uint64_t label_len, const uint64_t* challenges_override, plonk_verify_info* info) {
  const char* const api_fn = __func__;
  std::vector<uint8_t> cm;
  std::vector<uint64_t> yk;
  KztProofPlan plan;
  const int rc = plonk::api_guard(api_fn, [&]() -> int {
  if (!key || !root48 || !leaf_index || !values || !proof96 || (nodes && !path48) || (label_len && !label))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KztSets sets;
  if (kzt_sets(log_n, depth, leaf_index, count, KZT_MAX_CLAIMS, &sets) != PLONK_OK || kzt_proof_plan(sets, &plan) != PLONK_OK)
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a shape out of range, no index, an index that is repeated or out of range, or a proof above 65536 nodes or 2^20 items");
  if (nodes != plan.path_nodes) API_FAIL(PLONK_ERR_ARG, "invalid argument: `nodes` is not the number of path commitments these indices imply");
  KztSeed seed;
  if (!kzt_map_seed(&seed)) API_FAIL(PLONK_ERR_STATE, "the transcript does not meet a node's bytes where the map expects them");
  cm.resize(48 * plan.vectors);
  memcpy(cm.data(), root48, 48);
  if (nodes) memcpy(cm.data() + 48, path48, 48 * nodes);
  // the items of level l < D-1 claim h of the path commitments of level l + 1, in their order; the last `count` the leaves
  yk.resize(4 * plan.items);
  for (uint64_t k = 0; k < nodes; ++k) {
    const Fr h = kzt_map_bytes(seed, cm.data() + 48 * (k + 1));
    memcpy(&yk[4 * k], h.l, 32);
  }
  for (uint64_t k = 0; k < count; ++k) memcpy(&yk[4 * (nodes + k)], values + 4 * sets.order[k], 32);
  return PLONK_OK;
  });
  if (rc != PLONK_OK) return rc;
  return plonk_kzg_multiproof_check(key, log_n, cm.data(), plan.vectors, plan.vector_index.data(), plan.point_index.data(), yk.data(),
                                    plan.items, proof96, label, label_len, challenges_override, info);
}

int plonk_kzg_tree_last(plonk_kzg_tree* tree, plonk_kzg_tree_info* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!tree || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  const KzgTree* t = tree->t;
  const KzgDomain* d = t->d;
  KZD_ENTER(d, api_fn, 0);
  plonk_kzg_tree_info info = t->last;
  info.log_n = t->log_n;
  info.depth = t->depth;
  info.built = t->built ? 1 : 0;
  info.leaves = kzt_leaves(t->log_n, t->depth);
  info.device_bytes = t->data_bytes + t->bytes();
  *out = info;
  return PLONK_OK;
  });
}

}  // extern "C"
