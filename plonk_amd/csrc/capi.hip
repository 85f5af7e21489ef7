// C-ABI of libplonk_hip.so (see include/plonk_hip.h for the contract and the
// reference interfaces each entry point replaces).
#include <chrono>
#include <cstdio>
#include <cstring>
#include <sched.h>
#include <thread>

#include "plonk_internal.hpp"
#include "hostg1.hpp"

namespace plonk {

static thread_local char g_last_error[512] = "";   // a fixed buffer: recording an error never allocates (it may be the out-of-memory error)

void set_last_error(const char* what, const char* detail, const char* file, int line) {
  snprintf(g_last_error, sizeof g_last_error, "%s:%d: %s -> %s", file, line, what ? what : "?", detail ? detail : "?");
}

int srs_generate_device(Ctx* c, const Fr& tau, const Fr& g_scalar, uint64_t n, G1Affine* out_dev);

int ctx_refuse_poisoned(const char* api_fn) {
  set_last_error(api_fn, "context unusable: a collective timed out and its stream never drained (comm_sync); destroy the context", __FILE__, __LINE__);
  return PLONK_ERR_STATE;
}

// Destroy paths of a poisoned context: hipStreamSynchronize, hipFree (an implicit device-wide wait) and
// hipStreamDestroy would all block behind the dead collective — the hang comm_sync's bounded drain exists to prevent.  Poll
// both streams for at most 2 s; if they are still busy the caller LEAKS the context's device memory, streams and pinned
// buffers (the process is expected to exit or hipDeviceReset; a leak is recoverable, a hung destructor is not).
bool ctx_abandon(Ctx* c) {
  if (!c->comm_poisoned) return false;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const bool busy = (c->main_stream && hipStreamQuery(c->main_stream) == hipErrorNotReady) ||
                      (c->side_stream && hipStreamQuery(c->side_stream) == hipErrorNotReady);
    if (!busy) return false;   // drained after all: the ordinary teardown is safe
    if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > 2000) return true;
    std::this_thread::sleep_for(std::chrono::microseconds(500));
  }
}

void xyzz_to_affine97_host(const G1& p, uint8_t out[97]) {
  G1Affine a;
  const bool finite = p.to_affine(&a);
  memcpy(out, a.x.l, 48);
  memcpy(out + 48, a.y.l, 48);
  out[96] = finite ? 0 : 1;
}

// ---- hipEvent instrumentation ------------------------------------------------
struct ProfRec { int slot; hipEvent_t a, b; };
struct ProfState {
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  std::vector<ProfRec> recs;
  hipEvent_t open[Ctx::PROF_SLOTS] = {nullptr};
};
static std::map<Ctx*, ProfState*> g_prof;
static std::mutex g_prof_mu;

static ProfState* prof_state(Ctx* c) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  auto it = g_prof.find(c);
  if (it != g_prof.end()) return it->second;
  return g_prof[c] = new ProfState();
}
static void prof_release(Ctx* c) {   // plonk_ctx_destroy: the context's event pool goes with it (and a later context at the same address starts clean)
  ProfState* ps = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_prof.find(c);
    if (it == g_prof.end()) return;
    ps = it->second;
    g_prof.erase(it);
  }
  for (hipEvent_t e : ps->pool) (void)hipEventDestroy(e);
  delete ps;
}
static void prof_forget(Ctx* c) {    // abandoned context: drop the bookkeeping, leave the events alone
  std::lock_guard<std::mutex> lk(g_prof_mu);
  auto it = g_prof.find(c);
  if (it != g_prof.end()) { delete it->second; g_prof.erase(it); }
}
static hipEvent_t prof_event(ProfState* ps) {
  if (ps->used == ps->pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    ps->pool.push_back(e);
  }
  return ps->pool[ps->used++];
}
void prof_begin(Ctx* c, int slot) {
  if (!c->profile) return;
  ProfState* ps = prof_state(c);
  hipEvent_t e = prof_event(ps);
  if (!e) return;
  (void)hipEventRecord(e, c->stream);
  ps->open[slot] = e;
}
void prof_end(Ctx* c, int slot) {
  if (!c->profile) return;
  ProfState* ps = prof_state(c);
  if (!ps->open[slot]) return;
  hipEvent_t e = prof_event(ps);
  if (!e) return;
  (void)hipEventRecord(e, c->stream);
  ps->recs.push_back({slot, ps->open[slot], e});
  ps->open[slot] = nullptr;
}
void prof_host_add(Ctx* c, int slot, double ms) {
  if (!c->profile) return;
  c->acc_ms[slot] += ms;
  c->acc_n[slot] += 1;
}
static int prof_collect(Ctx* c) {
  ProfState* ps = prof_state(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto& r : ps->recs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      c->acc_ms[r.slot] += ms;
      c->acc_n[r.slot] += 1;
    }
  }
  ps->recs.clear();
  ps->used = 0;
  return PLONK_OK;
}

static int ensure_ntt_staging(Ctx* c, uint64_t n) {
  if (n <= c->ntt_cap) return PLONK_OK;
  if (c->ntt_buf) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(c->ntt_buf)); HIP_TRY(hipFree(c->ntt_buf2)); HIP_TRY(hipFree(c->ntt_buf3)); HIP_TRY(hipFree(c->ntt_tmp));
    c->ntt_buf = c->ntt_buf2 = c->ntt_buf3 = c->ntt_tmp = nullptr; c->ntt_cap = 0;
  }
  HIP_TRY(hipMalloc((void**)&c->ntt_buf, sizeof(Fr) * n));
  HIP_TRY(hipMalloc((void**)&c->ntt_buf2, sizeof(Fr) * n));
  HIP_TRY(hipMalloc((void**)&c->ntt_buf3, sizeof(Fr) * n));
  HIP_TRY(hipMalloc((void**)&c->ntt_tmp, sizeof(Fr) * n));
  c->ntt_cap = n;
  return PLONK_OK;
}

int msm_group_sums(Ctx* c, const Fr* const* scalars_dev, const uint64_t* m, int cnt, G1* sums, const void* table, uint64_t table_n,
                   uint32_t table_rows) {
  G1* res[MSM_MAX_BATCH];
  for (int k = 0; k < cnt; ++k) res[k] = (G1*)c->msm.result + (size_t)k * MSM_BIT_SUMS;
  const int rc = msm_batch_device(c, scalars_dev, m, cnt, res, true, table, table_n, nullptr, nullptr, table_rows);
  if (rc) return rc;
  const uint32_t rows = table ? table_rows : c->srs_rows;
  HIP_TRY(hipMemcpyAsync(c->msm.result_host, c->msm.result, sizeof(G1) * MSM_BIT_SUMS * cnt, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int k = 0; k < cnt; ++k)
    sums[k] = finish_bit_sums(reinterpret_cast<const G1*>(c->msm.result_host) + (size_t)k * MSM_BIT_SUMS, c->msm.last_rowbits,
                              rows == MSM_ROWS_BITPOS);
  return PLONK_OK;
}

static int ensure_scalar_staging(Ctx* c, uint64_t m) {
  MsmWork& w = c->msm;
  if (m <= w.cap_stage) return PLONK_OK;
  if (w.scalars_stage) { HIP_TRY(hipFree(w.scalars_stage)); w.scalars_stage = nullptr; w.cap_stage = 0; }
  HIP_TRY(hipMalloc((void**)&w.scalars_stage, sizeof(Fr) * m));
  w.cap_stage = m;
  return PLONK_OK;
}

}  // namespace plonk

using namespace plonk;

namespace plonk {

// plonk_gpu_config -> Config.  Order: defaults, the caller's struct (fields beyond its struct_size keep their defaults), the
// environment overrides (A/B runs).  Called at context creation and plonk_ctx_set_config — the ONLY place where the library
// reads the environment for a behaviour switch.
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e && e[0] ? atoi(e) : dflt; }
static char env_chr(const char* name) { const char* e = getenv(name); return e ? e[0] : 0; }

void config_resolve(const plonk_gpu_config* user, int device, Config* out) {
  Config g;
  plonk_gpu_config u{};
  if (user) memcpy(&u, user, user->struct_size < sizeof(u) ? user->struct_size : sizeof(u));
  g.table_budget = u.table_budget_bytes;
  g.table_mode = u.table_mode;
  g.bucket_bits = u.msm_bucket_bits;
  g.quotient_domain = u.quotient_domain == 8 ? 8 : 4;
  g.wire_commit_coeff = u.wire_commit == 1;
  g.shard_quotient = u.shard_quotient;
  g.shard_z = u.shard_grand_product;
  g.shard_side = u.shard_side_stream;
  g.ntt_elog = u.ntt_elements_log2;
  g.comm_timeout_ms = u.comm_timeout_ms > 0 ? u.comm_timeout_ms : 120000;
  g.side_cus = u.side_stream_cus;
  // ---- environment overrides
  switch (env_chr("PLONK_MSM_TABLE")) { case 'w': g.table_mode = MSM_ROWS_WINDOW; break; case 'h': g.table_mode = MSM_ROWS_HALFPOS; break; case 'q': g.table_mode = MSM_ROWS_QUARTERPOS; break; case 'b': g.table_mode = MSM_ROWS_BITPOS; break; default: break; }
  if (const int mb = env_int("PLONK_TABLE_BUDGET_MB", 0); mb > 0) g.table_budget = (uint64_t)mb << 20;
  if (const int b = env_int("PLONK_MSM_BUCKETS", 0); b) g.bucket_bits = b;
  if (env_chr("PLONK_QUOTIENT_DOMAIN") == '8') g.quotient_domain = 8;
  if (env_chr("PLONK_QUOTIENT_DOMAIN") == '4') g.quotient_domain = 4;
  if (env_chr("PLONK_WIRE_COMMIT") == 'c') g.wire_commit_coeff = 1;
  if (env_chr("PLONK_Z_COMMIT") == 'c') g.z_commit_coeff = 1;
  if (env_chr("PLONK_Z_COMMIT") == 'e') g.z_commit_coeff = -1;
  if (const char v = env_chr("PLONK_SHARD_QUOTIENT")) g.shard_quotient = v == '0' ? -1 : 1;
  if (const char v = env_chr("PLONK_SHARD_Z")) g.shard_z = v == '1' ? 1 : -1;
  if (const char v = env_chr("PLONK_SHARD_SIDE")) g.shard_side = v == '0' ? -1 : 1;
  if (const char v = env_chr("PLONK_NTT_ELOG"); v == '2' || v == '3') g.ntt_elog = v - '0';
  if (const int t = env_int("PLONK_COMM_TIMEOUT_MS", 0); t > 0) g.comm_timeout_ms = t;
  if (getenv("PLONK_SIDE_CUS")) g.side_cus = env_int("PLONK_SIDE_CUS", 0);
  g.ksl = env_int("PLONK_MSM_KSL", 0);
  g.prof_fine = env_chr("PLONK_PROF_FINE") == '1';
  g.acc_lds = env_chr("PLONK_MSM_ACC") == 'l';
  if (const char v = env_chr("PLONK_MSM_ORDER")) g.order = v == '1' ? 1 : 0;
  g.tail_serial = env_chr("PLONK_MSM_TAIL") == 's';
  g.bsum_lane = env_chr("PLONK_MSM_BSUM") == 'l';
  g.rc_lane_tree = env_chr("PLONK_MSM_RCTREE") == 'l';
  g.lps = env_int("PLONK_MSM_LPS", 0);
  g.rcwv = env_int("PLONK_MSM_RCWV", 0);
  if (const char v = env_chr("PLONK_MSM_SORT13")) g.sort13 = v == '1' ? 1 : 0;
  g.acc_wg = env_int("PLONK_MSM_ACC_WG", 0);
  g.ntt_direct = env_chr("PLONK_NTT_DIRECT") != '0';
  g.bi_cfg = env_int("PLONK_BI_CFG", -1);
  if (const char v = env_chr("PLONK_SIDE_DEFER")) g.side_defer = v == '1' ? 1 : (v == '2' ? 2 : 0);
  if (const char v = env_chr("PLONK_SIDE_AFTER_ELOG"); v == '2' || v == '3') g.side_after_elog = v - '0';
  if (const char v = env_chr("PLONK_WIRE_POLYS_SIDE")) g.wire_polys_side = v == '1' ? 1 : 0;
  if (env_chr("PLONK_WIRE_BY_COLUMN") == '0') g.wire_by_column = -1;
  if (env_chr("PLONK_WIRE_BY_COLUMN") == '1') g.wire_by_column = 1;
  if (env_chr("PLONK_WIRE_BY_COLUMN") == '2') g.wire_by_column = 2;
  if (getenv("PLONK_HOST_THREADS")) g.host_threads = env_int("PLONK_HOST_THREADS", -1);
  // ---- resolution
  if (g.table_mode != (int)MSM_ROWS_WINDOW && g.table_mode != (int)MSM_ROWS_QUARTERPOS && g.table_mode != (int)MSM_ROWS_HALFPOS && g.table_mode != (int)MSM_ROWS_BITPOS) g.table_mode = 0;
  if (g.ntt_elog != 2 && g.ntt_elog != 3) g.ntt_elog = 0;
  if (g.side_cus < 0) g.side_cus = 0;
  if (g.host_threads < 0) {   // the CPUs this process may run on (taskset / cpuset), not the machine's: helper threads spin
    cpu_set_t set;
    CPU_ZERO(&set);
    const int cpus = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
    g.host_threads = cpus >= 8 ? 3 : 0;
  }
  if (g.host_threads > 7) g.host_threads = 7;
  if (g.table_budget == 0) {
    size_t total = 0;   // (takes the device ordinal: the calling thread's current device is left alone)
    if (hipDeviceTotalMem(&total, device) != hipSuccess || total == 0) total = 256ull << 30;
    g.table_budget = (uint64_t)total / 10 * 8;
  }
  *out = g;
}

static int config_check(const plonk_gpu_config* u, const char* api_fn) {
  if (!u) return PLONK_OK;
  if (u->struct_size < 8 || u->struct_size > 4096) return (set_last_error("invalid argument", "plonk_gpu_config.struct_size is not set", __FILE__, __LINE__), PLONK_ERR_ARG);
  plonk_gpu_config c{};
  memcpy(&c, u, u->struct_size < sizeof(c) ? u->struct_size : sizeof(c));
  auto bad = [&](const char* what) { set_last_error(api_fn, what, __FILE__, __LINE__); return PLONK_ERR_ARG; };
  if (c.table_mode != PLONK_TABLE_AUTO && c.table_mode != PLONK_TABLE_WINDOW && c.table_mode != PLONK_TABLE_QUARTERPOS && c.table_mode != PLONK_TABLE_HALFPOS && c.table_mode != PLONK_TABLE_BITPOS) return bad("plonk_gpu_config.table_mode");
  if (c.msm_bucket_bits != 0 && c.msm_bucket_bits != 15 && c.msm_bucket_bits != 17 && c.msm_bucket_bits != 19) return bad("plonk_gpu_config.msm_bucket_bits");
  if (c.quotient_domain != 0 && c.quotient_domain != 4 && c.quotient_domain != 8) return bad("plonk_gpu_config.quotient_domain");
  if (c.wire_commit != 0 && c.wire_commit != 1) return bad("plonk_gpu_config.wire_commit");
  if (c.ntt_elements_log2 != 0 && c.ntt_elements_log2 != 2 && c.ntt_elements_log2 != 3) return bad("plonk_gpu_config.ntt_elements_log2");
  for (int v : {c.shard_quotient, c.shard_grand_product, c.shard_side_stream}) if (v < -1 || v > 1) return bad("plonk_gpu_config.shard_*: -1, 0 or 1");
  if (c.comm_timeout_ms < 0 || c.side_stream_cus < -1 || c.side_stream_cus > 200) return bad("plonk_gpu_config.comm_timeout_ms / side_stream_cus");
  return PLONK_OK;
}

// plonk_gpu_config.side_stream_cus = k > 0: the side stream is re-created on k compute units (hipExtStreamCreateWithCUMask),
// spread evenly over the XCDs; the main stream keeps the whole chip.  Side-stream transforms can then use the faster
// four-wave pass kernels (ntt.hip ELOG = 2) without spreading over every CU and taking issue slots from the critical
// path's kernels (DESIGN.md 7.5 / VERDICT r4 item 4): whatever they steal, they steal on k CUs only.
static int side_stream_partition(Ctx* c) {
  const int k = c->cfg.side_cus;
  if (k <= 0) return PLONK_OK;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, c->device));
  const int ncu = prop.multiProcessorCount;
  if (k >= ncu) return (set_last_error("plonk_gpu_config.side_stream_cus", "must be smaller than the device's compute-unit count", __FILE__, __LINE__), PLONK_ERR_ARG);
  const int words = (ncu + 31) / 32;
  std::vector<uint32_t> side(words, 0u);
  for (int i = 0; i < ncu; ++i)   // every (ncu / k)-th bit: the mask interleaves the XCDs, so the k CUs come from all of them
    if ((int64_t)i * k / ncu != (int64_t)(i + 1) * k / ncu) side[i / 32] |= 1u << (i % 32);
  hipStream_t ss = nullptr;
  if (hipExtStreamCreateWithCUMask(&ss, (uint32_t)words, side.data()) != hipSuccess) return (set_last_error("hipExtStreamCreateWithCUMask", "side stream", __FILE__, __LINE__), PLONK_ERR_HIP);
  // NOTE: hipExtStreamCreateWithCUMask takes neither flags nor a priority — the masked stream has DEFAULT priority and is a
  // blocking stream (it synchronises with the NULL stream), unlike the low-priority non-blocking side stream it replaces.
  // The library never uses the NULL stream, and the option is an A/B switch that measured slower at every mask size
  // (DESIGN.md 7.5), so this is documented (include/plonk_hip.h, side_stream_cus) rather than compensated.
  (void)hipStreamDestroy(c->side_stream);
  c->side_stream = ss;
  return PLONK_OK;
}

}  // namespace plonk

extern "C" {

const char* plonk_last_error(void) { return g_last_error; }

static int create_context(plonk_ctx** out, int dev, const plonk_gpu_config* config, const char* api_fn) {
  if (!out) return PLONK_ERR_ARG;
  { const int rc = config_check(config, api_fn); if (rc) return rc; }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    set_last_error("hipGetDeviceCount", "no HIP device visible", __FILE__, __LINE__);
    return PLONK_ERR_NO_GPU;
  }
  if (dev < 0 || dev >= count) return PLONK_ERR_ARG;
  HIP_TRY(hipSetDevice(dev));
  auto* ctx = new plonk_ctx();
  ctx->c.device = dev;
  config_resolve(config, dev, &ctx->c.cfg);
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  hipError_t e = hipStreamCreateWithPriority(&ctx->c.stream, hipStreamNonBlocking, prio_greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->c.side_stream, hipStreamNonBlocking, prio_least);
  ctx->c.main_stream = ctx->c.stream;
  if (e != hipSuccess) {
    set_last_error("hipStreamCreate", hipGetErrorString(e), __FILE__, __LINE__);
    delete ctx;
    return PLONK_ERR_HIP;
  }
  { const int rc = side_stream_partition(&ctx->c); if (rc) { (void)hipStreamDestroy(ctx->c.stream); (void)hipStreamDestroy(ctx->c.side_stream); delete ctx; return rc; } }
  *out = ctx;
  return PLONK_OK;
}

int plonk_ctx_create(plonk_ctx** out, const int* devices, int ndev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!out || ndev > 1 || ndev < 0) return PLONK_ERR_ARG;
  return create_context(out, (devices && ndev == 1) ? devices[0] : 0, nullptr, api_fn);
  });
}

int plonk_ctx_create_ex(plonk_ctx** out, int device, const plonk_gpu_config* config) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int { return create_context(out, device, config, api_fn); });
}

int plonk_ctx_get_config(plonk_ctx* ctx, plonk_gpu_config* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out || out->struct_size < 8 || out->struct_size > 4096) return (set_last_error("invalid argument", "plonk_ctx_get_config: set struct_size = sizeof(plonk_gpu_config)", __FILE__, __LINE__), PLONK_ERR_ARG);
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  const Config& g = ctx->c.cfg;
  plonk_gpu_config full{};
  full.struct_size = (uint32_t)sizeof(plonk_gpu_config);
  full.table_budget_bytes = g.table_budget;
  full.table_mode = g.table_mode;
  full.msm_bucket_bits = g.bucket_bits;
  full.quotient_domain = g.quotient_domain;
  full.wire_commit = g.wire_commit_coeff;
  full.shard_quotient = g.shard_quotient;
  full.shard_grand_product = g.shard_z;
  full.shard_side_stream = g.shard_side;
  full.ntt_elements_log2 = g.ntt_elog;
  full.comm_timeout_ms = g.comm_timeout_ms;
  full.side_stream_cus = g.side_cus;
  const uint32_t want = out->struct_size < sizeof(full) ? out->struct_size : (uint32_t)sizeof(full);
  memcpy(out, &full, want);
  out->struct_size = want;
  return PLONK_OK;
  });
}

int plonk_ctx_set_config(plonk_ctx* ctx, const plonk_gpu_config* config) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx) return PLONK_ERR_ARG;
  { const int rc = config_check(config, api_fn); if (rc) return rc; }
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  // resolve into a temporary, validate, THEN commit (a rejected call used to leave every other field replaced)
  Config next;
  config_resolve(config, ctx->c.device, &next);
  if (next.side_cus != ctx->c.cfg.side_cus)   // streams are created once: the partition of the CUs is fixed at creation
    return (set_last_error("plonk_ctx_set_config", "side_stream_cus can only be chosen at plonk_ctx_create_ex", __FILE__, __LINE__), PLONK_ERR_STATE);
  ctx->c.cfg = next;
  return PLONK_OK;
  });
}

int plonk_ctx_table_bytes(plonk_ctx* ctx, uint64_t* in_use, uint64_t* budget) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  if (in_use) *in_use = ctx->c.table_bytes;
  if (budget) *budget = ctx->c.cfg.table_budget;
  return PLONK_OK;
  });
}

static void plan_out(const plonk_msm_plan_internal& p, plonk_msm_plan* out) {
  memset(out, 0, sizeof(*out));
  out->table_rows = p.table_rows; out->bucket_bits = p.bucket_bits; out->digit_width = p.digit_width;
  out->slice_entries = p.slice_entries; out->ordered_lanes = p.ordered_lanes; out->wide_words = p.wide_words; out->flags = p.flags; out->terms = p.terms;
  snprintf(out->accumulate_kernel, sizeof(out->accumulate_kernel), "%s", p.kernel);
}

int plonk_ctx_describe_msm(plonk_ctx* ctx, uint64_t m, int count, int bit_sum_tail, uint32_t table_rows, uint64_t table_points, plonk_msm_plan* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out || count < 1 || count > MSM_MAX_BATCH) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  Ctx& c = ctx->c;
  if (table_rows == 0) { table_rows = c.srs_rows; table_points = c.srs_n; if (!c.srs_table) return PLONK_ERR_NO_SRS; }
  if (table_rows != MSM_ROWS_WINDOW && table_rows != MSM_ROWS_QUARTERPOS && table_rows != MSM_ROWS_HALFPOS && table_rows != MSM_ROWS_BITPOS) return PLONK_ERR_ARG;
  plonk_msm_plan_internal p;
  msm_plan(&c, table_rows, table_points, m, count, bit_sum_tail != 0, &p);
  plan_out(p, out);
  return PLONK_OK;
  });
}

int plonk_ctx_last_msm(plonk_ctx* ctx, plonk_msm_plan* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  if (!ctx->c.last_plan.table_rows) return (set_last_error("plonk_ctx_last_msm", "no MSM has run on this context", __FILE__, __LINE__), PLONK_ERR_STATE);
  plan_out(ctx->c.last_plan, out);
  return PLONK_OK;
  });
}

void plonk_ctx_destroy(plonk_ctx* ctx) {
  if (!ctx) return;
  (void)plonk_comm_destroy(ctx);
  Ctx& c = ctx->c;
  finish_pool_release(&c);   // host helper threads (asleep between proofs): joined on every path, nothing of the device is touched
  (void)hipSetDevice(c.device);
  if (ctx_abandon(&c)) {   // poisoned and still busy: every wait / hipFree / hipStreamDestroy below would hang — leak the device side
    prof_forget(&c);
    delete ctx;
    return;
  }
  (void)hipStreamSynchronize(c.stream);
  verify_ws_release(&c);
  kzg_ws_release(&c);
  msm_points_ws_release(&c);
  for (auto& kv : c.ntt_tables) {
    NttTables* t = kv.second;
    (void)hipFree(t->tw_lo); (void)hipFree(t->tw_hi); (void)hipFree(t->tw_lo_scaled);
    (void)hipFree(t->w512); (void)hipFree(t->g_lo); (void)hipFree(t->g_hi);
    (void)hipFree(t->tw_lo29); (void)hipFree(t->tw_hi29); (void)hipFree(t->tw_lo_scaled29);
    (void)hipFree(t->w512_29); (void)hipFree(t->g_lo29); (void)hipFree(t->g_hi29);
    (void)hipFree(t->tw_a29); (void)hipFree(t->tw_b29);
    delete t;
  }
  (void)hipFree(c.ntt_buf); (void)hipFree(c.ntt_buf2); (void)hipFree(c.ntt_buf3); (void)hipFree(c.ntt_tmp);
  if (c.down_stream) (void)hipStreamDestroy(c.down_stream);
  if (c.copy_stream) (void)hipStreamDestroy(c.copy_stream); (void)hipFree(c.srs_table); (void)hipFree(c.table_scratch);
  MsmWork& w = c.msm;
  (void)hipFree(w.tmp_words); (void)hipFree(w.entries); (void)hipFree(w.coarse_cnt); (void)hipFree(w.coarse_off); (void)hipFree(w.coarse_cur); (void)hipFree(w.big_off); (void)hipFree(w.big_cnt); (void)hipFree(w.nheavy); (void)hipFree(w.heavy_list); (void)hipFree(w.seg_sum);
  (void)hipFree(w.offsets); (void)hipFree(w.slice_off); (void)hipFree(w.full_off); (void)hipFree(w.part_list); (void)hipFree(w.partial); (void)hipFree(w.buckets);
  (void)hipFree(w.multi_list); (void)hipFree(w.layout);
  (void)hipFree(w.chunk); (void)hipFree(w.result); (void)hipFree(w.scalars_stage);
  if (w.result_host) (void)hipHostFree(w.result_host);
  prof_release(&c);
  (void)hipStreamDestroy(c.main_stream);
  if (c.side_stream) (void)hipStreamDestroy(c.side_stream);
  delete ctx;
}

int plonk_ctx_table_rows(plonk_ctx* ctx) { return ctx ? (int)ctx->c.srs_rows : 0; }
void* plonk_ctx_stream(plonk_ctx* ctx) { return ctx ? (void*)ctx->c.main_stream : nullptr; }   // never the side stream a running prove() may have swapped in

// ---- device memory helpers ----------------------------------------------------
int plonk_dev_alloc(plonk_ctx* ctx, uint64_t bytes, void** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out) return PLONK_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->c.device));
  HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
  return PLONK_OK;
  });
}
int plonk_dev_free(plonk_ctx* ctx, void* p) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  HIP_TRY(hipStreamSynchronize(ctx->c.main_stream));
  HIP_TRY(hipFree(p));
  return PLONK_OK;
  });
}
int plonk_dev_h2d(plonk_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || (!dst && bytes) || (!src && bytes)) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->c.main_stream));
  HIP_TRY(hipStreamSynchronize(ctx->c.main_stream));
  return PLONK_OK;
  });
}
int plonk_dev_d2h(plonk_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || (!dst && bytes) || (!src && bytes)) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->c.main_stream));
  HIP_TRY(hipStreamSynchronize(ctx->c.main_stream));
  return PLONK_OK;
  });
}
int plonk_dev_sync(plonk_ctx* ctx) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  HIP_TRY(hipStreamSynchronize(ctx->c.main_stream));
  return PLONK_OK;
  });
}

// ---- NTT ------------------------------------------------------------------------
int plonk_ntt_dev(plonk_ctx* ctx, const void* src, void* dst, void* tmp, uint32_t log_n, int inverse,
                  int coset, uint64_t in_len) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !src || !dst || log_n >= 28) return PLONK_ERR_ARG;
  if (log_n > 10 && !tmp) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  prof_begin(&ctx->c, 0);
  int rc = ntt_device(&ctx->c, (const Fr*)src, (Fr*)dst, (Fr*)tmp, log_n, inverse != 0, coset != 0, in_len);
  prof_end(&ctx->c, 0);
  return rc;
  });
}

int plonk_ntt(plonk_ctx* ctx, uint64_t* a, uint32_t log_n, int inverse, int coset, uint64_t in_len) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !a || log_n >= 28) return PLONK_ERR_ARG;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  const uint64_t n = 1ull << log_n;
  if (in_len > n) in_len = n;
  int rc = ensure_ntt_staging(&c, n);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c.ntt_buf, a, sizeof(Fr) * in_len, hipMemcpyHostToDevice, c.stream));
  rc = ntt_device(&c, c.ntt_buf, c.ntt_buf, c.ntt_tmp, log_n, inverse != 0, coset != 0, in_len);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(a, c.ntt_buf, sizeof(Fr) * n, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  return PLONK_OK;
  });
}

// The 5-way fan-out of compute_coset_evaluations (quotient_poly.rs:139-157) / the 4 wire iFFTs
// (prover.rs:464) as ONE call: a FULL-DUPLEX pipeline over three device buffers and three streams — the upload of
// transform k + 1 (copy stream), the transform of k (main stream) and the download of k - 1 (down stream) run at the same
// time, ordered by events only (no host thread, no host synchronisation until the end), so both PCIe directions are busy
// together: the batch costs ~max(upload, download) per transform instead of their sum.
int plonk_ntt_batch(plonk_ctx* ctx, uint64_t* const* a, int count, uint32_t log_n, int inverse, int coset,
                    const uint64_t* in_len) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !a || count < 0 || log_n >= 28) return PLONK_ERR_ARG;
  for (int i = 0; i < count; ++i) if (!a[i]) return PLONK_ERR_ARG;
  if (count == 0) return PLONK_OK;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  const uint64_t n = 1ull << log_n;
  int rc = ensure_ntt_staging(&c, n);
  if (rc) return rc;
  if (!c.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
  if (!c.down_stream) HIP_TRY(hipStreamCreateWithFlags(&c.down_stream, hipStreamNonBlocking));
  Fr* buf[3] = {c.ntt_buf, c.ntt_buf2, c.ntt_buf3};
  hipEvent_t up[3] = {nullptr, nullptr, nullptr}, done[3] = {nullptr, nullptr, nullptr}, freed[3] = {nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; ++k) {
    e = hipEventCreateWithFlags(&up[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&freed[k], hipEventDisableTiming);
  }
  for (int k = 0; k < count && e == hipSuccess && rc == PLONK_OK; ++k) {
    const int b = k % 3;
    uint64_t len = in_len ? in_len[k] : n;
    if (len > n) len = n;
    if (k >= 3) e = hipStreamWaitEvent(c.copy_stream, freed[b], 0);            // transform k - 3 has left this buffer
    if (e == hipSuccess) e = hipMemcpyAsync(buf[b], a[k], sizeof(Fr) * len, hipMemcpyHostToDevice, c.copy_stream);
    if (e == hipSuccess) e = hipEventRecord(up[b], c.copy_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c.stream, up[b], 0);
    if (e == hipSuccess) rc = ntt_device(&c, buf[b], buf[b], c.ntt_tmp, log_n, inverse != 0, coset != 0, len);
    if (e == hipSuccess && rc == PLONK_OK) e = hipEventRecord(done[b], c.stream);
    if (e == hipSuccess && rc == PLONK_OK) e = hipStreamWaitEvent(c.down_stream, done[b], 0);
    if (e == hipSuccess && rc == PLONK_OK) e = hipMemcpyAsync(a[k], buf[b], sizeof(Fr) * n, hipMemcpyDeviceToHost, c.down_stream);
    if (e == hipSuccess && rc == PLONK_OK) e = hipEventRecord(freed[b], c.down_stream);
  }
  // drain all three streams before the buffers / events go away, error or not
  const hipError_t e1 = hipStreamSynchronize(c.copy_stream), e2 = hipStreamSynchronize(c.stream), e3 = hipStreamSynchronize(c.down_stream);
  if (e == hipSuccess) e = e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3);
  for (int k = 0; k < 3; ++k) {
    if (up[k]) (void)hipEventDestroy(up[k]);
    if (done[k]) (void)hipEventDestroy(done[k]);
    if (freed[k]) (void)hipEventDestroy(freed[k]);
  }
  if (e != hipSuccess) { set_last_error("plonk_ntt_batch", hipGetErrorString(e), __FILE__, __LINE__); if (rc == PLONK_OK) rc = PLONK_ERR_HIP; }
  return rc;
  });
}

// ---- SRS / MSM ---------------------------------------------------------------------
int plonk_srs_load_dev(plonk_ctx* ctx, const void* xy96_dev, uint64_t npoints) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || (!xy96_dev && npoints)) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  return srs_load_device(&ctx->c, (const G1Affine*)xy96_dev, npoints);
  });
}

// The commit key is STREAMED from host memory: chunks of 2^18 points (24 MiB) alternate between two device
// staging buffers — the copy stream uploads chunk k + 1 while the main stream builds the window-table rows
// of chunk k — so no device copy of the raw key ever exists and the upload hides behind the table build
// (BASELINE config 5: "streamed SRS from host pinned memory"; with pinned memory, plonk_host_alloc, the
// uploads are truly asynchronous; pageable memory works, the runtime then stages each chunk itself).
// In a multi-GPU run every rank streams only its own point range of the host copy.
int plonk_srs_load(plonk_ctx* ctx, const uint8_t* xy96, uint64_t npoints) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || (!xy96 && npoints)) return PLONK_ERR_ARG;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  int rc = srs_table_begin(&c, npoints);
  if (rc || npoints == 0) return rc;
  constexpr uint64_t CHUNK = 1ull << 18;
  const uint64_t cap = npoints < CHUNK ? npoints : CHUNK;
  if (!c.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
  G1Affine* stage[2] = {nullptr, nullptr};
  hipEvent_t up[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  auto cleanup = [&] {
    (void)hipStreamSynchronize(c.copy_stream);
    (void)hipStreamSynchronize(c.stream);
    for (int k = 0; k < 2; ++k) {
      if (stage[k]) (void)hipFree(stage[k]);
      if (up[k]) (void)hipEventDestroy(up[k]);
      if (done[k]) (void)hipEventDestroy(done[k]);
    }
  };
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = hipMalloc((void**)&stage[k], sizeof(G1Affine) * cap);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&up[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
  }
  uint64_t k = 0;
  for (uint64_t first = 0; first < npoints && e == hipSuccess && rc == PLONK_OK; first += CHUNK, ++k) {
    const uint64_t cnt = npoints - first < CHUNK ? npoints - first : CHUNK;
    const int b = (int)(k & 1);
    if (k >= 2) e = hipStreamWaitEvent(c.copy_stream, done[b], 0);             // the staging buffer is free again
    if (e == hipSuccess) e = hipMemcpyAsync(stage[b], xy96 + 96 * first, sizeof(G1Affine) * cnt, hipMemcpyHostToDevice, c.copy_stream);
    if (e == hipSuccess) e = hipEventRecord(up[b], c.copy_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c.stream, up[b], 0);
    if (e == hipSuccess) rc = srs_table_chunk(&c, stage[b], npoints, first, cnt, c.stream);
    if (e == hipSuccess && rc == PLONK_OK) e = hipEventRecord(done[b], c.stream);
  }
  if (e == hipSuccess && rc == PLONK_OK) e = hipStreamSynchronize(c.stream);
  cleanup();
  srs_table_scratch_free(&c);
  if (e != hipSuccess) { set_last_error("plonk_srs_load", hipGetErrorString(e), __FILE__, __LINE__); rc = PLONK_ERR_HIP; }
  if (rc == PLONK_OK) c.srs_n = npoints;
  return rc;
  });
}

// pinned host memory for callers without HIP bindings (commit keys to stream, batch transform buffers)
int plonk_host_alloc(uint64_t bytes, void** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!out) return PLONK_ERR_ARG;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return PLONK_OK;
  });
}
int plonk_host_free(void* p) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (p) HIP_TRY(hipHostFree(p));
  return PLONK_OK;
  });
}

int plonk_srs_validate(plonk_ctx* ctx, const uint8_t* xy96, uint64_t npoints) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || (!xy96 && npoints)) return PLONK_ERR_ARG;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  G1Affine* tmp = nullptr;
  int* flag = nullptr;
  HIP_TRY(hipMalloc((void**)&tmp, sizeof(G1Affine) * (npoints ? npoints : 1)));
  if (hipMalloc((void**)&flag, sizeof(int)) != hipSuccess) { (void)hipFree(tmp); return PLONK_ERR_HIP; }
  int bad = 0;
  hipError_t e = hipMemcpyAsync(tmp, xy96, sizeof(G1Affine) * npoints, hipMemcpyHostToDevice, c.stream);
  int rc = (e == hipSuccess) ? srs_validate_device(&c, tmp, npoints, flag) : PLONK_ERR_HIP;
  if (rc == PLONK_OK && hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c.stream) != hipSuccess) rc = PLONK_ERR_HIP;
  if (hipStreamSynchronize(c.stream) != hipSuccess) rc = PLONK_ERR_HIP;
  (void)hipFree(tmp);
  (void)hipFree(flag);
  if (rc == PLONK_OK && bad) {
    plonk::set_last_error("PointMalformed", "commit key point off the curve or outside the prime-order subgroup", __FILE__, __LINE__);
    rc = PLONK_ERR_POINT;
  }
  return rc;
  });
}

int plonk_srs_generate_dev(plonk_ctx* ctx, const uint64_t tau[4], const uint64_t g_scalar[4], uint64_t npoints,
                           void* out_dev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !tau || !g_scalar || !out_dev) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  Fr t, g;
  memcpy(&t, tau, 32);
  memcpy(&g, g_scalar, 32);
  return srs_generate_device(&ctx->c, t, g, npoints, (G1Affine*)out_dev);
  });
}

int plonk_lagrange_key(plonk_ctx* ctx, uint32_t log_n, uint8_t* out_xy96) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !out_xy96 || log_n >= 27) return PLONK_ERR_ARG;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  const uint64_t n = 1ull << log_n;
  G1Affine* pts = nullptr;
  HIP_TRY(hipMalloc((void**)&pts, sizeof(G1Affine) * (n + 2)));
  int rc = lagrange_points_device(&c, log_n, pts);
  if (rc == PLONK_OK && hipMemcpyAsync(out_xy96, pts, sizeof(G1Affine) * (n + 2), hipMemcpyDeviceToHost, c.stream) != hipSuccess) rc = PLONK_ERR_HIP;
  if (hipStreamSynchronize(c.stream) != hipSuccess && rc == PLONK_OK) rc = PLONK_ERR_HIP;
  (void)hipFree(pts);
  return rc;
  });
}

int plonk_msm_dev(plonk_ctx* ctx, const void* scalars, uint64_t m, void* out97_dev) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || (!scalars && m) || !out97_dev) return PLONK_ERR_ARG;
  CTX_ENTER(ctx->c, api_fn);
  HIP_TRY(hipSetDevice(ctx->c.device));
  int rc = msm_reserve(&ctx->c, m ? m : 1);
  if (rc) return rc;
  rc = msm_device(&ctx->c, (const Fr*)scalars, m, (G1*)ctx->c.msm.result);
  if (rc) return rc;
  return xyzz_to_affine97_device(&ctx->c, (const G1*)ctx->c.msm.result, (uint8_t*)out97_dev);
  });
}

int plonk_msm(plonk_ctx* ctx, const uint64_t* scalars, uint64_t m, uint8_t out_xy_inf[97]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || (!scalars && m) || !out_xy_inf) return PLONK_ERR_ARG;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  if (m && !c.srs_table) return PLONK_ERR_NO_SRS;
  if (m > c.srs_n) return PLONK_ERR_DEGREE;
  int rc = msm_reserve(&c, m ? m : 1);
  if (rc) return rc;
  rc = ensure_scalar_staging(&c, m ? m : 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c.msm.scalars_stage, scalars, sizeof(Fr) * m, hipMemcpyHostToDevice, c.stream));
  // same tail as plonk_msm_batch: the 17 bit sums come back and the host finishes (15-term Horner chain + one Fp
  // inversion) — ~25 dependent additions and a Fermat inversion that a single GPU lane would otherwise serialise
  const Fr* sc = c.msm.scalars_stage;
  G1 sum;
  rc = msm_group_sums(&c, &sc, &m, 1, &sum);
  if (rc) return rc;
  xyzz_to_affine97_host(sum, out_xy_inf);
  return PLONK_OK;
  });
}

// Prover::commit_polynomials' 4-way rayon::join fan-out (prover.rs:187-210) as ONE call: up to
// MSM_MAX_BATCH scalar sets over the shared commit key go through the pipeline as one group (one
// launch of every kernel, one latency-bound reduction tail), the 16 bit sums per commitment come back
// in one copy and the host finishes them with one shared Fp inversion.
int plonk_msm_batch(plonk_ctx* ctx, const uint64_t* const* scalars, const uint64_t* m, int count, uint8_t* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !scalars || !m || !out || count < 0) return PLONK_ERR_ARG;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  uint64_t mmax = 0;
  for (int i = 0; i < count; ++i) {
    if (!scalars[i] && m[i]) return PLONK_ERR_ARG;
    if (m[i] && !c.srs_table) return PLONK_ERR_NO_SRS;
    if (m[i] > c.srs_n) return PLONK_ERR_DEGREE;
    if (m[i] > mmax) mmax = m[i];
  }
  int rc = msm_reserve(&c, mmax ? mmax : 1);
  if (rc) return rc;
  rc = ensure_scalar_staging(&c, (mmax ? mmax : 1) * MSM_MAX_BATCH);
  if (rc) return rc;
  for (int k0 = 0; k0 < count; k0 += MSM_MAX_BATCH) {
    const int cnt = count - k0 < MSM_MAX_BATCH ? count - k0 : MSM_MAX_BATCH;
    const Fr* sc[MSM_MAX_BATCH];
    uint64_t ms[MSM_MAX_BATCH];
    for (int k = 0; k < cnt; ++k) {
      Fr* dst = c.msm.scalars_stage + (uint64_t)k * (mmax ? mmax : 1);
      if (m[k0 + k]) HIP_TRY(hipMemcpyAsync(dst, scalars[k0 + k], sizeof(Fr) * m[k0 + k], hipMemcpyHostToDevice, c.stream));
      sc[k] = dst;
      ms[k] = m[k0 + k];
    }
    G1 sums[MSM_MAX_BATCH];
    rc = msm_group_sums(&c, sc, ms, cnt, sums);
    if (rc) return rc;
    batch_xyzz_to_affine97(sums, cnt, reinterpret_cast<uint8_t (*)[97]>(out + 97 * (size_t)k0));
  }
  return PLONK_OK;
  });
}

// ---- measurement -------------------------------------------------------------------
int plonk_profile_enable(plonk_ctx* ctx, int on) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  ctx->c.profile = on != 0;
  return PLONK_OK;
  });
}
int plonk_profile_read(plonk_ctx* ctx, int slot, double* total_ms, uint64_t* launches) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || slot < 0 || slot >= plonk::Ctx::PROF_SLOTS) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  int rc = prof_collect(&ctx->c);
  if (rc) return rc;
  if (total_ms) *total_ms = ctx->c.acc_ms[slot];
  if (launches) *launches = ctx->c.acc_n[slot];
  return PLONK_OK;
  });
}
int plonk_profile_reset(plonk_ctx* ctx) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->c.mu);
  int rc = prof_collect(&ctx->c);
  for (int i = 0; i < plonk::Ctx::PROF_SLOTS; ++i) { ctx->c.acc_ms[i] = 0; ctx->c.acc_n[i] = 0; }
  return rc;
  });
}

}  // extern "C"
