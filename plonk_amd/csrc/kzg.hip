// KZG10 openings: CommitKey::compute_aggregate_witness + commit (open_single / open_multiple), AggregateProof::flatten,
// OpeningKey::batch_check of the reference (src/commitment_scheme/kzg10/key.rs:394-417, 571-591, 661-707, 724-809;
// proof.rs:15-111), and plonk_srs_check: a loaded commit key against an opening key with one pairing.
//
//   plonk_kzg_open[_dev]    trimmed lengths (kzg_trim_kernel for resident polynomials), v^i on the device
//                           (kzg_powers_kernel), fold + evaluations in one pass over the coefficients
//                           (kzg_fold_eval_kernel / kzg_eval_final_kernel, poly.hip), Ruffini (poly_ruffini, or the shift
//                           at the point 0), the witness through the ordinary commitment path (msm_batch_device), the
//                           polynomial commitments through grouped launches of it (MSM_MAX_BATCH per launch)
//   plonk_kzg_flatten       sum v^i C_i with the verifier's decode + MSM kernels, sum v^i e_i on the host
//   plonk_kzg_batch_check   decode of the 2K commitments, the 3K + 1 terms of kzg_core.hpp, ONE launch of the verifier's
//                           two-sum MSM (verify.hip msm_run), one pairing check on the host
//   plonk_srs_check         r^i on the device (power_array_kernel), both sums as one group of two ordinary commitments
//                           over the context's tables (the second reads the same scalars one place further), one pairing
// Everything device-side lives in the context's grow-only KzgWork and is released with the context (kzg_ws_release).
#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/plonk_hip.h"
#include "plonk_internal.hpp"
#include "api_guard.hpp"
#include "poly.hpp"
#include "fr29.cuh"
#include "hostg1.hpp"
#include "hostpairing.hpp"
#include "verify_core.hpp"
#include "kzg_core.hpp"
#include "kzg_key.hpp"

namespace plonk {

static constexpr uint64_t KZG_STAGE_MIN = 1ull << 16;   // coefficients a staging buffer holds at least

struct KzgBufs {
  enum { DESC, VPOW, EVALS, PARTIAL, FOLD, SCRATCH, TOTALS, STAGE0, STAGE1, PTS, KIND, COMP, SC, IDS, PART, POWERS,
         E_POINTS, E_PROOFS, E_PAIRS, E_PRE, E_VERDICT, E_VALUES, NBUF };   // E_*: the per-item checks (pairing.hip)
};
struct KzgWork : KzgBufs, DevBufs<KzgBufs::NBUF> {
  hipEvent_t up[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  ~KzgWork() {   // the events go before the buffers, which the base frees
    for (int b = 0; b < 2; ++b) {
      if (up[b]) (void)hipEventDestroy(up[b]);
      if (done[b]) (void)hipEventDestroy(done[b]);
    }
  }
  int events() {
    for (int b = 0; b < 2; ++b) {
      if (!up[b]) HIP_TRY(hipEventCreateWithFlags(&up[b], hipEventDisableTiming));
      if (!done[b]) HIP_TRY(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
    }
    return PLONK_OK;
  }
};

static KzgWork& kzg_work(Ctx* c) {
  if (!c->kzg_ws) c->kzg_ws = new KzgWork();
  return *(KzgWork*)c->kzg_ws;
}
void kzg_ws_release(Ctx* c) {
  delete (KzgWork*)c->kzg_ws;
  c->kzg_ws = nullptr;
}

// the two upload buffers of the host forms (each at least `values` Fr) with their events and the copy stream: kzg_evals.hip
// stages vectors of values through the buffers plonk_kzg_open stages coefficients through
int kzg_stage_reserve(Ctx* c, uint64_t values, Fr* stage[2], hipEvent_t up[2], hipEvent_t done[2]) {
  KzgWork& w = kzg_work(c);
  PTRY(w.need(KzgWork::STAGE0, sizeof(Fr) * values));
  PTRY(w.need(KzgWork::STAGE1, sizeof(Fr) * values));
  PTRY(w.events());
  if (!c->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b) {
    stage[b] = w.at<Fr>(b ? KzgWork::STAGE1 : KzgWork::STAGE0);
    up[b] = w.up[b];
    done[b] = w.done[b];
  }
  return PLONK_OK;
}

// commitments of up to MSM_MAX_BATCH resident scalar sets (every m > 0) as one grouped launch, finished on the host like
// plonk_msm_batch's: 48-byte compressed each
static int commit_group(Ctx* c, const Fr* const* sc, const uint64_t* m, int cnt, uint8_t* out48) {
  G1 sums[MSM_MAX_BATCH];
  uint8_t aff[MSM_MAX_BATCH][97];
  PTRY(msm_group_sums(c, sc, m, cnt, sums));
  batch_xyzz_to_affine97(sums, cnt, aff);
  for (int k = 0; k < cnt; ++k) g1_compress97(aff[k], out48 + 48 * k);
  return PLONK_OK;
}

// commitments of the polynomials desc[0, cnt) (device pointers, trimmed lengths) into out48[0, cnt): grouped launches
static int commit_polys(Ctx* c, const KzgDesc* desc, uint32_t cnt, uint8_t* out48) {
  const Fr* sc[MSM_MAX_BATCH];
  uint64_t m[MSM_MAX_BATCH];
  uint32_t which[MSM_MAX_BATCH];
  uint8_t tmp[MSM_MAX_BATCH * 48];
  int g = 0;
  for (uint32_t i = 0; i <= cnt; ++i) {
    if (i < cnt) {
      if (!desc[i].len) { identity48(out48 + 48ull * i); continue; }
      sc[g] = desc[i].p; m[g] = desc[i].len; which[g] = i; ++g;
    }
    if (g == MSM_MAX_BATCH || (i == cnt && g)) {
      PTRY(commit_group(c, sc, m, g, tmp));
      for (int k = 0; k < g; ++k) memcpy(out48 + 48ull * which[k], tmp + 48 * k, 48);
      g = 0;
    }
  }
  return PLONK_OK;
}

// One fold launch over desc_dev[first, first + cnt): the first launch of a call covers the whole fold and overwrites it
static int fold_group(Ctx* c, KzgWork& w, uint32_t first, uint32_t cnt, uint64_t group_len, uint64_t L, bool* started, const Fr& z) {
  KzgFoldArgs a;
  a.desc = w.at<const KzgDesc>(KzgWork::DESC);
  a.vpow = w.p[KzgWork::VPOW];
  a.first = first;
  a.count = cnt;
  a.len = *started ? group_len : L;
  a.accumulate = *started ? 1 : 0;
  a.fold = w.at<Fr>(KzgWork::FOLD);
  a.partial = w.at<Fr>(KzgWork::PARTIAL);
  a.point = z;
  *started = true;
  return poly_kzg_fold_eval(c, a, w.at<Fr>(KzgWork::EVALS) + first);
}

static int kzg_open_body(const char* api_fn, Ctx& c, const void* const* polys, const uint64_t* lens, uint64_t count, const Fr& z,
                         const Fr& v, uint64_t* evaluations, uint8_t* commitments, uint8_t* witness48, bool resident);

static int kzg_open_impl(const char* api_fn, plonk_ctx* ctx, const void* const* polys, const uint64_t* lens, uint64_t count,
                         const uint64_t* point, const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments,
                         uint8_t* witness48, bool resident) {
  if (!ctx || !point || !witness48 || (count && (!polys || !lens || !evaluations)) || (count > 1 && !v_challenge))
    API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count > KZG_MAX_OPEN) API_FAIL(PLONK_ERR_ARG, "invalid argument: at most 65536 polynomials per call");
  Fr z, v = Fr::one();
  if (!kzg_fr_load(point, &z) || (v_challenge && !kzg_fr_load(v_challenge, &v))) API_FAIL(PLONK_ERR_DATA, "non-canonical scalar");
  for (uint64_t i = 0; i < count; ++i)
    if (lens[i] && !polys[i]) API_FAIL(PLONK_ERR_ARG, "invalid argument: polys[i] is NULL with lens[i] > 0");
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  if (c.nccl_comm) API_FAIL(PLONK_ERR_STATE, "a context with a communicator holds only a range of the commit key");
  if (count && !c.srs_table) return PLONK_ERR_NO_SRS;
  const int rc = kzg_open_body(api_fn, c, polys, lens, count, z, v, evaluations, commitments, witness48, resident);
  if (rc != PLONK_OK) {   // an error leaves nothing of the call queued (the evaluations' copy, a staged upload) and no profile slot open
    if (c.copy_stream) (void)hipStreamSynchronize(c.copy_stream);
    (void)hipStreamSynchronize(c.stream);
    for (int slot = 12; slot <= 14; ++slot) prof_end(&c, slot);
  }
  return rc;
}

static int kzg_open_body(const char* api_fn, Ctx& c, const void* const* polys, const uint64_t* lens, uint64_t count, const Fr& z,
                         const Fr& v, uint64_t* evaluations, uint8_t* commitments, uint8_t* witness48, bool resident) {
  KzgWork& w = kzg_work(&c);
  const uint32_t n = (uint32_t)count;
  // trimmed lengths (Polynomial::from_coefficients_vec): the degree CommitKey::commit checks
  std::vector<KzgDesc> desc(n);
  if (resident) {
    for (uint32_t i = 0; i < n; ++i) desc[i] = KzgDesc{(const Fr*)polys[i], lens[i]};
    if (n) {
      PTRY(w.need(KzgWork::DESC, sizeof(KzgDesc) * n));
      prof_begin(&c, 12);
      HIP_TRY(hipMemcpyAsync(w.p[KzgWork::DESC], desc.data(), sizeof(KzgDesc) * n, hipMemcpyHostToDevice, c.stream));
      PTRY(poly_kzg_trim(&c, w.at<KzgDesc>(KzgWork::DESC), n));
      HIP_TRY(hipMemcpyAsync(desc.data(), w.p[KzgWork::DESC], sizeof(KzgDesc) * n, hipMemcpyDeviceToHost, c.stream));
      prof_end(&c, 12);
      HIP_TRY(hipStreamSynchronize(c.stream));
    }
  } else {
    for (uint32_t i = 0; i < n; ++i) desc[i] = KzgDesc{nullptr, host_trimmed((const uint64_t*)polys[i], lens[i])};
  }
  uint64_t L = 0;
  for (uint32_t i = 0; i < n; ++i) L = desc[i].len > L ? desc[i].len : L;
  if (L > c.srs_n) return PLONK_ERR_DEGREE;
  identity48(witness48);
  if (!L) {   // every polynomial is zero: zero evaluations, identity commitments, Polynomial::zero() as the witness
    for (uint64_t i = 0; i < 4 * count; ++i) evaluations[i] = 0;
    if (commitments) for (uint32_t i = 0; i < n; ++i) identity48(commitments + 48ull * i);
    return PLONK_OK;
  }
  PTRY(msm_reserve(&c, L));
  PTRY(w.need(KzgWork::DESC, sizeof(KzgDesc) * n));
  PTRY(w.need(KzgWork::VPOW, sizeof(Fr29Slot) * n));
  PTRY(w.need(KzgWork::EVALS, sizeof(Fr) * n));
  PTRY(w.need(KzgWork::PARTIAL, sizeof(Fr) * KZG_GROUP * kzg_fold_waves(L)));
  PTRY(w.need(KzgWork::FOLD, sizeof(Fr) * (L + 1)));
  PTRY(w.need(KzgWork::SCRATCH, sizeof(Fr) * (L + 1)));
  PTRY(w.need(KzgWork::TOTALS, sizeof(Fr) * (L / 2048 + 2)));
  prof_begin(&c, 12);
  PTRY(poly_kzg_powers(&c, w.p[KzgWork::VPOW], n, v));
  HIP_TRY(hipMemsetAsync(w.p[KzgWork::EVALS], 0, sizeof(Fr) * n, c.stream));
  bool started = false;
  if (resident) {
    for (uint32_t first = 0; first < n; first += KZG_GROUP) {
      const uint32_t cnt = n - first < KZG_GROUP ? n - first : KZG_GROUP;
      uint64_t glen = 0;
      for (uint32_t i = 0; i < cnt; ++i) glen = desc[first + i].len > glen ? desc[first + i].len : glen;
      if (glen) PTRY(fold_group(&c, w, first, cnt, glen, L, &started, z));
    }
    prof_end(&c, 12);
    if (commitments) PTRY(commit_polys(&c, desc.data(), n, commitments));
  } else {
    // groups of polynomials packed into one of two staging buffers: the upload of group g + 1 (copy stream) runs under the
    // fold kernel of group g (main stream); a buffer is reused once the work that read it has finished
    const uint64_t S = L > KZG_STAGE_MIN ? L : KZG_STAGE_MIN;
    PTRY(w.need(KzgWork::STAGE0, sizeof(Fr) * S));
    PTRY(w.need(KzgWork::STAGE1, sizeof(Fr) * S));
    PTRY(w.events());
    if (!c.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
    prof_end(&c, 12);
    HIP_TRY(hipStreamSynchronize(c.stream));   // the copy stream is not ordered behind what the main stream still runs
    uint32_t first = 0, g = 0;
    int rc = PLONK_OK;
    while (first < n && rc == PLONK_OK) {
      const int b = g & 1;
      Fr* stage = w.at<Fr>(b ? KzgWork::STAGE1 : KzgWork::STAGE0);
      uint64_t used = 0, glen = 0;
      uint32_t cnt = 0;
      while (first + cnt < n && cnt < KZG_GROUP && used + desc[first + cnt].len <= S) {
        desc[first + cnt].p = stage + used;
        used += desc[first + cnt].len;
        glen = desc[first + cnt].len > glen ? desc[first + cnt].len : glen;
        ++cnt;
      }
      hipError_t e = hipSuccess;
      if (g >= 2) e = hipStreamWaitEvent(c.copy_stream, w.done[b], 0);
      for (uint32_t i = 0; i < cnt && e == hipSuccess; ++i)
        if (desc[first + i].len)
          e = hipMemcpyAsync((void*)desc[first + i].p, polys[first + i], sizeof(Fr) * desc[first + i].len, hipMemcpyHostToDevice, c.copy_stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(w.at<KzgDesc>(KzgWork::DESC) + first, desc.data() + first, sizeof(KzgDesc) * cnt, hipMemcpyHostToDevice, c.copy_stream);
      if (e == hipSuccess) e = hipEventRecord(w.up[b], c.copy_stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(c.stream, w.up[b], 0);
      if (e != hipSuccess) { set_last_error(api_fn, hipGetErrorString(e), __FILE__, __LINE__); rc = PLONK_ERR_HIP; break; }
      if (glen) {   // slot 12 takes the fold launches, not the uploads they wait for nor the polynomial commitments
        prof_begin(&c, 12);
        rc = fold_group(&c, w, first, cnt, glen, L, &started, z);
        prof_end(&c, 12);
      }
      if (rc == PLONK_OK && commitments) rc = commit_polys(&c, desc.data() + first, cnt, commitments + 48ull * first);
      if (rc == PLONK_OK && hipEventRecord(w.done[b], c.stream) != hipSuccess) rc = PLONK_ERR_HIP;
      first += cnt;
      ++g;
    }
    if (rc != PLONK_OK) return rc;
  }
  HIP_TRY(hipMemcpyAsync(evaluations, w.p[KzgWork::EVALS], sizeof(Fr) * n, hipMemcpyDeviceToHost, c.stream));
  // the witness: fold / (X - z), remainder dropped (Polynomial::ruffini)
  const Fr* wit = nullptr;
  if (L > 1) {
    prof_begin(&c, 13);
    if (z.is_zero()) {
      PTRY(poly_shift_down(&c, w.at<Fr>(KzgWork::FOLD), w.at<Fr>(KzgWork::SCRATCH), L));
      wit = w.at<Fr>(KzgWork::SCRATCH);
    } else {
      PTRY(poly_ruffini(&c, w.at<Fr>(KzgWork::FOLD), w.at<Fr>(KzgWork::FOLD), L, z, z.inv(), w.at<Fr>(KzgWork::SCRATCH),
                          w.at<Fr>(KzgWork::TOTALS)));
      wit = w.at<Fr>(KzgWork::FOLD);
    }
    prof_end(&c, 13);
    const uint64_t m = L - 1;
    prof_begin(&c, 14);
    const int rc = commit_group(&c, &wit, &m, 1, witness48);
    prof_end(&c, 14);
    PTRY(rc);
  }
  HIP_TRY(hipStreamSynchronize(c.stream));
  return PLONK_OK;
}

// ---- the opening key (kzg_key.hpp) ---------------------------------------------------------------------------------------
static int check_reserve(KzgWork& w, uint64_t npts, uint64_t nterms) {
  PTRY(w.need(KzgWork::PTS, sizeof(G1Affine) * npts));
  PTRY(w.need(KzgWork::KIND, 4 * npts));
  PTRY(w.need(KzgWork::COMP, 48 * npts));
  PTRY(w.need(KzgWork::SC, 32 * nterms));
  PTRY(w.need(KzgWork::IDS, 4 * nterms));
  PTRY(w.need(KzgWork::PART, sizeof(G1) * 2 * VERIFY_MSM_MAX_BLOCKS));
  return PLONK_OK;
}

static void compress_h1(const H1& s, uint8_t out48[48]) {
  const G1Aff64 a = xyzz_to_aff(s);
  uint8_t raw[97];
  memset(raw, 0, sizeof raw);
  if (a.inf) raw[96] = 1;
  else { memcpy(raw, a.x.l, 48); memcpy(raw + 48, a.y.l, 48); }
  g1_compress97(raw, out48);
}

// ---- per-item verdicts (pairing.hip) ----------------------------------------------------------------------------------
static void each_info(plonk_verify_info* info, uint64_t count, uint64_t terms_per_item, uint32_t checked, uint32_t rejected,
                      double ms_decode, double ms_scalars, double ms_msm, double ms_pairing) {
  if (!info) return;
  info->proofs = count;
  info->msm_terms = terms_per_item * checked;
  info->pairing_checks = checked;
  info->rejected = rejected;
  info->ms_decode = ms_decode;
  info->ms_scalars = ms_scalars;
  info->ms_msm = ms_msm;
  info->ms_pairing = ms_pairing;
}

// plonk_kzg_pairing_check_each and its test hook (values != NULL: 72 words per check)
static int pairing_each_body(plonk_kzg_key* key, const uint8_t* a48, const uint8_t* b48, uint64_t count, int32_t* verdicts,
                             plonk_verify_info* info, uint64_t* values) {
  KzgKey* kk = key->k;
  Ctx& c = *kk->c;
  KzgWork& w = kzg_work(&c);
  PTRY(pairing_tables_create(&c, kk->x_h, kk->h, &kk->pair_tables));
  const uint64_t npts = 2 * count;
  PTRY(check_reserve(w, npts, 1));
  PTRY(w.need(KzgWork::E_PAIRS, sizeof(G1) * npts));
  PTRY(w.need(KzgWork::E_PRE, 4 * count));
  PTRY(w.need(KzgWork::E_VERDICT, 4 * count));
  if (values) PTRY(w.need(KzgWork::E_VALUES, 8 * 72 * count));
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> comp(48 * npts);
  for (uint64_t k = 0; k < count; ++k) {
    memcpy(comp.data() + 96 * k, a48 + 48 * k, 48);
    memcpy(comp.data() + 96 * k + 48, b48 + 48 * k, 48);
  }
  std::vector<int32_t> st;
  PTRY(decode_points(&c, comp.data(), (uint32_t)npts, w.at<uint8_t>(KzgWork::COMP), w.at<G1Affine>(KzgWork::PTS),
                       w.at<int32_t>(KzgWork::KIND), &st));
  const auto t1 = std::chrono::steady_clock::now();
  PTRY(each_pairs_launch(&c, w.at<const G1Affine>(KzgWork::PTS), w.at<const int32_t>(KzgWork::KIND), count,
                           w.at<G1>(KzgWork::E_PAIRS), w.at<int32_t>(KzgWork::E_PRE)));
  PTRY(pairing_each_launch(&c, kk->pair_tables, w.at<const G1>(KzgWork::E_PAIRS), w.at<const int32_t>(KzgWork::E_PRE), count,
                             w.at<int32_t>(KzgWork::E_VERDICT), values ? w.at<uint64_t>(KzgWork::E_VALUES) : nullptr));
  if (values) HIP_TRY(hipMemcpyAsync(values, w.p[KzgWork::E_VALUES], 8 * 72 * count, hipMemcpyDeviceToHost, c.stream));
  uint32_t checked = 0, rejected = 0;
  PTRY(each_finish(&c, w.at<const int32_t>(KzgWork::E_VERDICT), w.at<const int32_t>(KzgWork::E_PRE), count, verdicts, &checked,
                     &rejected));
  const auto t2 = std::chrono::steady_clock::now();
  each_info(info, count, 0, checked, rejected, ms_between(t0, t1), 0, 0, ms_between(t1, t2));
  return rejected ? PLONK_ERR_VERIFY : PLONK_OK;
}

static int kzg_check_each_body(plonk_kzg_key* key, const uint64_t* points, const plonk_kzg_proof* proofs, uint64_t count,
                               int32_t* verdicts, plonk_verify_info* info) {
  KzgKey* kk = key->k;
  Ctx& c = *kk->c;
  KzgWork& w = kzg_work(&c);
  PTRY(pairing_tables_create(&c, kk->x_h, kk->h, &kk->pair_tables));
  const uint64_t npts = 1 + 2 * count, nterms = KZG_EACH_TERMS * count;
  PTRY(check_reserve(w, npts, nterms));
  PTRY(w.need(KzgWork::E_POINTS, 32 * count));
  PTRY(w.need(KzgWork::E_PROOFS, sizeof(plonk_kzg_proof) * count));
  PTRY(w.need(KzgWork::E_PAIRS, sizeof(G1) * 2 * count));
  PTRY(w.need(KzgWork::E_PRE, 4 * count));
  PTRY(w.need(KzgWork::E_VERDICT, 4 * count));
  const auto t0 = std::chrono::steady_clock::now();
  // the point table [g | C_0 W_0 | C_1 W_1 ...], as plonk_kzg_batch_check's
  std::vector<uint8_t> comp(48 * npts);
  memcpy(comp.data(), kk->opening_key, 48);
  for (uint64_t k = 0; k < count; ++k) {
    memcpy(comp.data() + 48 * (1 + 2 * k), proofs[k].commitment, 48);
    memcpy(comp.data() + 48 * (2 + 2 * k), proofs[k].witness, 48);
  }
  std::vector<int32_t> st;
  PTRY(decode_points(&c, comp.data(), (uint32_t)npts, w.at<uint8_t>(KzgWork::COMP), w.at<G1Affine>(KzgWork::PTS),
                       w.at<int32_t>(KzgWork::KIND), &st));
  const auto t1 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpyAsync(w.p[KzgWork::E_POINTS], points, 32 * count, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(w.p[KzgWork::E_PROOFS], proofs, sizeof(plonk_kzg_proof) * count, hipMemcpyHostToDevice, c.stream));
  PTRY(kzg_each_pack_launch(&c, w.at<const uint64_t>(KzgWork::E_POINTS), w.at<const plonk_kzg_proof>(KzgWork::E_PROOFS),
                              w.at<const int32_t>(KzgWork::KIND), count, w.at<uint32_t>(KzgWork::SC), w.at<uint32_t>(KzgWork::IDS),
                              w.at<int32_t>(KzgWork::E_PRE)));
  HIP_TRY(hipStreamSynchronize(c.stream));
  const auto t2 = std::chrono::steady_clock::now();
  PTRY(each_sums_launch(&c, w.at<const uint32_t>(KzgWork::SC), w.at<const uint32_t>(KzgWork::IDS), 1, 3, count,
                          w.at<const G1Affine>(KzgWork::PTS), w.at<const int32_t>(KzgWork::KIND), w.at<const int32_t>(KzgWork::E_PRE),
                          w.at<G1>(KzgWork::E_PAIRS)));
  HIP_TRY(hipStreamSynchronize(c.stream));
  const auto t3 = std::chrono::steady_clock::now();
  PTRY(pairing_each_launch(&c, kk->pair_tables, w.at<const G1>(KzgWork::E_PAIRS), w.at<const int32_t>(KzgWork::E_PRE), count,
                             w.at<int32_t>(KzgWork::E_VERDICT), nullptr));
  uint32_t checked = 0, rejected = 0;
  PTRY(each_finish(&c, w.at<const int32_t>(KzgWork::E_VERDICT), w.at<const int32_t>(KzgWork::E_PRE), count, verdicts, &checked,
                     &rejected));
  const auto t4 = std::chrono::steady_clock::now();
  each_info(info, count, KZG_EACH_TERMS, checked, rejected, ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, t3),
            ms_between(t3, t4));
  return rejected ? PLONK_ERR_VERIFY : PLONK_OK;
}

}  // namespace plonk

using namespace plonk;

extern "C" {

int plonk_kzg_pairing_check_each(plonk_kzg_key* key, const uint8_t* a48, const uint8_t* b48, uint64_t count, int32_t* verdicts,
                                 plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!key || !a48 || !b48 || !verdicts) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count == 0 || count > KZG_MAX_BATCH) API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 2^24]");
  if (info) memset(info, 0, sizeof *info);
  Ctx& c = *key->k->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  const int rc = pairing_each_body(key, a48, b48, count, verdicts, info, nullptr);
  if (rc != PLONK_OK && rc != PLONK_ERR_VERIFY) (void)hipStreamSynchronize(c.stream);   // nothing of the call stays queued
  if (rc == PLONK_ERR_VERIFY) set_last_error(api_fn, "at least one pairing check fails", __FILE__, __LINE__);
  return rc;
  });
}

int plonk_kzg_check_each(plonk_kzg_key* key, const uint64_t* points, const plonk_kzg_proof* proofs, uint64_t count,
                         int32_t* verdicts, plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!key || !points || !proofs || !verdicts) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count == 0 || count > KZG_MAX_BATCH) API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 2^24]");
  if (info) memset(info, 0, sizeof *info);
  Ctx& c = *key->k->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  const int rc = kzg_check_each_body(key, points, proofs, count, verdicts, info);
  if (rc != PLONK_OK && rc != PLONK_ERR_VERIFY) (void)hipStreamSynchronize(c.stream);
  if (rc == PLONK_ERR_VERIFY) set_last_error(api_fn, "at least one opening does not verify", __FILE__, __LINE__);
  return rc;
  });
}

// Test hook (not in include/plonk_hip.h, not part of the API): plonk_kzg_pairing_check_each that also writes each check's
// final-exponentiated Fp12 value as 12 canonical integers of 6 words (tower order: put_f12 of tests/csrc/host_verify.cpp; zeros
// for an item that did not reach the pairing).  The binding's KzgKey._pairing_each_values calls it for
// tests/test_gpu_pairing_each.py.
int plonk_test_pairing_each(plonk_kzg_key* key, const uint8_t* a48, const uint8_t* b48, uint64_t count, uint64_t* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!key || !a48 || !b48 || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count == 0 || count > (1ull << 16)) API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 2^16]");
  Ctx& c = *key->k->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  std::vector<int32_t> verdicts(count);
  const int rc = pairing_each_body(key, a48, b48, count, verdicts.data(), nullptr, out);
  if (rc != PLONK_OK && rc != PLONK_ERR_VERIFY) (void)hipStreamSynchronize(c.stream);
  return rc == PLONK_ERR_VERIFY ? PLONK_OK : rc;
  });
}

int plonk_kzg_open(plonk_ctx* ctx, const uint64_t* const* polys, const uint64_t* lens, uint64_t count, const uint64_t point[4],
                   const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments, uint8_t witness48[48]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::kzg_open_impl(api_fn, ctx, (const void* const*)polys, lens, count, point, v_challenge, evaluations, commitments,
                                witness48, false);
  });
}

int plonk_kzg_open_dev(plonk_ctx* ctx, const void* const* polys_dev, const uint64_t* lens, uint64_t count, const uint64_t point[4],
                       const uint64_t* v_challenge, uint64_t* evaluations, uint8_t* commitments, uint8_t witness48[48]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
    return plonk::kzg_open_impl(api_fn, ctx, polys_dev, lens, count, point, v_challenge, evaluations, commitments, witness48, true);
  });
}

int plonk_kzg_flatten(plonk_ctx* ctx, const uint8_t* commitments, const uint64_t* evaluations, uint64_t count, const uint64_t v[4],
                      const uint8_t witness48[48], plonk_kzg_proof* out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !commitments || !evaluations || !v || !witness48 || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count == 0 || count > KZG_MAX_OPEN) API_FAIL(PLONK_ERR_ARG, "invalid argument: count must be in [1, 65536]");
  Fr vv;
  std::vector<Fr> ev(count);
  bool canon = kzg_fr_load(v, &vv);
  for (uint64_t i = 0; i < count; ++i) canon &= kzg_fr_load(evaluations + 4 * i, &ev[i]);
  if (!canon) API_FAIL(PLONK_ERR_DATA, "non-canonical scalar");
  std::vector<uint32_t> sc(8 * count), ids(count);
  const Fr e = kzg_flatten_scalars(vv, ev.data(), count, sc.data());
  for (uint64_t i = 0; i < count; ++i) ids[i] = (uint32_t)i;
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  KzgWork& w = kzg_work(&c);
  PTRY(check_reserve(w, count, count));
  std::vector<int32_t> st;
  PTRY(decode_points(&c, commitments, (uint32_t)count, w.at<uint8_t>(KzgWork::COMP), w.at<G1Affine>(KzgWork::PTS),
                       w.at<int32_t>(KzgWork::KIND), &st));
  for (uint64_t i = 0; i < count; ++i)
    if (st[i] == VDEC_BAD) API_FAIL(PLONK_ERR_POINT, "a commitment is not a valid compressed point of G1");
  HIP_TRY(hipMemcpyAsync(w.p[KzgWork::SC], sc.data(), 32 * count, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(w.p[KzgWork::IDS], ids.data(), 4 * count, hipMemcpyHostToDevice, c.stream));
  H1 sums[2];
  PTRY(msm_run(&c, w.at<const uint32_t>(KzgWork::SC), w.at<const uint32_t>(KzgWork::IDS), count, 0, w.at<const G1Affine>(KzgWork::PTS),
                 w.at<const int32_t>(KzgWork::KIND), w.at<G1>(KzgWork::PART), sums));
  compress_h1(sums[0], out->commitment);
  memcpy(out->evaluation, e.l, 32);
  memcpy(out->witness, witness48, 48);
  return PLONK_OK;
  });
}

int plonk_kzg_key_create(plonk_ctx* ctx, const uint8_t opening_key240[240], plonk_kzg_key** out) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!ctx || !opening_key240 || !out) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  *out = nullptr;
  if (const char* why = opening_key_invalid(opening_key240)) API_FAIL(PLONK_ERR_DATA, why);
  std::unique_ptr<KzgKey> k(new KzgKey());
  memcpy(k->opening_key, opening_key240, OPENING_KEY_LEN);
  k->h = g2_prepare(g2_decode_valid(opening_key240 + 48));
  k->x_h = g2_prepare(g2_decode_valid(opening_key240 + 144));
  k->last_u = Fr::zero();
  k->last_r = Fr::zero();
  Ctx& c = ctx->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  k->c = &c;
  KzgWork& w = kzg_work(&c);
  PTRY(check_reserve(w, 1, 1));
  std::vector<int32_t> st;
  PTRY(decode_points(&c, opening_key240, 1, w.at<uint8_t>(KzgWork::COMP), w.at<G1Affine>(KzgWork::PTS), w.at<int32_t>(KzgWork::KIND), &st));
  if (st[0] != VDEC_OK) API_FAIL(PLONK_ERR_STATE, "device decoding of the opening key's g disagrees with the host");
  HIP_TRY(hipMemcpy(&k->g_aff, w.p[KzgWork::PTS], sizeof(G1Affine), hipMemcpyDeviceToHost));
  *out = new plonk_kzg_key{k.release(), ctx};
  return PLONK_OK;
  });
}

void plonk_kzg_key_destroy(plonk_kzg_key* key) {
  if (!key) return;
  (void)plonk::api_guard(__func__, [&]() -> int {
    std::lock_guard<std::mutex> lk(key->ctx->c.mu);
    delete key->k;
    return PLONK_OK;
  });
  delete key;
}

int plonk_kzg_batch_check(plonk_kzg_key* key, const uint64_t* points, const plonk_kzg_proof* proofs, uint64_t count,
                          const uint8_t* label, uint64_t label_len, const uint64_t* u_override, plonk_verify_info* info) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!key || (count && (!points || !proofs)) || (label_len && !label)) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  if (count > KZG_MAX_BATCH) API_FAIL(PLONK_ERR_ARG, "invalid argument: at most 2^24 openings per call");
  if (info) memset(info, 0, sizeof *info);
  if (count == 0) API_FAIL(PLONK_ERR_VERIFY, "empty batch (Error::ProofVerificationError, key.rs:667)");
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<Fr> z(count);
  Fr u = Fr::one(), tmp;
  bool canon = !u_override || kzg_fr_load(u_override, &u);
  for (uint64_t k = 0; k < count; ++k) canon &= kzg_fr_load(points + 4 * k, &z[k]) && kzg_fr_load(proofs[k].evaluation, &tmp);
  if (!canon) API_FAIL(PLONK_ERR_DATA, "non-canonical scalar");
  KzgKey* kk = key->k;
  Ctx& c = *kk->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  KzgWork& w = kzg_work(&c);
  const uint64_t npts = 1 + 2 * count, nterms = 3 * count + 1;
  PTRY(check_reserve(w, npts, nterms));
  // the point table [g | C_0 W_0 | C_1 W_1 ...]: decoded and subgroup-checked on the device
  std::vector<uint8_t> comp(48 * npts);
  memcpy(comp.data(), kk->opening_key, 48);
  for (uint64_t k = 0; k < count; ++k) {
    memcpy(comp.data() + 48 * (1 + 2 * k), proofs[k].commitment, 48);
    memcpy(comp.data() + 48 * (2 + 2 * k), proofs[k].witness, 48);
  }
  std::vector<int32_t> st;
  PTRY(decode_points(&c, comp.data(), (uint32_t)npts, w.at<uint8_t>(KzgWork::COMP), w.at<G1Affine>(KzgWork::PTS),
                       w.at<int32_t>(KzgWork::KIND), &st));
  for (uint64_t i = 0; i < npts; ++i)
    if (st[i] == VDEC_BAD) API_FAIL(PLONK_ERR_POINT, "a commitment is not a valid compressed point of G1");
  const auto t1 = std::chrono::steady_clock::now();
  if (!u_override) u = kzg_batch_challenge(label, label_len, z.data(), proofs, count);
  kk->last_u = u;
  std::vector<uint32_t> sc(8 * nterms), ids(nterms);
  kzg_batch_terms(u, z.data(), proofs, count, sc.data(), ids.data());
  const auto t2 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpyAsync(w.p[KzgWork::SC], sc.data(), 32 * nterms, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipMemcpyAsync(w.p[KzgWork::IDS], ids.data(), 4 * nterms, hipMemcpyHostToDevice, c.stream));
  H1 sums[2];
  PTRY(msm_run(&c, w.at<const uint32_t>(KzgWork::SC), w.at<const uint32_t>(KzgWork::IDS), count, 2 * count + 1,
                 w.at<const G1Affine>(KzgWork::PTS), w.at<const int32_t>(KzgWork::KIND), w.at<G1>(KzgWork::PART), sums));
  const auto t3 = std::chrono::steady_clock::now();
  const bool ok = pairing_check(sums, kk->x_h, kk->h);
  const auto t4 = std::chrono::steady_clock::now();
  if (info) {
    info->proofs = count;
    info->msm_terms = nterms;
    info->pairing_checks = 1;
    info->rejected = ok ? 0 : (uint32_t)count;
    info->ms_decode = ms_between(t0, t1);
    info->ms_scalars = ms_between(t1, t2);
    info->ms_msm = ms_between(t2, t3);
    info->ms_pairing = ms_between(t3, t4);
  }
  if (!ok) API_FAIL(PLONK_ERR_VERIFY, "the batch of openings does not verify (Error::PairingCheckFailure)");
  return PLONK_OK;
  });
}

int plonk_srs_check(plonk_kzg_key* key, const uint8_t seed32[32]) {
  const char* const api_fn = __func__;
  return plonk::api_guard(api_fn, [&]() -> int {
  if (!key || !seed32) API_FAIL(PLONK_ERR_ARG, "invalid argument: a required pointer is NULL");
  KzgKey* kk = key->k;
  Ctx& c = *kk->c;
  CTX_ENTER(c, api_fn);
  HIP_TRY(hipSetDevice(c.device));
  if (c.nccl_comm) API_FAIL(PLONK_ERR_STATE, "a context with a communicator holds only a range of the commit key");
  if (!c.srs_table || !c.srs_n) return PLONK_ERR_NO_SRS;
  const uint64_t N = c.srs_n;
  const Fr r = kzg_srs_challenge(seed32, N, kk->opening_key);
  kk->last_r = r;
  KzgWork& w = kzg_work(&c);
  // t[0] = 1 for P_0, then t[1] = 0, t[2 + i] = r^i: sum A reads t + 2 (N - 1 terms over P_0 ..), sum B reads t + 1 (N terms:
  // the same scalars one place further, P_1 ..)
  PTRY(w.need(KzgWork::POWERS, sizeof(Fr) * (N + 2)));
  Fr* t = w.at<Fr>(KzgWork::POWERS);
  const Fr head[2] = {Fr::one(), Fr::zero()};
  HIP_TRY(hipMemcpyAsync(t, head, sizeof head, hipMemcpyHostToDevice, c.stream));
  PTRY(poly_power_array(&c, t + 2, N - 1, r));
  PTRY(msm_reserve(&c, N));
  const Fr* sc[3] = {t, t + 2, t + 1};
  const uint64_t m[3] = {1, N - 1, N};
  const int cnt = N > 1 ? 3 : 1;
  G1 s[3];
  PTRY(msm_group_sums(&c, sc, m, cnt, s));
  uint8_t p0[97];
  xyzz_to_affine97_host(s[0], p0);
  if (p0[96] || memcmp(p0, kk->g_aff.x.l, 48) || memcmp(p0 + 48, kk->g_aff.y.l, 48))
    API_FAIL(PLONK_ERR_VERIFY, "the first point of the commit key is not the opening key's g");
  if (N > 1) {
    const H1 sums[2] = {h1_of_g1(s[1]), h1_of_g1(s[2])};
    if (!pairing_check(sums, kk->x_h, kk->h)) API_FAIL(PLONK_ERR_VERIFY, "the commit key is not the powers of the opening key's tau");
  }
  return PLONK_OK;
  });
}

// Test hook (not in include/plonk_hip.h, not part of the API): the challenges the key's last plonk_kzg_batch_check (u) and
// plonk_srs_check (r) used, Montgomery limbs.  The binding's KzgKey._last_challenges calls it for tests/test_gpu_kzg.py.
int plonk_test_kzg_last(plonk_kzg_key* key, uint64_t u_out[4], uint64_t r_out[4]) {
  if (!key || !u_out || !r_out) return PLONK_ERR_ARG;
  std::lock_guard<std::mutex> lk(key->ctx->c.mu);
  memcpy(u_out, key->k->last_u.l, 32);
  memcpy(r_out, key->k->last_r.l, 32);
  return PLONK_OK;
}

}  // extern "C"
