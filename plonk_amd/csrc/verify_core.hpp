// Host half of proof verification (no HIP): Proof::verify of the reference (src/proof_system/proof.rs:218-513, V3 and the
// legacy V2 seeding) up to, but not including, its MSM and pairing.  For one proof it replays the transcript, checks the
// evaluations are canonical, evaluates PI(z) and L1(z) (compute_lagrange_and_barycentric_evaluations, proof.rs:997-1039)
// and turns r0, [D], [F], [E] into the scalars of the check
//
//     e(-L, x_h) * e(R, h) == 1,   L = [W_z] + u [W_zw],
//     R = z [W_z] + u z w [W_zw] + [F] - [E] + [D]  =  sum_j s_j VK_j + s_g g + sum_c s_c C_c
//
// over the 15 verifier-key points VK_j, the opening key's g and the proof's 11 commitments C_c.  The MSM (device,
// verify.hip) and the pairing (hostpairing.hpp) come after, for a whole batch.
// Included by verify.hip and by the CPU test harnesses (tests/csrc/host_verify.cpp, tests/csrc/host_verify_mixed.cpp).
#pragma once
#include <string>
#include <vector>

#include "transcript.hpp"
#include "widgets.hpp"
#include "fp_safegcd.cuh"   // fr_inv_gcd
#include "hostg2.hpp"      // g1_compressed_valid, g2_compressed_valid
#include "../../include/plonk_hip.h"

namespace plonk {
void set_last_error(const char* what, const char* detail, const char* file, int line);   // capi.hip (the CPU harness brings its own)

// Proof::to_bytes commitment order (proof.rs:137-162)
enum { PC_A = 0, PC_B, PC_C, PC_D, PC_Z, PC_TLOW, PC_TMID, PC_THIGH, PC_TFOURTH, PC_WZ, PC_WZW, PC_COUNT };
// VerifierKey::to_bytes order of the 15 commitments (widget.rs:84-111) -> PolyId
static const int VK_BLOB_ORDER[15] = {P_QM, P_QL, P_QR, P_QO, P_QF, P_QC, P_QARITH, P_QLOGIC, P_QRANGE, P_QFIXED, P_QVAR,
                                      P_S1, P_S2, P_S3, P_S4};
enum VerifyStatus { VS_OK = 0, VS_REJECT = 1, VS_DATA = 2, VS_POINT = 3 };
static constexpr uint64_t PROOF_BYTES = 1008;

struct VerifierCore {
  std::string label;
  uint64_t n = 0, constraints = 0;   // domain size, circuit size (vk.n)
  int version = 3;
  uint8_t vk[P_COUNT][48];           // compressed commitments, PolyId order
  Fr omega, n_inv, edwards_d;
  std::vector<uint64_t> pi_idx;      // the verifier's public-input rows
  std::vector<Fr> pi_root;           // omega^-idx, one per public input
  void init_constants() {
    uint32_t L = 0;
    while ((1ull << L) < n) ++L;
    omega = fr_domain_root(L);
    n_inv = Fr::from_u64(n).inv();
    edwards_d = (fr_small(10240) * fr_small(10241).inv()).neg();   // dusk_jubjub::EDWARDS_D
    const Fr omega_inv = omega.inv();
    pi_root.resize(pi_idx.size());
    for (size_t i = 0; i < pi_idx.size(); ++i) pi_root[i] = omega_inv.pow_u64(pi_idx[i]);
  }
};

// the scalars of one proof's check (Montgomery form)
struct ProofScalars {
  int status = VS_OK;
  Fr vk[P_COUNT];      // PolyId order
  Fr g;
  Fr comm[PC_COUNT];   // R side
  Fr u;                // L = [W_z] + u [W_zw]
};

// The replay and the scalars below are __host__ __device__ (field.cuh's HD): plonk_verify runs them on host threads through
// the VerifierCore wrappers (verify_scalars, barycentric_eval), plonk_verify_mixed in one device lane per proof
// (verify.hip), which reads a circuit's constants from this POD and its pi_root from a concatenated array.
struct SlotConst {
  uint64_t n, constraints;          // domain size, circuit size (vk.n)
  Fr omega, n_inv, edwards_d;
  uint64_t pi_count, pi_root_off;   // the circuit's pi_root: pi_root_all + pi_root_off
};

// compute_lagrange_and_barycentric_evaluations: false (Error::ProofVerificationError) when z = 1 or z is the root of a
// non-zero public input.  sum_i pi_i / d_i is accumulated as one fraction num / den, so one inversion of den_0 * den gives
// L1(z) = z_h / den_0 and PI(z) = z_h n^-1 num / den without scratch (the same field values as a batch inversion).
HD_NOINLINE bool barycentric_core(uint64_t n, const Fr& n_inv, const Fr* pi_root, uint64_t m, const Fr& z, const Fr* pi, const Fr& z_h,
                         Fr* l1, Fr* pi_eval) {
  const Fr one = Fr::one();
  const Fr den0 = Fr::from_u64(n) * (z - one);
  if (den0.is_zero()) return false;
  Fr num = Fr::zero(), den = one;
  for (uint64_t i = 0; i < m; ++i) {
    if (pi[i].is_zero()) continue;
    const Fr d = pi_root[i] * z - one;
    if (d.is_zero()) return false;
    num = num * d + pi[i] * den;
    den = den * d;
  }
  const Fr inv = fr_inv_gcd(den0 * den);
  *l1 = z_h * den * inv;
  *pi_eval = num * den0 * inv * z_h * n_inv;
  return true;
}
static bool barycentric_eval(const VerifierCore& v, const Fr& z, const Fr* pi, const Fr& z_h, Fr* l1, Fr* pi_eval) {
  return barycentric_core(v.n, v.n_inv, v.pi_root.data(), v.pi_root.size(), z, pi, z_h, l1, pi_eval);
}

HD bool fr_from_canonical(const uint8_t b[32], Fr* out) {   // BlsScalar::from_bytes: only values < q
  Fr x;
  memcpy(x.l, b, 32);
  uint64_t borrow = 0;   // x - q borrows iff x < q
#pragma unroll
  for (int i = 0; i < 8; ++i) borrow = (((uint64_t)x.l[i] - FrP::MOD[i] - borrow) >> 63) & 1;
  if (!borrow) return false;
  *out = x.to_mont();
  return true;
}

// Proof::verify up to its MSM (proof.rs:218-502) from a transcript already seeded with the label and the verifier key
// (seed_transcript_vk).  pi: the circuit's public inputs in Montgomery form.  digest (may be null): the proof digest of a
// mixed batch, challenge_bytes("batch digest", 32) drawn after u; zero when the evaluations are not canonical.
HD void replay_scalars(const SlotConst& v, const Fr* pi_root, Transcript& tr, const uint8_t* proof, const Fr* pi,
                       ProofScalars* out, uint8_t* digest) {
  ProofScalars& o = *out;
  o.status = VS_OK;
#pragma unroll
  for (int j = 0; j < P_COUNT; ++j) o.vk[j] = Fr::zero();
#pragma unroll
  for (int c = 0; c < PC_COUNT; ++c) o.comm[c] = Fr::zero();
  o.g = Fr::zero();
  o.u = Fr::zero();
  Fr raw[15];   // Proof::to_bytes evaluation order
  bool canonical = true;
#pragma unroll
  for (int k = 0; k < 15; ++k) canonical = fr_from_canonical(proof + PC_COUNT * 48 + 32 * k, &raw[k]) && canonical;
  if (!canonical) {
    o.status = VS_DATA;
    if (digest) memset(digest, 0, 32);
    return;
  }
  Evals ev;
  ev.a = raw[0]; ev.b = raw[1]; ev.c = raw[2]; ev.d = raw[3]; ev.a_w = raw[4]; ev.b_w = raw[5]; ev.d_w = raw[6];
  ev.q_arith = raw[7]; ev.q_c = raw[8]; ev.q_l = raw[9]; ev.q_r = raw[10]; ev.s1 = raw[11]; ev.s2 = raw[12]; ev.s3 = raw[13];
  ev.z = raw[14];
  const uint8_t* cm = proof;   // 11 x 48 compressed commitments
  // the public inputs (prover.rs:440-442, proof.rs:231-245)
  for (uint64_t i = 0; i < v.pi_count; ++i) tr.append_scalar("pi", pi[i]);
  tr.append_commitment("a_comm", cm + 48 * PC_A);
  tr.append_commitment("b_comm", cm + 48 * PC_B);
  tr.append_commitment("c_comm", cm + 48 * PC_C);
  tr.append_commitment("d_comm", cm + 48 * PC_D);
  const Fr beta = tr.challenge_scalar("beta");
  tr.append_scalar("beta", beta);
  const Fr gamma = tr.challenge_scalar("gamma");
  tr.append_commitment("z_comm", cm + 48 * PC_Z);
  const Fr alpha = tr.challenge_scalar("alpha");
  const Fr range_ch = tr.challenge_scalar("range separation challenge");
  const Fr logic_ch = tr.challenge_scalar("logic separation challenge");
  const Fr fixed_ch = tr.challenge_scalar("fixed base separation challenge");
  const Fr var_ch = tr.challenge_scalar("variable base separation challenge");
  tr.append_commitment("t_low_comm", cm + 48 * PC_TLOW);
  tr.append_commitment("t_mid_comm", cm + 48 * PC_TMID);
  tr.append_commitment("t_high_comm", cm + 48 * PC_THIGH);
  tr.append_commitment("t_fourth_comm", cm + 48 * PC_TFOURTH);
  const Fr z = tr.challenge_scalar("z_challenge");
  tr.append_scalar("a_eval", ev.a);
  tr.append_scalar("b_eval", ev.b);
  tr.append_scalar("c_eval", ev.c);
  tr.append_scalar("d_eval", ev.d);
  tr.append_scalar("s_sigma_1_eval", ev.s1);
  tr.append_scalar("s_sigma_2_eval", ev.s2);
  tr.append_scalar("s_sigma_3_eval", ev.s3);
  tr.append_scalar("z_eval", ev.z);
  tr.append_scalar("a_w_eval", ev.a_w);
  tr.append_scalar("b_w_eval", ev.b_w);
  tr.append_scalar("d_w_eval", ev.d_w);
  tr.append_scalar("q_arith_eval", ev.q_arith);
  tr.append_scalar("q_c_eval", ev.q_c);
  tr.append_scalar("q_l_eval", ev.q_l);
  tr.append_scalar("q_r_eval", ev.q_r);
  const Fr vch = tr.challenge_scalar("v_challenge");
  const Fr v_w = tr.challenge_scalar("v_w_challenge");
  tr.append_commitment("w_z_chall_comm", cm + 48 * PC_WZ);
  tr.append_commitment("w_z_chall_w_comm", cm + 48 * PC_WZW);
  const Fr u = tr.challenge_scalar("u_challenge");

  if (digest) tr.challenge_bytes("batch digest", digest, 32);

  const Fr one = Fr::one();
  const Fr z_n = z.pow_u64(v.n), z_h = z_n - one;
  Fr l1, pi_eval;
  if (!barycentric_core(v.n, v.n_inv, pi_root, v.pi_count, z, pi, z_h, &l1, &pi_eval)) { o.status = VS_REJECT; return; }
  const Fr a2 = alpha.sqr();
  const Fr perm = (ev.a + beta * ev.s1 + gamma) * (ev.b + beta * ev.s2 + gamma) * (ev.c + beta * ev.s3 + gamma);
  const Fr r0 = pi_eval - l1 * a2 - alpha * perm * (ev.d + gamma) * ev.z;
  // v^1 .. v^11, then v_w u, v_w^2 u, v_w^3 u  (proof.rs:330-353)
  Fr vc[14];
  vc[0] = vch;
#pragma unroll
  for (int i = 1; i < 11; ++i) vc[i] = vc[i - 1] * vch;
  vc[11] = v_w * u;
  vc[12] = vc[11] * v_w;
  vc[13] = vc[12] * v_w;
  const Fr e_evals[14] = {ev.a, ev.b, ev.c, ev.d, ev.s1, ev.s2, ev.s3, ev.q_arith, ev.q_c, ev.q_l, ev.q_r, ev.a_w, ev.b_w, ev.d_w};
  Fr e_scalar = u * ev.z - r0;
#pragma unroll
  for (int i = 0; i < 14; ++i) e_scalar = e_scalar + e_evals[i] * vc[i];

  // [D]: the widgets' linearisation terms (append_linearization_commitment_terms, proof.rs:808-889)
  const Fr qa = ev.q_arith;
  o.vk[P_QM] = ev.a * ev.b * qa;
  o.vk[P_QL] = ev.a * qa;
  o.vk[P_QR] = ev.b * qa;
  o.vk[P_QO] = ev.c * qa;
  o.vk[P_QF] = ev.d * qa;
  o.vk[P_QC] = qa;
  o.vk[P_QRANGE] = range_identity(range_ch, ev) * range_ch;
  o.vk[P_QLOGIC] = logic_identity(logic_ch, ev) * logic_ch;
  o.vk[P_QFIXED] = fixed_identity(fixed_ch, ev, v.edwards_d) * fixed_ch;
  o.vk[P_QVAR] = var_identity(var_ch, ev, v.edwards_d) * var_ch;
  // permutation (permutation/verifierkey.rs:46-104)
  const Fr x = (ev.a + beta * z + gamma) * (ev.b + beta * fr_small(7) * z + gamma) * (ev.c + beta * fr_small(13) * z + gamma) *
               (ev.d + beta * fr_small(17) * z + gamma) * alpha;
  o.comm[PC_Z] = x + l1 * a2 + u;
  o.vk[P_S4] = (perm * beta * ev.z * alpha).neg();
  const Fr nzh = z_h.neg();
  o.comm[PC_TLOW] = nzh;
  o.comm[PC_TMID] = z_n * nzh;
  o.comm[PC_THIGH] = z_n * z_n * nzh;
  o.comm[PC_TFOURTH] = z_n * z_n * z_n * nzh;
  // [F]: v^i on a, b, c, d, s1, s2, s3, q_arith, q_c, q_l, q_r; the shifted a, b, d add v_w^k u
  o.comm[PC_A] = vc[0] + vc[11];
  o.comm[PC_B] = vc[1] + vc[12];
  o.comm[PC_C] = vc[2];
  o.comm[PC_D] = vc[3] + vc[13];
  o.vk[P_S1] = vc[4];
  o.vk[P_S2] = vc[5];
  o.vk[P_S3] = vc[6];
  o.vk[P_QARITH] = o.vk[P_QARITH] + vc[7];
  o.vk[P_QC] = o.vk[P_QC] + vc[8];
  o.vk[P_QL] = o.vk[P_QL] + vc[9];
  o.vk[P_QR] = o.vk[P_QR] + vc[10];
  o.g = e_scalar.neg();
  o.comm[PC_WZ] = z;
  o.comm[PC_WZW] = u * z * v.omega;
  o.u = u;
}

// the replay's inputs from a VerifierCore: the constants of its circuit and its seeded transcript (label, version, VK)
static SlotConst slot_const(const VerifierCore& v, uint64_t pi_root_off) {
  SlotConst s;
  s.n = v.n;
  s.constraints = v.constraints;
  s.omega = v.omega;
  s.n_inv = v.n_inv;
  s.edwards_d = v.edwards_d;
  s.pi_count = v.pi_idx.size();
  s.pi_root_off = pi_root_off;
  return s;
}
static Transcript seeded_transcript(const VerifierCore& v) {   // transcript_for_version + seed_transcript (prover.rs:440)
  Transcript tr((const uint8_t*)v.label.data(), v.label.size());
  seed_transcript_vk(tr, v.constraints, v.vk, v.version);   // the prover's seeding (widgets.hpp)
  return tr;
}

// Proof::verify up to its MSM for plonk_verify's host threads: the shared replay from a freshly seeded transcript
static ProofScalars verify_scalars(const VerifierCore& v, const uint8_t proof[PROOF_BYTES], const Fr* pi) {
  ProofScalars o;
  Transcript tr = seeded_transcript(v);
  replay_scalars(slot_const(v, 0), v.pi_root.data(), tr, proof, pi, &o, nullptr);
  return o;
}

// the batch challenge rho (in the style of OpeningKey::batch_check's batch_challenge, key.rs:571-592): a transcript of
// its own over the sub-batch — its length, every proof's bytes and public inputs — so rho is fixed only after the batch is
static Fr batch_challenge(const uint8_t* proofs, const Fr* pi, uint64_t pi_count, const uint32_t* which, size_t m) {
  Transcript tr((const uint8_t*)"plonk-batch-verify-v1", 21);
  tr.append_u64("batch length", m);
  for (size_t i = 0; i < m; ++i) {
    tr.append_message("proof", proofs + PROOF_BYTES * which[i], PROOF_BYTES);
    for (uint64_t j = 0; j < pi_count; ++j) tr.append_scalar("pi", pi[which[i] * pi_count + j]);
  }
  return tr.challenge_scalar("rho");
}

static uint64_t be64_at(const uint8_t* p) {
  uint64_t x = 0;
  for (int i = 0; i < 8; ++i) x = (x << 8) | p[i];
  return x;
}
static uint64_t le64_at(const uint8_t* p) {
  uint64_t x = 0;
  for (int i = 7; i >= 0; --i) x = (x << 8) | p[i];
  return x;
}
static constexpr uint64_t VK_BLOB_BYTES = 20 * 48 + 8, OPENING_KEY_LEN = 48 + 96 + 96;
#define VFAIL(code, msg) return (set_last_error("plonk_verifier_from_bytes", msg, __FILE__, __LINE__), code)

// OpeningKey::from_bytes + try_new (key.rs:609-648) on the 240 bytes g || h || x_h: nullptr when valid, else what is wrong
// (shared by plonk_verifier_from_bytes and plonk_kzg_key_create)
static const char* opening_key_invalid(const uint8_t* p) {
  if ((p[0] & 0x40) || (p[48] & 0x40) || (p[144] & 0x40)) return "opening key: g, h and x_h must not be the identity";
  if (!g1_compressed_valid(p)) return "opening key: g is not a valid compressed G1 point";
  if (!g2_compressed_valid(p + 48)) return "opening key: h is not a valid compressed G2 point";
  if (!g2_compressed_valid(p + 144)) return "opening key: x_h is not a valid compressed G2 point";
  return nullptr;
}

// Verifier::try_from_bytes (verifier.rs:121-200) -> VerifierKey::from_slice (widget.rs:113-134), OpeningKey::from_slice
// (key.rs:596-648), Verifier::new
static int parse_verifier_blob(const uint8_t* blob, uint64_t len, VerifierCore* core, uint8_t g48[48], uint8_t h96[96],
                        uint8_t xh96[96]) {
  if (len < 48) VFAIL(PLONK_ERR_BYTES, "shorter than the six length fields");
  const uint64_t label_len = be64_at(blob), vk_len = be64_at(blob + 8), ok_len = be64_at(blob + 16), pi_len = be64_at(blob + 24);
  const uint64_t size = be64_at(blob + 32), constraints = be64_at(blob + 40);
  uint64_t pi_bytes, req;
  if (__builtin_mul_overflow(pi_len, (uint64_t)8, &pi_bytes) || __builtin_add_overflow(label_len, vk_len, &req) ||
      __builtin_add_overflow(req, ok_len, &req) || __builtin_add_overflow(req, pi_bytes, &req))
    VFAIL(PLONK_ERR_BYTES, "length fields overflow");
  if (len - 48 < req) VFAIL(PLONK_ERR_BYTES, "blob shorter than its length fields");
  const uint8_t* p = blob + 48;
  core->label.assign((const char*)p, label_len);
  p += label_len;
  if (vk_len < VK_BLOB_BYTES) VFAIL(PLONK_ERR_BYTES, "verifier key length");
  const uint64_t vk_n = le64_at(p);
  for (int j = 0; j < 15; ++j) {
    if (!g1_compressed_valid(p + 8 + 48 * j)) VFAIL(PLONK_ERR_DATA, "verifier key commitment is not a valid compressed G1 point");
    memcpy(core->vk[VK_BLOB_ORDER[j]], p + 8 + 48 * j, 48);
  }
  p += vk_len;
  if (ok_len < OPENING_KEY_LEN) VFAIL(PLONK_ERR_BYTES, "opening key length");
  if (const char* why = opening_key_invalid(p)) VFAIL(PLONK_ERR_DATA, why);
  memcpy(g48, p, 48);
  memcpy(h96, p + 48, 96);
  memcpy(xh96, p + 144, 96);
  p += ok_len;
  // Verifier::new: EvaluationDomain::new(size) (a power of two up to 2^32); the transcript is seeded with vk.n and
  // constraints, which every compiled circuit has equal (serial_check.hpp refuses a prover blob where they differ)
  if (size == 0 || size > (1ull << 32) || (size & (size - 1))) VFAIL(PLONK_ERR_DATA, "domain size is not a power of two <= 2^32");
  if (vk_n != constraints) VFAIL(PLONK_ERR_DATA, "verifier_key.n != constraints");
  if (constraints > size) VFAIL(PLONK_ERR_DATA, "more constraints than the domain holds");
  core->pi_idx.resize(pi_len);
  for (uint64_t i = 0; i < pi_len; ++i) {
    core->pi_idx[i] = be64_at(p + 8 * i);
    if (core->pi_idx[i] >= size) VFAIL(PLONK_ERR_DATA, "public input index beyond the domain");
  }
  core->n = size;
  core->constraints = constraints;
  core->init_constants();
  return PLONK_OK;
}
#undef VFAIL

// ---- mixed batches (plonk_verify_mixed) ---------------------------------------------------------------------------------
// The verifier digest: everything a circuit's check depends on besides the proof — its label, transcript version, domain
// size, constraints, the 15 VK commitments (VerifierKey::to_bytes order), the 240-byte opening key and the public-input
// indexes.
static void verifier_digest(const VerifierCore& v, const uint8_t opening_key[OPENING_KEY_LEN], uint8_t out[32]) {
  const char* dom = "plonk-verifier-digest-v1";
  Transcript tr((const uint8_t*)dom, cstr_len(dom));
  tr.append_message("label", (const uint8_t*)v.label.data(), v.label.size());
  tr.append_u64("version", (uint64_t)v.version);
  tr.append_u64("size", v.n);
  tr.append_u64("constraints", v.constraints);
  for (int j = 0; j < 15; ++j) tr.append_commitment("vk", v.vk[VK_BLOB_ORDER[j]]);
  tr.append_message("opening key", opening_key, OPENING_KEY_LEN);
  tr.append_u64("public inputs", v.pi_idx.size());
  for (uint64_t idx : v.pi_idx) tr.append_u64("public input index", idx);
  tr.challenge_bytes("circuit digest", out, 32);
}

// rho of a mixed (sub-)batch: its length, every verifier slot it uses (ascending) with that slot's verifier digest, then
// every proof's slot and proof digest.  used: the slots, ascending; slot_digest: 32 bytes per slot; circuit / proof_digest:
// per proof of the call; which: the m proofs of the sub-batch.
static Fr mixed_batch_challenge(const uint32_t* used, size_t nused, const uint8_t* slot_digest, const uint32_t* circuit,
                                const uint8_t* proof_digest, const uint32_t* which, size_t m) {
  const char* dom = "plonk-batch-verify-mixed-v1";
  Transcript tr((const uint8_t*)dom, cstr_len(dom));
  tr.append_u64("batch length", m);
  for (size_t i = 0; i < nused; ++i) {
    tr.append_u64("slot", used[i]);
    tr.append_message("circuit", slot_digest + 32ull * used[i], 32);
  }
  for (size_t i = 0; i < m; ++i) {
    tr.append_u64("circuit", circuit[which[i]]);
    tr.append_message("proof", proof_digest + 32ull * which[i], 32);
  }
  return tr.challenge_scalar("rho");
}

}  // namespace plonk
