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
// Included by verify.hip and by the CPU test harness.
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
    omega = fr_root_of_unity();
    for (uint32_t i = L; i < 32; ++i) omega = omega.sqr();
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

// compute_lagrange_and_barycentric_evaluations: false (Error::ProofVerificationError) when z = 1 or z is the root of a
// non-zero public input
static bool barycentric_eval(const VerifierCore& v, const Fr& z, const Fr* pi, const Fr& z_h, Fr* l1, Fr* pi_eval) {
  const Fr one = Fr::one();
  const size_t m = v.pi_root.size();
  std::vector<Fr> den(m + 1), pre(m + 1);
  den[0] = Fr::from_u64(v.n) * (z - one);
  std::vector<size_t> idx;
  Fr run = one;
  for (size_t i = 0; i <= m; ++i) {
    if (i) {
      if (pi[i - 1].is_zero()) continue;
      den[i] = v.pi_root[i - 1] * z - one;
    }
    if (den[i].is_zero()) return false;
    pre[i] = run;
    run = run * den[i];
    idx.push_back(i);
  }
  Fr inv = fr_inv_gcd(run), acc = Fr::zero();
  for (size_t j = idx.size(); j-- > 0;) {
    const size_t i = idx[j];
    const Fr di = inv * pre[i];
    inv = inv * den[i];
    if (i) acc = acc + di * pi[i - 1];
    else *l1 = z_h * di;
  }
  *pi_eval = acc * z_h * v.n_inv;
  return true;
}

static bool fr_from_canonical(const uint8_t b[32], Fr* out) {
  Fr x;
  memcpy(x.l, b, 32);
  for (int i = 7; i >= 0; --i)
    if (x.l[i] != FrP::MOD[i]) {
      if (x.l[i] > FrP::MOD[i]) return false;
      break;
    } else if (i == 0) {
      return false;   // == q
    }
  *out = x.to_mont();
  return true;
}

// Proof::verify up to its MSM (proof.rs:218-502).  pi: the verifier's public inputs in Montgomery form.
static ProofScalars verify_scalars(const VerifierCore& v, const uint8_t proof[PROOF_BYTES], const Fr* pi) {
  ProofScalars o;
  Evals ev;
  Fr* order[15] = {&ev.a, &ev.b, &ev.c, &ev.d, &ev.a_w, &ev.b_w, &ev.d_w, &ev.q_arith, &ev.q_c, &ev.q_l,
                   &ev.q_r, &ev.s1, &ev.s2, &ev.s3, &ev.z};
  for (int k = 0; k < 15; ++k)
    if (!fr_from_canonical(proof + PC_COUNT * 48 + 32 * k, order[k])) { o.status = VS_DATA; return o; }
  const uint8_t* cm = proof;   // 11 x 48 compressed commitments
  // transcript_for_version + the public inputs (prover.rs:440-442, proof.rs:231-245)
  Transcript tr((const uint8_t*)v.label.data(), v.label.size());
  seed_transcript_vk(tr, v.constraints, v.vk, v.version);   // the prover's seeding (widgets.hpp)
  for (size_t i = 0; i < v.pi_idx.size(); ++i) tr.append_scalar("pi", pi[i]);
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

  const Fr one = Fr::one();
  const Fr z_n = z.pow_u64(v.n), z_h = z_n - one;
  Fr l1, pi_eval;
  if (!barycentric_eval(v, z, pi, z_h, &l1, &pi_eval)) { o.status = VS_REJECT; return o; }
  const Fr a2 = alpha.sqr();
  const Fr perm = (ev.a + beta * ev.s1 + gamma) * (ev.b + beta * ev.s2 + gamma) * (ev.c + beta * ev.s3 + gamma);
  const Fr r0 = pi_eval - l1 * a2 - alpha * perm * (ev.d + gamma) * ev.z;
  // v^1 .. v^11, then v_w u, v_w^2 u, v_w^3 u  (proof.rs:330-353)
  Fr vc[14];
  vc[0] = vch;
  for (int i = 1; i < 11; ++i) vc[i] = vc[i - 1] * vch;
  vc[11] = v_w * u;
  vc[12] = vc[11] * v_w;
  vc[13] = vc[12] * v_w;
  const Fr e_evals[14] = {ev.a, ev.b, ev.c, ev.d, ev.s1, ev.s2, ev.s3, ev.q_arith, ev.q_c, ev.q_l, ev.q_r, ev.a_w, ev.b_w, ev.d_w};
  Fr e_scalar = u * ev.z - r0;
  for (int i = 0; i < 14; ++i) e_scalar = e_scalar + e_evals[i] * vc[i];

  for (int j = 0; j < P_COUNT; ++j) o.vk[j] = Fr::zero();
  for (int c = 0; c < PC_COUNT; ++c) o.comm[c] = Fr::zero();
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
  if ((p[0] & 0x40) || (p[48] & 0x40) || (p[144] & 0x40)) VFAIL(PLONK_ERR_DATA, "opening key: g, h and x_h must not be the identity");
  if (!g1_compressed_valid(p)) VFAIL(PLONK_ERR_DATA, "opening key: g is not a valid compressed G1 point");
  if (!g2_compressed_valid(p + 48)) VFAIL(PLONK_ERR_DATA, "opening key: h is not a valid compressed G2 point");
  if (!g2_compressed_valid(p + 144)) VFAIL(PLONK_ERR_DATA, "opening key: x_h is not a valid compressed G2 point");
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

}  // namespace plonk
