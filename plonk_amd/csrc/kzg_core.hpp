// KZG10 opening checks: the scalar side of OpeningKey::batch_check and AggregateProof::flatten (reference
// src/commitment_scheme/kzg10/key.rs:571-591, 661-707; proof.rs:69-109) and the challenge of plonk_srs_check.  Like
// verify_core.hpp everything is __host__ __device__ in place (the HD convention of field.cuh): kzg.hip runs it on the host,
// tests/csrc/host_kzg.cpp compiles it with g++ against the plain-Python restatement tests/kzg_ref.py.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/plonk_hip.h"
#include "transcript.hpp"

namespace plonk {

static constexpr uint64_t KZG_MAX_OPEN = 65536;          // polynomials per plonk_kzg_open
static constexpr uint64_t KZG_MAX_BATCH = 1ull << 24;    // openings per plonk_kzg_batch_check

// Montgomery limbs of the ABI -> Fr; false when the limbs are not a canonical residue (>= q)
HD bool kzg_fr_load(const uint64_t limbs[4], Fr* out) {
  memcpy(out->l, limbs, 32);
  for (int i = 7; i >= 0; --i) {
    if (out->l[i] < FrP::MOD[i]) return true;
    if (out->l[i] > FrP::MOD[i]) return false;
  }
  return false;   // == q
}

// coefficients (4 limbs each) up to the last non-zero one: Polynomial::from_coefficients_vec's trim on the host
HD uint64_t host_trimmed(const uint64_t* p, uint64_t len) {
  while (len && !(p[4 * len - 4] | p[4 * len - 3] | p[4 * len - 2] | p[4 * len - 1])) --len;
  return len;
}

// batch_challenge (key.rs:571-591) on a fresh Transcript::new(label)
HD Fr kzg_batch_challenge(const uint8_t* label, size_t label_len, const Fr* points, const plonk_kzg_proof* proofs, uint64_t count) {
  Transcript tr(label, label_len);
  tr.append_message("dom-sep", (const uint8_t*)"kzg10-batch-check-v1", 20);
  tr.append_u64("batch-len", count);
  for (uint64_t k = 0; k < count; ++k) {
    Fr e;
    memcpy(e.l, proofs[k].evaluation, 32);
    tr.append_scalar("batch-point", points[k]);
    tr.append_commitment("batch-polynomial-commitment", proofs[k].commitment);
    tr.append_scalar("batch-evaluation", e);
    tr.append_commitment("batch-witness-commitment", proofs[k].witness);
  }
  return tr.challenge_scalar("batch-challenge");
}

// r of plonk_srs_check: bound to the caller's seed, the number of points and the opening key under test
HD Fr kzg_srs_challenge(const uint8_t seed32[32], uint64_t npoints, const uint8_t opening_key[240]) {
  const char* dom = "plonk-srs-check-v1";
  Transcript tr((const uint8_t*)dom, cstr_len(dom));
  tr.append_message("seed", seed32, 32);
  tr.append_u64("points", npoints);
  tr.append_message("opening key", opening_key, 240);
  return tr.challenge_scalar("r");
}

HD void kzg_put_canonical(uint32_t* dst, const Fr& s_mont) {
  const Fr s = s_mont.from_mont();
  for (int w = 0; w < 8; ++w) dst[w] = s.l[w];
}

// The 3K + 1 terms of batch_check over the point table [g | C_0 W_0 | C_1 W_1 | ...] (g = 0, C_k = 1 + 2k, W_k = 2 + 2k):
//   total_w: terms [0, K)            u^k        W_k
//   total_c: terms [K, 2K)           u^k        C_k
//                  [2K, 3K)          u^k z_k    W_k
//                  3K                -(sum_k u^k v_k)  g
// sc: canonical scalars, 8 words per term; ids: point index per term.  The powers of u are the running product the
// reference's util::powers_of builds; the g scalar is accumulated and negated once, as key.rs:679-692 does.
HD void kzg_batch_terms(const Fr& u, const Fr* points, const plonk_kzg_proof* proofs, uint64_t K, uint32_t* sc, uint32_t* ids) {
  Fr w = Fr::one(), g = Fr::zero();
  for (uint64_t k = 0; k < K; ++k) {
    Fr e;
    memcpy(e.l, proofs[k].evaluation, 32);
    kzg_put_canonical(sc + 8 * k, w);
    ids[k] = (uint32_t)(2 + 2 * k);
    kzg_put_canonical(sc + 8 * (K + k), w);
    ids[K + k] = (uint32_t)(1 + 2 * k);
    kzg_put_canonical(sc + 8 * (2 * K + k), w * points[k]);
    ids[2 * K + k] = (uint32_t)(2 + 2 * k);
    g = g + w * e;
    w = w * u;
  }
  kzg_put_canonical(sc + 8 * (3 * K), g.neg());
  ids[3 * K] = 0;
}

// AggregateProof::flatten's scalars: sc[i] = v^i (canonical, 8 words each) and the flattened evaluation sum_i v^i e_i
HD Fr kzg_flatten_scalars(const Fr& v, const Fr* evals, uint64_t count, uint32_t* sc) {
  Fr w = Fr::one(), acc = Fr::zero();
  for (uint64_t i = 0; i < count; ++i) {
    kzg_put_canonical(sc + 8 * i, w);
    acc = acc + w * evals[i];
    w = w * v;
  }
  return acc;
}

}  // namespace plonk
