// CPU test harness of plonk_verify_mixed's shared host / device code: verify_core.hpp's replay driven the way the replay
// kernel of verify.hip drives it (from a per-circuit SlotConst POD, a pre-seeded transcript copied as bytes and a
// concatenated pi_root array), the verifier digest, the mixed batch challenge rho, and a whole mixed fold with a NAIVE
// host MSM in place of the device's.  Built with g++ and driven from tests/test_verify_mixed_host.py through ctypes.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonk_amd/csrc/g1codec.cuh"
#include "../../plonk_amd/csrc/hostpairing.hpp"
#include "../../plonk_amd/csrc/verify_core.hpp"

namespace plonk {
void set_last_error(const char*, const char*, const char*, int) {}
}
using namespace plonk;

namespace {

struct Circuit {   // one parsed verifier blob and the kernel-shaped inputs of its replay
  VerifierCore core;
  uint8_t g48[48], h96[96], xh96[96], ok[OPENING_KEY_LEN];
  SlotConst slot;
  std::vector<uint8_t> seeded;   // the pre-seeded transcript as the device receives it: bytes
  int parse(const uint8_t* blob, uint64_t len, int version, std::vector<Fr>* roots) {
    const int rc = parse_verifier_blob(blob, len, &core, g48, h96, xh96);
    if (rc) return rc;
    core.version = version;
    memcpy(ok, g48, 48);
    memcpy(ok + 48, h96, 96);
    memcpy(ok + 144, xh96, 96);
    slot = slot_const(core, roots->size());
    roots->insert(roots->end(), core.pi_root.begin(), core.pi_root.end());
    const Transcript tr = seeded_transcript(core);
    seeded.assign((const uint8_t*)&tr, (const uint8_t*)&tr + sizeof tr);
    return PLONK_OK;
  }
  void replay(const std::vector<Fr>& roots, const uint8_t* proof, const Fr* pi, ProofScalars* o, uint8_t digest[32]) const {
    alignas(Transcript) uint8_t buf[sizeof(Transcript)];
    memcpy(buf, seeded.data(), sizeof buf);
    replay_scalars(slot, roots.data() + slot.pi_root_off, *(Transcript*)buf, proof, pi, o, digest);
  }
};

void put_scalars(const ProofScalars& s, uint32_t* out) {   // vk[15], g, comm[11], u: 28 x 8 words, Montgomery
  memcpy(out, s.vk, 32 * P_COUNT);
  memcpy(out + 8 * 15, s.g.l, 32);
  memcpy(out + 8 * 16, s.comm, 32 * PC_COUNT);
  memcpy(out + 8 * 27, s.u.l, 32);
}

bool g1_from48(const uint8_t* in, G1Aff64* out) {
  G1Affine a;
  const int rc = g1_decompress48(in, &a);
  memset(out, 0, sizeof *out);
  if (rc == G1DEC_IDENTITY) { out->inf = true; return true; }
  if (rc != G1DEC_OK) return false;
  memcpy(out->x.l, a.x.l, 48);
  memcpy(out->y.l, a.y.l, 48);
  return true;
}

H1 mul_add(H1 acc, const G1Aff64& p, const Fr& k_mont) {   // acc + [k] p by double-and-add over the canonical bits
  if (p.inf) return acc;
  const Fr k = k_mont.from_mont();
  H1 P, r;
  P.X = p.x; P.Y = p.y; P.ZZ = to64(Fp::one()); P.ZZZ = P.ZZ;
  memset(&r, 0, sizeof r);
  for (int b = 255; b >= 0; --b) {
    r = h1_dbl(r);
    if ((k.l[b >> 5] >> (b & 31)) & 1) r = h1_add(r, P);
  }
  return h1_add(acc, r);
}

G1Aff64 to_affine(const H1& h) {
  G1Aff64 a;
  memset(&a, 0, sizeof a);
  if (h.inf()) { a.inf = true; return a; }
  const Fp64 inv = fp64_inv(fp64_mul(h.ZZ, h.ZZZ));
  a.x = fp64_mul(h.X, fp64_mul(inv, h.ZZZ));
  a.y = fp64_mul(h.Y, fp64_mul(inv, h.ZZ));
  return a;
}

}  // namespace

extern "C" {
// one proof through both paths: the kernel-shaped replay (status, scalars, digest) and verify_scalars (status, scalars)
int hm_replay(const uint8_t* blob, uint64_t len, int version, const uint8_t* proof, const uint32_t* pi_mont,
              int32_t* status_core, uint32_t* sc_core, uint8_t* digest, int32_t* status_ref, uint32_t* sc_ref) {
  Circuit c;
  std::vector<Fr> roots(3, Fr::one());   // a non-zero offset into the concatenated roots, as for a later slot
  const int rc = c.parse(blob, len, version, &roots);
  if (rc) return rc;
  ProofScalars a;
  c.replay(roots, proof, (const Fr*)pi_mont, &a, digest);
  *status_core = a.status;
  put_scalars(a, sc_core);
  const ProofScalars b = verify_scalars(c.core, proof, (const Fr*)pi_mont);
  *status_ref = b.status;
  put_scalars(b, sc_ref);
  return 0;
}

int hm_verifier_digest(const uint8_t* blob, uint64_t len, int version, uint8_t* out32) {
  Circuit c;
  std::vector<Fr> roots;
  const int rc = c.parse(blob, len, version, &roots);
  if (rc) return rc;
  verifier_digest(c.core, c.ok, out32);
  return 0;
}

// rho of a sub-batch, canonical little-endian bytes
int hm_rho(const uint32_t* used, uint64_t nused, const uint8_t* slot_digest, const uint32_t* circuit, const uint8_t* proof_digest,
           const uint32_t* which, uint64_t m, uint8_t* out32) {
  fr_to_bytes(mixed_batch_challenge(used, nused, slot_digest, circuit, proof_digest, which, m), out32);
  return 0;
}

// A whole mixed check on the host: ncirc verifier blobs (concatenated; lens, versions), count proofs with their slots and
// their public inputs concatenated.  Replays every proof (kernel-shaped), draws rho over all slots used and all proofs,
// folds the checks with per-slot VK sums, one g sum and 11 commitment terms per proof (naive MSM), pairs once.
// 1 = accept, 0 = reject (also when a replay rejects), < 0 a parse / decode error.
int hm_fold(uint32_t ncirc, const uint8_t* blobs, const uint64_t* lens, const int32_t* versions, uint64_t count,
            const uint32_t* circuit, const uint8_t* proofs, const uint32_t* pi_mont) {
  std::vector<Circuit> cs(ncirc);
  std::vector<Fr> roots;
  std::vector<uint8_t> sd(32ull * ncirc);
  uint64_t off = 0;
  for (uint32_t s = 0; s < ncirc; ++s) {
    const int rc = cs[s].parse(blobs + off, lens[s], versions[s], &roots);
    if (rc) return rc;
    off += lens[s];
    verifier_digest(cs[s].core, cs[s].ok, sd.data() + 32ull * s);
  }
  std::vector<ProofScalars> ps(count);
  std::vector<uint8_t> pd(32 * count);
  std::vector<uint32_t> which(count);
  std::vector<bool> used(ncirc, false);
  const Fr* pi = (const Fr*)pi_mont;
  for (uint64_t k = 0; k < count; ++k) {
    const Circuit& c = cs[circuit[k]];
    c.replay(roots, proofs + PROOF_BYTES * k, pi, &ps[k], pd.data() + 32 * k);
    pi += c.core.pi_idx.size();
    if (ps[k].status != VS_OK) return 0;
    which[k] = (uint32_t)k;
    used[circuit[k]] = true;
  }
  std::vector<uint32_t> us;
  for (uint32_t s = 0; s < ncirc; ++s)
    if (used[s]) us.push_back(s);
  const Fr rho = count == 1 ? Fr::one() : mixed_batch_challenge(us.data(), us.size(), sd.data(), circuit, pd.data(), which.data(), count);
  std::vector<Fr> vk_sum(P_COUNT * ncirc, Fr::zero());
  Fr g_sum = Fr::zero(), w = Fr::one();
  H1 L, R;
  memset(&L, 0, sizeof L);
  memset(&R, 0, sizeof R);
  for (uint64_t k = 0; k < count; ++k) {
    const ProofScalars& p = ps[k];
    G1Aff64 cm[PC_COUNT];
    for (int c = 0; c < PC_COUNT; ++c)
      if (!g1_compressed_valid(proofs + PROOF_BYTES * k + 48 * c) || !g1_from48(proofs + PROOF_BYTES * k + 48 * c, &cm[c])) return -10;
    L = mul_add(L, cm[PC_WZ], w);
    L = mul_add(L, cm[PC_WZW], w * p.u);
    for (int c = 0; c < PC_COUNT; ++c) R = mul_add(R, cm[c], w * p.comm[c]);
    for (int j = 0; j < P_COUNT; ++j) vk_sum[P_COUNT * circuit[k] + j] = vk_sum[P_COUNT * circuit[k] + j] + w * p.vk[j];
    g_sum = g_sum + w * p.g;
    w = w * rho;
  }
  for (uint32_t s : us)
    for (int j = 0; j < P_COUNT; ++j) {
      G1Aff64 q;
      g1_from48(cs[s].core.vk[j], &q);
      R = mul_add(R, q, vk_sum[P_COUNT * s + j]);
    }
  G1Aff64 g;
  g1_from48(cs[us[0]].g48, &g);
  R = mul_add(R, g, g_sum);
  G1Aff64 pr[2] = {to_affine(L), to_affine(R)};
  if (!pr[0].inf) { Fp64 z; memset(&z, 0, sizeof z); pr[0].y = fp64_sub(z, pr[0].y); }
  const G2Prepared h = g2_prepare(g2_decode_valid(cs[us[0]].h96)), xh = g2_prepare(g2_decode_valid(cs[us[0]].xh96));
  const G2Prepared* qs[2] = {&xh, &h};
  return f12_is_one(final_exponentiation(multi_miller_loop(pr, qs, 2))) ? 1 : 0;
}
}
