// CPU test harness of the host half of the KZG10 opening checks: kzg_core.hpp (the batch challenge, the 3K + 1 terms, the
// flatten scalars, the challenge of plonk_srs_check) compiled with g++ and driven from tests/test_kzg_host.py through ctypes.
// hk_batch_check is a whole OpeningKey::batch_check with a NAIVE host MSM in place of the device's (verify.hip msm_run).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonk_amd/csrc/g1codec.cuh"
#include "../../plonk_amd/csrc/hostpairing.hpp"
#include "../../plonk_amd/csrc/verify_core.hpp"
#include "../../plonk_amd/csrc/kzg_core.hpp"

namespace plonk {
void set_last_error(const char*, const char*, const char*, int) {}
}
using namespace plonk;

static bool g1_from48(const uint8_t* in, G1Aff64* out) {
  G1Affine a;
  const int rc = g1_decompress48(in, &a);
  memset(out, 0, sizeof *out);
  if (rc == G1DEC_IDENTITY) { out->inf = true; return true; }
  if (rc != G1DEC_OK) return false;
  memcpy(out->x.l, a.x.l, 48);
  memcpy(out->y.l, a.y.l, 48);
  return true;
}
static H1 mul_add(H1 acc, const G1Aff64& p, const uint32_t k[8]) {   // acc + [k] p, k canonical
  if (p.inf) return acc;
  H1 P, r;
  P.X = p.x; P.Y = p.y; P.ZZ = to64(Fp::one()); P.ZZZ = P.ZZ;
  memset(&r, 0, sizeof r);
  for (int b = 255; b >= 0; --b) {
    r = h1_dbl(r);
    if ((k[b >> 5] >> (b & 31)) & 1) r = h1_add(r, P);
  }
  return h1_add(acc, r);
}
static G1Aff64 to_aff(const H1& h) {
  G1Aff64 a;
  memset(&a, 0, sizeof a);
  if (h.inf()) { a.inf = true; return a; }
  const Fp64 inv = fp64_inv(fp64_mul(h.ZZ, h.ZZZ));
  a.x = fp64_mul(h.X, fp64_mul(inv, h.ZZZ));
  a.y = fp64_mul(h.Y, fp64_mul(inv, h.ZZ));
  return a;
}
static bool load_points(const uint64_t* limbs, uint64_t count, std::vector<Fr>* out) {
  out->resize(count);
  bool ok = true;
  for (uint64_t k = 0; k < count; ++k) ok &= kzg_fr_load(limbs + 4 * k, &(*out)[k]);
  return ok;
}

extern "C" {

uint64_t hk_proof_size(void) { return sizeof(plonk_kzg_proof); }

// u of a batch (Montgomery limbs); 0, or PLONK_ERR_DATA for a non-canonical point
int hk_batch_challenge(const uint8_t* label, uint64_t label_len, const uint64_t* points, const plonk_kzg_proof* proofs, uint64_t count,
                       uint64_t* u_out) {
  std::vector<Fr> z;
  if (!load_points(points, count, &z)) return PLONK_ERR_DATA;
  const Fr u = kzg_batch_challenge(label, label_len, z.data(), proofs, count);
  memcpy(u_out, u.l, 32);
  return 0;
}
// the 3K + 1 terms: sc (8 canonical words each) and ids
int hk_batch_terms(const uint64_t* u, const uint64_t* points, const plonk_kzg_proof* proofs, uint64_t count, uint32_t* sc, uint32_t* ids) {
  std::vector<Fr> z;
  Fr uu;
  if (!load_points(points, count, &z) || !kzg_fr_load(u, &uu)) return PLONK_ERR_DATA;
  kzg_batch_terms(uu, z.data(), proofs, count, sc, ids);
  return 0;
}
// OpeningKey::batch_check through the host core: 0, PLONK_ERR_VERIFY, PLONK_ERR_POINT or PLONK_ERR_DATA
int hk_batch_check(const uint8_t* opening_key, const uint64_t* points, const plonk_kzg_proof* proofs, uint64_t count,
                   const uint8_t* label, uint64_t label_len, const uint64_t* u_override) {
  if (!count) return PLONK_ERR_VERIFY;
  std::vector<Fr> z;
  Fr u = Fr::one(), tmp;
  bool canon = load_points(points, count, &z) && (!u_override || kzg_fr_load(u_override, &u));
  for (uint64_t k = 0; k < count; ++k) canon &= kzg_fr_load(proofs[k].evaluation, &tmp);
  if (!canon) return PLONK_ERR_DATA;
  std::vector<G1Aff64> pts(1 + 2 * count);
  if (!g1_from48(opening_key, &pts[0])) return PLONK_ERR_POINT;
  for (uint64_t k = 0; k < count; ++k)
    if (!g1_compressed_valid(proofs[k].commitment) || !g1_from48(proofs[k].commitment, &pts[1 + 2 * k]) ||
        !g1_compressed_valid(proofs[k].witness) || !g1_from48(proofs[k].witness, &pts[2 + 2 * k]))
      return PLONK_ERR_POINT;
  if (!u_override) u = kzg_batch_challenge(label, label_len, z.data(), proofs, count);
  std::vector<uint32_t> sc(8 * (3 * count + 1)), ids(3 * count + 1);
  kzg_batch_terms(u, z.data(), proofs, count, sc.data(), ids.data());
  H1 L, R;
  memset(&L, 0, sizeof L);
  memset(&R, 0, sizeof R);
  for (uint64_t t = 0; t < count; ++t) L = mul_add(L, pts[ids[t]], sc.data() + 8 * t);
  for (uint64_t t = count; t < 3 * count + 1; ++t) R = mul_add(R, pts[ids[t]], sc.data() + 8 * t);
  G1Aff64 pr[2] = {to_aff(L), to_aff(R)};
  if (!pr[0].inf) { Fp64 zero; memset(&zero, 0, sizeof zero); pr[0].y = fp64_sub(zero, pr[0].y); }
  const G2Prepared h = g2_prepare(g2_decode_valid(opening_key + 48)), xh = g2_prepare(g2_decode_valid(opening_key + 144));
  const G2Prepared* qs[2] = {&xh, &h};
  return f12_is_one(final_exponentiation(multi_miller_loop(pr, qs, 2))) ? PLONK_OK : PLONK_ERR_VERIFY;
}
// AggregateProof::flatten's scalar side: sc[i] = v^i (canonical words), *e_out = sum v^i e_i (Montgomery limbs)
int hk_flatten_scalars(const uint64_t* v, const uint64_t* evals, uint64_t count, uint32_t* sc, uint64_t* e_out) {
  std::vector<Fr> ev;
  Fr vv;
  if (!load_points(evals, count, &ev) || !kzg_fr_load(v, &vv)) return PLONK_ERR_DATA;
  const Fr e = kzg_flatten_scalars(vv, ev.data(), count, sc);
  memcpy(e_out, e.l, 32);
  return 0;
}
void hk_srs_challenge(const uint8_t* seed32, uint64_t npoints, const uint8_t* opening_key, uint64_t* r_out) {
  const Fr r = kzg_srs_challenge(seed32, npoints, opening_key);
  memcpy(r_out, r.l, 32);
}
int hk_opening_key_valid(const uint8_t* opening_key) { return opening_key_invalid(opening_key) == nullptr; }
}
