// CPU test harness of the host half of proof verification: hostpairing.hpp (the pairing) and verify_core.hpp (blob parser,
// barycentric evaluation, the per-proof scalars) compiled with g++ and driven from tests/test_verify_host.py through ctypes.
// hv_verify is a whole single-proof verification with a NAIVE host MSM in place of the device's (verify.hip).
#include <cstdint>
#include <cstring>

#include "../../plonk_amd/csrc/g1codec.cuh"
#include "../../plonk_amd/csrc/hostpairing.hpp"
#include "../../plonk_amd/csrc/verify_core.hpp"

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
static void put_f12(const F12& f, uint64_t* out) {   // 12 canonical Fp values, tower order
  const F2* c = &f.c0.c0;
  for (int i = 0; i < 6; ++i) {
    const Fp64 a = fp64_canon(c[i].a), b = fp64_canon(c[i].b);
    memcpy(out + 12 * i, a.l, 48);
    memcpy(out + 12 * i + 6, b.l, 48);
  }
}

extern "C" {
// prod_i e(P_i, Q_i)  (n pairs: n x 48 compressed G1, n x 96 compressed G2, both validated by the caller)
int hv_multi_pairing(int n, const uint8_t* g1s, const uint8_t* g2s, uint64_t* out72) {
  G1Aff64 ps[8];
  G2Prepared qs[8];
  const G2Prepared* qp[8];
  if (n < 1 || n > 8) return -1;
  for (int i = 0; i < n; ++i) {
    if (!g1_from48(g1s + 48 * i, &ps[i])) return -2;
    if (!g2_compressed_valid(g2s + 96 * i)) return -3;
    qs[i] = g2_prepare(g2_decode_valid(g2s + 96 * i));
    qp[i] = &qs[i];
  }
  put_f12(final_exponentiation(multi_miller_loop(ps, qp, n)), out72);
  return 0;
}
// f^(p^k) of the result of a pairing, and whether it is one (for the order / Frobenius checks)
int hv_pairing_pow_q_is_one(const uint8_t* g1, const uint8_t* g2) {
  G1Aff64 p;
  if (!g1_from48(g1, &p)) return -2;
  const F12 e = pairing(p, g2_prepare(g2_decode_valid(g2)));
  F12 acc = f12_one();   // e^q by square-and-multiply over the bits of q
  for (int b = 254; b >= 0; --b) {
    acc = f12_sqr(acc);
    if ((FrP::MOD[b >> 5] >> (b & 31)) & 1) acc = f12_mul(acc, e);
  }
  return f12_is_one(acc) ? 1 : 0;
}
// compute_lagrange_and_barycentric_evaluations: returns 1 and (l1, pi_eval) in Montgomery form, or 0 (rejected)
int hv_barycentric(uint64_t n, uint64_t pi_count, const uint64_t* pi_idx, const uint32_t* pi_mont, const uint32_t* z_mont,
                   uint32_t* l1_out, uint32_t* pi_out) {
  VerifierCore v;
  v.n = n;
  v.pi_idx.assign(pi_idx, pi_idx + pi_count);
  v.init_constants();
  Fr z;
  memcpy(z.l, z_mont, 32);
  std::vector<Fr> pi(pi_count);
  memcpy(pi.data(), pi_mont, 32 * pi_count);
  const Fr z_h = z.pow_u64(n) - Fr::one();
  Fr l1, pe;
  if (!barycentric_eval(v, z, pi.data(), z_h, &l1, &pe)) return 0;
  memcpy(l1_out, l1.l, 32);
  memcpy(pi_out, pe.l, 32);
  return 1;
}

// Verifier::try_from_bytes: PLONK_OK or the error code of plonk_verifier_from_bytes
int hv_parse(const uint8_t* blob, uint64_t len) {
  VerifierCore v;
  uint8_t g[48], h[96], xh[96];
  return parse_verifier_blob(blob, len, &v, g, h, xh);
}
// one proof: 0, PLONK_ERR_VERIFY, PLONK_ERR_DATA or PLONK_ERR_POINT (the verdict plonk_verify gives), or the parser's error
int hv_verify(const uint8_t* blob, uint64_t len, int version, const uint8_t* proof, const uint32_t* pi_mont) {
  VerifierCore v;
  uint8_t g48[48], h96[96], xh96[96];
  const int rc = parse_verifier_blob(blob, len, &v, g48, h96, xh96);
  if (rc) return rc;
  v.version = version;
  G1Aff64 pts[P_COUNT + 1 + PC_COUNT];   // VK (PolyId), g, the proof's commitments
  for (int j = 0; j < P_COUNT; ++j) g1_from48(v.vk[j], &pts[j]);
  g1_from48(g48, &pts[P_COUNT]);
  for (int c = 0; c < PC_COUNT; ++c)
    if (!g1_compressed_valid(proof + 48 * c) || !g1_from48(proof + 48 * c, &pts[P_COUNT + 1 + c])) return PLONK_ERR_POINT;
  const ProofScalars s = verify_scalars(v, proof, (const Fr*)pi_mont);
  if (s.status == VS_DATA) return PLONK_ERR_DATA;
  if (s.status != VS_OK) return PLONK_ERR_VERIFY;
  // naive MSM: double-and-add per term over the canonical scalar bits
  auto mul_add = [](H1 acc, const G1Aff64& p, const Fr& k_mont) {
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
  };
  H1 L, R;
  memset(&L, 0, sizeof L);
  memset(&R, 0, sizeof R);
  L = mul_add(L, pts[P_COUNT + 1 + PC_WZ], Fr::one());
  L = mul_add(L, pts[P_COUNT + 1 + PC_WZW], s.u);
  for (int j = 0; j < P_COUNT; ++j) R = mul_add(R, pts[j], s.vk[j]);
  R = mul_add(R, pts[P_COUNT], s.g);
  for (int c = 0; c < PC_COUNT; ++c) R = mul_add(R, pts[P_COUNT + 1 + c], s.comm[c]);
  G1Aff64 pr[2];
  const H1* hs[2] = {&L, &R};
  for (int i = 0; i < 2; ++i) {
    memset(&pr[i], 0, sizeof pr[i]);
    if (hs[i]->inf()) { pr[i].inf = true; continue; }
    const Fp64 inv = fp64_inv(fp64_mul(hs[i]->ZZ, hs[i]->ZZZ));
    pr[i].x = fp64_mul(hs[i]->X, fp64_mul(inv, hs[i]->ZZZ));
    pr[i].y = fp64_mul(hs[i]->Y, fp64_mul(inv, hs[i]->ZZ));
  }
  if (!pr[0].inf) { Fp64 z; memset(&z, 0, sizeof z); pr[0].y = fp64_sub(z, pr[0].y); }
  const G2Prepared h = g2_prepare(g2_decode_valid(h96)), xh = g2_prepare(g2_decode_valid(xh96));
  const G2Prepared* qs[2] = {&xh, &h};
  return f12_is_one(final_exponentiation(multi_miller_loop(pr, qs, 2))) ? PLONK_OK : PLONK_ERR_VERIFY;
}
}
