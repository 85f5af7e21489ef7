// CPU test harness of the device pairing: plonk_amd/csrc/pairing28.cuh (the code pairing.hip runs in one lane per check)
// compiled with g++ next to hostpairing.hpp and compared with it bit for bit, driven from tests/test_pairing28_host.py
// through ctypes.
#include <cstdint>
#include <cstring>

#include "../../plonk_amd/csrc/g1codec.cuh"
#include "../../plonk_amd/csrc/pairing28.cuh"

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
static void put_f12(const F12& f, uint64_t* out) {   // as tests/csrc/host_verify.cpp
  const F2* c = &f.c0.c0;
  for (int i = 0; i < 6; ++i) {
    const Fp64 a = fp64_canon(c[i].a), b = fp64_canon(c[i].b);
    memcpy(out + 12 * i, a.l, 48);
    memcpy(out + 12 * i + 6, b.l, 48);
  }
}
// the affine point as an XYZZ point with ZZ = lam^2, ZZZ = lam^3 (so that the lane's normalisation has work to do)
static G1 xyzz_of(const G1Aff64& p, uint64_t lam) {
  if (p.inf) return G1::identity();
  const Fp l = Fp::from_u64(lam), l2 = l * l, l3 = l2 * l;
  G1 r;
  r.X = from64(p.x) * l2;
  r.Y = from64(p.y) * l3;
  r.ZZ = l2;
  r.ZZZ = l3;
  return r;
}
static uint64_t rng_state;
static uint32_t rng28() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) & Fp28::MASK;
}
static Fp28 rand_p28(uint32_t top_bound) {   // normalised, top limb below top_bound
  Fp28 r;
  for (int i = 0; i < Fp28::N; ++i) r.l[i] = rng28();
  r.l[Fp28::N - 1] %= top_bound;
  return r;
}
// a coordinate of the operand classes of tests/arith_vectors.py (tower_coords): one in four is 0, 1, p (zero in its upper
// representative), 1 + p, 2p - 1 or p - 1 with every low limb saturated below p's top limb; the others random below p
static Fp28 rand_coord() {
  Fp28 p, r;
  for (int i = 0; i < Fp28::N; ++i) p.l[i] = Fp28::mod(i);
  const uint32_t pick = rng28() & 31;
  switch (pick) {
    case 0: return Fp28::zero();
    case 1: return Fp28::one();
    case 2: return p;
    case 3: return Fp28::add(Fp28::one(), p);
    case 4: r = Fp28::add(p, p); r.l[0] -= 1; return r;                          // 2p's low limb is not zero
    case 5: for (int i = 0; i < Fp28::N - 1; ++i) r.l[i] = Fp28::MASK; r.l[Fp28::N - 1] = Fp28::mod(Fp28::N - 1) - 1; return r;
    case 6: r = p; r.l[0] -= 1; return r;
    case 7: return Fp28::add(rand_p28(Fp28::mod(Fp28::N - 1)), p);               // a random residue in its upper representative
    default: return rand_p28(Fp28::mod(Fp28::N - 1));
  }
}
static void rand_f12r(F12r* x) {
  F2r* c = &x->c0.c0;
  for (int i = 0; i < 6; ++i) c[i] = F2r{rand_coord(), rand_coord()};
}

extern "C" {
// e(-A, x_h) e(B, h) after the final exponentiation, by pairing28.cuh (out_dev) and by hostpairing.hpp (out_host), 72 words
// each.  Returns bit 0: pairing28's is_one, bit 1: the host's; negative on bad input.
int hp_pairing2(const uint8_t* a48, const uint8_t* b48, const uint8_t* xh96, const uint8_t* h96, uint64_t* out_dev,
                uint64_t* out_host) {
  G1Aff64 ps[2];
  if (!g1_from48(a48, &ps[0]) || !g1_from48(b48, &ps[1])) return -2;
  if (!g2_compressed_valid(xh96) || !g2_compressed_valid(h96)) return -3;
  const G2Prepared xh = g2_prepare(g2_decode_valid(xh96)), h = g2_prepare(g2_decode_valid(h96));
  static PairingTables28 T;
  if (!pairing_tables_fill(xh, h, &T)) return -4;
  F12r v;
  pairing_check_value_28(&v, &T, xyzz_of(ps[0], 7), xyzz_of(ps[1], 11));
  f12r_put(&v, out_dev);
  int rc = f12r_is_one(&v) ? 1 : 0;
  if (!ps[0].inf) {
    Fp64 z;
    memset(&z, 0, sizeof z);
    ps[0].y = fp64_sub(z, ps[0].y);
  }
  const G2Prepared* qs[2] = {&xh, &h};
  const F12 e = final_exponentiation(multi_miller_loop(ps, qs, 2));
  put_f12(e, out_host);
  if (f12_is_one(e)) rc |= 2;
  return rc;
}
// f12r_inv(x) * x == 1 on `rounds` random x: the number of failures
int hp_f12_inv_check(uint64_t seed, int rounds) {
  rng_state = seed;
  int bad = 0;
  for (int i = 0; i < rounds; ++i) {
    F12r x, y;
    rand_f12r(&x);
    f12r_inv(&y, &x);
    f12r_mul(&y, &y, &x);
    if (!f12r_is_one(&y)) ++bad;
  }
  return bad;
}
static bool f12r_same(const F12r* x, const F12r* y) {
  uint64_t a[72], b[72];
  f12r_put(x, a);
  f12r_put(y, b);
  return memcmp(a, b, sizeof a) == 0;
}
// the specialised routines against the generic f12r_mul on random inputs: f12r_sqr on any x, the sparse line product on a
// random line and point, the cyclotomic squaring on an element of the cyclotomic subgroup (x^((p^6 - 1)(p^2 + 1))): failures
int hp_special_check(uint64_t seed, int rounds, const uint8_t* xh96, const uint8_t* h96) {
  rng_state = seed;
  const G2Prepared xh = g2_prepare(g2_decode_valid(xh96)), h = g2_prepare(g2_decode_valid(h96));
  static PairingTables28 T;
  if (!pairing_tables_fill(xh, h, &T)) return -4;
  int bad = 0;
  for (int i = 0; i < rounds; ++i) {
    F12r x, a, b;
    rand_f12r(&x);
    f12r_sqr(&a, &x);
    f12r_mul(&b, &x, &x);
    if (!f12r_same(&a, &b)) ++bad;
    const Line28 l = {F2r{rand_p28(Fp28::mod(Fp28::N - 1)), rand_p28(Fp28::mod(Fp28::N - 1))},
                      F2r{rand_p28(Fp28::mod(Fp28::N - 1)), rand_p28(Fp28::mod(Fp28::N - 1))},
                      F2r{rand_p28(Fp28::mod(Fp28::N - 1)), rand_p28(Fp28::mod(Fp28::N - 1))}};
    const Fp28 px = rand_p28(Fp28::mod(Fp28::N - 1)), py = rand_p28(Fp28::mod(Fp28::N - 1));
    a = x;
    b = x;
    f12r_mul_line(&a, &l, &px, &py);
    f12r_mul_line_generic(&b, &l, &px, &py);
    if (!f12r_same(&a, &b)) ++bad;
    F12r m, t;
    f12r_conj(&t, &x);
    f12r_inv(&m, &x);
    f12r_mul(&m, &t, &m);
    f12r_frob(&t, &m, 2, &T);
    f12r_mul(&m, &t, &m);
    f12r_cyc_sqr(&a, &m);
    f12r_mul(&b, &m, &m);
    if (!f12r_same(&a, &b)) ++bad;
    f12r_cyc_sqr(&m, &m);   // in place
    if (!f12r_same(&m, &b)) ++bad;
  }
  return bad;
}
// p28_red on random normalised values below 64p: the same residue, below 2p, normalised: the number of failures
int hp_red_check(uint64_t seed, int rounds) {
  rng_state = seed;
  int bad = 0;
  for (int i = 0; i < rounds; ++i) {
    const Fp28 v = rand_p28(i & 1 ? 64 * Fp28::mod(Fp28::N - 1) : 6 * Fp28::mod(Fp28::N - 1));
    const Fp28 r = p28_red(v), rc = r.canon(), vc = v.canon();
    bool ok = r.l[Fp28::N - 1] <= 2 * Fp28::mod(Fp28::N - 1) + 1;
    for (int k = 0; k < Fp28::N; ++k) ok = ok && rc.l[k] == vc.l[k] && (k == Fp28::N - 1 || r.l[k] <= Fp28::MASK);
    if (!ok) ++bad;
  }
  return bad;
}
// the tables of (x_h, h) converted back to the host's form equal the prepared points and the Frobenius constants: 1 / 0
int hp_tables_roundtrip(const uint8_t* xh96, const uint8_t* h96) {
  const G2Prepared xh = g2_prepare(g2_decode_valid(xh96)), h = g2_prepare(g2_decode_valid(h96));
  static PairingTables28 T;
  if (!pairing_tables_fill(xh, h, &T)) return -4;
  const G2Prepared* src[2] = {&xh, &h};
  const Line28* got[2] = {T.xh, T.h};
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < PAIRING_LINES; ++i) {
      const LineCoeffs& l = src[s]->lines[i];
      if (!f2_eq(f2_of_f2r(got[s][i].c0), l.c0) || !f2_eq(f2_of_f2r(got[s][i].c1), l.c1) || !f2_eq(f2_of_f2r(got[s][i].c2), l.c2))
        return 0;
    }
  const FrobConsts& fc = frob_consts();
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 6; ++j)
      if (!f2_eq(f2_of_f2r(T.frob[k][j]), fc.g[k][j])) return 0;
  return (int)sizeof(PairingTables28);
}
}
