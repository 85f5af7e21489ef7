// Host-side shim exposing the product's __host__ __device__ field/curve code
// (plonk_amd/csrc/field.cuh, curve.cuh, ...) to ctypes so it can be checked bit for
// bit against the big-int oracle on a CPU-only box.  Test code only.
// The pure arithmetic bodies live in arith_cases.hpp, shared with the device twin (dev_arith.hip): the h_* entry points
// below pack their arguments into a case record and run the same body; h_case_<family> runs a whole array of records.
#include <cstring>
#include "arith_cases.hpp"
using namespace plonk;
using namespace arith;

#define HOST_FAMILY(name, In, Out)                                                                          \
  extern "C" int h_case_##name(const void* in, size_t in_bytes, void* out, size_t out_bytes, int n) {     \
    if (n < 0 || in_bytes != (size_t)n * sizeof(In) || out_bytes != (size_t)n * sizeof(Out)) return -1;    \
    for (int i = 0; i < n; ++i) {   /* through aligned copies: the caller's buffers are byte strings */    \
      In r;                                                                                                 \
      Out o;                                                                                                \
      memcpy(&r, (const char*)in + (size_t)i * sizeof(In), sizeof(In));                                     \
      case_##name(r, o);                                                                                    \
      memcpy((char*)out + (size_t)i * sizeof(Out), &o, sizeof(Out));                                        \
    }                                                                                                       \
    return 0;                                                                                               \
  }                                                                                                         \
  extern "C" int h_record_size_##name(int which) { return (int)(which ? sizeof(Out) : sizeof(In)); }
ARITH_FAMILIES(HOST_FAMILY)

// The shared buffer of the families that read PairingTables28: blob = the compressed x_h || h (2 x 96 bytes), prepared
// and converted once by the product's pairing_tables_fill.  0, or a negative code for a blob that is not two G2 points.
extern "C" int h_shared_tables(const void* blob, size_t bytes) {
  static PairingTables28 T;
  static uint8_t have[192];
  static bool filled = false;
  if (bytes != sizeof have) return -1;
  if (filled && memcmp(have, blob, sizeof have) == 0) return 0;
  const uint8_t* b = (const uint8_t*)blob;
  if (!g2_compressed_valid(b) || !g2_compressed_valid(b + 96)) return -3;
  if (!pairing_tables_fill(g2_prepare(g2_decode_valid(b)), g2_prepare(g2_decode_valid(b + 96)), &T)) return -4;
  memcpy(have, blob, sizeof have);
  filled = true;
  arith::h_pairing_tables = &T;
  return 0;
}

static void fr_op(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  FrIn in{}; in.op = op;
  if (a) memcpy(in.a, a, 32);
  if (b) memcpy(in.b, b, 32);
  FrOut out; case_fr(in, out); memcpy(o, out.r, 32);
}
static void fp_op(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  FpIn in{}; in.op = op;
  if (a) memcpy(in.a, a, 48);
  if (b) memcpy(in.b, b, 48);
  FpOut out; case_fp(in, out); memcpy(o, out.r, 48);
}
// points: affine 96 B (x||y Montgomery); result affine 96 B + return 1, or 0 for identity
static int g1_op(uint32_t op, const uint8_t* a, const uint8_t* b, uint32_t k, uint8_t* o) {
  G1In in{}; in.op = op; in.k = k;
  if (a) memcpy(in.a, a, 96);
  if (b) memcpy(in.b, b, 96);
  G1Out out; case_g1(in, out); memcpy(o, out.p, 96);
  return (int)out.rc;
}
extern "C" {
void h_fr_mul(const uint32_t* a, const uint32_t* b, uint32_t* o) { fr_op(FR_MUL, a, b, o); }
void h_fr_add(const uint32_t* a, const uint32_t* b, uint32_t* o) { fr_op(FR_ADD, a, b, o); }
void h_fr_sub(const uint32_t* a, const uint32_t* b, uint32_t* o) { fr_op(FR_SUB, a, b, o); }
void h_fr_inv(const uint32_t* a, uint32_t* o) { fr_op(FR_INV, a, nullptr, o); }
void h_fr_from_mont(const uint32_t* a, uint32_t* o) { fr_op(FR_FROM_MONT, a, nullptr, o); }
void h_fr_consts(uint32_t* o) { fr_op(FR_GENERATOR, nullptr, nullptr, o); fr_op(FR_ROOT, nullptr, nullptr, o + 8); fr_op(FR_ONE, nullptr, nullptr, o + 16); }
void h_fp_mul(const uint32_t* a, const uint32_t* b, uint32_t* o) { fp_op(FP_MUL, a, b, o); }
void h_fp_add(const uint32_t* a, const uint32_t* b, uint32_t* o) { fp_op(FP_ADD, a, b, o); }
void h_fp_sub(const uint32_t* a, const uint32_t* b, uint32_t* o) { fp_op(FP_SUB, a, b, o); }
void h_fp_inv(const uint32_t* a, uint32_t* o) { fp_op(FP_INV, a, nullptr, o); }
int h_g1_add_aff(const uint8_t* a, const uint8_t* b, uint8_t* o) { return g1_op(G1_ADD_AFF, a, b, 0, o); }
int h_g1_add_full(const uint8_t* a, const uint8_t* b, uint8_t* o) {
  G1FullIn in; memcpy(in.a, a, 96); memcpy(in.b, b, 96);
  G1FullOut out; case_g1_full(in, out); memcpy(o, out.p, 96);
  return (int)out.rc;
}
int h_g1_mul_u32(const uint8_t* a, uint32_t k, uint8_t* o) { return g1_op(G1_MUL_U32, a, nullptr, k, o); }
int h_g1_neg_add(const uint8_t* a, uint8_t* o) { return g1_op(G1_NEG_ADD, a, nullptr, 0, o); }
}
// ---- reduced-radix Fp (fp28.cuh) ----
// inputs/outputs in the 12 x 32-bit R = 2^384 form; computation done in Fp28
static uint32_t fp28_op(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  Fp28In in{}; in.op = op;
  memcpy(in.a, a, 48);
  if (b) memcpy(in.b, b, 48);
  Fp28Out out; case_fp28(in, out);
  if (o) memcpy(o, out.r, 48);
  return out.flags;
}
extern "C" {
void h_fp28_mul(const uint32_t* a, const uint32_t* b, uint32_t* o) { fp28_op(FP28_MUL, a, b, o); }
void h_fp28_chain(const uint32_t* a, const uint32_t* b, uint32_t* o) { fp28_op(FP28_CHAIN, a, b, o); }
int h_fp28_zero_test(const uint32_t* a) { return (int)fp28_op(FP28_ZERO_TEST, a, nullptr, nullptr); }
void h_fp28_roundtrip(const uint32_t* a, uint32_t* o) { fp28_op(FP28_ROUNDTRIP, a, nullptr, o); }
}
static void fp28_raw_op(uint32_t op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* o) {
  Fp28RawIn in{}; in.op = op;
  memcpy(in.a, a, 56); memcpy(in.b, b, 56);
  if (c) memcpy(in.c, c, 56);
  if (d) memcpy(in.d, d, 56);
  Fp28RawOut out; case_fp28_raw(in, out); memcpy(o, out.r, 56);
}
// raw-limb access (14 x u32, possibly lazy): op 0 = mul(a,b), 1 = a.sqr(), 2 = mul2(a,b,c,d)
extern "C" void h_fp28_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* o) {
  fp28_raw_op(op == 0 ? RAW_MUL : op == 1 ? RAW_SQR : RAW_MUL2, a, b, c, d, o);
}
// lazy helpers on normalised inputs: op 0 = sub_lazy<32>(a,b), 1 = neg_lazy<16>(b), 2 = add_lazy(a,b)
extern "C" void h_fp28_lazy(int op, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  fp28_raw_op(op == 0 ? RAW_SUB_LAZY32 : op == 1 ? RAW_NEG_LAZY16 : RAW_ADD_LAZY, a, b, nullptr, nullptr, o);
}

// ---- XYZZ over Fp28 (curve28.cuh) ----
// n <= G1R_MAX_POINTS points, 96 B each in the 32-bit form; -1 when n is out of range
static int g1r_op(uint32_t op, const uint8_t* pts, const uint8_t* neg, int n, uint32_t k, uint8_t* o, int* used_pair) {
  if (n < 0 || n > G1R_MAX_POINTS) return -1;
  G1rIn in{}; in.op = op; in.n = (uint32_t)n; in.k = k;
  memcpy(in.pts, pts, 96 * (size_t)n);
  if (neg) memcpy(in.neg, neg, (size_t)n);
  G1rOut out; case_g1r(in, out); memcpy(o, out.p, 96);
  if (used_pair) *used_pair = (int)out.used_pair;
  return (int)out.rc;
}
extern "C" {
// sum_{i<n} (neg[i] ? -P_i : P_i) with mixed additions
int h_g1r_accumulate(const uint8_t* pts, const uint8_t* neg, int n, uint8_t* o) { return g1r_op(G1R_ACCUMULATE, pts, neg, n, 0, o, nullptr); }
// (sum of first half) + (sum of second half) via the full addition; then * k
int h_g1r_tree(const uint8_t* pts, int n, uint32_t k, uint8_t* o) { return g1r_op(G1R_TREE, pts, nullptr, n, k, o, nullptr); }
// The accumulation lanes' first step (msm.hip ACC_FIRST_PAIR); *used_pair = 1 when the pair formula ran.
int h_g1r_accumulate_pair_first(const uint8_t* pts, const uint8_t* neg, int n, uint8_t* o, int* used_pair) {
  return g1r_op(G1R_PAIR_FIRST, pts, neg, n, 0, o, used_pair);
}
int h_g1r_affine_roundtrip(const uint8_t* pt, uint8_t* o) { return g1r_op(G1R_AFFINE_ROUNDTRIP, pt, nullptr, 1, 0, o, nullptr); }
// [k] P through the endomorphism (curve28.cuh g1r_mul_glv); k: 8 x 32-bit limbs, canonical; pre = doublings applied to P first
int h_g1r_mul_glv(const uint8_t* pt, const uint32_t* k, int pre, uint8_t* o) {
  GlvIn in{}; in.op = GLV_MUL; in.pre = (uint32_t)pre;
  memcpy(in.k, k, 32); memcpy(in.pt, pt, 96);
  GlvOut out; case_glv(in, out); memcpy(o, out.p, 96);
  return (int)out.rc;
}
void h_glv_split(const uint32_t* k, uint64_t* out4) {
  GlvIn in{}; in.op = GLV_SPLIT;
  memcpy(in.k, k, 32);
  GlvOut out; case_glv(in, out);
  for (int i = 0; i < 4; ++i) out4[i] = (uint64_t)out.split[2 * i] | ((uint64_t)out.split[2 * i + 1] << 32);
}
}
// ---- reduced-radix Fr (fr29.cuh) ----
static void fr29_op(uint32_t op, uint32_t stages, const uint32_t* a, const uint32_t* b, const uint32_t* w, uint32_t* o0, uint32_t* o1) {
  Fr29In in{}; in.op = op; in.stages = stages;
  memcpy(in.a, a, 32); memcpy(in.b, b, 32);
  if (w) memcpy(in.w, w, 32);
  Fr29Out out; case_fr29(in, out);
  memcpy(o0, out.o0, 32);
  if (o1) memcpy(o1, out.o1, 32);
}
extern "C" {
// DIF butterfly on Montgomery (R = 2^256) inputs: out0 = a + b, out1 = (a - b) * w
void h_fr29_butterfly(const uint32_t* a, const uint32_t* b, const uint32_t* w, uint32_t* o0, uint32_t* o1) { fr29_op(FR29_BUTTERFLY, 0, a, b, w, o0, o1); }
// chained stages on a vector of 2 elements: exercises the lazy ranges (sum path and product path)
void h_fr29_chain(const uint32_t* a, const uint32_t* b, const uint32_t* w, int stages, uint32_t* o0, uint32_t* o1) { fr29_op(FR29_CHAIN, (uint32_t)stages, a, b, w, o0, o1); }
void h_fr29_mul2(const uint32_t* a, const uint32_t* w1, const uint32_t* w2, uint32_t* o) { fr29_op(FR29_MUL2, 0, a, w1, w2, o, nullptr); }   // a * (w1 * w2)
void h_fr29_sub_reduce(const uint32_t* a, const uint32_t* b, uint32_t* o) { fr29_op(FR29_SUB_REDUCE, 0, a, b, nullptr, o, nullptr); }
}

// ---- host transcript (transcript.hpp): Merlin's published test protocol ----
extern "C" void h_merlin_simple(uint8_t out[32]) {
  MerlinIn in{}; MerlinOut o; case_merlin(in, o); memcpy(out, o.challenge, 32);
}

// ---- widgets.hpp: lowest 7 coefficients of the quotient from the lowest 7 of every polynomial ----
#include "../../plonk_amd/csrc/widgets.hpp"
// key_low: 15 x 7 Fr (PolyId order), has: 11 flags, low: a b c d z pi (6 x 7 Fr),
// ch: alpha beta gamma range logic fixed var edwards_d omega n_inv (10 Fr); out: 7 Fr.  All Montgomery limbs.
extern "C" void h_quotient_low(const uint32_t* key_low, const uint8_t* has, const uint32_t* low, const uint32_t* ch, uint32_t* out) {
  using namespace plonk;
  Fr kl[P_COUNT][7];
  memcpy(kl, key_low, sizeof kl);
  bool hs[WQS_COUNT];
  for (int i = 0; i < WQS_COUNT; ++i) hs[i] = has[i] != 0;
  Fr lows[42], c[10], o[7];
  memcpy(lows, low, sizeof lows);
  memcpy(c, ch, sizeof c);
  QuotientLowIn in;
  in.low = lows;
  in.alpha = c[0]; in.beta = c[1]; in.gamma = c[2]; in.range_ch = c[3]; in.logic_ch = c[4]; in.fixed_ch = c[5];
  in.var_ch = c[6]; in.edwards_d = c[7]; in.omega = c[8]; in.n_inv = c[9];
  quotient_low(kl, hs, in, o);
  memcpy(out, o, sizeof o);
}

// ---- hostg1.hpp: MSM finishing (Horner over the 16 bit sums), group normalisation, compression ----
#include "../../plonk_amd/csrc/hostg1.hpp"
// pts: 16 affine points (96 B raw each; a point with x = y = 0 stands for the identity) -> XYZZ bit sums
// -> finish_bit_sums -> batch affine -> 48-byte compressed.  out48: the commitment.
// rb row bit sums, 7 column bit sums, C_128, and (bitpos != 0) S: the result is 2 W - S (bit-position entries weigh 2 b + 1)
extern "C" void h_finish_bit_sums(const uint8_t* pts96, int rb, int bitpos, uint8_t out48[48]) {
  using namespace plonk;
  G1 bits[MSM_ROWBITS_MAX + 9];
  bits[rb + 8] = G1::identity();
  for (int k = 0; k < rb + 8 + (bitpos ? 1 : 0); ++k) {
    G1Affine a;
    memcpy(&a, pts96 + 96 * k, 96);
    bits[k] = (a.x.is_zero() && a.y.is_zero()) ? G1::identity() : G1::from_affine(a);
    if (k & 1) bits[k] = bits[k].dbl().add(bits[k].neg());   // a non-trivial ZZ: 2P - P
  }
  const G1 w = finish_bit_sums(bits, rb, bitpos != 0);
  uint8_t aff[1][97];
  batch_xyzz_to_affine97(&w, 1, aff);
  g1_compress97(aff[0], out48);
}
// count <= 16 XYZZ points given as affine (made projective with odd scalings) -> compressed encodings
extern "C" void h_batch_compress(const uint8_t* pts96, int count, uint8_t* out48) {
  using namespace plonk;
  G1 p[16];
  for (int k = 0; k < count; ++k) {
    G1Affine a;
    memcpy(&a, pts96 + 96 * k, 96);
    if (a.x.is_zero() && a.y.is_zero()) { p[k] = G1::identity(); continue; }
    p[k] = G1::from_affine(a);
    for (int j = 0; j < k % 3; ++j) p[k] = p[k].dbl().add(p[k].neg()).add(G1::identity());
  }
  uint8_t aff[16][97];
  batch_xyzz_to_affine97(p, count, aff);
  for (int k = 0; k < count; ++k) g1_compress97(aff[k], out48 + 48 * k);
}

// sum of `n` points (affine in, made projective with odd scalings) with the 64-bit-limb additions of a sharded proof's
// partial-sum step (h1_sum_strided) -> compressed
extern "C" void h_sum_strided(const uint8_t* pts96, int n, uint8_t out48[48]) {
  using namespace plonk;
  G1 p[64];
  for (int k = 0; k < n; ++k) {
    G1Affine a;
    memcpy(&a, pts96 + 96 * k, 96);
    if (a.x.is_zero() && a.y.is_zero()) { p[k] = G1::identity(); continue; }
    p[k] = G1::from_affine(a);
    for (int j = 0; j < k % 3; ++j) p[k] = p[k].dbl().add(p[k].neg());
  }
  const G1 w = h1_sum_strided(reinterpret_cast<const uint8_t*>(p), sizeof(G1), n);
  uint8_t aff[1][97];
  batch_xyzz_to_affine97(&w, 1, aff);
  g1_compress97(aff[0], out48);
}
// ---- finish_pool.hpp: the host helper threads of fetch_commitments ----
#include "../../plonk_amd/csrc/finish_pool.hpp"
namespace {
struct PoolProbe { std::atomic<int> hits[16]; std::atomic<long> sum; int spin; };
void pool_probe_task(void* arg, int i) {
  PoolProbe* pp = (PoolProbe*)arg;
  volatile unsigned x = 1;
  for (int k = 0; k < pp->spin; ++k) x = x * 1664525u + 1013904223u;   // a few hundred ns .. a few us of work
  pp->hits[i].fetch_add(1);
  pp->sum.fetch_add(i + 1);
}
}
// `rounds` jobs of 0..16 tasks with every arming pattern fetch_commitments can produce (armed + run, armed + withdrawn,
// late arming, jobs back to back): returns 0 when every task of every job ran exactly once and run() returned only after
// the last one; workers == 0 is the inline path.
extern "C" int h_finish_pool_selftest(int workers, int rounds) {
  using namespace plonk;
  FinishPool pool(workers);
  if (pool.workers() > (workers < 0 ? 0 : (workers > 7 ? 7 : workers))) return -1;   // (fewer only if the process is out of threads)
  unsigned lcg = 12345u + (unsigned)workers;
  for (int r = 0; r < rounds; ++r) {
    lcg = lcg * 1664525u + 1013904223u;
    const int count = (int)((lcg >> 8) % 17);
    const int pattern = (int)((lcg >> 16) % 4);
    PoolProbe probe;
    for (auto& h : probe.hits) h.store(0);
    probe.sum.store(0);
    probe.spin = (int)((lcg >> 20) % 2000);
    if (pattern == 1) { Armed withdrawn(workers > 0 ? &pool : nullptr); }   // armed, nothing to do (an early return)
    {
      Armed a(pattern == 2 ? nullptr : (workers > 0 ? &pool : nullptr));     // pattern 2: the inline path of a one-commitment group
      if (pattern == 3) std::this_thread::sleep_for(std::chrono::microseconds(200));   // workers awake and spinning before the job
      a.run(pool_probe_task, &probe, count);
    }
    long want = 0;
    for (int i = 0; i < 16; ++i) {
      if (probe.hits[i].load() != (i < count ? 1 : 0)) return 100 + r;
      if (i < count) want += i + 1;
    }
    if (probe.sum.load() != want) return 200 + r;
  }
  return 0;
}

// ---- permutation.hpp: copy constraints -> sigma mappings (Permutation::compute_sigma_permutations) ----
#include "../../plonk_amd/csrc/permutation.hpp"
extern "C" int h_sigma_mappings(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint64_t constraints,
                                uint64_t n, uint64_t witnesses, uint32_t* out) {
  const uint32_t* wires[4] = {a, b, c, d};
  return plonk::sigma_mappings(wires, constraints, n, witnesses, out) ? 0 : -1;
}

// G1Affine::from_bytes on a 48-byte compressed encoding (g1codec.cuh): returns the decoder's code, out = x || y (96 B, Montgomery)
extern "C" int h_g1_decompress48(const uint8_t* in, uint8_t* out96) {
  DecompressIn r; memcpy(r.enc, in, 48);
  DecompressOut o; case_decompress(r, o); memcpy(out96, o.p, 96);
  return (int)o.rc;
}

// ---- msm_recode.cuh: scalar -> (row, bucket, sign) digits of both recodings ----
// canonical scalar (8 x u32) -> out[4 j .. 4 j + 3] = slot, row, bucket, sign; returns the number of digits.
// bitpos: 0 windows, 1 width-17 NAF, 2 the same from the strided LDS-parked form, 21 width-21 NAF, 120 / 116 even positions
extern "C" int h_msm_recode(const uint32_t* scalar, int bitpos, uint32_t* out) {
  RecodeIn r; r.mode = (uint32_t)bitpos; memcpy(r.s, scalar, 32);
  RecodeOut o; case_recode(r, o);
  memcpy(out, o.d, 16 * (o.n < (uint32_t)MSM_DIGITS ? o.n : (uint32_t)MSM_DIGITS));
  return (int)o.n;
}

// ---- fp_safegcd.cuh: Bernstein-Yang inversion against Fermat (fp28_inv) and the oracle ----
static void safegcd_op(uint32_t op, const uint32_t* a, uint32_t* o, size_t bytes) {
  SafegcdIn in{}; in.op = op; memcpy(in.a, a, bytes);
  SafegcdOut out; case_safegcd(in, out); memcpy(o, out.r, bytes);
}
// a: Fp (12 x u32, R = 2^384 Montgomery) -> o: its inverse in the same form, through Fp28 and the safegcd inverse
extern "C" void h_fp_inv_gcd(const uint32_t* a, uint32_t* o) { safegcd_op(GCD_FP28, a, o, 48); }
// same input scaled lazily (value 5x + 3x = 8x as unreduced limbs < 64p): the inverse of 8x
extern "C" void h_fp_inv_gcd_lazy(const uint32_t* a, uint32_t* o) { safegcd_op(GCD_FP28_LAZY, a, o, 48); }
// Fr: a (8 x u32, R = 2^256 Montgomery) -> its inverse in the same form, through twiddle form and the safegcd inverse
extern "C" void h_fr_inv_gcd(const uint32_t* a, uint32_t* o) { safegcd_op(GCD_FR29_TW, a, o, 32); }
// the composer's out-of-line inversion (composer_core.hpp cg_inv)
extern "C" void h_cg_inv(const uint32_t* a, uint32_t* o) { safegcd_op(GCD_CG_INV, a, o, 32); }

// ---- hostg2.hpp: validity of a compressed G2 encoding (OpeningKey::from_slice's test of h and x_h) ----
#include "../../plonk_amd/csrc/hostg2.hpp"
extern "C" int h_g2_compressed_valid(const uint8_t in[96]) { return plonk::g2_compressed_valid(in) ? 1 : 0; }
extern "C" int h_g1_compressed_valid(const uint8_t in[48]) { return plonk::g1_compressed_valid(in) ? 1 : 0; }

// ---- hostg1.hpp: the host-side Fp inverse (Montgomery in, Montgomery out): safegcd (mode 0) and the Fermat chain (mode 1) ----
extern "C" void h_fp64_inv(const uint8_t in[48], int fermat, uint8_t out[48]) {
  plonk::Fp64 a;
  memcpy(a.l, in, 48);
  const plonk::Fp64 r = fermat ? plonk::fp64_inv_fermat(a) : plonk::fp64_inv(a);
  memcpy(out, r.l, 48);
}
// the Montgomery-in / Montgomery-out Fr inverse the host driver uses per proof (fp_safegcd.cuh fr_inv_gcd)
extern "C" void h_fr_inv_gcd_mont(const uint32_t* a, uint32_t* o) { safegcd_op(GCD_FR_MONT, a, o, 32); }

// ---- api_guard.hpp: the exception barrier every int-returning C-ABI entry point runs inside ----
#include <cstdio>
#include <stdexcept>
#include "../../plonk_amd/csrc/api_guard.hpp"
static char g_guard_msg[256];
namespace plonk {
void set_last_error(const char* what, const char* detail, const char*, int) { snprintf(g_guard_msg, sizeof g_guard_msg, "%s -> %s", what, detail); }
}
// kind 0: the body's own return value; 1: std::bad_alloc; 2: std::runtime_error; 3: a non-std exception
extern "C" int h_api_guard(int kind, char msg_out[256]) {
  g_guard_msg[0] = 0;
  const int rc = plonk::api_guard("h_api_guard", [&]() -> int {
    if (kind == 1) throw std::bad_alloc();
    if (kind == 2) throw std::runtime_error("boom");
    if (kind == 3) throw 42;
    return 7;
  });
  memcpy(msg_out, g_guard_msg, 256);
  return rc;
}

// ---- tools/ubench/coop_mul.hpp: the 16-lane cooperative Montgomery product, lanes emulated with arrays ----
#include "../../tools/ubench/coop_mul.hpp"
namespace {
struct HostLanes {   // a value per lane of one 16-lane DPP row; shifts fill with zero like row_shr / row_shl with bound_ctrl
  struct u32 { uint32_t v[16]; };
  struct u64 { uint64_t v[16]; };
  static u64 zero64() { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = 0; return r; }
  static u64 mad(const u64& acc, uint32_t uni, const u32& lane) { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = acc.v[k] + (uint64_t)uni * lane.v[k]; return r; }
  template <int S> static u32 shr32(const u32& x) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = k - S >= 0 ? x.v[k - S] : 0; return r; }
  template <int S> static u32 shl32(const u32& x) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = k + S <= 15 ? x.v[k + S] : 0; return r; }
  template <int S> static u64 shr64(const u64& x) { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = k - S >= 0 ? x.v[k - S] : 0; return r; }
  template <int S> static u64 shl64(const u64& x) { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = k + S <= 15 ? x.v[k + S] : 0; return r; }
  static u32 lane_lt(int n) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = k < n ? 0xffffffffu : 0u; return r; }
  static u32 lane_eq(int n) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = k == n ? 0xffffffffu : 0u; return r; }
  static u64 select64(const u32& m, const u64& a, const u64& b) { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = m.v[k] ? a.v[k] : b.v[k]; return r; }
  static u32 and32(const u32& a, uint32_t c) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = a.v[k] & c; return r; }
  static u32 and32(const u32& a, const u32& b) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = a.v[k] & b.v[k]; return r; }
  static u32 add32(const u32& a, const u32& b) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = a.v[k] + b.v[k]; return r; }
  static u64 add64(const u64& a, const u64& b) { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = a.v[k] + b.v[k]; return r; }
  static u32 lo32(const u64& a) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = (uint32_t)a.v[k]; return r; }
  static u64 widen(const u32& a) { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = a.v[k]; return r; }
  static u64 shr64_bits(const u64& a, int s) { u64 r; for (int k = 0; k < 16; ++k) r.v[k] = a.v[k] >> s; return r; }
  static u32 nonzero32(const u32& a) { u32 r; for (int k = 0; k < 16; ++k) r.v[k] = a.v[k] ? 0xffffffffu : 0u; return r; }
};
}  // namespace
// a: 14 uniform limbs, b: 14 limbs (lane j holds limb j) -> the 16 lanes of the result (lanes 14, 15 must come out zero)
extern "C" void h_coop_mul(const uint32_t a[14], const uint32_t b[14], uint32_t out[16]) {
  HostLanes::u32 bd;
  for (int k = 0; k < 16; ++k) bd.v[k] = k < 14 ? b[k] : 0;
  coop::Uniform au;
  for (int k = 0; k < 14; ++k) au.l[k] = a[k];
  const HostLanes::u32 r = coop::Mul<HostLanes>::mul(au, bd);
  for (int k = 0; k < 16; ++k) out[k] = r.v[k];
}
