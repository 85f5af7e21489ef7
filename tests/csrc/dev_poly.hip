// extern "C" doors to the launchers of plonk_amd/csrc/poly.hip, one launcher (or one named chain) per door, for
// tests/test_gpu_poly_kernels.py.  No kernels here: the code that runs is libplonk_hip.so's own.  Every door takes the
// plonk_ctx* the Python binding holds (Context.handle), device pointers from Context.alloc and plain host arguments
// (field elements as 4 x u64 Montgomery limbs), queues on the context's stream, waits for that stream and returns the
// launcher's code (PLONK_ERR_*, negative) or, when the launcher was content, the HIP error of the wait (positive).
// Test code only.
#include "plonk_internal.hpp"
#include "poly.hpp"

using namespace plonk;

namespace {

int finish(Ctx& c, int rc) {
  const hipError_t e = hipStreamSynchronize(c.stream);
  if (rc) return rc;
  return (int)e;
}
struct BiCfg {   // the batch-inversion geometry of one call
  Ctx& c;
  int saved;
  BiCfg(Ctx& ctx, int cfg) : c(ctx), saved(ctx.cfg.bi_cfg) { c.cfg.bi_cfg = cfg; }
  ~BiCfg() { c.cfg.bi_cfg = saved; }
};

}  // namespace

#define DOOR(H) \
  Ctx& c = (H)->c; \
  std::lock_guard<std::mutex> lk(c.mu)

extern "C" {

int dp_batch_inverse(plonk_ctx* h, Fr* v, uint64_t n, int twiddle_form, int bi_cfg) {
  DOOR(h);
  BiCfg geometry(c, bi_cfg);
  return finish(c, poly_batch_inverse(&c, v, n, twiddle_form != 0));
}
int dp_scan_prefix_product(plonk_ctx* h, Fr* data, uint64_t n, Fr* totals) {
  DOOR(h);
  return finish(c, scan_prefix_product(&c, data, n, totals));
}
int dp_scan_prefix_product_local(plonk_ctx* h, Fr* data, uint64_t n, Fr* totals) {
  DOOR(h);
  return finish(c, scan_prefix_product_local(&c, data, n, totals));
}
int dp_scan_prefix_product_apply(plonk_ctx* h, Fr* data, uint64_t n, const Fr* totals, const Fr* carry_twiddle) {
  DOOR(h);
  return finish(c, scan_prefix_product_apply(&c, data, n, totals, *carry_twiddle));
}
uint32_t dp_scan_prefix_blocks(uint64_t n) { return scan_prefix_blocks(n); }
int dp_scan_suffix_sum(plonk_ctx* h, Fr* data, uint64_t n, Fr* totals) {
  DOOR(h);
  return finish(c, scan_suffix_sum(&c, data, n, totals));
}
// items k < count: polys[k], lens[k], xs[k]; a count above the 16 slots of EvalArgs is handed on as it is (refused)
int dp_poly_eval(plonk_ctx* h, const Fr* const* polys, const uint64_t* lens, const Fr* xs, int count, uint64_t max_len,
                 Fr* partial, uint32_t max_blocks, Fr* out_dev) {
  DOOR(h);
  EvalArgs a;
  for (int k = 0; k < count && k < 16; ++k) {
    a.items[k].poly = polys[k];
    a.items[k].len = lens[k];
    a.items[k].x = xs[k];
  }
  a.partial = partial;
  a.max_blocks = max_blocks;
  return finish(c, poly_eval(&c, a, count, max_len, out_dev));
}
int dp_poly_lincomb(plonk_ctx* h, const Fr* const* polys, const uint64_t* lens, const Fr* scalars, int count, uint64_t len,
                    const Fr* constant, Fr* out) {
  DOOR(h);
  if (count < 0 || count > 24) return PLONK_ERR_ARG;
  LinCombArgs a;
  for (int k = 0; k < count; ++k) {
    a.t[k].p = polys[k];
    a.t[k].len = lens[k];
    a.t[k].s = scalars[k];
  }
  a.count = count;
  a.len = len;
  a.constant = *constant;
  a.out = out;
  return finish(c, poly_lincomb(&c, a));
}
int dp_poly_ruffini(plonk_ctx* h, const Fr* src, Fr* dst, uint64_t len, const Fr* z, const Fr* zinv, Fr* scratch, Fr* totals) {
  DOOR(h);
  return finish(c, poly_ruffini(&c, src, dst, len, *z, *zinv, scratch, totals));
}
int dp_poly_ruffini_local(plonk_ctx* h, const Fr* src, uint64_t lo, uint64_t len, const Fr* z, Fr* scratch, Fr* totals) {
  DOOR(h);
  return finish(c, poly_ruffini_local(&c, src, lo, len, *z, scratch, totals));
}
int dp_poly_ruffini_finish(plonk_ctx* h, const Fr* scratch, Fr* dst, uint64_t lo, uint64_t len, const Fr* zinv, const Fr* carry,
                           uint64_t last) {
  DOOR(h);
  return finish(c, poly_ruffini_finish(&c, scratch, dst, lo, len, *zinv, *carry, last));
}
int dp_poly_mul_arrays(plonk_ctx* h, Fr* a, const Fr* b, uint64_t n, int* zero_flag_dev) {
  DOOR(h);
  return finish(c, poly_mul_arrays(&c, a, b, n, zero_flag_dev));
}
int dp_poly_trimmed_len(plonk_ctx* h, const Fr* p, uint64_t n, unsigned long long* out_dev) {
  DOOR(h);
  return finish(c, poly_trimmed_len(&c, p, n, out_dev));
}
int dp_poly_split_t(plonk_ctx* h, Fr* t, uint64_t n, uint64_t np, Fr* out, const Fr* b3, uint64_t len4) {
  DOOR(h);
  SplitArgs a;
  for (int k = 0; k < 3; ++k) a.b[k] = b3[k];
  a.len4 = len4;
  return finish(c, poly_split_t(&c, t, n, np, out, a));
}
int dp_poly_fold(plonk_ctx* h, const Fr* src, Fr* dst, uint64_t n, uint32_t extra, const Fr* cn) {
  DOOR(h);
  return finish(c, poly_fold(&c, src, dst, n, extra, *cn));
}
// The grand product of a proof's round 2 as prove() queues it (prover.hip): the forward root tables of log n, the
// numerator / denominator terms, the twiddle-form inversion of the denominators, their product and the scan.  count == 0:
// all n evaluation indices, finished by scan_prefix_product.  count > 0: the indices [first, first + count) as one rank of a
// sharded proof runs them, up to scan_prefix_product_local — the carry and _apply are the caller's, as they are the host's
// in prove().  wires / sigma: 4 device arrays of n; num / den: n each; flag_dev: set when a denominator is zero.
int dp_grand_product(plonk_ctx* h, uint32_t L, const Fr* const* wires, const Fr* const* sigma, const Fr* beta, const Fr* gamma,
                     uint64_t first, uint64_t count, Fr* num, Fr* den, Fr* totals, int* flag_dev) {
  DOOR(h);
  NttTables* tbn = nullptr;
  int rc = ntt_tables(&c, L, false, &tbn);
  if (rc) return finish(c, rc);
  const uint64_t n = 1ull << L;
  PermArgs pa;
  pa.n = n;
  pa.first = first;
  pa.count = count;
  for (int k = 0; k < 4; ++k) { pa.wires[k] = wires[k]; pa.sigma[k] = sigma[k]; }
  pa.beta = *beta; pa.gamma = *gamma;
  pa.ks[0] = Fr::one(); pa.ks[1] = Fr::from_u64(7); pa.ks[2] = Fr::from_u64(13); pa.ks[3] = Fr::from_u64(17);
  pa.tw_lo29 = tbn->tw_lo29; pa.tw_hi29 = tbn->tw_hi29; pa.lobits = L < 13 ? L : 13; pa.use_hi = L > 13;
  pa.num = num; pa.den = den;
  const uint64_t cnt = count ? count : n;
  rc = poly_perm_terms(&c, pa);
  if (!rc) rc = poly_batch_inverse(&c, den + first, cnt, true);
  if (!rc) rc = poly_mul_arrays(&c, num + first, den + first, cnt, flag_dev);
  if (!rc) rc = count ? scan_prefix_product_local(&c, num + first, cnt, totals) : scan_prefix_product(&c, num, n, totals);
  return finish(c, rc);
}

}  // extern "C"
