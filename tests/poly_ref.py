"""Big-int models of the O(n) kernels of plonk_amd/csrc/poly.hip, one per launcher, for tests/test_gpu_poly_kernels.py
(the device side) and tests/test_poly_ref_host.py (which pins them to oracle.plonk).  Plain Python over oracle.bls12_381.Q.

Number forms (poly.hip, fr29.cuh).  A field element x travels as one of two raw integers below q, 32 bytes little-endian:

  data form      x * 2^256   the Montgomery form of the reference; what plonk_amd.fr_to_bytes_mont writes
  twiddle form   x * 2^261   closed under the reduced-radix product: (a 2^261)(b 2^261) / 2^261 = ab 2^261

  poly_batch_inverse, data form      raw r -> r^-1 * 2^512   (x 2^256 -> x^-1 2^256); zeros stay zero
  poly_batch_inverse, twiddle form   raw r -> r^-1 * 2^522   (x 2^261 -> x^-1 2^261); zeros stay zero
  poly_mul_arrays                    twiddle form in both operands and out
  scan_prefix_product                twiddle form in, data form out, inclusive
  scan_prefix_product_local          twiddle form in; leaves the inclusive products WITHIN each block of
                                     256 * pscan_e(n) elements, twiddle form, and in totals[b] the product of the
                                     blocks 0..b (twiddle form): the range's product is totals[scan_prefix_blocks(n) - 1]
  scan_prefix_product_apply          element of block b *= totals[b - 1] (b > 0) * carry (twiddle form), data form out
  everything else                    data form in and out; those operations are linear in the coefficients, so their
                                     models apply to raw data-form integers as they stand (scalars and points canonical)

Every model takes and returns canonical integers unless its name ends in _raw."""
from oracle.bls12_381 import Q, K1, K2, K3

R = pow(2, 256, Q)        # data form
T = pow(2, 261, Q)        # twiddle form
RINV = pow(R, Q - 2, Q)
TINV = pow(T, Q - 2, Q)
BI_CONST = {False: pow(2, 512, Q), True: pow(2, 522, Q)}   # raw_in * raw_out of a batch inversion, by twiddle_form
SPECIALS = (1, 2, Q - 1, (Q + 1) // 2)                     # edge operands besides 0


def inv(x):
    assert x % Q
    return pow(x, Q - 2, Q)


def to_data(v):
    return [x * R % Q for x in v]


def from_data(v):
    return [x * RINV % Q for x in v]


def to_tw(v):
    return [x * T % Q for x in v]


def from_tw(v):
    return [x * TINV % Q for x in v]


def raw_bytes(raws):
    return b"".join(r.to_bytes(32, "little") for r in raws)


def raw_ints(buf):
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


# ---- batch inversion ------------------------------------------------------------------------------------------------
BI_GEOMETRY = {0: (256, 16), 1: (64, 4), 2: (64, 16), 3: (128, 8)}   # bi_cfg -> lanes, elements per lane


def bi_auto(n):
    """the geometry poly_batch_inverse picks when bi_cfg is not 0..3"""
    return 1 if n <= (1 << 17) else 0


def batch_inverse(v):
    return [inv(x) if x % Q else 0 for x in v]


def batch_inverse_raw(raws, twiddle_form):
    k = BI_CONST[bool(twiddle_form)]
    return [inv(r) * k % Q if r else 0 for r in raws]


# ---- scans ------------------------------------------------------------------------------------------------------------
SCAN_T = 256


def pscan_e(n):
    return 2 if n <= (1 << 17) else 8


def scan_prefix_blocks(n):
    blk = SCAN_T * pscan_e(n)
    return (n + blk - 1) // blk


def prefix_product(v):
    out, acc = [], 1
    for x in v:
        acc = acc * x % Q
        out.append(acc)
    return out


def prefix_product_raw(raws):
    """scan_prefix_product: twiddle-form raws in, data-form raws out"""
    out, acc = [], R
    for r in raws:
        acc = acc * r % Q * TINV % Q
        out.append(acc)
    return out


def prefix_local_raw(raws):
    """scan_prefix_product_local -> (data, totals), both twiddle-form raws"""
    n = len(raws)
    blk = SCAN_T * pscan_e(n)
    data, totals, run = [], [], T
    for b in range(0, n, blk):
        acc = T
        for r in raws[b:b + blk]:
            acc = acc * r % Q * TINV % Q
            data.append(acc)
        run = run * acc % Q * TINV % Q
        totals.append(run)
    return data, totals


def prefix_apply_raw(local, totals, carry_raw):
    """scan_prefix_product_apply on what _local left: data-form raws out"""
    n = len(local)
    blk = SCAN_T * pscan_e(n)
    out = []
    for b in range(0, n, blk):
        off = carry_raw * TINV % Q * R % Q * TINV % Q                   # carry (twiddle) -> a factor that lands in data form
        if b:
            off = off * totals[b // blk - 1] % Q * TINV % Q
        out.extend(x * off % Q for x in local[b:b + blk])
    return out


def carry_next_raw(carry_raw, range_total_raw):
    """the host step of a sharded grand product (prover.hip): carry * total, both and the result in twiddle form"""
    return carry_raw * range_total_raw % Q * TINV % Q


def suffix_sum(v):
    out, acc = [0] * len(v), 0
    for i in range(len(v) - 1, -1, -1):
        acc = (acc + v[i]) % Q
        out[i] = acc
    return out


# ---- evaluation, linear combination -------------------------------------------------------------------------------
def poly_eval(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % Q
    return acc


def suffix_evals(c, x, starts):
    """{k: evaluation at x of the polynomial c[k:]} for k in starts, from ONE Horner pass over c"""
    want, out, acc = set(starts), {}, 0
    for i in range(len(c) - 1, -1, -1):
        acc = (acc * x + c[i]) % Q
        if i in want:
            out[i] = acc
    return out


EVAL_T = 256


def eval_blocks(max_len):
    """workgroups (= partials per item) poly_eval launches for max_len coefficients"""
    per = EVAL_T << (2 if max_len <= (1 << 17) else 4)
    return (max_len + per - 1) // per


def lincomb(terms, length, constant):
    """terms: (coefficients, scalar); out[i] = sum_k s_k p_k[i] over the terms that reach i, + constant at i = 0"""
    out = [0] * length
    for p, s in terms:
        for i in range(min(len(p), length)):
            out[i] = (out[i] + p[i] * s) % Q
    if length:
        out[0] = (out[0] + constant) % Q
    return out


# ---- division by X - z ----------------------------------------------------------------------------------------------
def ruffini(c, z):
    """poly_ruffini: len(c) slots, the quotient in the first len - 1 and zero in the last (the remainder is dropped)"""
    out, k = [0] * len(c), 0
    for i in range(len(c) - 1, 0, -1):
        k = (c[i] + k * z) % Q
        out[i - 1] = k
    return out


def ruffini_local(c_range, lo, z):
    """poly_ruffini_local over c[lo, lo + len): len + 1 scratch slots; slot 0 is the range's share of sum_j c_j z^j"""
    p, d = pow(z, lo, Q), []
    for v in c_range:
        d.append(v * p % Q)
        p = p * z % Q
    return suffix_sum(d) + [0]


def ruffini_finish(scratch, lo, zinv, carry):
    """poly_ruffini_finish: the slots dst[lo, lo + len) (before the caller's `last` slot is zeroed)"""
    out, p = [], pow(zinv, lo + 1, Q)
    for i in range(len(scratch) - 1):
        out.append((scratch[i + 1] + carry) * p % Q)
        p = p * zinv % Q
    return out


def ruffini_by_ranges(c, z, cuts):
    """the whole division from ranges [cuts[k], cuts[k + 1]) as a sharded proof combines them"""
    bounds = [0] + list(cuts) + [len(c)]
    parts = [(lo, ruffini_local(c[lo:hi], lo, z)) for lo, hi in zip(bounds, bounds[1:])]
    out, zinv = [0] * len(c), inv(z)
    for k, (lo, scratch) in enumerate(parts):
        carry = sum(s[0] for _, s in parts[k + 1:]) % Q
        got = ruffini_finish(scratch, lo, zinv, carry)
        out[lo:lo + len(got)] = got
    out[len(c) - 1] = 0
    return out


# ---- small kernels ----------------------------------------------------------------------------------------------------
def mul_arrays(a, b):
    return [x * y % Q for x, y in zip(a, b)], int(any(y % Q == 0 for y in b))


def trimmed_len(v):
    n = len(v)
    while n and v[n - 1] % Q == 0:
        n -= 1
    return n


def split_t(t, n, np, b):
    """poly_split_t (prover.rs:547-574): t_low, t_mid, t_high as three arrays of np slots
         part k, slot i < n: t[k n + i];  slot n: b[k];  slots above: 0;  slot 0 of part k >= 1: -= b[k - 1]
    and t itself with t[3 n] -= b[2] (t_fourth stays in place).  Returns (out, t)."""
    out = []
    for k in range(3):
        part = [t[k * n + i] if i < n else (b[k] if i == n else 0) for i in range(np)]
        if k:
            part[0] = (part[0] - b[k - 1]) % Q
        out.extend(part)
    t = list(t)
    t[3 * n] = (t[3 * n] - b[2]) % Q
    return out, t


def fold(src, n, extra, c):
    """poly_fold: src (n + extra coefficients) mod (X^n - c)"""
    return [(src[i] + c * src[n + i]) % Q if i < extra else src[i] for i in range(n)]


# ---- permutation grand product ----------------------------------------------------------------------------------------
def perm_terms(roots, wires, sigma, beta, gamma):
    """poly_perm_terms: (num, den) with num[0] = den[0] = 1 and the factors of row i - 1 at index i"""
    n = len(roots)
    ks = [1, K1, K2, K3]
    num, den = [1], [1]
    for r in range(n - 1):
        a = b = 1
        for k in range(4):
            a = a * (wires[k][r] + beta * roots[r] * ks[k] + gamma) % Q
            b = b * (wires[k][r] + beta * sigma[k][r] + gamma) % Q
        num.append(a)
        den.append(b)
    return num, den


def grand_product(roots, wires, sigma, beta, gamma):
    """the chain of prove(): terms, inverted denominators, their product, the inclusive scan -> (z evaluations, flag)"""
    num, den = perm_terms(roots, wires, sigma, beta, gamma)
    ratio, flag = mul_arrays(num, batch_inverse(den))
    return prefix_product(ratio), flag
