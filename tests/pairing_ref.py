"""Plain-Python optimal-ate pairing of BLS12-381 for the tests of plonk_amd/csrc/hostpairing.hpp, written independently of
it: Fp12 = Fp[w] / (w^12 - 2 w^6 + 2) as coefficient lists (u = w^6 - 1, so w^6 = 1 + u and v = w^2), G2 untwisted by
(x', y') -> (x' / w^2, y' / w^3), an affine Miller loop on E(Fp12) with textbook tangent / chord lines, and the final
exponentiation as one big power.  pairing() returns e(P, Q)^3 with e the reduced optimal-ate pairing for x < 0 — the value
the product code computes (its hard part is the x-chain of 3 (p^4 - p^2 + 1) / r).  Test infrastructure only; slow
(~1 s per pairing)."""
from oracle.bls12_381 import P, Q

import g2_ref as G2

BLS_X = 0xD201000000010000      # |x|, x < 0
MOD = [2] + [0] * 5 + [P - 2] + [0] * 5    # w^12 = 2 w^6 - 2  ->  reduction coefficients of w^0 .. w^11


def f12(coeffs):
    return [c % P for c in coeffs] + [0] * (12 - len(coeffs))


ONE = f12([1])


def f12_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):    # w^k = w^(k-12) (2 w^6 - 2)
        c = t[k]
        if c:
            t[k - 6] += 2 * c
            t[k - 12] -= 2 * c
    return [x % P for x in t[:12]]


def f12_add(a, b): return [(x + y) % P for x, y in zip(a, b)]
def f12_sub(a, b): return [(x - y) % P for x, y in zip(a, b)]
def f12_scale(a, k): return [x * k % P for x in a]


def f12_pow(a, e):
    acc = ONE
    for bit in bin(e)[2:]:
        acc = f12_mul(acc, acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


def from_fp2(x):
    """a + b u  ->  a + b (w^6 - 1)"""
    a, b = x
    return f12([a - b, 0, 0, 0, 0, 0, b])


W = f12([0, 1])
INV2 = pow(2, -1, P)
U_NEG_HALF = f12_scale(f12_sub(ONE, f12([0, 0, 0, 0, 0, 0, 1])), INV2)      # -u / 2 = 1 / w^12 ... (w^12 = 2 u, 1/u = -u)
W_INV2 = f12_mul(f12_pow(W, 10), U_NEG_HALF)     # w^-2 = w^10 / w^12
W_INV3 = f12_mul(f12_pow(W, 9), U_NEG_HALF)      # w^-3 = w^9 / w^12
W_INV1 = f12_mul(f12_pow(W, 11), U_NEG_HALF)


def line(t, lam, p):
    """the line of slope lam (on the twist) through untwist(t), at the G1 point p: (y_P - y_T) - lam w^-1 (x_P - x_T)"""
    xt = f12_mul(from_fp2(t[0]), W_INV2)
    yt = f12_mul(from_fp2(t[1]), W_INV3)
    lam12 = f12_mul(from_fp2(lam), W_INV1)
    return f12_sub(f12_sub(f12([p[1]]), yt), f12_mul(lam12, f12_sub(f12([p[0]]), xt)))


def miller_loop(p, q):
    """f_{|x|, Q}(P) with affine steps on the twist"""
    if p is None or q is None:
        return ONE
    f, t = ONE, q
    for bit in bin(BLS_X)[3:]:
        lam = G2.f2_mul(G2.f2_mul((3, 0), G2.f2_sqr(t[0])), G2.f2_inv(G2.f2_mul((2, 0), t[1])))
        f = f12_mul(f12_mul(f, f), line(t, lam, p))
        t = G2.g2_add(t, t)
        if bit == "1":
            lam = G2.f2_mul(G2.f2_sub(q[1], t[1]), G2.f2_inv(G2.f2_sub(q[0], t[0])))
            f = f12_mul(f, line(t, lam, p))
            t = G2.g2_add(t, q)
    return f


FINAL = 3 * (P ** 12 - 1) // Q
ORDER = P ** 12 - 1


def final_exp(f, negative_x=True):
    """f^(3 (p^12 - 1) / r), inverted for x < 0 (f_{x,Q} = 1 / f_{|x|,Q} up to vertical lines)"""
    return f12_pow(f, (ORDER - FINAL) if negative_x else FINAL)


def pairing(p, q):
    return final_exp(miller_loop(p, q))


def multi_pairing(pairs):
    f = ONE
    for p, q in pairs:
        f = f12_mul(f, miller_loop(p, q))
    return final_exp(f)


def from_tower(c):
    """12 Fp values in the order of hostpairing.hpp's F12 (c0.c0.a, c0.c0.b, c0.c1.a, ..., c1.c2.b) -> this basis:
    coefficient of c_h.c_i is w^(2 i + h)"""
    out = f12([])
    for h in range(2):
        for i in range(3):
            a, b = c[12 * 0 + 6 * h + 2 * i], c[6 * h + 2 * i + 1]
            term = f12_mul(from_fp2((a, b)), f12_pow(W, 2 * i + h))
            out = f12_add(out, term)
    return out
