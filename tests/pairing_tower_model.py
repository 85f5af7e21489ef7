"""Plain-Python model of the extension tower of plonk_amd/csrc/pairing28.cuh, written independently of it: Python integers
modulo p and nothing else.  Fp2 = Fp[u] / (u^2 + 1) as pairs (a, b) = a + b u, Fp6 = Fp2[v] / (v^3 - xi) with xi = 1 + u as
triples, Fp12 = Fp6[w] / (w^2 - v) as pairs.  Every product is the schoolbook one and every square is a product, so that the
specialised routines of the header (Karatsuba, the complex-method square, the sparse line products, the Granger-Scott
square) are compared with something that shares none of their structure; Frobenius maps, the map into the cyclotomic
subgroup and the final exponentiation are POWERS (x^(p^k); x^(3 (p^12 - 1) / r) with x^(p^6) taken as the conjugation), with
no table of constants anywhere.  tests/test_pairing_tower_model_host.py pins this model to tests/pairing_ref.py (the flat w basis,
itself held to the oracle).  Test infrastructure only; a final exponentiation takes a good part of a second."""
import functools

from oracle.bls12_381 import P, Q

BLS_X = 0xD201000000010000      # |x|, x < 0

# ---- Fp2 ------------------------------------------------------------------------------------------------------------------
F2_ZERO, F2_ONE = (0, 0), (1, 0)


def f2_add(x, y): return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)
def f2_sub(x, y): return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)
def f2_neg(x): return (-x[0] % P, -x[1] % P)
def f2_conj(x): return (x[0], -x[1] % P)
def f2_mul_xi(x): return ((x[0] - x[1]) % P, (x[0] + x[1]) % P)                # (a + b u)(1 + u)
def f2_mul(x, y): return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)
def f2_sqr(x): return f2_mul(x, x)
def f2_mul_fp(x, k): return (x[0] * k % P, x[1] * k % P)


def f2_inv(x):
    n = pow(x[0] * x[0] + x[1] * x[1], -1, P)
    return (x[0] * n % P, -x[1] * n % P)


# ---- Fp6 ------------------------------------------------------------------------------------------------------------------
F6_ZERO, F6_ONE = (F2_ZERO, F2_ZERO, F2_ZERO), (F2_ONE, F2_ZERO, F2_ZERO)


def f6_add(x, y): return tuple(f2_add(a, b) for a, b in zip(x, y))
def f6_sub(x, y): return tuple(f2_sub(a, b) for a, b in zip(x, y))
def f6_neg(x): return tuple(f2_neg(a) for a in x)
def f6_mul_v(x): return (f2_mul_xi(x[2]), x[0], x[1])                           # v^3 = xi


def f6_mul(x, y):
    """schoolbook: the nine Fp2 products summed by degree as unreduced integers, v^3 and v^4 folded with xi, one reduction"""
    t = [[0, 0] for _ in range(5)]
    for i, (a, b) in enumerate(x):
        for j, (c, d) in enumerate(y):
            t[i + j][0] += a * c - b * d
            t[i + j][1] += a * d + b * c
    return (((t[0][0] + t[3][0] - t[3][1]) % P, (t[0][1] + t[3][0] + t[3][1]) % P),
            ((t[1][0] + t[4][0] - t[4][1]) % P, (t[1][1] + t[4][0] + t[4][1]) % P), (t[2][0] % P, t[2][1] % P))


def f6_sqr(x): return f6_mul(x, x)


def f6_inv(x):
    """through the norm to Fp2: x * x' * x'' with the two conjugates over Fp2 taken as the cofactor of the 3 x 3 matrix of
    multiplication by x, written out"""
    a, b, c = x
    A = f2_sub(f2_sqr(a), f2_mul_xi(f2_mul(b, c)))
    B = f2_sub(f2_mul_xi(f2_sqr(c)), f2_mul(a, b))
    C = f2_sub(f2_sqr(b), f2_mul(a, c))
    n = f2_inv(f6_mul(x, (A, B, C))[0])
    r = (f2_mul(A, n), f2_mul(B, n), f2_mul(C, n))
    assert f6_mul(x, r) == F6_ONE
    return r


# ---- Fp12 -----------------------------------------------------------------------------------------------------------------
F12_ZERO, F12_ONE = (F6_ZERO, F6_ZERO), (F6_ONE, F6_ZERO)


def f12_add(x, y): return (f6_add(x[0], y[0]), f6_add(x[1], y[1]))
def f12_sub(x, y): return (f6_sub(x[0], y[0]), f6_sub(x[1], y[1]))
def f12_neg(x): return (f6_neg(x[0]), f6_neg(x[1]))
def f12_conj(x): return (x[0], f6_neg(x[1]))                                    # w -> -w: x^(p^6)


def f12_mul(x, y):                                                              # w^2 = v
    return (f6_add(f6_mul(x[0], y[0]), f6_mul_v(f6_mul(x[1], y[1]))), f6_add(f6_mul(x[0], y[1]), f6_mul(x[1], y[0])))


def f12_sqr(x): return f12_mul(x, x)


def f12_inv(x):
    n = f6_inv(f6_sub(f6_sqr(x[0]), f6_mul_v(f6_sqr(x[1]))))                    # (c0 + c1 w)(c0 - c1 w) = c0^2 - v c1^2
    r = (f6_mul(x[0], n), f6_neg(f6_mul(x[1], n)))
    assert f12_mul(x, r) == F12_ONE
    return r


def f12_pow(x, e):
    """x^e, e >= 0, by 4-bit windows (plain square-and-multiply with fewer products)"""
    tab = [F12_ONE, x]
    for _ in range(14):
        tab.append(f12_mul(tab[-1], x))
    acc = F12_ONE
    for shift in range((max(e.bit_length(), 1) + 3) // 4 * 4 - 4, -1, -4):
        for _ in range(4):
            acc = f12_mul(acc, acc)
        d = (e >> shift) & 15
        if d:
            acc = f12_mul(acc, tab[d])
    return acc


def line_element(c0, c1, c2, px, py):
    """(c0 + (c1 px) v) + ((c2 py) v) w: a prepared line (three Fp2 coefficients) at the G1 point (px, py)"""
    return ((c0, f2_mul_fp(c1, px), F2_ZERO), (F2_ZERO, f2_mul_fp(c2, py), F2_ZERO))


def sparse_014(a0, a1, b1):
    return ((a0, a1, F2_ZERO), (F2_ZERO, b1, F2_ZERO))


def f4_sqr(a, b):
    """(a + b s)^2 in Fp4 = Fp2[s] / (s^2 - xi)"""
    return (f2_add(f2_sqr(a), f2_mul_xi(f2_sqr(b))), f2_mul_fp(f2_mul(a, b), 2))


def frobenius(x, k):
    return f12_pow(x, P ** k)


def to_cyclotomic(x):
    """x^((p^6 - 1)(p^2 + 1)): the easy part of the final exponentiation, onto the cyclotomic subgroup.  x^(p^6) is the
    conjugation, so x^(p^6 - 1) = conj(x) / x; the factor p^2 + 1 is a power and a product"""
    y = f12_mul(f12_conj(x), f12_inv(x))
    return f12_mul(f12_pow(y, P ** 2), y)


def cyc_pow_x(x):
    """x^|BLS_X| conjugated: x^BLS_X for the negative parameter, on elements whose inverse is their conjugate"""
    return f12_conj(f12_pow(x, BLS_X))


FINAL = 3 * (P ** 12 - 1) // Q
HARD = 3 * (P ** 4 - P ** 2 + 1) // Q
assert (P ** 6 - 1) * (P ** 2 + 1) * HARD == FINAL


@functools.lru_cache(None)
def final_exponentiation(x):
    """x^FINAL, with the exponent split as above (a third of the cost of the one power, which the model's test compares it
    with); x not zero"""
    return f12_pow(to_cyclotomic(x), HARD)


# ---- the Miller loop, affine on the twist -----------------------------------------------------------------------------------


def _g2_step(t, q):
    """(slope, t + q) on the twist y^2 = x^3 + 4 (1 + u); q is t for a doubling"""
    if t == q:
        lam = f2_mul(f2_mul_fp(f2_sqr(t[0]), 3), f2_inv(f2_mul_fp(t[1], 2)))
    else:
        lam = f2_mul(f2_sub(q[1], t[1]), f2_inv(f2_sub(q[0], t[0])))
    x3 = f2_sub(f2_sub(f2_sqr(lam), t[0]), q[0])
    return lam, (x3, f2_sub(f2_mul(lam, f2_sub(t[0], x3)), t[1]))


def _line(t, lam, p):
    """the line of slope lam through the untwisted t = (x_T / w^2, y_T / w^3), at p = (x_P, y_P), times w^3 (an element of Fp4,
    which the final exponentiation sends to 1): (lam x_T - y_T) - lam x_P v + y_P v w"""
    return line_element(f2_sub(f2_mul(lam, t[0]), t[1]), f2_neg(lam), F2_ONE, p[0], p[1])


def miller_loop(p, q):
    """f_{x, Q}(P) for the negative parameter, up to factors the final exponentiation removes; p a G1 point (x, y), q a
    point of the twist ((x0, x1), (y0, y1)), either None for the identity"""
    if p is None or q is None:
        return F12_ONE
    f, t = F12_ONE, q
    for bit in bin(BLS_X)[3:]:
        lam, t2 = _g2_step(t, t)
        f = f12_mul(f12_sqr(f), _line(t, lam, p))
        t = t2
        if bit == "1":
            lam, t2 = _g2_step(t, q)
            f = f12_mul(f, _line(t, lam, p))
            t = t2
    return f12_conj(f)


# ---- flat views --------------------------------------------------------------------------------------------------------------


def f12_coords(x):
    """the 12 Fp values in the order of the header's F12r: c0.c0.a, c0.c0.b, c0.c1.a, ..., c1.c2.b"""
    return [c for h in x for f2 in h for c in f2]


def f12_of_coords(c):
    c = list(c)
    assert len(c) == 12
    return tuple(tuple((c[6 * h + 2 * i] % P, c[6 * h + 2 * i + 1] % P) for i in range(3)) for h in range(2))


def f6_coords(x): return [c for f2 in x for c in f2]


def f6_of_coords(c):
    c = list(c)
    assert len(c) == 6
    return tuple((c[2 * i] % P, c[2 * i + 1] % P) for i in range(3))
