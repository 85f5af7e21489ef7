"""CPU: the tower model of tests/pairing_tower_model.py (what the pairing families of tests/arith_vectors.py expect) pinned
to tests/pairing_ref.py, the flat-basis Fp12 that is itself held to the oracle, through from_tower.  The two share no code:
one multiplies coefficient lists modulo w^12 - 2 w^6 + 2, the other nested pairs and triples."""
import random

import g2_ref as G2
import kzg_ref as K
import pairing_ref as PR
import pairing_tower_model as M
from oracle import bls12_381 as E

P, Q = E.P, E.Q


def flat(x):
    return PR.from_tower(M.f12_coords(x))


def rand_f12(rnd):
    return M.f12_of_coords(rnd.randrange(P) for _ in range(12))


def structured():
    """single coefficients, the all-(p - 1) element, one with its last coefficients empty"""
    out = [M.f12_of_coords([0] * i + [v] + [0] * (11 - i)) for i, v in ((1, 1), (4, P - 1), (7, 2), (11, (P - 1) // 2))]
    return out + [M.f12_of_coords([P - 1] * 12), M.f12_of_coords([3, P - 2, 0, 1] + [0] * 8)]


def test_the_tower_product_is_the_flat_product():
    rnd = random.Random(1201)
    xs = [rand_f12(rnd) for _ in range(4)] + structured()
    for x in xs:
        for y in xs[:3] + xs[-3:]:
            assert flat(M.f12_mul(x, y)) == PR.f12_mul(flat(x), flat(y))
    x, y = xs[0], xs[1]
    assert flat(M.f12_add(x, y)) == PR.f12_add(flat(x), flat(y)) and flat(M.f12_sub(x, y)) == PR.f12_sub(flat(x), flat(y))
    assert flat(M.F12_ONE) == PR.ONE and M.f12_sqr(x) == M.f12_mul(x, x)
    # the levels below: an Fp6 / Fp2 product is the Fp12 product of the embedded elements
    assert (M.f6_mul(x[0], y[1]), M.F6_ZERO) == M.f12_mul((x[0], M.F6_ZERO), (y[1], M.F6_ZERO))
    assert M.f6_mul_v(x[0]) == M.f6_mul(x[0], (M.F2_ZERO, M.F2_ONE, M.F2_ZERO))
    assert M.f12_mul((x[0], M.F6_ZERO), (M.F6_ZERO, M.F6_ONE)) == (M.F6_ZERO, x[0])
    a, b = x[0][0], y[0][1]
    assert ((M.f2_mul(a, b), M.F2_ZERO, M.F2_ZERO), M.F6_ZERO) == M.f12_mul(((a, M.F2_ZERO, M.F2_ZERO), M.F6_ZERO), ((b, M.F2_ZERO, M.F2_ZERO), M.F6_ZERO))
    assert M.f2_mul_xi(a) == M.f2_mul(a, (1, 1)) and M.f2_mul(a, M.f2_inv(a)) == M.F2_ONE and M.f6_mul(x[1], M.f6_inv(x[1])) == M.F6_ONE
    assert M.f4_sqr(a, b) == (M.f2_add(M.f2_mul(a, a), M.f2_mul((1, 1), M.f2_mul(b, b))), M.f2_add(M.f2_mul(a, b), M.f2_mul(a, b)))


def test_the_tower_inverse_is_the_power_by_the_group_order_less_one():
    rnd = random.Random(1202)
    for x in (rand_f12(rnd), structured()[1]):
        assert flat(M.f12_inv(x)) == PR.f12_pow(flat(x), PR.ORDER - 1)


def test_frobenius_and_conjugation_are_the_flat_powers():
    rnd = random.Random(1203)
    x, s = rand_f12(rnd), structured()
    for k, t in ((1, s[0]), (2, s[3]), (3, s[5])):
        for y in (x, t):
            assert flat(M.frobenius(y, k)) == PR.f12_pow(flat(y), P ** k)
    assert M.f12_conj(x) == M.frobenius(M.frobenius(x, 3), 3)


def test_the_final_exponentiation_and_the_model_pairing_are_the_flat_ones():
    rnd = random.Random(1204)
    x = rand_f12(rnd)
    assert flat(M.final_exponentiation(x)) == PR.final_exp(flat(x), negative_x=False)
    assert M.final_exponentiation(x) == M.f12_pow(x, M.FINAL) and M.FINAL == PR.FINAL
    m = M.to_cyclotomic(x)
    assert m == M.f12_pow(x, (P ** 6 - 1) * (P ** 2 + 1))
    assert M.f12_mul(m, M.f12_conj(m)) == M.F12_ONE and M.cyc_pow_x(m) == M.f12_inv(M.f12_pow(m, PR.BLS_X))
    # the model's Miller loops, after its final exponentiation, give the pairing of pairing_ref.py
    a, b = E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)), E.g1_mul(E.G1_GEN, rnd.randrange(1, Q))
    xh = G2.g2_mul(G2.G2_GEN, K.TAU)
    f = M.f12_mul(M.miller_loop(a, xh), M.miller_loop(b, G2.G2_GEN))
    assert flat(M.final_exponentiation(f)) == PR.multi_pairing([(a, xh), (b, G2.G2_GEN)])
