"""CPU-only: the models of tests/poly_ref.py (what tests/test_gpu_poly_kernels.py holds the kernels of poly.hip to) against
what the suite already trusts — oracle.plonk's batch_inversion, poly_eval, poly_ruffini and permutation_vec — on random
inputs and inputs with zeros and edge operands; the range forms (_local / _apply, _local / _finish) recombined must equal the
whole; and the door library tests/_build/libdev_poly.so exists and exports every door.  All comparisons are exact."""
import ctypes
import os
import random

import pytest

import poly_ref as M
from oracle import plonk as O
from oracle.bls12_381 import Q
from oracle.fft import EvaluationDomain

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libdev_poly.so")
DOORS = ["dp_batch_inverse", "dp_scan_prefix_product", "dp_scan_prefix_product_local", "dp_scan_prefix_product_apply",
         "dp_scan_prefix_blocks", "dp_scan_suffix_sum", "dp_poly_eval", "dp_poly_lincomb", "dp_poly_ruffini",
         "dp_poly_ruffini_local", "dp_poly_ruffini_finish", "dp_poly_mul_arrays", "dp_poly_trimmed_len", "dp_poly_split_t",
         "dp_poly_fold", "dp_grand_product"]


def mixed(rnd, n, zeros=True):
    """random values with 0 (optionally) and the edge operands among them"""
    pool = M.SPECIALS + ((0,) if zeros else ())
    return [rnd.choice(pool) if rnd.random() < 0.3 else rnd.randrange(1, Q) for _ in range(n)]


def test_number_forms():
    assert M.R == pow(2, 256, Q) and M.T == M.R * 32 % Q
    import plonk_amd
    v = [0, 1, 2, Q - 1, (Q + 1) // 2, 12345]
    assert plonk_amd.fr_to_bytes_mont(v) == M.raw_bytes(M.to_data(v))
    assert M.raw_ints(M.raw_bytes(v)) == v
    assert M.from_data(M.to_data(v)) == v == M.from_tw(M.to_tw(v))


def test_batch_inverse_is_the_oracles_in_both_forms():
    rnd = random.Random(1)
    for n in (1, 2, 7, 100):
        v = mixed(rnd, n)
        want = O.batch_inversion(v)
        assert M.batch_inverse(v) == want
        assert M.from_data(M.batch_inverse_raw(M.to_data(v), False)) == want
        assert M.from_tw(M.batch_inverse_raw(M.to_tw(v), True)) == want
        for tw, raws in ((False, M.to_data(v)), (True, M.to_tw(v))):
            for r, o in zip(raws, M.batch_inverse_raw(raws, tw)):
                assert (o == 0) if r == 0 else (r * o % Q == M.BI_CONST[tw])
    assert M.batch_inverse([0, 0]) == [0, 0]
    assert [M.bi_auto(n) for n in (1, 1 << 17, (1 << 17) + 1)] == [1, 1, 0]


def test_prefix_product_forms_and_ranges_recombine():
    rnd = random.Random(2)
    assert [M.scan_prefix_blocks(n) for n in (1, 512, 513, 1 << 17, (1 << 17) + 1, (1 << 19) + 1)] == [1, 1, 2, 256, 65, 257]
    for n in (1, 2, 511, 513, 1500):
        v = mixed(rnd, n, zeros=False)
        if n == 1500:
            v[700] = 0
        want = M.prefix_product(v)
        assert want[0] == v[0] and all(want[i] == want[i - 1] * v[i] % Q for i in range(1, n))
        assert M.from_data(M.prefix_product_raw(M.to_tw(v))) == want
        # one range with the neutral carry is the whole scan
        local, totals = M.prefix_local_raw(M.to_tw(v))
        assert len(totals) == M.scan_prefix_blocks(n)
        assert M.from_tw(totals)[-1] == want[-1]
        assert M.from_data(M.prefix_apply_raw(local, totals, M.T)) == want
    # three unequal ranges, the products carried forward on the host
    n = 2100
    v = mixed(rnd, n, zeros=False)
    want, got, carry = M.prefix_product(v), [], M.T
    for lo, hi in ((0, 5), (5, 1300), (1300, n)):
        local, totals = M.prefix_local_raw(M.to_tw(v[lo:hi]))
        assert totals[-1] * M.TINV % Q * (want[lo - 1] if lo else 1) % Q == want[hi - 1]
        got += M.prefix_apply_raw(local, totals, carry)
        carry = M.carry_next_raw(carry, totals[-1])
    assert M.from_data(got) == want


def test_suffix_sum():
    rnd = random.Random(3)
    v = mixed(rnd, 50)
    got = M.suffix_sum(v)
    assert got == [sum(v[i:]) % Q for i in range(50)] and M.suffix_sum([]) == []


def test_eval_and_lincomb_are_the_oracles():
    rnd = random.Random(4)
    for n in (0, 1, 2, 33):
        c = mixed(rnd, n)
        for x in (0, 1, Q - 1, rnd.randrange(Q)):
            assert M.poly_eval(c, x) == O.poly_eval(c, x)
    c, x = mixed(rnd, 40), rnd.randrange(Q)
    assert M.suffix_evals(c, x, [0, 7, 39]) == {k: O.poly_eval(c[k:], x) for k in (0, 7, 39)}
    # evaluation is linear: the model applied to data-form raws gives the data-form result
    assert M.poly_eval(M.to_data(c), x) == O.poly_eval(c, x) * M.R % Q
    assert [M.eval_blocks(n) for n in (1, 1024, 1025, 1 << 17, (1 << 17) + 1, (1 << 20) + 1)] == [1, 1, 2, 128, 33, 257]
    a, b, s, t, k = mixed(rnd, 9), mixed(rnd, 4), rnd.randrange(Q), 0, rnd.randrange(Q)
    want = O.poly_add(O.poly_add(O.poly_scale(a, s), O.poly_scale(b, t)), [k])
    got = M.lincomb([(a, s), (b, t)], 9, k)
    assert O.poly_trim(got) == want and len(got) == 9
    assert M.lincomb([], 3, k) == [k, 0, 0]
    assert M.lincomb([(a, s)], 4, 0) == [v * s % Q for v in a[:4]]


def test_ruffini_is_the_oracles_and_ranges_recombine():
    rnd = random.Random(5)
    for n in (1, 2, 3, 64, 200):
        c = mixed(rnd, n)
        for z in (1, Q - 1, rnd.randrange(2, Q)):
            got = M.ruffini(c, z)
            assert len(got) == n and got[n - 1] == 0
            assert O.poly_trim(got) == O.poly_ruffini(c, z)
            # one range from 0 is the whole division
            assert M.ruffini_by_ranges(c, z, []) == got
            if n >= 3:
                assert M.ruffini_by_ranges(c, z, [1, n - 1]) == got
            if n == 200:
                assert M.ruffini_by_ranges(c, z, [3, 130]) == got
    # quotient * (X - z) + remainder = c
    c, z = mixed(rnd, 20), rnd.randrange(1, Q)
    q = M.ruffini(c, z)[:-1]
    back = [((q[i - 1] if i else 0) - z * (q[i] if i < 19 else 0)) % Q for i in range(20)]
    back[0] = (back[0] + O.poly_eval(c, z)) % Q
    assert back == [v % Q for v in c]
    assert M.ruffini_local(c[4:9], 4, z)[0] == sum(c[j] * pow(z, j, Q) for j in range(4, 9)) % Q


def test_small_kernel_models():
    rnd = random.Random(6)
    a, b = mixed(rnd, 10, zeros=False), mixed(rnd, 10, zeros=False)
    assert M.mul_arrays(a, b) == ([x * y % Q for x, y in zip(a, b)], 0)
    b[3] = 0
    assert M.mul_arrays(a, b)[1] == 1 and M.mul_arrays(b, a)[1] == 0
    for v in ([], [0, 0], [5], [0, 5, 0, 0], [1, 0, 7]):
        assert M.trimmed_len(v) == len(O.poly_trim(v))
    # split: t = t_low + X^n t_mid + X^2n t_high + X^3n t_fourth is unchanged by the blinding (prover.rs:547-574)
    n, np_ = 4, 8
    t, bl = mixed(rnd, 3 * n + 3), [rnd.randrange(Q) for _ in range(3)]
    out, t2 = M.split_t(t, n, np_, bl)
    x = rnd.randrange(Q)
    parts = [out[k * np_:(k + 1) * np_] for k in range(3)] + [t2[3 * n:]]
    assert sum(O.poly_eval(p, x) * pow(x, k * n, Q) for k, p in enumerate(parts)) % Q == O.poly_eval(t, x)
    assert all(p[n] == bl[k] and p[n + 1:] == [0] * (np_ - n - 1) for k, p in enumerate(parts[:3]))
    # fold: the same values wherever x^n = c
    src, c = mixed(rnd, n + 3), pow(x, n, Q)
    assert O.poly_eval(M.fold(src, n, 3, c), x) == O.poly_eval(src, x)


@pytest.mark.parametrize("log_n", [1, 2, 5])
def test_grand_product_is_the_oracles_permutation_vec(log_n):
    rnd = random.Random(7 + log_n)
    n = 1 << log_n
    dom = EvaluationDomain(n)
    roots = dom.elements()
    wires = [mixed(rnd, n) for _ in range(4)]
    pos = [k * r % Q for k in (1, 7, 13, 17) for r in roots]
    rnd.shuffle(pos)
    sigma = [pos[k * n:(k + 1) * n] for k in range(4)]
    beta, gamma = rnd.randrange(Q), rnd.randrange(Q)
    z, flag = M.grand_product(roots, wires, sigma, beta, gamma)
    assert flag == 0 and z == O.permutation_vec(dom, wires, beta, gamma, sigma)
    # a zero denominator factor: the flag, and the other elements stay finite
    wires[2][0] = (-beta * sigma[2][0] - gamma) % Q
    num, den = M.perm_terms(roots, wires, sigma, beta, gamma)
    assert den[1] == 0 and M.grand_product(roots, wires, sigma, beta, gamma)[1] == 1


def test_door_library_is_built_and_exports_every_door():
    import plonk_amd
    import __graft_entry__
    if not os.path.exists(plonk_amd.LIB_PATH):      # nothing built yet (as test_capi_symbols.py): build the pair
        __graft_entry__.build_hip(verbose=False)
    if not os.path.exists(SO):                      # a tree that lost tests/_build after build() (as test_field_host.py)
        __graft_entry__.build_dev_poly(verbose=False)
    assert os.path.exists(SO), "tests/_build/libdev_poly.so is missing: run build() of __graft_entry__.py first"
    lib = ctypes.CDLL(SO)
    for name in DOORS:
        assert hasattr(lib, name), name
    # every extern "C" door of the source is in the list above
    import re
    src = open(os.path.join(HERE, "csrc", "dev_poly.hip")).read()
    assert sorted(set(re.findall(r"^(?:int|uint32_t) (dp_\w+)\(", src, flags=re.M))) == sorted(DOORS)
