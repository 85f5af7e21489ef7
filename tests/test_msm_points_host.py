"""CPU: what the host and the device share of plonk_msm_points — plonk_amd/csrc/msm_points_core.hpp, the plan of a call and
the signed-digit recoding of the two GLV halves — compiled with g++ (tests/csrc/host_msm_points.cpp) and checked against
plain integer arithmetic; and that file's host bucket pipeline over G1R, stage by stage what msm_points.hip runs on the
device, against the oracle's msm_naive on the point cases of the GPU test."""
import random

import pytest

from oracle import bls12_381 as E
from tests import msm_points_cases as C

Q, LAMBDA = C.Q, C.LAMBDA
WIDTHS = list(range(2, 17))


def check_recoding(k, c):
    k1, k2, d1, d2 = C.host_recode(k, c)
    W = -(-129 // c)
    assert len(d1) == len(d2) == W                                            # (b) the window count
    assert k1 < 1 << 128 and k2 < 1 << 128
    assert (k1 + k2 * LAMBDA) % Q == k % Q                                    # (a) the halves rebuild the scalar
    for half, digits in ((k1, d1), (k2, d2)):
        assert sum(d << (c * w) for w, d in enumerate(digits)) == half        # (a) the digits rebuild the half, exactly
        assert all(-(1 << (c - 1)) <= d <= 1 << (c - 1) for d in digits)      # (b) every digit in its range
    return d1, d2


def test_lambda_is_the_endomorphism_eigenvalue():
    assert (LAMBDA * LAMBDA + LAMBDA + 1) % Q == 0
    p = C.pool()[0]
    x, y = E.g1_mul(p, LAMBDA)
    assert y == p[1] and x != p[0] and pow(x, 3, E.P) == pow(p[0], 3, E.P)


@pytest.mark.parametrize("c", WIDTHS)
def test_digits_rebuild_the_edge_scalars(c):
    for k in C.edge_scalars():
        check_recoding(k, c)


@pytest.mark.parametrize("c", WIDTHS)
def test_every_digit_at_the_top_of_its_range(c):
    h = 1 << (c - 1)
    k = C.every_digit(c, h)
    d1, d2 = check_recoding(k, c)
    assert set(d1) <= {h, 0} and d1.count(h) >= 127 // c and not any(d2)
    # every window all ones: -1, then zeros carried up to a final +1
    k = C.every_digit(c, (1 << c) - 1)
    d1, _ = check_recoding(k, c)
    assert d1[0] == -1 and d1.count(1) == 1 and d1.count(0) == len(d1) - 2
    # the same digits in half 2
    _, d2 = check_recoding(C.every_digit(c, h) * LAMBDA % Q, c)
    assert set(d2) <= {h, 0} and d2.count(h) >= 127 // c


@pytest.mark.parametrize("c", WIDTHS)
def test_digits_rebuild_random_scalars(c):
    rnd = random.Random(1000 + c)
    for _ in range(200):
        check_recoding(rnd.randrange(Q), c)


def test_plan_follows_the_cost_model_and_the_forced_fields():
    for m in (0, 1, 2, 64, 65, 1000, 106512, 1 << 17, 1 << 20, 1 << 24):
        p = C.host_plan(m)
        cost = {c: -(-129 // c) * (2 * m + 4 * (1 << (c - 1))) for c in WIDTHS}
        best = min(WIDTHS, key=lambda c: (cost[c], c))
        assert p["window_bits"] == best and p["windows"] == -(-129 // best)
        assert p["slice_entries"] == min(64, max(4, (2 * m * p["windows"]) >> 17))
        assert p["path"] == (1 if m >= 64 else 0)   # the measured crossover
        assert C.host_plan(m, min_bucket_terms=1)["path"] == (1 if m else 0)   # 1 forces buckets
    assert C.host_plan(1 << 20)["window_bits"] >= 13 and C.host_plan(1)["window_bits"] == 2
    p = C.host_plan(100, window_bits=7, slice_entries=5, min_bucket_terms=101)
    assert (p["path"], p["window_bits"], p["windows"], p["slice_entries"]) == (0, 7, 19, 5)
    assert C.host_plan(101, min_bucket_terms=101)["path"] == 1


CASES = C.point_cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_host_pipeline_equals_the_oracle_on_the_point_cases(name):
    _, pts, scalars, opts, want = next(c for c in CASES if c[0] == name)
    assert len(pts) <= 64
    plan = C.host_plan(len(pts), opts.get("window_bits", 0))
    got, stats = C.host_msm(pts, scalars, plan["window_bits"], plan["slice_entries"])
    assert got == want
    assert stats["nonzero_digits"] == C.host_count_digits(pts, scalars, plan["window_bits"])
    # a width with many entries per bucket and slices of two: cut buckets, equal and opposite points inside one slice
    got, stats = C.host_msm(pts, scalars, 3, 2)
    assert got == want and stats["slices"] >= stats["nonzero_digits"] // 2


def test_host_pipeline_on_the_edge_scalars():
    s = C.edge_scalars([2, 5, 13, 16])
    pts = C.pool()[:len(s)]
    want = E.msm_naive(pts, s)
    for c in (2, 5, 13):
        assert C.host_msm(pts, s, c, 4)[0] == want
