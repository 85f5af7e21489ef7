"""CPU: the KZG10 multiproofs in the exponent.  The big-int model tests/kzg_multiproof_model.py (g built group by group with the
derivative entry, the weights, h, the quotient at t, both challenges) is pinned to the oracle's ifft + Ruffini division + fft
route and to the verification equation for a known tau, for log_n 1..5, M in {1, 3} and K in {1, 2, 7, 40}, valid and tampered;
plonk_amd/csrc/kzg_multiproof_core.hpp (the argument checks in their order, both counting sorts, the plan, the challenge bytes)
is compiled with g++ (tests/csrc/host_kzg_multiproof.cpp) and checked against the same model."""
import ctypes
import os
import random
import subprocess

import pytest

import plonk_amd
from oracle.fft import EvaluationDomain
from tests import kzg_multiproof_model as M
from tests import kzg_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_multiproof.so")
Q = M.Q
TAU = K.TAU
CASES = [(log_n, nv, k) for log_n in range(1, 6) for nv in (1, 3) for k in (1, 2, 7, 40)]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_multiproof.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, vp, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    lib.hkm_check_items.argtypes = [u32, u64, vp, vp, u64, ci, ci]
    lib.hkm_check_counts.argtypes = [u32, u64, u64, ci, ci]
    lib.hkm_check_override.argtypes = [vp, u32, vp]
    lib.hkm_counting_sort.argtypes = [vp, u64, u64, vp, vp]
    lib.hkm_counting_sort.restype = None
    lib.hkm_sort_points.argtypes = [vp, u64, u64, vp, vp, vp]
    lib.hkm_sort_points.restype = u64
    lib.hkm_plan.argtypes = [u32, u64, u64, u64, ci, ci, vp]
    lib.hkm_plan.restype = None
    lib.hkm_challenges.argtypes = [vp, u64, u32, vp, u64, vp, vp, vp, u64, vp, vp]
    lib.hkm_challenges.restype = None
    return lib


def u32s(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def instance(log_n, nv, k, rnd):
    n = 1 << log_n
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(nv)]
    items = [(rnd.randrange(nv), rnd.randrange(n)) for _ in range(k)]
    return vectors, items


def naive_g(vectors, items, r, log_n):
    """sum_k r^k (p_(j_k) - y_k) / (X - w^(m_k)) through coefficients: ifft, synthetic division, fft"""
    n = 1 << log_n
    dom = EvaluationDomain(n)
    pts = M.domain_points(log_n)
    assert list(dom.elements()) == pts
    coeffs = [dom.ifft(list(e)) for e in vectors]
    acc, rp = [0] * n, 1
    for j, m in items:
        f = list(coeffs[j])
        f[0] = (f[0] - vectors[j][m]) % Q
        q = K.ruffini(f, pts[m])
        for i, c in enumerate(q):
            acc[i] = (acc[i] + rp * c) % Q
        rp = rp * r % Q
    assert acc[n - 1] == 0                                  # degree <= n - 2
    return dom.fft(acc)


# ---- the model against the coefficient route and the equation ---------------------------------------------------------------------
@pytest.mark.parametrize("log_n,nv,k", CASES)
def test_g_equals_the_coefficient_route(log_n, nv, k):
    rnd = random.Random(1000 * log_n + 10 * nv + k)
    vectors, items = instance(log_n, nv, k, rnd)
    r = rnd.randrange(Q)
    assert M.aggregate(vectors, items, r, log_n) == naive_g(vectors, items, r, log_n)


def test_g_with_every_pair_duplicates_and_the_edge_indexes():
    log_n, nv = 3, 2
    n = 1 << log_n
    rnd = random.Random(5)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(nv)]
    for items in ([(j, m) for j in range(nv) for m in range(n)], [(1, 0), (1, 0), (0, n - 1), (1, 0)], [(0, 0)], [(0, n - 1)]):
        for r in (0, 1, rnd.randrange(Q)):
            assert M.aggregate(vectors, items, r, log_n) == naive_g(vectors, items, r, log_n)


@pytest.mark.parametrize("log_n,nv,k", CASES)
def test_the_equation_holds_in_the_exponent_and_y_is_h_minus_g_at_t(log_n, nv, k):
    rnd = random.Random(2000 * log_n + 10 * nv + k)
    vectors, items = instance(log_n, nv, k, rnd)
    r, t = rnd.randrange(Q), rnd.randrange(Q)
    p = M.prove_scalars(vectors, items, r, t, log_n)
    # y = h(t) - g(t): an identity, nothing to evaluate
    lt = M.EV.lagrange_at(t, log_n)
    ht = sum(a * b for a, b in zip(p["h"], lt)) % Q
    gt = sum(a * b for a, b in zip(p["g"], lt)) % Q
    assert p["y"] == (ht - gt) % Q
    values, cexp, d, pi = M.prove_exponent(vectors, items, r, t, log_n, TAU)
    assert pi == ((sum(s * c for s, c in zip(p["s"], cexp)) - d - p["y"]) * pow((TAU - t) % Q, -1, Q)) % Q
    assert M.check_exponent(cexp, items, values, d, pi, r, t, log_n, TAU)


@pytest.mark.parametrize("log_n,nv,k", [(1, 1, 2), (3, 3, 7), (5, 3, 40)])
def test_the_equation_fails_for_every_tampering(log_n, nv, k):
    rnd = random.Random(3000 * log_n + k)
    n = 1 << log_n
    vectors, items = instance(log_n, nv, k, rnd)
    r, t = rnd.randrange(Q), rnd.randrange(Q)
    values, cexp, d, pi = M.prove_exponent(vectors, items, r, t, log_n, TAU)
    ok = lambda **kw: M.check_exponent(kw.get("c", cexp), kw.get("items", items), kw.get("values", values), kw.get("d", d), kw.get("pi", pi),
                                       r, t, log_n, TAU)
    assert ok()
    bad_values = list(values)
    bad_values[k // 2] = (bad_values[k // 2] + 1) % Q
    assert not ok(values=bad_values)
    j, m = items[0]
    assert not ok(items=[(j, (m + 1) % n)] + items[1:])
    if nv > 1:
        assert not ok(items=[((j + 1) % nv, m)] + items[1:])
    assert not ok(c=[(cexp[0] + 1) % Q] + cexp[1:])
    assert not ok(d=(d + 1) % Q)
    assert not ok(pi=(pi + 1) % Q)
    # two items swapped without proving again: the weights r^k belong to positions
    a, b = 0, k - 1
    if items[a] != items[b]:
        sw_items, sw_values = list(items), list(values)
        sw_items[a], sw_items[b] = sw_items[b], sw_items[a]
        sw_values[a], sw_values[b] = sw_values[b], sw_values[a]
        assert not ok(items=sw_items, values=sw_values)


def test_a_predictable_r_lets_two_false_items_cancel():
    """The voiding demonstration: with r and t known before the claims are made, two false values whose weighted errors cancel
    in y pass the equation with the honest proof; under the transcript the changed values change r and the forgery fails."""
    log_n, nv, k = 3, 2, 5
    rnd = random.Random(77)
    vectors, items = instance(log_n, nv, k, rnd)
    commitments = [K.scalar_commit(M.at_tau(e, log_n, TAU)) for e in vectors]
    values = M.values_of(vectors, items)

    def prove(claimed):
        tr, r = M.transcript_r(b"void", log_n, commitments, items, claimed)
        g = M.aggregate(vectors, items, r, log_n)
        t = M.transcript_t(tr, K.scalar_commit(M.at_tau(g, log_n, TAU)))
        return r, t

    r, t = prove(values)
    _, cexp, d, pi = M.prove_exponent(vectors, items, r, t, log_n, TAU)
    wt, _, _ = M.weights(items, values, r, t, log_n, nv)
    forged = list(values)
    forged[0] = (forged[0] + 1) % Q
    forged[1] = (forged[1] - wt[0] * pow(r * wt[1] % Q, -1, Q)) % Q
    assert forged != values
    assert M.check_exponent(cexp, items, forged, d, pi, r, t, log_n, TAU)           # the verifier was handed r and t
    r2, t2 = prove(forged)                                                           # what an honest verifier derives
    assert (r2, t2) != (r, t)
    assert not M.check_exponent(cexp, items, forged, d, pi, r2, t2, log_n, TAU)


# ---- kzg_multiproof_core.hpp ---------------------------------------------------------------------------------------------------------
def test_core_argument_checks_in_their_order(lib):
    E = M.ERR_ARG
    for host_form in (0, 1):
        for check in (0, 1):
            for log_n, nv, vi, mi in [(3, 2, [0, 1], [7, 0]), (3, 2, [2], [0]), (3, 2, [0], [8]), (1, 1, [0], [1]), (1, 1, [0], [2])]:
                assert lib.hkm_check_items(log_n, nv, u32s(vi), u32s(mi), len(vi), host_form, check) == \
                    M.check_items(log_n, nv, vi, mi, bool(host_form), bool(check)), (log_n, nv, vi, mi)
            for log_n, nv, k in [(3, 1, 0), (3, 1, 1 << 20), (3, 1, (1 << 20) + 1), (3, 0, 1), (3, 65536, 1), (3, 65537, 1),
                                 (12, 65536, 1), (13, 32768, 1), (13, 32769, 1), (20, 256, 1), (20, 257, 1), (0, 1, 1), (21, 1, 1)]:
                if log_n == 21 and host_form:
                    continue
                assert lib.hkm_check_counts(log_n, nv, k, host_form, check) == M.check_items(log_n, nv, [0] * k, [0] * k, bool(host_form), bool(check)), \
                    (log_n, nv, k, host_form, check)
    # the order: the counts before the indexes, the host cap last
    assert lib.hkm_check_items(3, 0, u32s([5]), u32s([9]), 1, 1, 1) == E
    assert lib.hkm_check_counts(20, 257, 1, 1, 0) == E and lib.hkm_check_counts(20, 257, 1, 0, 0) == 0
    assert lib.hkm_check_counts(0, 1, 1, 0, 1) == E and lib.hkm_check_counts(21, 1, 1, 0, 1) == E


def test_core_override_check(lib):
    log_n = 4
    w = M.domain_points(log_n)
    out = (ctypes.c_uint64 * 8)()
    assert lib.hkm_check_override(None, log_n, out) == 0
    for r, t, want in [(5, 9, 0), (0, 9, 0), (5, w[3], M.ERR_DATA), (5, 1, M.ERR_DATA), (5, 0, 0)]:
        assert lib.hkm_check_override(plonk_amd.fr_to_bytes_mont([r, t]), log_n, out) == want == M.check_override(r, t, log_n)
        if want == 0:
            assert plonk_amd.fr_from_bytes_mont(bytes(out)) == [r, t]
    raw_q = Q.to_bytes(32, "little")
    good = plonk_amd.fr_to_bytes_mont([5])
    assert lib.hkm_check_override(raw_q + good, log_n, out) == M.ERR_DATA
    assert lib.hkm_check_override(good + raw_q, log_n, out) == M.ERR_DATA
    assert lib.hkm_check_override(good + b"\xff" * 32, log_n, out) == M.ERR_DATA


@pytest.mark.parametrize("n,k", [(2, 1), (8, 1), (8, 40), (32, 7), (128, 200), (1 << 12, 5000)])
def test_core_sorts(lib, n, k):
    rnd = random.Random(n + k)
    for keys in ([rnd.randrange(n) for _ in range(k)], [n - 1] * k, [0] * k, [i % n for i in range(k)]):
        perm, off = (ctypes.c_uint32 * k)(), (ctypes.c_uint32 * (n + 1))()
        lib.hkm_counting_sort(u32s(keys), k, n, perm, off)
        want_perm, want_off = M.counting_sort(keys, n)
        assert (list(perm), list(off)) == (want_perm, want_off)
        gm, goff = (ctypes.c_uint32 * min(k, n))(), (ctypes.c_uint32 * (min(k, n) + 1))()
        groups = lib.hkm_sort_points(u32s(keys), k, n, perm, gm, goff)
        want_perm, want_gm, want_goff = M.sort_points(keys, n)
        assert groups == len(want_gm)
        assert (list(perm), list(gm)[:groups], list(goff)[:groups + 1]) == (want_perm, want_gm, want_goff)


def test_core_plan(lib):
    names = ["point_groups", "agg_launches", "agg_blocks", "waves", "partial_values", "products", "fold_launches", "commitments_computed",
             "msm_launches", "msm_terms", "stage_values"]
    for log_n in (1, 5, 10, 11, 17, 20):
        for nv, k, groups in [(1, 1, 1), (3, 40, 7), (64, 64, 64), (65, 65, 65), (16, 16384, 129), (65536, 1 << 20, 1)]:
            for compute in (0, 1):
                for host_form in (0, 1):
                    out = (ctypes.c_uint64 * 11)()
                    lib.hkm_plan(log_n, nv, k, groups, compute, host_form, out)
                    assert dict(zip(names, out)) == M.plan(log_n, nv, k, groups, bool(compute), bool(host_form))


def test_core_challenges_and_what_they_bind(lib):
    rnd = random.Random(11)
    log_n, nv = 4, 3
    commitments = [K.scalar_commit(rnd.randrange(1, Q)) for _ in range(nv)]
    items = [(rnd.randrange(nv), rnd.randrange(1 << log_n)) for _ in range(6)]
    values = [rnd.randrange(Q) for _ in items]
    d48 = K.scalar_commit(rnd.randrange(1, Q))

    def native(label, log_n, commitments, items, values, d48):
        out = ctypes.create_string_buffer(64)
        lib.hkm_challenges(label, len(label), log_n, b"".join(commitments), len(commitments), u32s([j for j, _ in items]),
                           u32s([m for _, m in items]), plonk_amd.fr_to_bytes_mont(values), len(items), d48, out)
        return int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")

    def model(label, log_n, commitments, items, values, d48):
        tr, r = M.transcript_r(label, log_n, commitments, items, values)
        return r, M.transcript_t(tr, d48)

    base = (b"label", log_n, commitments, items, values, d48)
    seen = {native(*base)}
    assert native(*base) == model(*base)
    assert native(b"", log_n, commitments[:1], [(0, 0)], [0], K.IDENTITY48) == model(b"", log_n, commitments[:1], [(0, 0)], [0], K.IDENTITY48)
    variants = [
        (b"labem",) + base[1:],
        (base[0], log_n + 1) + base[2:],
        base[:2] + (commitments[::-1],) + base[3:],
        base[:2] + (commitments + commitments[:1],) + base[3:],
        base[:3] + ([(items[0][0], items[0][1] ^ 1)] + items[1:],) + base[4:],
        base[:3] + ([((items[0][0] + 1) % nv, items[0][1])] + items[1:],) + base[4:],
        base[:3] + (items[::-1], values[::-1], d48),
        base[:3] + (items[:-1], values[:-1], d48),
        base[:4] + ([(values[0] + 1) % Q] + values[1:], d48),
    ]
    for v in variants:
        got = native(*v)
        assert got == model(*v)
        assert got[0] not in {s[0] for s in seen} and got[1] not in {s[1] for s in seen}, v
        seen.add(got)
    other_d = native(*base[:5], K.scalar_commit(3))
    assert other_d == model(*base[:5], K.scalar_commit(3))
    assert other_d[0] == native(*base)[0] and other_d[1] != native(*base)[1]          # D binds t alone
