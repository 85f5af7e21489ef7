"""CPU: the KZG10 cell recovery.  The big-int model tests/kzg_recover_model.py (the five steps with the kernels' index
arithmetic) is pinned to naive Lagrange interpolation through the a l given points and to oracle/fft.py (the transforms and the
coset of 7), for log_n 2..6, every cell size, every subset size a from ceil(d / l) to r up to log_n = 4 and sampled subsets
above; plonk_amd/csrc/kzg_recover_core.hpp (index maps, the checks in their order, the plan, the counts) is compiled with g++
(tests/csrc/host_kzg_recover.cpp) and checked against the same model."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle.fft import EvaluationDomain
from tests import kzg_cells_model as C
from tests import kzg_recover_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_recover.so")
Q = M.Q
NONE = (1 << 64) - 1
SHAPES = [(log_n, log_cell) for log_n in range(2, 7) for log_cell in range(1, log_n)]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_recover.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, i32p, u32p, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_int
    for name in ("hkr_scatter_src", "hkr_period", "hkr_point_exp", "hkr_tail_first"):
        getattr(lib, name).restype = u64
    lib.hkr_max_log_r.restype = u32
    lib.hkr_scatter_src.argtypes = [u32, u32, u64, i32p]
    lib.hkr_period.argtypes = [u32, u32, u64]
    lib.hkr_point_exp.argtypes = [u32, u64]
    lib.hkr_point_on_coset.argtypes = [u32, u64]
    lib.hkr_tail_first.argtypes = [u64]
    lib.hkr_check_args.argtypes = [ci, u32, u32, u64, u32p, u64, ci, ci, u64, ci]
    lib.hkr_check_degree.argtypes = [u32, u64, u64]
    lib.hkr_plan.argtypes = [u32, u32, u64, u64, u64, ci, ctypes.POINTER(u64)]
    lib.hkr_plan.restype = None
    return lib


def points_of(cell_ids, log_n, log_cell):
    """the a l domain points of the given cells, in the order of the packed values"""
    w, l, r = M.root(log_n), 1 << log_cell, 1 << (log_n - log_cell)
    return [pow(w, k + r * j, Q) for k in cell_ids for j in range(l)]


def lagrange(xs, ys):
    """the coefficients of the polynomial of degree < len(xs) through (xs, ys), naively: N(X) = prod (X - x_j), the basis
    polynomial of x_i is N / (X - x_i) / N'(x_i)"""
    m = len(xs)
    big = [1]
    for x in xs:
        nxt = [0] * (len(big) + 1)
        for i, c in enumerate(big):
            nxt[i + 1] = (nxt[i + 1] + c) % Q
            nxt[i] = (nxt[i] - c * x) % Q
        big = nxt
    out = [0] * m
    for x, y in zip(xs, ys):
        quo, carry = [0] * m, 0
        for i in range(m, 0, -1):                              # synthetic division of N by X - x
            carry = (big[i] + carry * x) % Q
            quo[i - 1] = carry
        den = C.evaluate(quo, x)
        s = y * pow(den, -1, Q) % Q
        for i in range(m):
            out[i] = (out[i] + s * quo[i]) % Q
    return out


def subsets(r, a, rnd, exhaustive):
    """cell sets of size a in shuffled order: a few shaped ones and random ones"""
    out = [list(range(a)), list(range(r - a, r))]
    for _ in range(3 if exhaustive else 2):
        ids = rnd.sample(range(r), a)
        out.append(ids)
    return out


def lengths(log_n, log_cell):
    n, l = 1 << log_n, 1 << log_cell
    return sorted({1, l - 1, l, l + 1, n // 2, n} - {0})


# ---- the transforms of the model are the oracle's --------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [2, 3, 4, 5, 6])
def test_model_transforms_are_the_oracles(log_n):
    n = 1 << log_n
    dom = EvaluationDomain(n)
    assert dom.group_gen == M.root(log_n)
    rnd = random.Random(log_n)
    v = [rnd.randrange(Q) for _ in range(n)]
    assert M.ntt(v, log_n) == dom.fft(v) and M.intt(v, log_n) == dom.ifft(v)
    assert M.coset_ntt(v, log_n) == dom.coset_fft(v) and M.coset_intt(v, log_n) == dom.coset_ifft(v)
    for log_cell in range(1, log_n):
        cells = M.cells_of(v, log_n, log_cell)
        assert cells == C.cells_horner(v, log_n, log_cell)


# ---- the five steps against the polynomial itself and against Lagrange interpolation ---------------------------------------
@pytest.mark.parametrize("log_n,log_cell", SHAPES)
def test_recovery_returns_the_polynomial_and_the_interpolant(log_n, log_cell):
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(100 * log_n + log_cell)
    exhaustive = log_n <= 4
    for d in lengths(log_n, log_cell):
        f = [rnd.randrange(1, Q) for _ in range(d)]
        cells = M.cells_of(f, log_n, log_cell)
        lo = -(-d // l)
        sizes = range(lo, r + 1) if exhaustive else sorted({lo, min(lo + 1, r), (lo + r) // 2, r})
        for a in sizes:
            for ids in subsets(r, a, rnd, exhaustive):
                vals = M.packed(cells, ids, log_cell)
                g, flag = M.recover(ids, vals, log_n, log_cell, d)
                assert (g, flag) == (f + [0] * (n - d), 0), (d, ids)
                assert M.cells_of(g, log_n, log_cell) == cells
                if a * l > d:                                  # redundancy: one changed value is always detected
                    bad = list(vals)
                    at = rnd.randrange(len(bad))
                    bad[at] = (bad[at] + 1 + rnd.randrange(Q - 1)) % Q
                    assert M.recover(ids, bad, log_n, log_cell, d)[1] == 1, (d, ids, at)
                    if d < n:                                  # a polynomial of d + 1 coefficients presented with max_len = d
                        f1 = f + [rnd.randrange(1, Q)]
                        v1 = M.packed(M.cells_of(f1, log_n, log_cell), ids, log_cell)
                        assert M.recover(ids, v1, log_n, log_cell, d)[1] == 1
                        if a * l >= d + 1:
                            assert M.recover(ids, v1, log_n, log_cell, d + 1) == (f1 + [0] * (n - d - 1), 0)
    # no redundancy: every input is consistent and the result is the interpolant through the a l points
    for a in (range(1, r + 1) if exhaustive else sorted({1, r // 2, r - 1, r})):
        for ids in subsets(r, a, rnd, exhaustive)[1:4]:
            vals = [rnd.randrange(Q) for _ in range(a * l)]
            g, flag = M.recover(ids, vals, log_n, log_cell, a * l)
            assert flag == 0 and g[a * l:] == [0] * (n - a * l)
            assert g[:a * l] == lagrange(points_of(ids, log_n, log_cell), vals), ids
            assert M.packed(M.cells_of(g, log_n, log_cell), ids, log_cell) == vals


def test_the_vanishing_values_are_those_of_the_product_polynomial():
    """Z(X) = prod_(m in M) (X^l - phi^m) evaluated by Horner at w^(k + r j) and at 7 w^i: constant on a cell, periodic on the coset"""
    for log_n, log_cell in [(3, 1), (4, 2), (5, 2), (6, 1)]:
        n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
        w, phi = M.root(log_n), pow(M.root(log_n), l, Q)
        rnd = random.Random(log_n)
        for nm in sorted({0, 1, r // 2, r - 1}):
            miss = sorted(rnd.sample(range(r), nm))
            z = [1]
            for m in miss:                                     # times (X^l - phi^m)
                nxt = [0] * (len(z) + l)
                for i, c in enumerate(z):
                    nxt[i + l] = (nxt[i + l] + c) % Q
                    nxt[i] = (nxt[i] - c * pow(phi, m, Q)) % Q
                z = nxt
            zdom, zcoset = M.vanish(log_n, log_cell, miss)
            for i in range(n):
                assert C.evaluate(z, pow(w, i, Q)) == zdom[M.period(log_n, log_cell, i)]
                assert C.evaluate(z, M.GEN * pow(w, i, Q) % Q) == zcoset[M.period(log_n, log_cell, i)] != 0
            assert [k for k in range(r) if zdom[k] == 0] == miss


# ---- kzg_recover_core.hpp against the model ---------------------------------------------------------------------------------
def test_core_index_maps(lib):
    assert lib.hkr_max_log_r() == M.MAX_LOG_R and lib.hkr_vanish_slices() == M.VANISH_SLICES
    assert [lib.hkr_vanish_first(s) for s in range(M.VANISH_SLICES)] == [list(range(100))[s::M.VANISH_SLICES][0] for s in range(M.VANISH_SLICES)]
    rnd = random.Random(1)
    for log_n, log_cell in SHAPES + [(12, 6), (12, 1), (13, 2), (20, 9)]:
        n, r = 1 << log_n, 1 << (log_n - log_cell)
        ids = rnd.sample(range(r), max(r // 2, 1))
        slot = M.slot_table(r, ids)
        assert sorted(M.missing_list(slot) + ids) == list(range(r))
        arr = (ctypes.c_int32 * r)(*slot)
        idx = range(n) if n <= 64 else [0, 1, r - 1, r, r + 1, n // 2, n - r, n - 1] + [rnd.randrange(n) for _ in range(32)]
        seen = []
        for i in idx:
            want = M.scatter_src(log_n, log_cell, i, slot)
            assert lib.hkr_scatter_src(log_n, log_cell, i, arr) == (NONE if want is None else want)
            assert lib.hkr_period(log_n, log_cell, i) == M.period(log_n, log_cell, i) == i % r
            if want is not None:
                seen.append(want)
        if n <= 64:
            assert sorted(seen) == list(range(len(ids) << log_cell))      # every packed value is read exactly once
        for p in (0, 1, r - 1, r, 2 * r - 1):
            assert lib.hkr_point_exp(log_n - log_cell, p) == M.point_exp(log_n - log_cell, p)
            assert bool(lib.hkr_point_on_coset(log_n - log_cell, p)) == M.point_on_coset(log_n - log_cell, p) == (p >= r)
    for d in (1, 5, 1 << 20):
        assert lib.hkr_tail_first(d) == M.tail_first(d) == d


def call_args(lib, has_domain, log_n, log_cell, count, ids, available, has_values, all_set, max_len, any_output):
    arr = None if ids is None else (ctypes.c_uint32 * max(len(ids), 1))(*ids)
    return lib.hkr_check_args(int(has_domain), log_n, log_cell, count, arr, available, int(has_values), int(all_set), max_len, int(any_output))


def test_core_checks_in_their_order(lib):
    good = dict(has_domain=True, log_n=6, log_cell=3, count=2, ids=[5, 0, 3], available=3, has_values=True, all_set=True, max_len=24,
                any_output=True)

    def both(**kw):
        a = dict(good, **kw)
        got = call_args(lib, a["has_domain"], a["log_n"], a["log_cell"], a["count"], a["ids"], a["available"], a["has_values"], a["all_set"],
                        a["max_len"], a["any_output"])
        want = M.check_args(a["has_domain"], a["log_n"], a["log_cell"], a["count"], a["ids"], a["available"], a["has_values"], a["all_set"],
                            a["max_len"], a["any_output"])
        assert got == want, kw
        return got

    assert both() == M.OK
    assert both(has_domain=False) == M.ERR_ARG
    for lc in (0, 6, 7, 64, 0xffffffff):
        assert both(log_cell=lc) == M.ERR_ARG
    assert both(log_n=13, log_cell=2) == M.OK and both(log_n=13, log_cell=1) == M.ERR_ARG        # r = 2048 is the cap
    assert both(log_n=20, log_cell=9) == M.OK and both(log_n=20, log_cell=8) == M.ERR_ARG
    assert both(count=65536) == M.OK and both(count=65537) == M.ERR_ARG
    assert both(available=0, ids=[]) == M.ERR_ARG and both(available=9, ids=list(range(8)) + [0]) == M.ERR_ARG
    assert both(available=8, ids=list(range(8))) == M.OK
    assert both(ids=[5, 8, 3]) == M.ERR_ARG and both(ids=[5, 3, 5]) == M.ERR_ARG and both(ids=[5, 0xffffffff, 3]) == M.ERR_ARG
    assert both(ids=None) == M.ERR_ARG and both(has_values=False, all_set=False) == M.ERR_ARG and both(all_set=False) == M.ERR_ARG
    assert both(ids=None, has_values=False, all_set=False, count=0) == M.OK                       # NULL arrays are legal with count == 0
    assert both(ids=[5, 5, 3], count=0) == M.ERR_ARG
    assert both(max_len=0) == M.ERR_ARG and both(max_len=65) == M.ERR_ARG and both(max_len=64) == M.OK
    assert both(any_output=False) == M.ERR_ARG and both(any_output=False, count=0) == M.ERR_ARG
    # the degree check comes after the arguments (and the state): too few cells for that length
    for lc, a, d in [(3, 3, 24), (3, 3, 25), (3, 1, 8), (3, 1, 9), (1, 5, 10), (1, 5, 11)]:
        assert lib.hkr_check_degree(lc, a, d) == M.check_degree(lc, a, d) == (M.ERR_DEGREE if d > (a << lc) else M.OK)
    # the whole order in the model: ARG before STATE before count == 0 before DEGREE before DATA
    assert M.check_call(True, 6, 3, 2, [1, 1], 2, True, True, 64, True, state_ok=False, canonical=False) == M.ERR_ARG
    assert M.check_call(True, 6, 3, 2, [1, 2], 2, True, True, 64, True, state_ok=False, canonical=False) == M.ERR_STATE
    assert M.check_call(True, 6, 3, 0, [1, 2], 2, True, True, 64, True, canonical=False) == M.OK
    assert M.check_call(True, 6, 3, 2, [1, 2], 2, True, True, 64, True, canonical=False) == M.ERR_DEGREE
    assert M.check_call(True, 6, 3, 2, [1, 2], 2, True, True, 16, True, canonical=False) == M.ERR_DATA
    assert M.check_call(True, 6, 3, 2, [1, 2], 2, True, True, 16, True) == M.OK


def test_core_plan_and_counts(lib):
    out = (ctypes.c_uint64 * 7)()
    names = ["missing", "chunk_polys", "chunks", "ws_bytes", "passes", "transforms", "vanish_muls"]
    for log_n, log_cell in SHAPES + [(12, 6), (12, 1), (13, 2), (16, 6), (20, 9), (20, 10)]:
        n, r = 1 << log_n, 1 << (log_n - log_cell)
        per_poly = 3 * n * 32
        for count in (0, 1, 2, 3, 5, 16, 4096, 4097, 65536):
            for a in sorted({1, r // 2, r}):
                for cap in (0, 1, per_poly, 2 * per_poly, 3 * per_poly - 1, M.WS_CAP_DEFAULT, 1 << 44):
                    for want in (False, True):
                        lib.hkr_plan(log_n, log_cell, count, a, cap, int(want), out)
                        p = M.plan(log_n, log_cell, count, a, cap, want)
                        assert list(out) == [p[k] for k in names], (log_n, log_cell, count, a, cap, want)
                        if count:
                            assert 1 <= p["chunk_polys"] <= M.MAX_CHUNK and p["chunks"] * p["chunk_polys"] >= count
                            assert p["ws_bytes"] <= max(cap, per_poly)
    # caps that force 1, 2 and 3 chunks of five polynomials at log_n 6: one pass, then two
    per = 3 * 64 * 32
    plans = [M.plan(6, 3, 5, 4, cap) for cap in (5 * per, 3 * per, 2 * per)]
    assert [p["chunks"] for p in plans] == [1, 2, 3] and [p["passes"] for p in plans] == [1, 2, 2]
    assert [p["transforms"] for p in plans] == [5 * 4, 5 * 7, 5 * 7]
    assert M.plan(6, 3, 5, 4, want_values=False)["transforms"] == 15
    assert M.plan(12, 1, 1, 1024)["vanish_muls"] == 2 * 2048 * 1024 and M.plan(6, 3, 1, 8)["vanish_muls"] == 0
