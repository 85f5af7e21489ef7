"""CPU: the KZG10 cell proofs in the exponent.  The big-int model tests/kzg_cells_model.py (the steps with the kernels' index
arithmetic, the slice split and the reduction order) is pinned to the closed form — proof k is
[(f(tau) - r_k(tau)) / (tau^l - x_k)] g — to the naive sum over H_m, to both forms of the remainder's coefficients c_j and to
the cell-major order by Horner evaluation, for log_n 2..6, every cell size, every length 0..n up to log_n = 4 and the lengths
{0, 1, l-1, l, l+1, n-1, n} above; plonk_amd/csrc/kzg_cells_core.hpp (index maps, slice split, plan, counts, the argument
check) is compiled with g++ (tests/csrc/host_kzg_cells.cpp) and checked against the same model."""
import ctypes
import os
import random
import subprocess

import pytest

from tests import kzg_cells_model as M
from tests import kzg_domain_model as D
from tests import kzg_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_cells.so")
Q = M.Q
NONE = (1 << 64) - 1
SHAPES = [(log_n, log_cell) for log_n in range(2, 7) for log_cell in range(1, log_n)]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_cells.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    for name in ("hkc_fill_lanes", "hkc_a_src", "hkc_g_src", "hkc_cell_dst", "hkc_slice_terms", "hkc_slice_first", "hkc_partial_slot"):
        getattr(lib, name).restype = u64
    lib.hkc_check_cell.argtypes = [u32, u32]
    lib.hkc_a_src.argtypes = [u32, u64, u64, u64]
    lib.hkc_g_src.argtypes = [u32, u64, u64, u64]
    lib.hkc_cell_dst.argtypes = [u32, u32, u64]
    lib.hkc_slice_terms.argtypes = [u32, u64]
    lib.hkc_slice_first.argtypes = [u32, u64, u64]
    lib.hkc_partial_slot.argtypes = [u64, u64, u64]
    lib.hkc_plan.argtypes = [u32, u32, u64, u64, u64, ctypes.POINTER(u64)]
    lib.hkc_plan.restype = None
    return lib


def key(n, tau=K.TAU):
    return [pow(tau, i, Q) for i in range(n)]


def lengths(log_n, log_cell):
    n, l = 1 << log_n, 1 << log_cell
    return list(range(n + 1)) if log_n <= 4 else sorted({0, 1, l - 1, l, l + 1, n - 1, n})


# ---- the model against the closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_cell", SHAPES)
def test_steps_equal_the_closed_form_the_naive_sum_and_horner_at_every_length(log_n, log_cell):
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(100 * log_n + log_cell)
    k_ = key(n)
    table = M.tables(log_n, log_cell, k_)
    x, shift = M.cell_points(log_n, log_cell)
    assert len(set(x)) == r and all((pow(K.TAU, l, Q) - xk) % Q for xk in x)
    for length in lengths(log_n, log_cell):
        f = [rnd.randrange(1, Q) for _ in range(length)]
        counts = [0, 0]
        cells, proofs = M.steps(f, log_n, log_cell, k_, 1, counts, table)
        assert proofs == [M.proof_closed_form(f, log_n, log_cell, k, K.TAU) for k in range(r)], length
        assert proofs == M.proofs_naive(f, log_n, log_cell, k_), length
        assert cells == M.cells_horner(f, log_n, log_cell), length
        p = M.plan(log_n, log_cell, 1)
        assert counts == [p["stage_launches"], p["scalar_muls"]]
        if length <= l:
            assert proofs == [0] * r
        for k in {0, 1, r - 1}:                                # both forms of the remainder
            c = M.remainder_coeffs(f, log_n, log_cell, k)
            assert c == M.remainder_from_cell(cells[k * l:(k + 1) * l], log_n, log_cell, k), (length, k)
            if length <= l:
                assert c == f + [0] * (l - length)
            # the remainder interpolates the cell: r_k(shift_k * (w^r)^j) = cells[k l + j]
            wr = pow(M.root(log_n), r, Q)
            assert [M.evaluate(c, shift[k] * pow(wr, j, Q) % Q) for j in range(l)] == cells[k * l:(k + 1) * l]


@pytest.mark.parametrize("log_n,log_cell", [(4, 1), (4, 2), (4, 3), (6, 3)])
def test_every_admissible_slice_count_gives_the_same_sums(log_n, log_cell):
    n, l = 1 << log_n, 1 << log_cell
    rnd = random.Random(log_n)
    f = [rnd.randrange(Q) for _ in range(n)]
    k_ = key(n)
    table = M.tables(log_n, log_cell, k_)
    want = M.steps(f, log_n, log_cell, k_, 1, None, table)
    S = 2
    while S <= l:
        counts = [0, 0]
        assert M.steps(f, log_n, log_cell, k_, S, counts, table) == want
        p = M.plan(log_n, log_cell, 1, forced_slices=S)
        assert p["slices"] == S and counts == [p["stage_launches"], p["scalar_muls"]]
        S *= 2
    # the slices partition the terms in order
    for S in (1, 2, l):
        assert [M.slice_first(log_cell, S, s) + t for s in range(S) for t in range(M.slice_terms(log_cell, S))] == list(range(l))


def test_shaped_polynomials_in_the_model():
    for log_n, log_cell in [(3, 1), (3, 2), (4, 2), (6, 3)]:
        n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
        k_ = key(n)
        table = M.tables(log_n, log_cell, k_)
        x, _ = M.cell_points(log_n, log_cell)
        for u in (0, l - 1):
            for t in (0, r - 1):                               # a single coefficient at u + l t
                f = [0] * (u + l * t) + [1]
                cells, proofs = M.steps(f, log_n, log_cell, k_, 1, None, table)
                assert proofs == [M.proof_closed_form(f, log_n, log_cell, k, K.TAU) for k in range(r)]
                assert cells == M.cells_horner(f, log_n, log_cell)
        for k in (0, 1, r - 1):                                # f = X^l - x_k: proof k is [1] g and cell k is zero
            f = [(-x[k]) % Q] + [0] * (l - 1) + [1]
            cells, proofs = M.steps(f, log_n, log_cell, k_, 1, None, table)
            assert proofs[k] == 1 and cells[k * l:(k + 1) * l] == [0] * l
            assert proofs == [M.proof_closed_form(f, log_n, log_cell, j, K.TAU) for j in range(r)]


def test_degenerate_key_in_the_model():
    """tau = (2n-th root of unity)^3: tau^n = -1, and no tau^l - x_k vanishes since x_k^r = 1 while (tau^l)^r = -1"""
    for log_n in (3, 4):
        n = 1 << log_n
        tau = pow(M.root(log_n + 1), 3, Q)
        assert pow(tau, n, Q) == Q - 1
        k_ = key(n, tau)
        rnd = random.Random(log_n)
        f = [rnd.randrange(Q) for _ in range(n)]
        for log_cell in range(1, log_n):
            l, r = 1 << log_cell, 1 << (log_n - log_cell)
            x, _ = M.cell_points(log_n, log_cell)
            assert all((pow(tau, l, Q) - xk) % Q for xk in x)
            _, proofs = M.steps(f, log_n, log_cell, k_)
            assert proofs == [M.proof_closed_form(f, log_n, log_cell, k, tau) for k in range(r)]


def test_the_verifier_equation_in_the_exponent():
    """proof_k tau^l == C - r_k(tau) + x_k proof_k: what e(proof_k, [tau^l] h) == e(C - commit(r_k) + x_k proof_k, h) states"""
    log_n, log_cell = 5, 2
    n, l, r = 32, 4, 8
    rnd = random.Random(9)
    f = [rnd.randrange(Q) for _ in range(n)]
    cells, proofs = M.steps(f, log_n, log_cell, key(n))
    x, _ = M.cell_points(log_n, log_cell)
    C = M.evaluate(f, K.TAU)
    for k in range(r):
        c = M.remainder_from_cell(cells[k * l:(k + 1) * l], log_n, log_cell, k)
        assert proofs[k] * pow(K.TAU, l, Q) % Q == (C - M.evaluate(c, K.TAU) + x[k] * proofs[k]) % Q


# ---- kzg_cells_core.hpp against the model -----------------------------------------------------------------------------------
def test_core_index_maps(lib):
    assert lib.hkc_fill_lanes() == M.FILL_LANES
    for log_n, log_cell in SHAPES + [(12, 6), (14, 13), (14, 1)]:
        l, r = 1 << log_cell, 1 << (log_n - log_cell)
        us = sorted({0, 1, l // 2, l - 1})
        vs = sorted({0, 1, r - 2, r - 1, r, 2 * r - 1}) if r > 64 else range(2 * r)
        for u in us:
            for v in vs:
                a, g = M.a_src(log_cell, r, u, v), M.g_src(log_cell, r, u, v)
                assert lib.hkc_a_src(log_cell, r, u, v) == (NONE if a is None else a)
                assert lib.hkc_g_src(log_cell, r, u, v) == (NONE if g is None else g)
                assert a is None or a < (1 << log_n) - l and (g is None or l <= g < (1 << log_n))
        n = 1 << log_n
        idx = range(n) if n <= 64 else [0, 1, r - 1, r, n // 2, n - 1]
        dst = [lib.hkc_cell_dst(log_n, log_cell, i) for i in idx]
        assert dst == [M.cell_dst(log_n, log_cell, i) for i in idx]
        if n <= 64:
            assert sorted(dst) == list(range(n))
        S = 1
        while S <= l:
            assert lib.hkc_slice_terms(log_cell, S) == M.slice_terms(log_cell, S)
            for s in {0, S // 2, S - 1}:
                assert lib.hkc_slice_first(log_cell, S, s) == M.slice_first(log_cell, S, s)
                for p in (0, 2 * r - 1):
                    assert lib.hkc_partial_slot(r, s, p) == M.partial_slot(r, s, p) < S * 2 * r
            S *= 2


def test_core_plan(lib):
    out = (ctypes.c_uint64 * 7)()
    names = ["slices", "chunk_polys", "chunks", "ws_bytes", "table_bytes", "stage_launches", "scalar_muls"]
    for log_n, log_cell in SHAPES + [(12, 6), (13, 6), (14, 13), (14, 1), (16, 6), (20, 6), (20, 10)]:
        l, r = 1 << log_cell, 1 << (log_n - log_cell)
        forced = [0] + [1 << s for s in range(log_cell + 1)] + [3, 2 * l]        # every admissible S; 3 and 2l are ignored
        for count in (0, 1, 2, 3, 5, 16, 4096, 4097, 65536):
            for S in forced:
                own = M.plan(log_n, log_cell, count, forced_slices=S)
                per_poly = own["slices"] * 2 * r * 256
                for cap in (0, 1, per_poly, 2 * per_poly, 3 * per_poly - 1, M.WS_CAP_DEFAULT, 1 << 40):
                    lib.hkc_plan(log_n, log_cell, count, cap, S, out)
                    p = M.plan(log_n, log_cell, count, cap, S)
                    assert list(out) == [p[k] for k in names], (log_n, log_cell, count, S, cap)
                    assert p["slices"] <= l and l % p["slices"] == 0
                    if count:
                        assert 1 <= p["chunk_polys"] <= M.MAX_CHUNK and p["chunks"] * p["chunk_polys"] >= count
                        assert p["ws_bytes"] <= max(cap, per_poly)
    # caps that force 1, 2 and 3 chunks of five polynomials at log_n 6 / log_cell 3
    per = M.plan(6, 3, 5)["slices"] * 2 * 8 * 256
    assert [M.plan(6, 3, 5, cap)["chunks"] for cap in (5 * per, 3 * per, 2 * per)] == [1, 2, 3]
    # S fills the chip and goes no further
    assert M.plan(16, 6, 1)["slices"] == 32 and M.plan(16, 6, 16)["slices"] == 2 and M.plan(20, 6, 1)["slices"] == 2
    assert M.plan(20, 10, 1)["slices"] == 32 and M.plan(12, 6, 1)["slices"] == 64 and M.plan(14, 13, 1)["slices"] == 8192
    assert M.plan(16, 6, 1)["scalar_muls"] == 2 * 65536 + D.transform_muls(11) + D.transform_muls(10)


def test_core_argument_check(lib):
    for log_n in range(0, 22):
        for log_cell in (0, 1, 2, log_n - 2, log_n - 1, log_n, log_n + 1, 31, 0xffffffff):
            if log_cell < 0:
                continue
            assert lib.hkc_check_cell(log_n, log_cell) == M.check_cell(log_n, log_cell), (log_n, log_cell)
    assert all(M.check_cell(1, c) == M.ERR_ARG for c in range(0, 5))
    assert M.check_cell(2, 1) == M.OK and M.check_cell(20, 19) == M.OK and M.check_cell(20, 20) == M.ERR_ARG
