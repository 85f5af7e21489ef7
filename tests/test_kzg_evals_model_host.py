"""CPU: KZG10 in evaluation form in the exponent.  The big-int model tests/kzg_evals_model.py (shared inverses, lane m, y_j,
F, Y, q with the kernels' formulas) is pinned to the oracle: its q must be the values on the domain of the oracle's ifft,
folded and divided by (X - z) in coefficient form (tests/kzg_ref.py ruffini), and its y_j must be Horner evaluations — for every
n from 2 to 32, count 1 and 3, z random, 0, 1, w^(n-1) and w^(n/2).  plonk_amd/csrc/kzg_evals_core.hpp (argument checks, launch
geometry, plan, in-domain test, the factor of the barycentric sum) is compiled with g++ (tests/csrc/host_kzg_evals.cpp, like
tests/csrc/host_kzg_domain.cpp) and checked against the same model."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

from oracle.fft import EvaluationDomain
from tests import kzg_evals_model as M
from tests import kzg_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_evals.so")
Q = M.Q
LOGS = [1, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_evals.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.hke_const.restype = u64
    lib.hke_const.argtypes = [ci]
    for name in ("hke_fold_waves", "hke_fold_blocks", "hke_quotient_blocks"):
        getattr(lib, name).restype = u32
        getattr(lib, name).argtypes = [u64]
    lib.hke_in_domain.argtypes = [ctypes.POINTER(u64), u32]
    lib.hke_eval_scale.argtypes = [ctypes.POINTER(u64), u32, ctypes.POINTER(u64)]
    lib.hke_eval_scale.restype = None
    lib.hke_plan.argtypes = [u32, u64, ci, ci, ci, ctypes.POINTER(u64)]
    lib.hke_plan.restype = None
    lib.hke_check_commit.argtypes = [ci, ci, ci, u64]
    lib.hke_check_open.argtypes = [ci, ci, ci, ci, ci, u64]
    return lib


def points_of(log_n, rnd):
    n = 1 << log_n
    w = M.root(log_n)
    return [rnd.randrange(2, Q), 0, 1, pow(w, n - 1, Q), pow(w, n // 2, Q)]


# ---- the model against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("count", [1, 3])
def test_model_equals_ifft_fold_ruffini_and_horner(log_n, count):
    n = 1 << log_n
    rnd = random.Random(100 * log_n + count)
    dom = EvaluationDomain(n)
    pts = M.domain_points(log_n)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(count)]
    coeffs = [dom.ifft(e) for e in vectors]
    for p, e in zip(coeffs, vectors):
        assert [K.evaluate(p, x) for x in pts] == e              # the oracle's domain is the model's
    v = rnd.randrange(Q) if count > 1 else 1
    for z in points_of(log_n, rnd):
        s = M.scalar_stage(vectors, z, v, log_n)
        assert s["y"] == [K.evaluate(p, z) for p in coeffs], z
        folded = K.fold(coeffs, v)
        assert s["F"] == [K.evaluate(folded, x) for x in pts]
        assert s["Y"] == K.evaluate(folded, z)
        quotient = K.ruffini(folded, z)
        assert s["q"] == [K.evaluate(quotient, x) for x in pts], z
        assert (s["m"] != M.NONE) == M.in_domain(z, log_n)
        if s["m"] != M.NONE:
            assert pts[s["m"]] == z and s["inv"][s["m"]] == 0
        for i, x in enumerate(pts):
            if i != s["m"]:
                assert s["inv"][i] * (x - z) % Q == 1


def test_model_shaped_vectors():
    """all zero, constant (zero quotient), q - 1 everywhere, a single non-zero value at the lane m"""
    for log_n in (1, 3, 5):
        n = 1 << log_n
        pts = M.domain_points(log_n)
        dom = EvaluationDomain(n)
        for m in (0, n - 1):
            single = [0] * n
            single[m] = 5
            for e in ([0] * n, [7] * n, [Q - 1] * n, single):
                for z in (pts[m], 12345):
                    s = M.scalar_stage([e], z, 1, log_n)
                    p = dom.ifft(e)
                    assert s["y"] == [K.evaluate(p, z)]
                    assert s["q"] == [K.evaluate(K.ruffini(p, z), x) for x in pts]
                    if len(set(e)) == 1:
                        assert s["q"] == [0] * n


def test_lagrange_scalars_commit_to_the_polynomial():
    rnd = random.Random(5)
    for log_n in LOGS:
        n = 1 << log_n
        lag = M.lagrange_at(K.TAU, log_n)
        e = [rnd.randrange(Q) for _ in range(n)]
        p = EvaluationDomain(n).ifft(e)
        assert sum(a * b for a, b in zip(e, lag)) % Q == K.evaluate(p, K.TAU)
        pts = M.domain_points(log_n)
        assert M.lagrange_at(pts[n - 1], log_n) == [0] * (n - 1) + [1]


# ---- kzg_evals_core.hpp against the model ------------------------------------------------------------------------------------
def limbs(x):
    return (ctypes.c_uint64 * 4)(*[(x >> (64 * i)) & (2**64 - 1) for i in range(4)])


def test_constants_and_geometry(lib):
    assert [lib.hke_const(i) for i in range(8)] == [M.MAX_COUNT, M.GROUP, M.FOLD_T, M.FOLD_E, M.Q_T, M.STAGE_MIN, M.POINT_BYTES, M.NONE]
    for n in (1, 2, 63, 64, 1023, 1024, 1025, 2048, 2049, 1 << 20):
        blocks = (n + M.FOLD_BLOCK - 1) // M.FOLD_BLOCK
        assert lib.hke_fold_blocks(n) == blocks and lib.hke_fold_waves(n) == blocks * (M.FOLD_T // 64)
        assert lib.hke_quotient_blocks(n) == (n + M.Q_T - 1) // M.Q_T


def test_in_domain_and_eval_scale(lib):
    rnd = random.Random(9)
    for log_n in (1, 2, 5, 10, 20):
        n = 1 << log_n
        w = M.root(log_n)
        for z in [rnd.randrange(Q), 0, 1, Q - 1, w, pow(w, n - 1, Q), pow(w, n // 2, Q), M.root(log_n + 1)]:
            assert bool(lib.hke_in_domain(limbs(z), log_n)) == M.in_domain(z, log_n), (log_n, z)
            out = (ctypes.c_uint64 * 4)()
            lib.hke_eval_scale(limbs(z), log_n, out)
            assert sum(out[i] << (64 * i) for i in range(4)) == M.eval_scale(z, log_n), (log_n, z)


def test_plan(lib):
    for log_n, count, cm, wit, host in itertools.product((1, 5, 10, 15, 16, 17, 20), (0, 1, 3, 64, 65, 200, 65536), (0, 1), (0, 1), (0, 1)):
        out = (ctypes.c_uint64 * 6)()
        lib.hke_plan(log_n, count, cm, wit, host, out)
        p = M.plan(log_n, count, bool(cm), bool(wit), bool(host))
        assert list(out) == [p["group_vectors"], p["groups"], p["stage_values"], p["msm_launches"], p["msm_terms"], p["lagrange_bytes"]]
    assert M.plan(17, 5, True, True, True)["group_vectors"] == 1 and M.plan(10, 200, False, True, True)["group_vectors"] == 64
    assert M.plan(16, 5, False, False, False)["lagrange_bytes"] == 0


def test_argument_checks(lib):
    for flags in itertools.product((0, 1), repeat=3):
        for count in (0, 1, 2, 65536, 65537):
            assert lib.hke_check_commit(*flags, count) == M.check_commit(*map(bool, flags), count)
    for flags in itertools.product((0, 1), repeat=5):
        for count in (0, 1, 2, 65536, 65537):
            assert lib.hke_check_open(*flags, count) == M.check_open(*map(bool, flags), count)
    assert lib.hke_check_open(1, 1, 1, 0, 1, 1) == 0 and lib.hke_check_open(1, 1, 1, 0, 1, 2) == M.ERR_ARG
    assert lib.hke_check_open(1, 0, 1, 0, 0, 0) == 0 and lib.hke_check_commit(1, 0, 0, 0) == 0
