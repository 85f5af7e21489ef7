"""CPU: the whole-domain KZG10 openings in the exponent.  The big-int model tests/kzg_domain_model.py (the six steps with the
kernels' index arithmetic) is pinned to the closed form of tests/kzg_ref.py — witness i is [(f(tau) - f(w^i)) / (tau - w^i)] g —
and to its own naive Toeplitz sum, for every n in {2, 4, 8, 16, 32} and every length 0..n; plonk_amd/csrc/kzg_domain_core.hpp
(index maps, twiddle selection, chunk plan, workspace bytes, operation counts, argument validation) is compiled with g++
(tests/csrc/host_kzg_domain.cpp, like tests/csrc/host_kzg.cpp) and checked against the same model."""
import ctypes
import os
import random
import subprocess

import pytest

from tests import kzg_domain_model as M
from tests import kzg_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_domain.so")
Q = M.Q
NONE = (1 << 64) - 1
LOGS = [1, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_domain.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    for name in ("hkd_const", "hkd_rev", "hkd_g_src", "hkd_h_src", "hkd_twiddle", "hkd_stage_muls", "hkd_transform_muls"):
        getattr(lib, name).restype = u64
    lib.hkd_const.argtypes = [ci]
    lib.hkd_rev.argtypes = [u64, u32]
    lib.hkd_g_src.argtypes = [u64, u64]
    lib.hkd_h_src.argtypes = [u64, u64]
    lib.hkd_twiddle.argtypes = [u32, u64, u64, u32, ci, ctypes.POINTER(ci)]
    lib.hkd_stage_muls.argtypes = [u32, u64]
    lib.hkd_transform_muls.argtypes = [u32]
    lib.hkd_plan.argtypes = [u32, u64, u64, ctypes.POINTER(u64)]
    lib.hkd_plan.restype = None
    lib.hkd_check_create.argtypes = [u32, ci, ci, u64]
    lib.hkd_check_len.argtypes = [u32, u64]
    return lib


def key(n):
    return [pow(K.TAU, i, Q) for i in range(n)]


# ---- the model against the closed form and against its own definition --------------------------------------------------
@pytest.mark.parametrize("log_n", LOGS)
def test_six_steps_equal_the_closed_form_and_the_naive_toeplitz_sum_at_every_length(log_n):
    n = 1 << log_n
    rnd = random.Random(1000 + log_n)
    pts = M.domain_points(log_n)
    assert len(set(pts)) == n and pow(pts[1], n, Q) == 1 and K.TAU not in pts
    for length in range(n + 1):
        f = [rnd.randrange(1, Q) for _ in range(length)]
        counts = [0, 0]
        ev, pi = M.six_steps(f, log_n, key(n), counts)
        assert ev == [K.evaluate(f, z) for z in pts]
        assert pi == [K.witness_scalar([f], z, 1) for z in pts]
        assert pi == M.witnesses_naive(f, log_n, key(n))
        p = M.plan(log_n, 1)
        assert counts == [p["stage_launches"], p["scalar_muls"]]
        if length <= 1:
            assert pi == [0] * n


def test_shaped_polynomials_in_the_model():
    for log_n in (2, 3, 4):
        n = 1 << log_n
        pts = M.domain_points(log_n)
        shapes = {"x^(n-1)": [0] * (n - 1) + [1], "x - 1": [Q - 1, 1], "x^(n-1) - x^(n-3)": [0] * (n - 3) + [Q - 1, 0, 1],
                  "padded": [5, 7, 0, 0][:n], "q - 1": [Q - 1] * n}
        for name, f in shapes.items():
            ev, pi = M.six_steps(f, log_n, key(n))
            assert pi == [K.witness_scalar([f], z, 1) for z in pts], name
            assert ev == [K.evaluate(f, z) for z in pts], name
        assert M.six_steps(shapes["x - 1"], log_n, key(n))[0][0] == 0
        # x^(n-1) - x^(n-3): G_0 = g(1) = 0 and G_n = g(-1) = 0, so identities enter the inverse transform
        f = shapes["x^(n-1) - x^(n-3)"]
        g = [f[M.g_src(n, t)] if M.g_src(n, t) is not None else 0 for t in range(2 * n)]
        G = M.dft(g, M.root(log_n + 1))
        assert G[0] == 0 and G[n] == 0


def test_degenerate_key_in_the_model():
    """tau = (2n-th root of unity)^3: a key whose transform A holds identities; the closed form still holds"""
    for log_n in (3, 4):
        n = 1 << log_n
        tau = pow(M.root(log_n + 1), 3, Q)
        pts = M.domain_points(log_n)
        assert tau not in pts
        k = [pow(tau, i, Q) for i in range(n)]
        assert pow(tau, 2 * n, Q) == 1 and len(set(k)) == n      # the key's points repeat with period 2n > n: all distinct here
        rnd = random.Random(log_n)
        f = [rnd.randrange(Q) for _ in range(n)]
        _, pi = M.six_steps(f, log_n, k)
        assert pi == [K.witness_scalar([f], z, 1, tau=tau) for z in pts]


def test_model_transforms_are_the_dft_and_its_inverse():
    rnd = random.Random(5)
    for size_log in (1, 2, 3, 6):
        for tw_log in (size_log, size_log + 1, size_log + 3):
            size = 1 << size_log
            tw = M.twiddle_table(tw_log)
            v = [rnd.randrange(Q) for _ in range(size)]
            w = M.root(size_log)
            fwd = M.forward(v, size_log, tw, tw_log)
            assert [fwd[M.rev(i, size_log)] for i in range(size)] == M.dft(v, w)
            back = M.inverse(fwd, size_log, tw, tw_log)
            assert back == [x * size % Q for x in v]
            nat = M.inverse([v[M.rev(i, size_log)] for i in range(size)], size_log, tw, tw_log)
            assert nat == M.dft(v, pow(w, -1, Q))


# ---- kzg_domain_core.hpp against the model ----------------------------------------------------------------------------------
def test_core_constants(lib):
    assert [lib.hkd_const(i) for i in range(7)] == [M.MIN_LOG, M.MAX_LOG, M.MAX_COUNT, M.SLOT_BYTES, M.WS_CAP_DEFAULT, M.MAX_CHUNK, NONE]


def test_core_index_maps(lib):
    for bits in range(1, 12):
        for i in list(range(min(1 << bits, 64))) + [(1 << bits) - 1]:
            assert lib.hkd_rev(i, bits) == M.rev(i, bits)
    assert lib.hkd_rev((1 << 21) - 2, 21) == M.rev((1 << 21) - 2, 21)
    for n in (2, 4, 8, 64):
        for t in range(2 * n):
            want = M.g_src(n, t)
            assert lib.hkd_g_src(n, t) == (NONE if want is None else want)
        for k in range(n):
            want = M.h_src(n, k)
            assert lib.hkd_h_src(n, k) == (NONE if want is None else want)


def test_core_twiddle_selection_and_counts(lib):
    for size_log in range(1, 8):
        for tw_log in (size_log, size_log + 1, 21 if size_log > 5 else size_log + 2):
            muls = 0
            for s in range(size_log):
                half = 1 << s
                stage = 0
                for j in range(half):
                    for inv in (False, True):
                        neg = ctypes.c_int(-1)
                        got = lib.hkd_twiddle(size_log, half, j, tw_log, int(inv), ctypes.byref(neg))
                        want, wneg = M.twiddle(size_log, half, j, tw_log, inv)
                        assert got == (NONE if want is None else want) and bool(neg.value) == wneg
                        if want is not None:
                            assert 0 < want < (1 << (tw_log - 1))
                    stage += ((1 << size_log) // (2 * half)) * (1 if j else 0)
                assert lib.hkd_stage_muls(size_log, half) == M.stage_muls(size_log, half) == stage
                muls += stage
            assert lib.hkd_transform_muls(size_log) == M.transform_muls(size_log) == muls
    # the inverse factor really is minus the entry at T - e
    tw = M.twiddle_table(5)
    for j in range(1, 8):
        e, neg = M.twiddle(4, 8, j, 5, True)
        assert neg and (-tw[e]) % Q == pow(M.root(4), -j, Q)


def test_core_plan(lib):
    out = (ctypes.c_uint64 * 5)()
    caps = [0, 1, 1024, 3 * 2 * 64 * 256, 2 * 64 * 256 * 2, M.WS_CAP_DEFAULT, 1 << 40]
    for log_n in (1, 2, 6, 8, 12, 16, 20):
        for count in (0, 1, 2, 3, 5, 17, 4096, 4097, 65536):
            for cap in caps:
                lib.hkd_plan(log_n, count, cap, out)
                p = M.plan(log_n, count, cap)
                assert list(out) == [p["chunk_polys"], p["chunks"], p["ws_bytes"], p["stage_launches"], p["scalar_muls"]]
                if count:
                    assert 1 <= p["chunk_polys"] <= M.MAX_CHUNK and p["chunks"] * p["chunk_polys"] >= count
                    assert p["ws_bytes"] <= max(cap, 2 * (1 << log_n) * 256)
    assert M.plan(6, 5, 2 * 2 * 64 * 256)["chunks"] == 3      # the forced-chunking case of the GPU test
    assert M.plan(20, 16)["chunk_polys"] == 4                  # 2^20: 512 MiB of slots per polynomial under the 2 GiB cap


def test_core_argument_validation(lib):
    for log_n in (0, 1, 2, 20, 21, 31, 0xffffffff):
        for has_comm in (False, True):
            for has_srs in (False, True):
                for srs_n in (0, 1, 2, 3, 4, 1 << 20, (1 << 20) - 1):
                    assert lib.hkd_check_create(log_n, int(has_comm), int(has_srs), srs_n) == M.check_create(log_n, has_comm, has_srs, srs_n)
    assert lib.hkd_check_create(3, 0, 1, 8) == M.OK and lib.hkd_check_create(3, 0, 1, 7) == M.ERR_DEGREE
    assert lib.hkd_check_create(0, 1, 0, 0) == M.ERR_ARG and lib.hkd_check_create(3, 1, 0, 0) == M.ERR_STATE
    assert lib.hkd_check_create(3, 0, 0, 0) == M.ERR_NO_SRS
    for log_n in (1, 6):
        n = 1 << log_n
        assert [lib.hkd_check_len(log_n, m) for m in (0, 1, n, n + 1)] == [M.OK, M.OK, M.OK, M.ERR_DEGREE]
