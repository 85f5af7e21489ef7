"""Quarter-density commit-key tables (64 rows, T[r][i] = 2^(4 r) P_i): the recoding for_each_digit_quad of
plonk_amd/csrc/msm_recode.cuh compiled with g++ (tests/csrc/host_msm_quad.cpp) against a big-int model written here, the
mean digit count against the figures the layout was planned with, and the model's entries through the unchanged bucket
reduction (tests/msm_wide_model.py) against the oracle's MSM.  CPU-only."""
import ctypes
import os
import random
import subprocess

import pytest

from msm_wide_model import bit_sums, host_finish, quad_digits
from oracle import bls12_381 as E

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhost_msm_quad.so")
Q = E.Q
WIDTHS = ((16, 16), (20, 13))            # (digit width, most digits of a scalar)


def quad_msm_model(points, scalars, w: int):
    """bucket = |d| - 1 with weight bucket + 1 (the window convention) over table rows 16^r P_i: the entries go through the
    unchanged row / column / bit-sum reduction, no 2 W - S"""
    rows = []
    for pt in points:                                             # the 64 rows of a point by doubling, as srs_table_kernel builds them
        t, lst = E.to_jac(pt), []
        for _ in range(64):
            lst.append(t)
            for _ in range(4):
                t = E.jac_double(t)
        rows.append(lst)
    sums = {}
    for i, s in enumerate(scalars):
        for r, d in quad_digits(s % Q, w):
            t = rows[i][r]
            b = abs(d) - 1
            sums[b] = E.jac_add(sums.get(b, E.JAC_ID), E.jac_neg(t) if d < 0 else t)
    return host_finish(*bit_sums(sums, w))


def edge_scalars():
    vals = [0, 1, 15, 16, 17, Q - 1, Q - 2]
    for k in range(255):
        vals += [1 << k, (1 << k) - 1]
    for pat in ("8", "f", "7", "1", "10", "0f", "f0", "80000", "7ffff", "fffff", "8000", "7fff", "ffff", "0001", "00001"):
        vals.append(int((pat * 64)[:64], 16) % Q)
        vals.append(int((pat * 64)[:63], 16) % Q)
    vals += [(1 << 254) + 12345, (1 << 254) + (1 << 253), Q - 16, Q - 15, Q - 17]
    return [v for v in vals if v < Q]


def limbs_of(s):
    return (ctypes.c_uint32 * 8)(*[(s >> (32 * i)) & 0xFFFFFFFF for i in range(8)])


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_msm_quad.cpp")
    hdrs = [os.path.join(HERE, "..", "plonk_amd", "csrc", h) for h in ("msm_recode.cuh", "field.cuh")]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    lib.hmq_count.restype = ctypes.c_uint64
    lib.hmq_count.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
    return lib


def product_digits(lib, s, w, strided):
    out = (ctypes.c_uint32 * 64)()
    n = lib.hmq_digits(limbs_of(s), w, strided, out)
    assert n <= 16
    return [(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]) for j in range(n)]


def test_product_quad_recoding_matches_the_model(lib):
    """digit by digit (slot, row, bucket, sign), for both widths, from a register scalar and from a parked one"""
    assert lib.hmq_rows() == 64
    r = random.Random(6464)
    scalars = edge_scalars() + [r.randrange(Q) for _ in range(2000)]
    for w, most in WIDTHS:
        for s in scalars:
            model = quad_digits(s, w)
            want = [(j, row, abs(d) - 1, 1 if d < 0 else 0) for j, (row, d) in enumerate(model)]
            for strided in (0, 1):
                assert product_digits(lib, s, w, strided) == want, (hex(s), w, strided)
            # the properties of the recoding (the model reconstructs s by its own assertion)
            assert len(model) <= most, (hex(s), w)
            assert all(0 <= row < 64 for row, _ in model)
            assert all(d % 16 != 0 and 1 <= abs(d) <= (1 << (w - 1)) for _, d in model), (hex(s), w)
            assert all(row_b > row_a for (row_a, _), (row_b, _) in zip(model, model[1:]))
            assert sum((-(b + 1) if sg else b + 1) << (4 * row) for _, row, b, sg in want) == s
    # for_each_digit(s, 64, f), the run-time dispatch the host-side callers use: width 16
    for s in scalars[:200] + scalars[-50:]:
        assert product_digits(lib, s, 0, 0) == product_digits(lib, s, 16, 0)


def test_mean_digit_count(lib):
    """20 000 uniform canonical scalars: 12.99 additions per scalar over 2^19 buckets (w = 20), 15.97 over 2^15 (w = 16) — the
    figures of a CPU count made before the recoding was written; the standard error at this sample size is below 0.01"""
    r = random.Random(20000)
    n = 20000
    scalars = [r.randrange(Q) for _ in range(n)]
    flat = (ctypes.c_uint32 * (8 * n))(*[(s >> (32 * i)) & 0xFFFFFFFF for s in scalars for i in range(8)])
    for w, lo, hi in ((20, 12.9, 13.1), (16, 15.9, 16.0)):
        mean = lib.hmq_count(flat, n, w) / n
        print(f"w = {w}: {mean:.4f} digits per scalar")
        assert lo <= mean <= hi, (w, mean)
        assert sum(len(quad_digits(s, w)) for s in scalars) / n == mean


def test_quad_model_equals_the_oracle_msm():
    """40 random points and scalars, both widths, through the unchanged bucket reduction"""
    r = random.Random(4040)
    pts = [E.g1_mul(E.G1_GEN, r.randrange(1, Q)) for _ in range(40)]
    sc = [r.randrange(Q) for _ in range(40)]
    want = E.msm_pippenger(pts, sc)
    for w, _ in WIDTHS:
        assert quad_msm_model(pts, sc, w) == want, w
    edge = [0, 1, 15, 16, 17, Q - 1, Q - 2, 1 << 19, (1 << 20) - 1, (1 << 254) + 12345]
    assert quad_msm_model(pts[:10], edge, 20) == E.msm_naive(pts[:10], edge)
    assert quad_msm_model(pts[:10], edge, 16) == E.msm_naive(pts[:10], edge)
