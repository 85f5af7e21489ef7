"""Shared by tests/test_msm_points_host.py and tests/test_gpu_msm_points.py: the host harness (tests/csrc/host_msm_points.cpp,
built with g++), the edge scalars and the point cases of plonk_msm_points, and their expected sums from the oracle
(oracle/bls12_381.py: msm_naive / g1_mul) — computed once per process and never from the code under test."""
import ctypes
import functools
import os
import random
import subprocess

import plonk_amd
from oracle import bls12_381 as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_msm_points.so")
Q = E.Q
LAMBDA = 0xac45a4010001a40200000000ffffffff   # phi(P) = [LAMBDA] P; q = LAMBDA^2 + LAMBDA + 1


@functools.lru_cache(maxsize=None)
def host_lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_msm_points.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    lib.hmp_plan.argtypes = [u64, u32, u32, u32, vp]
    lib.hmp_plan.restype = None
    lib.hmp_recode.argtypes = [vp, u32, vp, vp]
    lib.hmp_recode.restype = u32
    lib.hmp_count_digits.argtypes = [vp, vp, u64, u32]
    lib.hmp_count_digits.restype = u64
    lib.hmp_msm.argtypes = [vp, vp, u64, u32, u32, vp, vp]
    return lib


def host_plan(m, window_bits=0, slice_entries=0, min_bucket_terms=0):
    """what plonk_amd/csrc/msm_points_core.hpp plans for m terms: the dict plonk_ctx_last_msm_points must report"""
    out = (ctypes.c_uint32 * 4)()
    host_lib().hmp_plan(m, window_bits, slice_entries, min_bucket_terms, out)
    return {"path": out[0], "window_bits": out[1], "windows": out[2], "slice_entries": out[3], "terms": m}


def host_recode(k, c):
    """(k1, k2, digits of k1, digits of k2) of the canonical scalar k from the shared header"""
    W = -(-129 // c)
    halves, digits = (ctypes.c_uint64 * 4)(), (ctypes.c_int32 * (2 * W))()
    got = host_lib().hmp_recode((k % Q).to_bytes(32, "little"), c, halves, digits)
    assert got == W, (got, W)
    return halves[0] | halves[1] << 64, halves[2] | halves[3] << 64, list(digits[:W]), list(digits[W:])


def host_count_digits(points, scalars, c):
    finite = bytes(0 if p is None else 1 for p in points)
    return host_lib().hmp_count_digits(plonk_amd.fr_to_bytes_mont(scalars), finite, len(scalars), c)


def raw96(points):
    return b"".join(bytes(96) if p is None else plonk_amd.g1_to_raw96(p) for p in points)


def host_msm(points, scalars, c, slice_entries):
    out, stats = ctypes.create_string_buffer(97), (ctypes.c_uint64 * 3)()
    assert host_lib().hmp_msm(raw96(points), plonk_amd.fr_to_bytes_mont(scalars), len(scalars), c, slice_entries, out, stats) == 0
    return plonk_amd.g1_from_raw97(out.raw), {"nonzero_digits": stats[0], "slices": stats[1], "longest_bucket": stats[2]}


def neg(p):
    return None if p is None else (p[0], (E.P - p[1]) % E.P)


@functools.lru_cache(maxsize=None)
def pool(n=260):
    """n distinct points of the subgroup: a seeded start and a seeded step (one oracle addition each)"""
    rnd = random.Random(0x6d7370)
    p, step = E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)), E.g1_mul(E.G1_GEN, rnd.randrange(1, Q))
    out = []
    for _ in range(n):
        out.append(p)
        p = E.g1_add(p, step)
    return out


def every_digit(c, raw):
    """the largest value below LAMBDA whose c-bit windows all hold `raw`"""
    k, w = 0, 0
    while k + (raw << (c * w)) < LAMBDA:
        k += raw << (c * w)
        w += 1
    return k


def edge_scalars(widths=range(2, 17)):
    s = [0, 1, 2, Q - 1, Q - 2, LAMBDA - 1, LAMBDA, LAMBDA + 1, Q - LAMBDA, 1 << 127, (1 << 128) - 1, 1 << 128]
    for c in widths:
        h = 1 << (c - 1)
        s += [h - 1, h, h + 1]
        # every digit 2^(c-1); every window 2^(c-1) + 1 and every window all ones (a carry that runs to the top window), in
        # half 1 and, times LAMBDA, in half 2
        for raw in (h, h + 1, (1 << c) - 1):
            k = every_digit(c, raw)
            s += [k, k * LAMBDA % Q, (k + k * LAMBDA) % Q]
    out = []
    for v in s:
        if v not in out:
            out.append(v)
    return out


def equal_sum(points, s):
    """sum_i s P_i = [s] (sum_i P_i): the closed form of the all-scalars-equal cases"""
    acc = None
    for p in points:
        acc = E.g1_add(acc, p)
    return E.g1_mul(acc, s % Q) if acc is not None else None


@functools.lru_cache(maxsize=None)
def point_cases(m=24):
    """[(name, points, scalars, opts, expected)]: the adversarial point sets, each with random scalars and with all scalars
    equal; m is the size of the plain part of each case"""
    rnd = random.Random(0x706f696e74)
    P = pool()
    sc = lambda n: [rnd.randrange(Q) for _ in range(n)]
    s_eq = rnd.randrange(Q)
    cases = []

    def add(name, pts, random_scalars, equal_scalar=s_eq, opts=None):
        if random_scalars is not None:
            cases.append((name + "-random", pts, random_scalars, opts or {}, E.msm_naive(pts, random_scalars)))
        if equal_scalar is not None:
            cases.append((name + "-equal", pts, [equal_scalar] * len(pts), opts or {}, equal_sum(pts, equal_scalar)))

    pts = list(P[:m])
    pts[0] = pts[m // 2] = pts[m - 1] = None
    add("identity-among", pts, sc(m))
    add("same-point", [P[3]] * m, sc(m))
    pairs = [q for p in P[:m // 2] for q in (p, neg(p))]
    pair_sc = [s for s in sc(m // 2) for _ in (0, 1)]
    add("opposite-pairs", pairs + P[40:43], pair_sc + sc(3), None)
    add("opposite-pairs", pairs + P[40:43], None)
    # P with a = a LAMBDA puts phi(P) into the buckets of a's digits (half 2); Q = phi(P) with a puts Q there too (half 1)
    phis = [E.g1_mul(p, LAMBDA) for p in P[:4]]
    a = [rnd.randrange(1, LAMBDA) for _ in range(4)]
    pts = [q for p, f in zip(P[:4], phis) for q in (p, f)]
    add("phi-explicit", pts + P[50:52], [s for x in a for s in (x * LAMBDA % Q, x)] + sc(2), None)
    add("phi-explicit", pts, [s for _ in a for s in (a[0] * LAMBDA % Q, a[0])], None)
    cases[-1] = ("phi-explicit-equal",) + cases[-1][1:]
    # the whole sum is the identity: the last point is minus the sum of the rest
    pts, s = list(P[60:60 + m]), sc(m)
    add("sum-identity", pts + [neg(E.msm_naive(pts, s))], s + [1], None)
    add("sum-identity", pairs, None)
    add("scalars-one", list(P[:m]), None, 1)
    add("top-bucket", list(P[:m]), None, 1 << 3, {"window_bits": 4})
    add("top-bucket-13", list(P[:m]), None, 1 << 12, {"window_bits": 13})
    for name, pts, s, _, want in cases:
        assert len(pts) == len(s)
        if name.startswith("sum-identity"):
            assert want is None
    return cases
