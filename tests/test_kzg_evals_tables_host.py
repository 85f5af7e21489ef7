"""CPU: what a KZG domain handle with Lagrange-basis tables decides and computes outside the MSM itself.

The plan of the grouped table launches (plonk_amd/csrc/kzg_evals_core.hpp kze_tables_plan) and the lane function of
kze_finish_kernel (kzg_evals_finish.cuh kze_finish_chain + g1codec.cuh g1r_compress48_words) are compiled with g++
(tests/csrc/host_kzg_evals_tables.cpp) and checked against the big-int model tests/kzg_evals_tables_model.py; the model itself
is pinned to the scalar chain of tests/msm_tail_model.py and to the oracle's group law and compression."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as E
from tests import kzg_evals_model as EM
from tests import kzg_evals_tables_model as M
from tests.msm_tail_model import finish_scalar

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_evals_tables.so")
Q = E.Q
ID48 = bytes([0xC0]) + bytes(47)
LAYOUTS = [(8, False), (8, True), (12, False), (12, True)]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_evals_tables.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, vp, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    lib.hkt_plan.argtypes = [u64, u64, u64, u64, vp]
    lib.hkt_plan.restype = None
    lib.hkt_const.argtypes = [ci]
    lib.hkt_const.restype = u64
    lib.hkt_finish.argtypes = [vp, u32, u32, ci, ci, vp]
    lib.hkt_finish.restype = None
    return lib


def c_plan(lib, commitments, group_vectors, joined, separate):
    out = (ctypes.c_uint64 * 5)()
    lib.hkt_plan(commitments, group_vectors, joined, separate, out)
    return dict(zip(("msms", "group_launches", "device_finished", "finish_launches", "last_chunk"), out))


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def test_constants(lib):
    assert [lib.hkt_const(k) for k in range(4)] == [M.TABLE_GROUP, M.FINISH_CHUNK, 64, M.SLOT_BYTES]


@pytest.mark.parametrize("count", [0, 1, 4, 5, 8, 9, 64, 65, 4095, 4096, 4097, 8192, 8193, 65536])
def test_plan_against_the_model(lib, count):
    for group_vectors in (1, 2, 4, 16, 64, max(count, 1)):
        for joined in (0, 1):
            for separate in (0, 2):
                got = c_plan(lib, count, group_vectors, joined, separate)
                assert got == M.plan(count, group_vectors, joined, separate), (group_vectors, joined, separate)


@pytest.mark.parametrize("count", [0, 1, 4, 5, 65536])
def test_group_launches_and_the_finishing_mode(lib, count):
    """ceil(commitments / 4) launches for the commitments of a resident call, one more for the witness; the host finishes
    exactly when the run is one launch"""
    groups = -(-count // 4)
    for witness in (0, 1):
        p = c_plan(lib, count, 64, witness, 0)
        assert p["msms"] == count + witness and p["group_launches"] == groups + witness
        assert p["device_finished"] == int(groups + witness > 1)
        assert (p["finish_launches"] == 0) == (groups + witness <= 1)
    # a multiproof: the computed commitments one run, D and pi a launch of their own each, host-finished
    p = c_plan(lib, count, max(count, 1), 0, 2)
    assert p == M.multiproof_plan(count)
    assert p["group_launches"] == groups + 2 and p["device_finished"] == int(groups > 1)


def test_chunk_boundaries(lib):
    """a chunk holds 4096 commitments: 4096 | 4097, with and without the witness"""
    assert c_plan(lib, 4096, 64, 0, 0) == {"msms": 4096, "group_launches": 1024, "device_finished": 1, "finish_launches": 1, "last_chunk": 4096}
    assert c_plan(lib, 4097, 64, 0, 0) == {"msms": 4097, "group_launches": 1025, "device_finished": 1, "finish_launches": 2, "last_chunk": 1}
    assert c_plan(lib, 4096, 64, 1, 0) == {"msms": 4097, "group_launches": 1025, "device_finished": 1, "finish_launches": 2, "last_chunk": 1}
    assert c_plan(lib, 4095, 64, 1, 0)["finish_launches"] == 1
    p = c_plan(lib, 65536, 64, 1, 0)
    assert (p["group_launches"], p["finish_launches"], p["last_chunk"]) == (16385, 17, 1)


def test_plan_follows_the_staging_groups_of_the_host_form():
    """the commitments are grouped inside the groups the evaluation-form calls stage their vectors by: 64 | 65 vectors at 2^5
    (one staging group and a second of one vector), one vector per staging group from 2^16 values on"""
    g5 = EM.plan(5, 65, True, False, True)["group_vectors"]
    assert g5 == 64
    assert M.evals_plan(g5, 64, True, False)["group_launches"] == 16
    assert M.evals_plan(g5, 65, True, False)["group_launches"] == 17
    g16 = EM.plan(16, 8, True, True, True)["group_vectors"]
    assert g16 == 1 and M.evals_plan(g16, 8, True, True)["group_launches"] == 9
    assert M.evals_plan(EM.plan(16, 8, True, True, False)["group_vectors"], 8, True, True)["group_launches"] == 3
    assert M.evals_plan(64, 0, True, True) == M.plan(0, 1, 0, 0)
    assert M.evals_plan(64, 3, False, False)["group_launches"] == 0


# ---- the finishing model against the oracle -------------------------------------------------------------------------------------
def points_of(k):
    return [E.g1_mul(E.G1_GEN, x) if x % Q else None for x in k]


@pytest.mark.parametrize("rb,bitpos", LAYOUTS)
def test_model_chain_on_points_equals_the_scalar_chain_and_the_oracle_compression(rb, bitpos):
    rnd = random.Random(100 * rb + bitpos)
    cases = dict(M.special_scalars(rb, bitpos))
    cases["random"] = [rnd.randrange(Q) for _ in range(rb + 9)]
    cases["random, sparse"] = [rnd.randrange(Q) if rnd.random() < 0.4 else 0 for _ in range(rb + 9)]
    for name, k in cases.items():
        want = E.g1_mul(E.G1_GEN, finish_scalar(list(k), rb, bitpos))
        got = M.finish_point(points_of(k), rb, bitpos)
        assert got == want, name
        assert M.compress48(got) == E.g1_compress(want) == M.finish_bytes_of_scalars(k, rb, bitpos), name
    assert M.compress48(None) == ID48
    assert M.finish_point(points_of(cases["all identity"]), rb, bitpos) is None
    assert M.finish_point(points_of(cases["opposite then identity addends"]), rb, bitpos) is None
    if bitpos:
        assert M.finish_point(points_of(cases["S == 2 W"]), rb, bitpos) is None


def test_slot_bytes_are_the_library_layout():
    import plonk_amd as P
    pt = E.g1_mul(E.G1_GEN, 77)
    raw = M.slot_bytes(pt)
    assert raw[:96] == P.g1_to_raw96(pt) == E.g1_to_raw96(pt) and raw[96:144] == raw[144:] == M.fp_mont48(1)
    assert len(M.commitment_bytes([None] * 17, 8)) == M.BIT_SUMS * M.SLOT_BYTES


# ---- the lane function of the finish kernel, compiled for the host -----------------------------------------------------------------
def run_finish(lib, blobs, rb, bitpos):
    raw = b"".join(blobs)
    out = ctypes.create_string_buffer(48 * len(blobs))
    lib.hkt_finish(raw, len(blobs), M.BIT_SUMS, rb, int(bitpos), out)
    return [out.raw[48 * i:48 * i + 48] for i in range(len(blobs))]


@pytest.mark.parametrize("rb,bitpos", LAYOUTS)
def test_lane_function_against_the_model(lib, rb, bitpos):
    rnd = random.Random(7 * rb + bitpos)
    cases = dict(M.special_scalars(rb, bitpos))
    for t in range(6):
        cases["random %d" % t] = [rnd.randrange(Q) if rnd.random() < 0.8 else 0 for _ in range(rb + 9)]
    names = list(cases)
    blobs, want = [], []
    for name in names:
        pts = points_of(cases[name])
        zs = [rnd.randrange(1, E.P) if name.startswith("random") else 1 for _ in pts]   # XYZZ slots that are not normalised
        blobs.append(M.commitment_bytes(pts, rb, zs))
        want.append(M.finish_bytes_of_scalars(cases[name], rb, bitpos))
    got = run_finish(lib, blobs, rb, bitpos)
    for name, g, w in zip(names, got, want):
        assert g == w, name
    assert got[names.index("all identity")] == ID48
    flags = {g[0] & 0xE0 for g in got}
    assert {0x80, 0xA0, 0xC0} <= flags, "y in either half and the identity all occur"
