"""CPU: the schedule of one proof.  plonk_amd/csrc/prove_schedule_core.hpp — what prover_prove and prover_prove_sharded read
their launch order from — is compiled with g++ (tests/csrc/host_prove_schedule.cpp) and compared field by field with the
model tests/prove_schedule_model.py over every combination of size, prover state and switch, one door call per size; a few
literal rows from DESIGN.md and the variant tests stand beside the grid, so that a mistake shared by the model and the header
cannot hide."""
import ctypes
import itertools
import os
import subprocess

import pytest

from tests import prove_schedule_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_prove_schedule.so")
INPUTS = ("logn", "lag_on", "lag_z", "wires_pending", "world", "sharded", "n", "rank_pts",
          "wire_by_column", "wire_polys_side", "side_defer", "z_commit_coeff", "shard_side", "shard_z")
SIZES = range(2, 28)
EDGE = (1 << 18) + 64


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_prove_schedule.cpp")
    deps = [src, os.path.join(ROOT, "plonk_amd", "csrc", "prove_schedule_core.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    lib.hps_schedule.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    lib.hps_schedule.restype = None
    return lib


def header(lib, rows):
    """rows of INPUTS -> rows of M.FIELDS, through one door call"""
    flat = [int(v) for row in rows for v in row]
    out = (ctypes.c_uint32 * (len(M.FIELDS) * len(rows)))()
    lib.hps_schedule((ctypes.c_int64 * len(flat))(*flat), len(rows), out)
    return [tuple(out[len(M.FIELDS) * i:len(M.FIELDS) * (i + 1)]) for i in range(len(rows))]


def model(row):
    s = M.prove_schedule(**dict(zip(INPUTS, row)))
    return tuple(int(s[f]) for f in M.FIELDS)


def single_rows(L):
    # rank_pts and the sharded path's two switches play no part on one GPU: values that would change a sharded schedule
    return [(L, lag_on, lag_z, pending, world, 0, 1 << L, 1, wbc, wps, sd, zcc, -1, 1)
            for lag_on, lag_z, pending in itertools.product((0, 1), repeat=3)
            for world in (1, 2) for wbc in (-1, 0, 1, 2) for wps in (-1, 0, 1) for sd in (-1, 0, 1, 2) for zcc in (-1, 0, 1)]


def sharded_rows(L):
    # ... and the single path's four switches and two flags none on the ranks
    return [(L, lag_on, 1, 1, world, 1, 1 << L, pts, 2, 1, 0, -1, side, sz)
            for world in (2, 4, 8) for lag_on in (0, 1) for side in (-1, 0, 1) for sz in (-1, 0, 1)
            for pts in (0, 1, EDGE - 1, EDGE, EDGE + 1, 1 << 22)]


@pytest.mark.parametrize("L", SIZES)
def test_single_path_grid(lib, L):
    rows = single_rows(L)
    assert len(rows) == 2304
    got = header(lib, rows)
    for row, g in zip(rows, got):
        assert g == model(row), dict(zip(INPUTS, row))
        assert g[6] == 0 and g[1] == (1 if not g[0] else 4 if row[8] == 2 else 3)


@pytest.mark.parametrize("L", [1] + list(SIZES))   # 2^1 .. 2^3 against eight ranks: n % world and n / world >= 2 both decide
def test_sharded_path_grid(lib, L):
    rows = sharded_rows(L)
    assert len(rows) == 324
    got = header(lib, rows)
    for row, g in zip(rows, got):
        assert g == model(row), dict(zip(INPUTS, row))
        assert g[0] == g[1] == g[5] == 0 and g[3] == g[4]


def test_the_grid_reaches_both_divisibility_rules():
    forced = [M.prove_schedule(L, 1, 0, 0, 8, 1, 1 << L, 1, 0, -1, -1, 0, 0, 1)["shard_z"] for L in (1, 2, 3, 4)]
    assert forced == [False, False, False, True]             # 2 % 8, 4 % 8; 8 / 8 < 2; 16 / 8 = 2
    assert M.prove_schedule(2, 1, 0, 0, 2, 1, 4, 1, 0, -1, -1, 0, 0, 1)["shard_z"]


def one(lib, **kw):
    base = dict(logn=20, lag_on=1, lag_z=1, wires_pending=0, world=1, sharded=0, n=None, rank_pts=0,
                wire_by_column=0, wire_polys_side=-1, side_defer=-1, z_commit_coeff=0, shard_side=0, shard_z=0)
    base.update(kw)
    if base["n"] is None:
        base["n"] = 1 << base["logn"]
    return dict(zip(M.FIELDS, header(lib, [tuple(base[k] for k in INPUTS)])[0]))


def test_literal_rows(lib):
    # DESIGN.md section 4.4 and tests/test_gpu_prover.py (host_wire_schedule): the default at 2^20 gates
    assert one(lib, wires_pending=1)["wire_parts"] == 3          # host columns: a, b, c + d
    assert one(lib, wires_pending=0)["wire_parts"] == 1          # resident columns: one grouped launch
    # tests/test_gpu_msm_variants.py: the switches at 2^12 gates
    assert one(lib, logn=12, wires_pending=1, wire_by_column=2)["wire_parts"] == 4
    assert one(lib, logn=12, wires_pending=1, wire_by_column=1)["wire_parts"] == 3
    assert one(lib, wires_pending=1, wire_by_column=-1)["wire_parts"] == 1
    assert one(lib, logn=12, wires_pending=1)["wire_parts"] == 1
    # z from its evaluations up to 2^17 gates
    assert one(lib, logn=17)["z_from_evals"] == 1
    assert one(lib, logn=18)["z_from_evals"] == 0
    assert one(lib, logn=18, z_commit_coeff=-1)["z_from_evals"] == 1
    assert one(lib, logn=17, lag_z=0)["z_from_evals"] == 0
    # side work waits and the wire polynomials ride along up to 2^19 gates (resident columns)
    assert [one(lib, logn=L)["polys_on_side"] for L in (19, 20)] == [1, 0]
    assert [one(lib, logn=L)["side_defer_r1"] for L in (19, 20)] == [1, 0]
    assert one(lib, logn=19, wires_pending=1)["side_defer_r1"] == 0   # host columns at 2^19 keep the phased launches' order
    s = one(lib, side_defer=2)
    assert (s["side_defer_r1"], s["side_defer_r2"]) == (1, 0)
    # the sharded grand product: from 2^19 gates and four ranks on
    assert one(lib, sharded=1, world=4, logn=19)["shard_z"] == 1
    assert one(lib, sharded=1, world=2, logn=20)["shard_z"] == 0
    assert one(lib, sharded=1, world=4, logn=18)["shard_z"] == 0
