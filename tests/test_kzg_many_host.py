"""CPU: what the host decides of the many-vector commitments on a KZG domain handle.

plonk_amd/csrc/kzg_many_core.hpp — the recoding the accumulation kernel runs per value, W(c), the table size and indexing, the
automatic width, the plans and the argument checks — is compiled with g++ (tests/csrc/host_kzg_many.cpp) and checked against
the big-int model tests/kzg_many_model.py."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as E
from tests import kzg_many_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_many.so")
Q = E.Q
WIDTHS = list(range(2, 9))
PLAN_KEYS = ("log_n", "window_bits", "windows", "slices", "count", "terms", "chunk_vectors", "chunks", "additions")


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_many.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, vp, ci = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    lib.hkm_windows.argtypes = [u32]
    lib.hkm_windows.restype = u32
    lib.hkm_recode.argtypes = [vp, u32, u32, vp]
    lib.hkm_recode.restype = u32
    lib.hkm_table_bytes.argtypes = [u32, u32]
    lib.hkm_table_bytes.restype = u64
    lib.hkm_entry.argtypes = [u32, u64, u32, u32]
    lib.hkm_entry.restype = u64
    lib.hkm_auto_width.argtypes = [u32, u64]
    lib.hkm_auto_width.restype = u32
    lib.hkm_slices.argtypes = [u32, u64, u32]
    lib.hkm_slices.restype = u32
    lib.hkm_plan.argtypes = [u32, u32, u64, u64, ci, u32, vp]
    lib.hkm_plan.restype = None
    lib.hkm_sparse_plan.argtypes = [u32, u32, vp, u64, u64, vp]
    lib.hkm_sparse_plan.restype = None
    lib.hkm_check_build.argtypes = [ci, u32, u32]
    lib.hkm_check_commit.argtypes = [ci, ci, ci, u64]
    lib.hkm_check_update.argtypes = [ci, vp, vp, ci, ci, u64, u32]
    lib.hkm_const.argtypes = [ci]
    lib.hkm_const.restype = u64
    return lib


def c_recode(lib, s, c, windows):
    limbs = (ctypes.c_uint32 * 8)(*[(s >> (32 * k)) & 0xFFFFFFFF for k in range(8)])
    digits = (ctypes.c_int32 * windows)()
    carry = lib.hkm_recode(limbs, c, windows, digits)
    return list(digits), carry


def c_plan(lib, *args):
    out = (ctypes.c_uint64 * 9)()
    lib.hkm_plan(*args, out)
    return dict(zip(PLAN_KEYS, out))


def c_sparse_plan(lib, log_n, c, offsets, cap):
    out = (ctypes.c_uint64 * 9)()
    arr = (ctypes.c_uint64 * len(offsets))(*offsets)
    lib.hkm_sparse_plan(log_n, c, arr, len(offsets) - 1, cap, out)
    return dict(zip(PLAN_KEYS, out))


def test_constants(lib):
    assert [lib.hkm_const(k) for k in range(10)] == [M.RESIDENT_WAVES, M.ENTRY_BYTES, M.SLOT_BYTES, M.CHUNK_MAX, M.TERM_BYTES,
                                                    M.MAX_COUNT, M.MAX_TERMS, M.LANES, M.LOG_N_MAX, M.MAX_SEGMENT]


# ---- the recoding ---------------------------------------------------------------------------------------------------------------
def scalars_of(c, W):
    half = 1 << (c - 1)
    out = {"0": 0, "1": 1, "q - 1": Q - 1, "q - 2": Q - 2}
    for w in range(W):
        for name, v in (("half", half), ("half - 1", half - 1), ("half + 1", half + 1)):
            if v << (c * w) < Q:
                out["%s in window %d" % (name, w)] = v << (c * w)
    every = sum(half << (c * w) for w in range(W))
    while every >= Q:                                  # every digit at the positive maximum, as far up as q allows
        W -= 1
        every = sum(half << (c * w) for w in range(W))
    out["every digit at the positive maximum"] = every
    out["a carry through all windows"] = (1 << 254) - 1        # window 0 gives -1 and carries, every window above 2^c -> 0 and carries on
    out["a carry through all windows from half + 1"] = (1 << 254) - 1 - ((1 << c) - 1) + half + 1
    rnd = random.Random(1000 + c)
    for t in range(300):
        out["random %d" % t] = rnd.randrange(Q)
    return out


@pytest.mark.parametrize("c", WIDTHS)
def test_recoding_against_the_definition_and_the_model(lib, c):
    W = lib.hkm_windows(c)
    half = 1 << (c - 1)
    for name, s in scalars_of(c, W).items():
        digits, carry = c_recode(lib, s, c, W)
        assert carry == 0, name
        assert sum(d << (c * w) for w, d in enumerate(digits)) == s, name
        assert all(-half <= d <= half for d in digits), name
        assert (digits, 0) == M.recode(s, c, W), name
    digits, _ = c_recode(lib, scalars_of(c, W)["every digit at the positive maximum"], c, W)
    assert digits.count(half) >= W - 1
    digits, _ = c_recode(lib, (1 << 254) - 1, c, W)
    assert digits[0] == -1 and not any(digits[1:254 // c]) and sum(d << (c * w) for w, d in enumerate(digits)) == (1 << 254) - 1


@pytest.mark.parametrize("c", WIDTHS)
def test_window_count_is_sufficient_and_minimal(lib, c):
    W = lib.hkm_windows(c)
    assert W == M.windows(c) == {2: 128, 3: 86, 4: 64, 5: 52, 6: 43, 7: 37, 8: 32}[c]
    digits, carry = c_recode(lib, Q - 1, c, W)
    assert carry == 0 and digits[-1] != 0, "the last window is used by q - 1"
    short, _ = c_recode(lib, Q - 1, c, W - 1)         # (what is left over is a carry or bits above the last window)
    assert M.recode(Q - 1, c, W - 1)[1] != 0, "one window fewer loses q - 1"
    assert short == M.recode(Q - 1, c, W - 1)[0] and sum(d << (c * w) for w, d in enumerate(short)) != Q - 1


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def test_table_bytes_and_entry_index(lib):
    for log_n in range(1, 13):
        for c in WIDTHS:
            assert lib.hkm_table_bytes(log_n, c) == M.table_bytes(log_n, c) == (1 << log_n) * M.windows(c) * (1 << (c - 1)) * 128
    assert M.table_bytes(8, 8) == 128 << 20
    for c in WIDTHS:
        W, half, n = M.windows(c), 1 << (c - 1), 256
        seen = set()
        for i in (0, 1, n - 1):
            for w in (0, 1, W - 1):
                for d in (1, half):
                    e = lib.hkm_entry(c, i, w, d)
                    assert e == M.entry_index(c, i, w, d) < M.table_entries(8, c)
                    seen.add(e)
        assert lib.hkm_entry(c, 0, 0, 1) == 0 and lib.hkm_entry(c, n - 1, W - 1, half) == M.table_entries(8, c) - 1
        assert len(seen) == (18 if half > 1 else 9)


def test_automatic_width(lib):
    for log_n in (1, 8, 12):
        b8, b4, b2 = (M.table_bytes(log_n, c) for c in (8, 4, 2))
        for left, want in ((b8, 8), (b8 + 1, 8), (1 << 62, 8), (b8 - 1, 7), (b4, 4), (M.table_bytes(log_n, 5) - 1, 4), (b2, 2),
                           (b2 - 1, 0), (0, 0)):
            assert lib.hkm_auto_width(log_n, left) == M.auto_width(log_n, left) == want, (log_n, left)


# ---- the plans ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65, 2047, 2048, 4097, 1 << 24])
def test_plan_against_the_model(lib, count):
    for log_n in (1, 2, 5, 6, 8, 12):
        for c in (2, 4, 5, 8):
            for host_form in (False, True):
                got = c_plan(lib, log_n, c, count, M.WS_CAP_DEFAULT, int(host_form), 0)
                assert got == M.plan(log_n, c, count, M.WS_CAP_DEFAULT, host_form), (log_n, c, host_form)
                assert got["additions"] == count * (1 << log_n) * M.windows(c)


def test_chunk_edge_at_caps_of_one_and_three_vectors(lib):
    log_n, c = 8, 8
    for host_form in (False, True):
        for count in (1, 2, 3, 4, 7, 4097):
            s = M.slices(log_n, count)
            per_vector = 256 * s + 48 + (64 * 256 if host_form else 0)
            for vectors, cap in ((1, per_vector), (1, 1), (1, 2 * per_vector - 1), (3, 3 * per_vector), (3, 4 * per_vector - 1)):
                got = c_plan(lib, log_n, c, count, cap, int(host_form), 0)
                assert got == M.plan(log_n, c, count, cap, host_form)
                assert got["chunk_vectors"] == min(vectors, count) and got["chunks"] == -(-count // min(vectors, count))
    assert c_plan(lib, 8, 8, (1 << 24), 1 << 62, 0, 0)["chunk_vectors"] == M.CHUNK_MAX


def test_slices_at_both_ends_of_the_rule(lib):
    """1 once the call fills the device; doubled below that, down to 64 values per slice: one per lane"""
    for log_n in range(1, 13):
        for c in WIDTHS:
            n = 1 << log_n
            most = max(n // 64, 1)
            for count in (1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 2047, 2048, 2049, 1 << 20):
                s = lib.hkm_slices(log_n, count, 0)
                assert s == M.slices(log_n, count) and s & (s - 1) == 0 and 1 <= s <= most
                assert s == 1 or count * s // 2 < M.RESIDENT_WAVES
                assert count * s >= M.RESIDENT_WAVES or s * 2 > most
            for force in (1, 2, 4, 64, 1 << 13):
                s = lib.hkm_slices(log_n, 1 << 20, force)
                assert s == M.slices(log_n, 1 << 20, force) == min(force, n)
    assert lib.hkm_slices(8, 1, 0) == 4 and lib.hkm_slices(8, 256, 0) == 4 and lib.hkm_slices(8, 511, 0) == 4
    assert lib.hkm_slices(8, 512, 0) == 4 and lib.hkm_slices(8, 1024, 0) == 2 and lib.hkm_slices(8, 2048, 0) == 1
    assert lib.hkm_slices(12, 1, 0) == 64 and lib.hkm_slices(12, 1024, 0) == 2
    assert lib.hkm_slices(6, 1, 0) == 1 and lib.hkm_slices(7, 1, 0) == 2 and lib.hkm_slices(1, 1, 0) == 1


def test_sparse_plan_against_the_model(lib):
    rnd = random.Random(5)
    shapes = {"empty call": [0], "one empty segment": [0, 0], "single updates": list(range(0, 4097)),
              "mixed": [0, 0, 1, 1, 300, 301, 301, 1000]}
    offs = [0]
    for _ in range(200):
        offs.append(offs[-1] + rnd.choice((0, 1, 2, 7, 64, 65, 500)))
    shapes["random"] = offs
    for name, offsets in shapes.items():
        for c in (2, 8):
            for cap in (1, 304 + 36, 3 * (304 + 36), 20000, M.WS_CAP_DEFAULT):
                assert c_sparse_plan(lib, 8, c, offsets, cap) == M.sparse_plan(8, c, offsets, cap), (name, c, cap)
    p = c_sparse_plan(lib, 8, 8, list(range(0, 8)), 3 * (304 + 36))
    assert (p["chunks"], p["chunk_vectors"], p["slices"], p["terms"], p["additions"]) == (3, 3, 1, 7, 7 * 32)
    assert c_sparse_plan(lib, 8, 8, [0, 1000, 1001], 1)["chunks"] == 2         # a chunk of one segment is always allowed


# ---- the argument checks --------------------------------------------------------------------------------------------------------------
def test_argument_checks(lib):
    assert lib.hkm_check_build(1, 8, 0) == 0 and lib.hkm_check_build(1, 12, 8) == 0 and lib.hkm_check_build(1, 1, 2) == 0
    for bad in ((0, 8, 0), (1, 13, 0), (1, 0, 0), (1, 8, 1), (1, 8, 9), (1, 8, 1 << 31)):
        assert lib.hkm_check_build(*bad) == M.ERR_ARG, bad
    assert lib.hkm_check_commit(1, 1, 1, M.MAX_COUNT) == 0 and lib.hkm_check_commit(1, 0, 0, 0) == 0
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, M.MAX_COUNT + 1)):
        assert lib.hkm_check_commit(*bad) == M.ERR_ARG, bad

    def upd(offsets, index, count=None, has_domain=1, has_deltas=1, has_out=1, log_n=3, null_offsets=False, null_index=False):
        o = (ctypes.c_uint64 * len(offsets))(*offsets)
        i = (ctypes.c_uint32 * max(len(index), 1))(*index)
        return lib.hkm_check_update(has_domain, None if null_offsets else o, None if null_index else i, has_deltas, has_out,
                                    len(offsets) - 1 if count is None else count, log_n)
    assert upd([0, 2, 2, 3], [0, 7, 7]) == 0
    assert upd([0], [], count=0, null_offsets=True, null_index=True, has_deltas=0, has_out=0) == 0
    assert upd([0, 0, 0], [], null_index=True, has_deltas=0) == 0, "empty segments need no terms"
    assert upd([0, 2], [0, 8]) == M.ERR_ARG, "an index >= n"
    assert upd([1, 2], [0, 1]) == M.ERR_ARG, "offsets start at 0"
    assert upd([0, 2, 1], [0, 1]) == M.ERR_ARG, "offsets never decrease"
    assert upd([0, 1], [0], has_domain=0) == M.ERR_ARG and upd([0, 1], [0], has_out=0) == M.ERR_ARG
    assert upd([0, 1], [0], has_deltas=0) == M.ERR_ARG and upd([0, 1], [0], null_index=True) == M.ERR_ARG
    assert upd([0, 1], [0], null_offsets=True) == M.ERR_ARG
    assert upd([0, M.MAX_TERMS + 1], [0], null_index=True) == M.ERR_ARG, "the total above its cap is refused before the indices are read"
    assert upd([0], [], count=M.MAX_COUNT + 1) == M.ERR_ARG
    long = [0] * M.MAX_SEGMENT
    assert upd([0, 1, 1 + M.MAX_SEGMENT], [0] + long) == 0, "a segment of 2^16 terms, 8192 n here, is the longest"
    assert upd([0, 1, 2 + M.MAX_SEGMENT], [0, 0] + long) == M.ERR_ARG, "one term more is refused"
