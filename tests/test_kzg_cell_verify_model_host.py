"""CPU: the KZG10 cell verifier in the exponent.  The big-int model tests/kzg_cell_verify_model.py (the twist with the kernel's
index arithmetic, the column sums by passes, the weights over the counting sort, both equations) is pinned to
kzg_cells_model.remainder_from_cell / remainder_coeffs, to proof_closed_form and to the naive per-item equation, for log_n
2..6, every cell size, valid and invalid batches; plonk_amd/csrc/kzg_cell_verify_core.hpp (the challenge bytes, the index maps,
the plan, the argument checks) is compiled with g++ (tests/csrc/host_kzg_cell_verify.cpp) and checked against the same model."""
import ctypes
import os
import random
import subprocess

import pytest

import plonk_amd
from tests import kzg_cell_verify_model as V
from tests import kzg_cells_model as M
from tests import kzg_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg_cell_verify.so")
Q = V.Q
TAU = K.TAU
SHAPES = [(log_n, log_cell) for log_n in range(2, 7) for log_cell in range(1, log_n)]


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg_cell_verify.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    u64, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
    for name in ("hkv_twist_groups", "hkv_twist_lds_bytes", "hkv_colsum_slices"):
        getattr(lib, name).restype = u64
    for name in ("hkv_items_per_group", "hkv_lanes_per_item", "hkv_colsum_passes"):
        getattr(lib, name).restype = u32
    lib.hkv_check_shape.argtypes = [u32, u32]
    lib.hkv_check_items.argtypes = [u32, u32, u64, vp, vp, u64]
    lib.hkv_check_counts.argtypes = [u32, u32, u64, u64]
    lib.hkv_canonical.argtypes = [vp]
    lib.hkv_items_per_group.argtypes = [u32]
    lib.hkv_lanes_per_item.argtypes = [u32]
    lib.hkv_twist_groups.argtypes = [u32, u64]
    lib.hkv_twist_lds_bytes.argtypes = [u32]
    lib.hkv_colsum_slices.argtypes = [u64]
    lib.hkv_colsum_passes.argtypes = [u64]
    lib.hkv_layout.argtypes = [u32, u64, u64, vp]
    lib.hkv_counting_sort.argtypes = [vp, u64, u64, vp, vp]
    lib.hkv_plan.argtypes = [u32, u64, u64, ctypes.c_int, u32, u32, vp]
    lib.hkv_challenge.argtypes = [vp, u64, u32, u32, vp, vp, u64, vp, vp, vp, vp, u64, vp]
    for name in ("hkv_layout", "hkv_counting_sort", "hkv_plan", "hkv_challenge"):
        getattr(lib, name).restype = None
    return lib


def u32s(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def blobs(log_n, log_cell, count, rnd):
    """per polynomial: (f, commitment exponent, cells, proof exponents)"""
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    out = []
    for _ in range(count):
        f = [rnd.randrange(Q) for _ in range(n)]
        cells = M.cells_horner(f, log_n, log_cell)
        out.append((f, M.evaluate(f, TAU), [cells[k * l:(k + 1) * l] for k in range(r)],
                    [M.proof_closed_form(f, log_n, log_cell, k, TAU) for k in range(r)]))
    return out


def all_items(bl):
    """every cell of every polynomial: (commitment index, cell index, values, proof exponent)"""
    return [(c, k, b[2][k], b[3][k]) for c, b in enumerate(bl) for k in range(len(b[2]))]


# ---- the model against the closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_cell", SHAPES)
def test_twist_equals_both_forms_of_the_remainder(log_n, log_cell):
    rnd = random.Random(100 * log_n + log_cell)
    r = 1 << (log_n - log_cell)
    (f, _, cells, _), = blobs(log_n, log_cell, 1, rnd)
    for k in range(r):
        c = V.twist(cells[k], log_n, log_cell, k)
        assert c == M.remainder_from_cell(cells[k], log_n, log_cell, k) == M.remainder_coeffs(f, log_n, log_cell, k), k
        w = rnd.randrange(Q)
        assert V.twist(cells[k], log_n, log_cell, k, w) == [x * w % Q for x in c]


@pytest.mark.parametrize("log_n,log_cell", SHAPES)
def test_both_equations_accept_valid_cells_and_reject_invalid_ones(log_n, log_cell):
    rnd = random.Random(200 * log_n + log_cell)
    l, r = 1 << log_cell, 1 << (log_n - log_cell)
    bl = blobs(log_n, log_cell, 2, rnd)
    comm = [b[1] for b in bl]
    items = all_items(bl)
    for c, k, values, proof in items:
        assert V.each_accepts(comm[c], k, values, proof, log_n, log_cell, TAU)
        assert V.naive_accepts(comm[c], k, values, proof, log_n, log_cell, TAU)
    for rho in (1, rnd.randrange(Q)):
        assert V.folded_accepts(comm, items, rho, log_n, log_cell, TAU)
    rho = rnd.randrange(2, Q)
    i = rnd.randrange(len(items))
    c, k, values, proof = items[i]

    def variants():
        bad = list(values)
        bad[l - 1] = (bad[l - 1] + 1) % Q
        yield (c, k, bad, proof)                                          # one value + 1 in the last slot
        if r > 2:                                                          # (n = 2l: the quotient of f by X^l - x_k is its upper half for every k)
            yield (c, k, values, bl[c][3][(k + 1) % r])                    # a neighbour's proof
        yield (1 - c, k, values, proof)                                    # a wrong commitment index
        yield (c, (k + 1) % r, values, proof)                              # a cell index off by one
        yield (c, k, values, 0)                                            # the identity as the proof
    for v in variants():
        assert not V.each_accepts(comm[v[0]], v[1], v[2], v[3], log_n, log_cell, TAU)
        assert not V.naive_accepts(comm[v[0]], v[1], v[2], v[3], log_n, log_cell, TAU)
        assert not V.folded_accepts(comm, items[:i] + [v] + items[i + 1:], rho, log_n, log_cell, TAU)


def test_a_predictable_rho_voids_the_folded_check():
    """the same cell twice, + d on a value of the first copy and - d on the second: with rho = 1 the two errors cancel in R_j"""
    log_n, log_cell = 4, 2
    rnd = random.Random(5)
    (f, c, cells, proofs), = blobs(log_n, log_cell, 1, rnd)
    d, j, k = rnd.randrange(1, Q), 1, 2
    up, down = list(cells[k]), list(cells[k])
    up[j], down[j] = (up[j] + d) % Q, (down[j] - d) % Q
    items = [(0, k, up, proofs[k]), (0, k, down, proofs[k])]
    assert V.folded_accepts([c], items, 1, log_n, log_cell, TAU)
    assert not V.folded_accepts([c], items, rnd.randrange(2, Q), log_n, log_cell, TAU)
    assert not any(V.each_accepts(c, k, v, proofs[k], log_n, log_cell, TAU) for v in (up, down))


def test_column_sums_by_passes_and_weights_over_the_counting_sort():
    rnd = random.Random(9)
    for K_, l in ((1, 2), (2, 4), (64, 2), (65, 2), (64 * 64 + 3, 2)):
        rows = [[rnd.randrange(Q) for _ in range(l)] for _ in range(K_)]
        assert V.colsum(rows, l) == [sum(r[j] for r in rows) % Q for j in range(l)]
    log_n, log_cell, M_ = 5, 2, 4
    cidx = [rnd.choice((0, 1, 3)) for _ in range(40)]                      # commitment 2 has no item
    kidx = [rnd.randrange(8) for _ in range(40)]
    rho = rnd.randrange(Q)
    pw, W, px = V.weights(rho, cidx, kidx, M_, log_n, log_cell)
    x, _ = M.cell_points(log_n, log_cell)
    assert W == [sum(pow(rho, i, Q) for i, c in enumerate(cidx) if c == cc) % Q for cc in range(M_)] and W[2] == 0
    assert px == [pow(rho, i, Q) * x[k] % Q for i, k in enumerate(kidx)]
    assert V.weights(rho, [0] * 7, [0] * 7, 1, log_n, log_cell)[1] == [sum(pow(rho, i, Q) for i in range(7)) % Q]


# ---- kzg_cell_verify_core.hpp against the model -------------------------------------------------------------------------------
def test_shape_and_item_checks(lib):
    for log_n in range(0, 23):
        for log_cell in range(0, 14):
            assert lib.hkv_check_shape(log_n, log_cell) == V.check_shape(log_n, log_cell), (log_n, log_cell)
    assert V.check_shape(20, 11) == V.OK and V.check_shape(20, 12) == V.ERR_ARG and V.check_shape(21, 6) == V.ERR_ARG
    assert V.check_shape(2, 1) == V.OK and V.check_shape(2, 2) == V.ERR_ARG
    for cidx, kidx, M_ in (([0, 1], [0, 7], 2), ([0, 2], [0, 7], 2), ([0, 1], [0, 8], 2), ([], [], 0), ([0], [0], 0)):
        assert lib.hkv_check_items(5, 2, M_, u32s(cidx), u32s(kidx), len(cidx)) == V.check_items(5, 2, M_, cidx, kidx)
    assert lib.hkv_check_counts(12, 6, 65536, 1) == V.OK and lib.hkv_check_counts(12, 6, 65537, 1) == V.ERR_ARG
    assert lib.hkv_check_counts(8, 1, 1, 1 << 20) == V.OK and lib.hkv_check_counts(8, 1, 1, (1 << 20) + 1) == V.ERR_ARG
    assert lib.hkv_check_counts(12, 6, 1, 1 << 19) == V.OK and lib.hkv_check_counts(12, 6, 1, (1 << 19) + 1) == V.ERR_ARG   # count * l > 2^25
    for v, want in ((0, 1), (Q - 1, 1), (Q, 0), (Q + 1, 0), ((1 << 256) - 1, 0)):
        assert lib.hkv_canonical(v.to_bytes(32, "little")) == want, v


def test_packing_passes_layout_and_plan(lib):
    for log_cell in range(1, 12):
        assert lib.hkv_items_per_group(log_cell) == V.items_per_group(log_cell)
        assert lib.hkv_lanes_per_item(log_cell) == V.lanes_per_item(log_cell)
        assert lib.hkv_twist_lds_bytes(log_cell) == V.twist_lds_bytes(log_cell) <= 65536
        assert V.items_per_group(log_cell) * V.lanes_per_item(log_cell) == V.LANES
        for K_ in (1, 2, 3, 4, 5, 127, 128, 129, 1000):
            assert lib.hkv_twist_groups(log_cell, K_) == V.twist_groups(log_cell, K_)
    assert V.items_per_group(6) == 4 and V.items_per_group(7) == 1
    for rows in (1, 2, 63, 64, 65, 4096, 4097, 1 << 20):
        assert lib.hkv_colsum_slices(rows) == V.colsum_slices(rows)
        assert lib.hkv_colsum_passes(rows) == V.colsum_passes(rows)
    assert [V.colsum_passes(x) for x in (64, 65, 4096, 4097)] == [1, 2, 2, 3]
    out = (ctypes.c_uint64 * 9)()
    for log_cell, M_, K_ in ((1, 1, 1), (3, 2, 16), (6, 16, 128), (11, 1, 2), (3, 5, 63), (3, 1, 64)):
        lib.hkv_layout(log_cell, M_, K_, out)
        lay = V.layout(log_cell, M_, K_)
        assert list(out)[:7] == [lay[k] for k in ("pt_commitment", "pt_proof", "points", "term_w", "term_x", "term_r", "terms")]
        for each in (0, 1):
            for mins in ((0, 0), (1, 1), (1 << 30, 1 << 30)):
                lib.hkv_plan(log_cell, M_, K_, each, mins[0], mins[1], out)
                p = V.plan(log_cell, M_, K_, bool(each), *mins)
                assert list(out) == [p[k] for k in ("transforms", "twist_groups", "colsum_passes", "msm_terms_left", "msm_terms_right",
                                                    "msm_path_left", "msm_path_right", "scalar_muls", "msm_terms_info")]
    # both sides of msm_points' 64-term rule for each of the two sums at l = 8, M = 2
    assert [(V.plan(3, 2, k, False)["msm_path_left"], V.plan(3, 2, k, False)["msm_path_right"]) for k in (1, 53, 54, 63, 64)] == \
        [(0, 0), (0, 0), (0, 1), (0, 1), (1, 1)]


def test_counting_sort(lib):
    rnd = random.Random(3)
    for K_, M_ in ((1, 1), (5, 1), (40, 4), (7, 9), (300, 17)):
        cidx = [rnd.randrange(M_) for _ in range(K_)]
        perm, off = (ctypes.c_uint32 * K_)(), (ctypes.c_uint32 * (M_ + 1))()
        lib.hkv_counting_sort(u32s(cidx), K_, M_, perm, off)
        want = V.counting_sort(cidx, M_)
        assert (list(perm), list(off)) == want
        assert sorted(want[0]) == list(range(K_)) and [cidx[i] for i in want[0]] == sorted(cidx)


def test_challenge_bytes(lib):
    rnd = random.Random(11)
    log_n, log_cell = 4, 2
    l = 1 << log_cell
    key = K.opening_key()
    comm = [K.scalar_commit(rnd.randrange(Q)) for _ in range(2)] + [K.IDENTITY48]
    items = [(rnd.randrange(3), rnd.randrange(4), [rnd.randrange(Q) for _ in range(l)], K.scalar_commit(rnd.randrange(Q))) for _ in range(5)]

    def native(label, log_n, log_cell, key, comm, items):
        out = ctypes.create_string_buffer(32)
        vals = b"".join(plonk_amd.fr_to_bytes_mont(it[2]) for it in items)
        lib.hkv_challenge(label, len(label), log_n, log_cell, key, b"".join(comm), len(comm), u32s([it[0] for it in items]),
                          u32s([it[1] for it in items]), vals, b"".join(it[3] for it in items), len(items), out)
        return int.from_bytes(out.raw, "little")
    base = native(b"label", log_n, log_cell, key, comm, items)
    assert base == V.challenge(b"label", log_n, log_cell, key, comm, items)
    assert native(b"", log_n, log_cell, key, comm, items[:1]) == V.challenge(b"", log_n, log_cell, key, comm, items[:1])
    seen = {base}
    changed = [(b"labek", log_n, log_cell, key, comm, items), (b"label", log_n + 1, log_cell, key, comm, items),
               (b"label", log_n, log_cell, key[:-1] + bytes([key[-1] ^ 1]), comm, items),
               (b"label", log_n, log_cell, key, comm[:2] + [comm[0]], items),
               (b"label", log_n, log_cell, key, comm, [(items[0][0] ^ 1,) + items[0][1:]] + items[1:]),
               (b"label", log_n, log_cell, key, comm, [(items[0][0], items[0][1] ^ 1) + items[0][2:]] + items[1:]),
               (b"label", log_n, log_cell, key, comm, items[:4] + [items[4][:2] + (items[4][2][:3] + [items[4][2][3] ^ 1], items[4][3])]),
               (b"label", log_n, log_cell, key, comm, items[:4] + [items[4][:3] + (comm[0],)])]
    for args in changed:
        got = native(*args)
        assert got == V.challenge(*args) and got not in seen
        seen.add(got)
