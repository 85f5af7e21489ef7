"""GPU: KZG10 commitments of many short vectors on a domain handle (plonk_kzg_many_tables_build, plonk_kzg_commit_many / _dev,
plonk_kzg_update_many), from the kernels up.

The kernels of plonk_amd/csrc/kzg_many.hip run alone through the door tests/csrc/dev_kzg_many.hip: the table build against the
model's entry (i, w, d), the accumulation and the compression over tables of TEST-OWNED points with known discrete logs — the
handle's real Lagrange points, and a designed set in which points repeat and cancel so that a lane's running sum meets its
next addend, its negative, and lane sums meet their opposites in the tree.  The calls are checked against the closed form
[sum_i e_i L_i(tau)] G (the tests know tau) and against plonk_kzg_commit_evals, an independently tested route."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

from oracle import bls12_381 as E
from tests import kzg_evals_model as EM
from tests import kzg_many_model as M
from tests import kzg_ref as K
from tests import msm_tail_model as T
from tests.test_gpu_kzg_evals import Guarded, load_key

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_many.so")
Q, P_MOD = E.Q, T.P
OK, ERR_ARG, ERR_STATE, ERR_DATA, ERR_POINT = 0, -1, -7, -9, -10
ID48 = K.IDENTITY48
KEY_POINTS = 1 << 8


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, KEY_POINTS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def door():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_many.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dkm_tables_fill.argtypes = [vp, vp, u32, u32, vp]
    so.dkm_commit.argtypes = [vp, vp, u32, u32, vp, u64, u32, vp, vp]
    so.dkm_sparse.argtypes = [vp, vp, u32, u32, vp, vp, vp, u64, vp, vp]
    so.dkm_set_slices.argtypes = [vp, u32]
    so.dkm_const.argtypes = [ci]
    so.dkm_const.restype = u64
    return so


def mont(values):
    import plonk_amd
    return plonk_amd.fr_to_bytes_mont(values)


def commit_of(scalar):
    """48 bytes of [scalar] G"""
    return E.g1_compress(T.affine_g(scalar)) if scalar % Q else ID48


def raw96(scalar):
    import plonk_amd
    return plonk_amd.g1_to_raw96(T.affine_g(scalar)) if scalar % Q else bytes(96)


# ---- the point sets: discrete logs the tests know ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lagrange_logs(log_n, tau=K.TAU):
    """L_i(tau) g: the discrete logs (to the base G) of the handle's Lagrange points"""
    return tuple(x * K.G_SCALAR % Q for x in EM.lagrange_at(tau, log_n))


def random_vector(rnd, n):
    return [rnd.randrange(Q) for _ in range(n)]


def designed(log_n):
    """(logs, vectors) for n = 2^log_n >= 128, one value per lane and pass (lane k owns the values k, k + 64, ...): random points
    except where a later value of a lane is given the point that makes its single entry EQUAL or OPPOSITE to what the lane has
    summed so far, and lanes 32 apart (the first level of the tree) are given equal and opposite points"""
    n = 1 << log_n
    rnd = random.Random(900 + log_n)
    logs = [rnd.randrange(1, Q) for _ in range(n)]
    r = [rnd.randrange(Q) for _ in range(8)]
    vectors = {}
    # the first pair of a lane is twice the same point: pair_distinct is false, the general path doubles
    logs[64 + 3] = logs[3]
    vectors["first pair equal"] = {3: 1, 64 + 3: 1}
    # ... and opposite points: the lane's sum is the identity
    logs[64 + 4] = Q - logs[4]
    vectors["first pair opposite"] = {4: 1, 64 + 4: 1}
    # a running sum of many entries equals its next addend: the doubling branch of add_affine with Z != 1
    logs[64 + 5] = r[0] * logs[5] % Q
    vectors["running sum equals the next addend"] = {5: r[0], 64 + 5: 1}
    # ... is the negative of its next addend: the identity mid-chain
    logs[64 + 6] = Q - r[1] * logs[6] % Q
    vectors["running sum cancels"] = {6: r[1], 64 + 6: 1}
    if n >= 256:   # and the chain goes on after it
        vectors["running sum cancels and the chain goes on"] = {6: r[1], 64 + 6: 1, 128 + 6: r[2], 192 + 6: r[3]}
    # two lane sums that enter the tree are opposite / equal (lanes 7 | 39, 8 | 40)
    logs[39] = Q - logs[7]
    vectors["tree: opposite lane sums"] = {7: r[4], 39: r[4], 20: 5}
    logs[40] = logs[8]
    vectors["tree: equal lane sums"] = {8: r[5], 40: r[5]}
    vectors["tree: everything cancels"] = {7: r[6], 39: r[6]}
    out = {}
    for name, sparse in vectors.items():
        v = [0] * n
        for i, x in sparse.items():
            v[i] = x
        out[name] = v
    out["random over the designed points"] = random_vector(rnd, n)
    return logs, out


def shaped_vectors(log_n, c):
    n, W = 1 << log_n, M.windows(c)
    rnd = random.Random(31 * log_n + c)
    half = 1 << (c - 1)
    top = sum(half << (c * w) for w in range(W - 1))                # every digit at its maximum (below q)
    assert top < Q and M.recode(top, c, W)[0].count(half) == W - 1
    out = {"all zeros": [0] * n, "q - 1 everywhere": [Q - 1] * n, "the all-maximum-digit value": [top] * n,
           "random": random_vector(rnd, n), "random, sparse": [rnd.randrange(Q) if rnd.random() < 0.3 else 0 for _ in range(n)]}
    for lane in sorted({0, min(63, n - 1), n - 1}):
        out["a single 1 at %d" % lane] = [int(i == lane) for i in range(n)]
    return out


class Tables:
    """window tables over points with the discrete logs `logs`, built through the door"""

    def __init__(self, ctx, door, log_n, c, logs):
        self.ctx, self.door, self.log_n, self.c, self.logs = ctx, door, log_n, c, list(logs)
        lag = ctx.alloc(96 << log_n)
        lag.upload(b"".join(raw96(x) for x in logs))
        self.buf = Guarded(ctx, M.table_bytes(log_n, c))
        assert door.dkm_tables_fill(ctx.handle, lag.ptr, log_n, c, self.buf.ptr) == OK
        lag.free()

    def words(self):
        return np.frombuffer(self.buf.read(), dtype=np.uint32).reshape(-1, 32)

    def commit(self, vectors, slices=1):
        """the 48-byte commitments of the vectors through accumulation + compression, outputs guarded"""
        n, count = 1 << self.log_n, len(vectors)
        vals = self.ctx.alloc(32 * n * count)
        vals.upload(b"".join(mont(v) for v in vectors))
        partial = Guarded(self.ctx, 256 * slices * count)
        out = Guarded(self.ctx, 48 * count)
        assert self.door.dkm_commit(self.ctx.handle, self.buf.ptr, self.log_n, self.c, vals.ptr, count, slices, partial.ptr, out.ptr) == OK
        raw = out.read()
        partial.read()
        for b in (vals, partial, out):
            b.free()
        return [raw[48 * j:48 * j + 48] for j in range(count)]

    def want(self, vector):
        return commit_of(sum(a * b for a, b in zip(vector, self.logs)) % Q)

    def free(self):
        self.buf.free()


def decode_entry(words32):
    """a table entry -> None (128 zero bytes) or the affine point, x, y < 2p checked"""
    if not words32.any():
        return None
    x, y = T.raw_coords(words32)
    assert x < 2 * P_MOD and y < 2 * P_MOD, "a table coordinate is not below 2p"
    return x * T.FP28_RINV % P_MOD, y * T.FP28_RINV % P_MOD


# ---- the table build alone --------------------------------------------------------------------------------------------------------
def test_every_table_entry_at_2_to_2_points_width_4(ctx, door):
    log_n, c = 2, 4
    t = Tables(ctx, door, log_n, c, lagrange_logs(log_n))
    words, W = t.words(), M.windows(c)
    assert len(words) == M.table_entries(log_n, c) == 4 * 64 * 8
    for i in range(4):
        for w in range(W):
            base = M.entry_scalar(log_n, c, i, w, 1) * K.G_SCALAR % Q
            assert base == (t.logs[i] << (c * w)) % Q
            for d in range(1, 9):
                assert decode_entry(words[M.entry_index(c, i, w, d)]) == T.affine_g(d * base), (i, w, d)
    t.free()


def test_corner_and_random_entries_at_2_to_8_points_width_8(ctx, door):
    log_n, c = 8, 8
    t = Tables(ctx, door, log_n, c, lagrange_logs(log_n))
    words, W = t.words(), M.windows(c)
    assert len(words) * 128 == 128 << 20
    rnd = random.Random(88)
    picks = {(i, w, d) for i in (0, 255) for w in (0, W - 1) for d in (1, 128)}
    while len(picks) < 8 + 64:
        picks.add((rnd.randrange(256), rnd.randrange(W), rnd.randrange(1, 129)))
    for i, w, d in sorted(picks):
        want = T.affine_g(M.entry_scalar(log_n, c, i, w, d) * K.G_SCALAR)
        assert decode_entry(words[M.entry_index(c, i, w, d)]) == want, (i, w, d)
    t.free()


def test_identity_lagrange_points_are_marked_and_skipped():
    """tau = w^1 at 2^2 points: L_1 = G's multiple, every other Lagrange point the identity"""
    import plonk_amd as P
    log_n, c = 2, 4
    tau = EM.domain_points(log_n)[1]
    cx = P.Context(0)
    load_key(cx, 8, tau=tau)
    dom = P.KzgDomain(cx, log_n)
    assert dom.build_many_tables(c)["built"] == 1
    rnd = random.Random(12)
    vectors = [[0, 5, 0, 0], [7, 0, 9, 11], random_vector(rnd, 4), [Q - 1] * 4, [0] * 4]
    want = [M.commitment(v, log_n, tau) for v in vectors]
    assert want[0] == K.scalar_commit(5) and want[1] == ID48 == want[4]
    assert dom.commit_many(vectors) == want == dom.commit_evals(vectors)
    assert dom.update_many([[(0, 3), (1, 4), (3, 9)], [(2, 1)]]) == [K.scalar_commit(4), ID48]
    dom.close()
    cx.close()


def test_identity_points_give_zero_entries_through_the_door(ctx, door):
    log_n, c = 2, 4
    t = Tables(ctx, door, log_n, c, [0, 77, 0, 0])
    words = t.words().reshape(4, -1)
    assert not words[0].any() and not words[2].any() and not words[3].any() and words[1].reshape(-1, 32).any(axis=1).all()
    rnd = random.Random(13)
    vectors = [random_vector(rnd, 4), [1, 0, 1, 1], [0, Q - 1, 0, 0]]
    assert t.commit(vectors) == [t.want(v) for v in vectors]
    assert t.want(vectors[1]) == ID48
    t.free()


# ---- accumulation and compression alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 5, 6, 7, 8])
def test_accumulation_and_compression_against_the_closed_form(ctx, door, log_n):
    """windows spread over the lanes (2^1, 2^2, 2^5 values), one value per lane (2^6), two and four per lane; widths 2, 4, 5, 8;
    one slice, two, and as many as a wave has lanes (one value per slice: its windows over all 64 lanes)"""
    flags = set()
    for c in (2, 4, 5, 8):
        t = Tables(ctx, door, log_n, c, lagrange_logs(log_n))
        shaped = shaped_vectors(log_n, c)
        names = list(shaped)
        want = [t.want(shaped[k]) for k in names]
        assert want[names.index("all zeros")] == ID48
        for slices in sorted({1, 2, min(1 << log_n, 64)}):
            got = t.commit([shaped[k] for k in names], slices)
            for k, g, w in zip(names, got, want):
                assert g == w, (c, slices, k)
        flags |= {w[0] & 0xE0 for w in want}
        t.free()
    assert {0x80, 0xA0, 0xC0} <= flags, "y in either half and the identity all occur"


@pytest.mark.parametrize("log_n", [7, 8])
def test_designed_points_doubling_cancelling_and_the_tree(ctx, door, log_n):
    logs, vectors = designed(log_n)
    names = list(vectors)
    for c in (4, 8):
        t = Tables(ctx, door, log_n, c, logs)
        want = [t.want(vectors[k]) for k in names]
        assert want[names.index("first pair opposite")] == ID48 == want[names.index("running sum cancels")]
        assert want[names.index("tree: everything cancels")] == ID48
        assert want[names.index("first pair equal")] == commit_of(2 * logs[3])
        assert want[names.index("tree: opposite lane sums")] == commit_of(5 * logs[20])
        for slices in (1, 2):           # two slices: the designed pairs 64 apart still share a lane at 2^8, lanes 32 apart always do
            got = t.commit([vectors[k] for k in names], slices)
            for k, g, w in zip(names, got, want):
                assert g == w, (c, slices, k)
        t.free()


def test_sparse_accumulation_through_the_door(ctx, door):
    """the second loader: segments of 0, 1, 2, 63, 64, 65 and 200 terms, repeated indices (the first pair of a lane equal: terms
    k and k + 64 of a segment), a segment that cancels"""
    log_n, c, n = 6, 8, 64
    t = Tables(ctx, door, log_n, c, lagrange_logs(log_n))
    rnd = random.Random(44)
    segs = [[(rnd.randrange(n), rnd.randrange(Q)) for _ in range(k)] for k in (0, 1, 2, 63, 64, 65, 200)]
    segs.append([(9, 1)] * 65)                                          # lane 0: 1 L_9 + 1 L_9
    segs.append([(5, 3), (5, Q - 3)])                                   # two lanes, opposite sums
    segs.append([(7, 1)] + [(0, 0)] * 63 + [(7, Q - 1)])                # one lane, sum then its negative
    offs = [0]
    for s in segs:
        offs.append(offs[-1] + len(s))
    flat = [x for s in segs for x in s]
    o = ctx.alloc(8 * len(offs))
    o.upload(np.array(offs, dtype=np.uint64).tobytes())
    ix = ctx.alloc(4 * len(flat))
    ix.upload(np.array([i for i, _ in flat], dtype=np.uint32).tobytes())
    dl = ctx.alloc(32 * len(flat))
    dl.upload(mont([x for _, x in flat]))
    partial, out = Guarded(ctx, 256 * len(segs)), Guarded(ctx, 48 * len(segs))
    assert door.dkm_sparse(ctx.handle, t.buf.ptr, log_n, c, o.ptr, ix.ptr, dl.ptr, len(segs), partial.ptr, out.ptr) == OK
    raw = out.read()
    partial.read()
    want = [commit_of(sum(x * t.logs[i] for i, x in s) % Q) for s in segs]
    assert [raw[48 * j:48 * j + 48] for j in range(len(segs))] == want
    assert want[0] == ID48 == want[8] == want[9] and want[7] == commit_of(65 * t.logs[9])
    for b in (o, ix, dl, partial, out, t):
        b.free()


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
def assert_many_last(dom, plan, built=None):
    last = dom.many_last()
    for k in ("log_n", "window_bits", "windows", "count", "terms", "chunks", "chunk_vectors", "slices", "additions"):
        assert last[k] == plan[k], k
    assert last["table_bytes"] == M.table_bytes(plan["log_n"], plan["window_bits"])
    if built is not None:
        assert last["built"] == built


def resident_commit(ctx, dom, vectors):
    n, count = dom.n, len(vectors)
    vals = ctx.alloc(max(32 * n * count, 32))
    if count:
        vals.upload(b"".join(mont(v) for v in vectors))
    out = Guarded(ctx, 48 * count)
    dom.commit_many_dev(vals.ptr, count, out.ptr)
    raw = out.read()
    vals.free()
    out.free()
    return [raw[48 * j:48 * j + 48] for j in range(count)]


@pytest.fixture(scope="module")
def dom6(ctx):
    import plonk_amd
    d = plonk_amd.KzgDomain(ctx, 6)
    info = d.build_many_tables(8)
    assert (info["window_bits"], info["windows"], info["built"], info["table_bytes"]) == (8, 32, 1, M.table_bytes(6, 8))
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def vectors6():
    rnd = random.Random(66)
    v = [random_vector(rnd, 64) for _ in range(65)]
    return v, [M.commitment(e, 6) for e in v]


@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65])
def test_commit_many_host_and_resident_against_the_closed_form(ctx, dom6, count):
    v, want = vectors6()
    assert dom6.commit_many(v[:count]) == want[:count]
    assert_many_last(dom6, M.plan(6, 8, count, host_form=True))
    assert resident_commit(ctx, dom6, v[:count]) == want[:count]
    assert_many_last(dom6, M.plan(6, 8, count, host_form=False))
    assert dom6.many_last()["slices"] == 1, "64 values: one per lane, nothing to cut"


def test_a_second_build_and_another_width(ctx, dom6):
    v, want = vectors6()
    held = ctx.table_bytes()[0]
    assert dom6.build_many_tables(8)["built"] == 0 and ctx.table_bytes()[0] == held
    info = dom6.build_many_tables(5)
    assert (info["window_bits"], info["windows"], info["built"]) == (5, 52, 1)
    assert ctx.table_bytes()[0] == held - M.table_bytes(6, 8) + M.table_bytes(6, 5)
    assert dom6.commit_many(v[:3]) == want[:3]
    assert_many_last(dom6, M.plan(6, 5, 3, host_form=True))
    assert dom6.build_many_tables(0)["window_bits"] == 8, "the widest width fits the default budget"
    assert ctx.table_bytes()[0] == held
    assert dom6.commit_many(v[:3]) == want[:3]


def test_forced_slices_and_a_chunk_boundary(ctx, door, dom6):
    v, want = vectors6()
    try:
        for slices in (1, 4):
            assert door.dkm_set_slices(dom6.handle, slices) == OK
            assert dom6.commit_many(v[:5]) == want[:5] == resident_commit(ctx, dom6, v[:5])
            assert_many_last(dom6, M.plan(6, 8, 5, force_slices=slices))
            assert dom6.many_last()["slices"] == slices
        # the cap lowered to three vectors of the resident form, four slices each: 7 vectors cross two chunk boundaries
        dom6._set_workspace_cap(3 * (256 * 4 + 48))
        assert resident_commit(ctx, dom6, v[:7]) == want[:7]
        p = M.plan(6, 8, 7, ws_cap=3 * (256 * 4 + 48), force_slices=4)
        assert (p["chunks"], p["chunk_vectors"]) == (3, 3)
        assert_many_last(dom6, p)
        # ... and to one vector of the host form
        dom6._set_workspace_cap(1)
        assert dom6.commit_many(v[:3]) == want[:3]
        p = M.plan(6, 8, 3, ws_cap=1, host_form=True, force_slices=4)
        assert (p["chunks"], p["chunk_vectors"]) == (3, 1)
        assert_many_last(dom6, p)
    finally:
        dom6._set_workspace_cap(0)
        door.dkm_set_slices(dom6.handle, 0)


def test_4097_vectors_of_4_values_equal_commit_evals(ctx):
    import plonk_amd as P
    dom = P.KzgDomain(ctx, 2)
    dom.build_many_tables()
    dom.build_tables()                                                   # the grouped table route for the comparison
    rnd = random.Random(4097)
    v = [random_vector(rnd, 4) for _ in range(4097)]
    got = dom.commit_many(v)
    assert_many_last(dom, M.plan(2, 8, 4097, host_form=True))
    assert dom.many_last()["slices"] == 1
    assert got == dom.commit_evals(v) == resident_commit(ctx, dom, v)
    assert got[:3] == [M.commitment(e, 2) for e in v[:3]]
    dom.close()


def test_update_many(ctx, dom6):
    v, want = vectors6()
    rnd = random.Random(67)
    n = 64
    # base == NULL: a sparse commit equals commit_many of the scattered vector
    ups = [[(rnd.randrange(n), rnd.randrange(Q)) for _ in range(k)] for k in (1, 0, 3, 64, 150)]
    ups.append([(11, 5), (11, 6), (11, Q - 11)])                        # a repeated index simply adds: here to zero
    scattered = []
    for u in ups:
        e = [0] * n
        for i, x in u:
            e[i] = (e[i] + x) % Q
        scattered.append(e)
    got = dom6.update_many(ups)
    assert got == dom6.commit_many(scattered) == [M.commitment(e, 6) for e in scattered]
    assert got[1] == ID48 == got[5]
    dom6.update_many(ups)
    assert_many_last(dom6, M.sparse_plan(6, 8, [0, 1, 1, 4, 68, 218, 221]))
    # with bases: the commitment of old + delta; an empty segment returns its base re-encoded; the identity is a legal base
    old = v[:6]
    base = want[:5] + [ID48]
    new = [[(a + b) % Q for a, b in zip(o, s)] for o, s in zip(old[:5], scattered[:5])] + [scattered[5]]
    got = dom6.update_many(ups, base=base)
    assert got == [M.commitment(e, 6) for e in new]
    assert got[1] == want[1] and got[5] == ID48
    assert dom6.update_many([[], [(0, 1)]], base=[ID48, ID48]) == [ID48, commit_of(lagrange_logs(6)[0])]
    # chunks of the sparse form: the cap lowered to two single-term segments
    dom6._set_workspace_cap(2 * (304 + 36))
    try:
        singles = [[(j % n, j + 1)] for j in range(5)]
        assert dom6.update_many(singles, base=want[:5]) == [M.updated(sum(a * b for a, b in zip(v[j], EM.lagrange_at(K.TAU, 6))), singles[j], 6)
                                                           for j in range(5)]
        p = M.sparse_plan(6, 8, list(range(6)), 2 * (304 + 36))
        assert (p["chunks"], p["chunk_vectors"]) == (3, 2)
        assert_many_last(dom6, p)
    finally:
        dom6._set_workspace_cap(0)


def test_errors_leave_the_outputs_untouched(ctx, dom6):
    lib, h, n = ctx.lib, dom6.handle, 64
    good = mont(list(range(1, 2 * n + 1)))
    noncanon = good[:32 * 70] + b"\xff" * 32 + good[32 * 71:]
    cm = ctypes.create_string_buffer(b"\xA5" * 144, 144)
    # commit_many, host form
    assert lib.plonk_kzg_commit_many(None, good, 2, cm) == ERR_ARG
    assert lib.plonk_kzg_commit_many(h, None, 2, cm) == ERR_ARG and lib.plonk_kzg_commit_many(h, good, 2, None) == ERR_ARG
    assert lib.plonk_kzg_commit_many(h, good, (1 << 24) + 1, cm) == ERR_ARG
    assert lib.plonk_kzg_commit_many(h, noncanon, 2, cm) == ERR_DATA
    # resident form: device pointers in and out
    vals, out = ctx.alloc(len(good)), Guarded(ctx, 96)
    vals.upload(noncanon)
    assert lib.plonk_kzg_commit_many_dev(h, vals.ptr, 2, out.ptr) == ERR_DATA
    assert lib.plonk_kzg_commit_many_dev(h, None, 2, out.ptr) == ERR_ARG and lib.plonk_kzg_commit_many_dev(h, vals.ptr, 2, None) == ERR_ARG
    assert lib.plonk_kzg_commit_many_dev(h, vals.ptr + 8, 1, out.ptr) == ERR_ARG, "misaligned values"
    assert lib.plonk_kzg_commit_many_dev(h, vals.ptr, 2, out.ptr + 1) == ERR_ARG, "misaligned output"
    assert out.read() == b"\xA5" * 96
    vals.upload(good)
    assert lib.plonk_kzg_commit_many_dev(h, vals.ptr, 1, out.ptr) == OK
    assert out.read() == M.commitment(list(range(1, n + 1)), 6) + b"\xA5" * 48
    vals.free()
    out.free()
    # update_many
    u64s, u32s = lambda xs: (ctypes.c_uint64 * len(xs))(*xs), lambda xs: (ctypes.c_uint32 * len(xs))(*xs)
    offs, idx, deltas = u64s([0, 1, 3]), u32s([1, 2, 63]), mont([4, 5, 6])
    base = commit_of(9) + ID48
    upd = lib.plonk_kzg_update_many
    assert upd(None, base, offs, idx, deltas, 2, cm) == ERR_ARG
    assert upd(h, base, None, idx, deltas, 2, cm) == ERR_ARG and upd(h, base, offs, None, deltas, 2, cm) == ERR_ARG
    assert upd(h, base, offs, idx, None, 2, cm) == ERR_ARG and upd(h, base, offs, idx, deltas, 2, None) == ERR_ARG
    assert upd(h, base, offs, idx, deltas, (1 << 24) + 1, cm) == ERR_ARG
    assert upd(h, base, u64s([1, 1, 3]), idx, deltas, 2, cm) == ERR_ARG, "offsets start at 0"
    assert upd(h, base, u64s([0, 3, 2]), idx, deltas, 2, cm) == ERR_ARG, "offsets never decrease"
    assert upd(h, base, u64s([0, 1, (1 << 28) + 1]), idx, deltas, 2, cm) == ERR_ARG, "the total above its cap"
    assert upd(h, base, u64s([0, 1, 2 + M.MAX_SEGMENT]), idx, deltas, 2, cm) == ERR_ARG, "one segment above its cap"
    assert upd(h, base, offs, u32s([1, 2, 64]), deltas, 2, cm) == ERR_ARG, "an index >= n"
    assert upd(h, base, offs, idx, mont([4, 5]) + b"\xff" * 32, 2, cm) == ERR_DATA
    off_curve = bytes([0x80]) + bytes(46) + bytes([2])                   # x = 2: x^3 + 4 = 12 is not a square mod p
    assert pow(12, (P_MOD - 1) // 2, P_MOD) != 1
    assert upd(h, base[:48] + b"\x00" * 48, offs, idx, deltas, 2, cm) == ERR_POINT, "a base without the compression flag"
    assert upd(h, base[:48] + off_curve, offs, idx, deltas, 2, cm) == ERR_POINT
    assert cm.raw == b"\xA5" * 144
    assert upd(h, base, offs, idx, deltas, 2, cm) == OK
    L = lagrange_logs(6)
    assert cm.raw[:96] == commit_of(9 + 4 * L[1]) + commit_of(5 * L[2] + 6 * L[63]) and cm.raw[96:] == b"\xA5" * 48
    # the build
    assert lib.plonk_kzg_many_tables_build(None, 8) == ERR_ARG and lib.plonk_kzg_many_tables_drop(None) == ERR_ARG
    for bits in (1, 9, 255):
        assert lib.plonk_kzg_many_tables_build(h, bits) == ERR_ARG
    import plonk_amd as P
    assert lib.plonk_kzg_many_last(h, None) == ERR_ARG and lib.plonk_kzg_many_last(None, ctypes.byref(P._KzgManyInfo())) == ERR_ARG
    assert dom6.many_last()["window_bits"] == 8


def test_a_base_outside_the_subgroup_is_refused(ctx, dom6):
    """a point of the curve that is not in the prime-order subgroup (the cofactor is not 1): found by trying x = 1, 2, ..."""
    x = 1
    while True:
        y2 = (x * x * x + 4) % P_MOD
        y = pow(y2, (P_MOD + 1) // 4, P_MOD)
        if y * y % P_MOD == y2 and E.g1_add(E.g1_mul((x, y), Q - 1), (x, y)) is not None:   # (g1_mul reduces its scalar mod q)
            break
        x += 1
    bad = E.g1_compress((x, y))
    cm = ctypes.create_string_buffer(b"\xA5" * 48, 48)
    offs, idx = (ctypes.c_uint64 * 2)(0, 1), (ctypes.c_uint32 * 1)(0)
    assert ctx.lib.plonk_kzg_update_many(dom6.handle, bad, offs, idx, mont([1]), 1, cm) == ERR_POINT
    assert cm.raw == b"\xA5" * 48


def test_calls_refuse_without_tables_after_a_drop_after_a_reload_and_on_a_communicator_context():
    import plonk_amd as P
    c = P.Context(0)
    load_key(c, 64)
    d = P.KzgDomain(c, 6)
    held = c.table_bytes()[0]
    e = [list(range(1, 65))]
    calls = (lambda: d.commit_many(e), lambda: d.update_many([[(0, 1)]]), lambda: d.commit_many([]))
    vals, out = c.alloc(32 * 64), Guarded(c, 48)
    vals.upload(mont(e[0]))

    def refused(fns, code=ERR_STATE):
        for call in fns:
            with pytest.raises(P.PlonkError) as ei:
                call()
            assert ei.value.code == code
        # the resident form, its output guarded: refused before anything is queued or written
        assert c.lib.plonk_kzg_commit_many_dev(d.handle, vals.ptr, 1, out.ptr) == code
        assert out.read() == b"\xA5" * 48
        cm = ctypes.create_string_buffer(b"\xA5" * 48, 48)
        assert c.lib.plonk_kzg_commit_many(d.handle, mont(e[0]), 1, cm) == code and cm.raw == b"\xA5" * 48
    assert d.many_last() == {"log_n": 6, "window_bits": 0, "windows": 0, "built": 0, "table_bytes": 0, "count": 0, "terms": 0,
                             "chunks": 0, "chunk_vectors": 0, "slices": 0, "additions": 0}
    refused(calls)                                                       # before the build: no silent fallback
    info = d.build_many_tables(4)
    assert c.table_bytes()[0] == held + M.table_bytes(6, 4) == held + info["table_bytes"]
    assert d.evals_last()["lagrange_bytes"] == 96 * 64                   # the build made the points
    want = d.commit_many(e)
    assert want == [M.commitment(e[0], 6)] == d.commit_evals(e)
    d.commit_many_dev(vals.ptr, 1, out.ptr)
    assert out.read() == want[0]
    out.buf.upload(b"\xA5" * out.buf.nbytes)
    d.drop_many_tables()
    assert c.table_bytes()[0] == held and d.many_last()["window_bits"] == 0
    refused(calls)                                                       # after the drop
    d.drop_many_tables()
    d.build_many_tables(4)
    # a communicator context
    c.comm_init(P.Context.comm_unique_id(), 0, 1)
    refused(calls)
    assert c.lib.plonk_kzg_many_tables_build(d.handle, 5) == ERR_STATE and d.many_last()["window_bits"] == 4
    c.comm_destroy()
    assert d.commit_many(e) == want
    # a reloaded key: the calls and the build refuse, the drop works and gives the bytes back
    with_tables = c.table_bytes()[0]
    load_key(c, 64)
    held = c.table_bytes()[0] - (with_tables - held)
    refused(calls)
    assert c.lib.plonk_kzg_many_tables_build(d.handle, 4) == ERR_STATE
    d.drop_many_tables()
    assert c.table_bytes()[0] == held
    d.close()
    vals.free()
    out.free()
    # destroy gives them back too
    d2 = P.KzgDomain(c, 6)
    d2.build_many_tables(4)
    assert c.table_bytes()[0] == held + M.table_bytes(6, 4) and d2.commit_many(e) == want
    d2.close()
    assert c.table_bytes()[0] == held
    d3 = P.KzgDomain(c, 6)
    d3.build_many_tables(2)
    c.lib.plonk_kzg_domain_destroy(d3.handle)                            # without the binding's own drop
    d3.handle = None
    assert c.table_bytes()[0] == held
    c.close()


def test_a_build_refused_for_budget_changes_nothing_and_the_automatic_width_follows_the_budget():
    import plonk_amd as P
    c = P.Context(0, P.GpuConfig(table_budget_bytes=64 << 20))
    load_key(c, 256)
    held, budget = c.table_bytes()
    left = budget - held
    d = P.KzgDomain(c, 8)
    want_c = M.auto_width(8, left)
    assert 2 <= want_c < 8, "128 MiB of width-8 tables do not fit a 64 MiB budget"
    assert c.lib.plonk_kzg_many_tables_build(d.handle, 8) == ERR_ARG
    assert c.table_bytes() == (held, budget) and d.many_last()["window_bits"] == 0 and d.evals_last()["lagrange_bytes"] == 0
    info = d.build_many_tables(0)
    assert info["window_bits"] == want_c and c.table_bytes()[0] == held + M.table_bytes(8, want_c)
    assert c.lib.plonk_kzg_many_tables_build(d.handle, 8) == ERR_ARG, "refused with tables held: they stay"
    assert d.many_last()["window_bits"] == want_c and c.table_bytes()[0] == held + M.table_bytes(8, want_c)
    rnd = random.Random(3)
    e = [random_vector(rnd, 256)]
    assert d.commit_many(e) == [M.commitment(e[0], 8)]
    assert d.many_last()["slices"] == 4, "too few vectors to fill the device: cut into slices of 64 values"
    # another width is built BESIDE the tables it replaces: both must fit the budget for that moment
    assert want_c == 6
    assert M.table_bytes(8, 5) > budget - c.table_bytes()[0] and M.table_bytes(8, 5) <= left
    assert c.lib.plonk_kzg_many_tables_build(d.handle, 5) == ERR_ARG, "no room beside the width-6 tables"
    assert d.many_last()["window_bits"] == 6 and c.table_bytes()[0] == held + M.table_bytes(8, 6)
    assert d.build_many_tables(4)["built"] == 1 and c.table_bytes()[0] == held + M.table_bytes(8, 4)
    assert d.commit_many(e) == [M.commitment(e[0], 8)]
    info = d.build_many_tables(0)                                        # the widest for the budget without the old tables
    assert (info["window_bits"], info["built"]) == (6, 1) and c.table_bytes()[0] == held + M.table_bytes(8, 6)
    assert d.build_many_tables(0)["built"] == 0
    d.close()
    assert c.table_bytes() == (held, budget)
    c.close()


def test_a_domain_above_2_to_12_is_refused():
    import plonk_amd as P
    c = P.Context(0)
    load_key(c, 1 << 13)
    d = P.KzgDomain(c, 13)
    held = c.table_bytes()
    assert c.lib.plonk_kzg_many_tables_build(d.handle, 2) == ERR_ARG and c.lib.plonk_kzg_many_tables_build(d.handle, 0) == ERR_ARG
    assert c.table_bytes() == held
    d.close()
    c.close()


def test_commitments_feed_a_multiproof(ctx, dom6):
    import plonk_amd as P
    v, want = vectors6()
    key = P.KzgKey(ctx, K.opening_key())
    vectors = v[:4]
    cms = dom6.commit_many(vectors)
    items = [(0, 3), (1, 3), (3, 63), (2, 0)]
    values, bound, proof = dom6.open_multi(vectors, items, commitments=cms)
    assert bound == cms and values == [vectors[j][m] for j, m in items]
    assert key.check_multi(6, cms, items, values, proof)
    key.close()


def test_context_left_as_found_with_the_tables_held():
    """plonk_ctx_last_msm, plonk_ctx_last_msm_points and a prover's proof bytes on the same context are what they were, with the
    handle's many-vector tables built, used and still held meanwhile; the only trace is the handle's share of plonk_ctx_table_bytes"""
    import plonk_amd as P
    from tests import circuits as C
    c = P.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=78)()
    case = C.compile_fast(comp, b"kzg-many")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = P.Prover.compile(c, b"kzg-many", cols["selectors"], cols["wires"], cols["witnesses"])
    rnd = random.Random(77)
    proof = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    c.msm([rnd.randrange(Q) for _ in range(100)])
    msm_report = c.last_msm()
    c.msm_points([E.g1_mul(E.G1_GEN, 3), E.g1_mul(E.G1_GEN, 5)], [2, 9])
    points_report = c.last_msm_points()
    dom = P.KzgDomain(c, 6)
    tables, rows = c.table_bytes(), c.table_rows()
    info = dom.build_many_tables()
    e = [random_vector(rnd, 64) for _ in range(6)]
    assert dom.commit_many(e) == [M.commitment(x, 6) for x in e]
    assert dom.update_many([[(1, 2)], []], base=[ID48, ID48])[1] == ID48
    assert c.last_msm() == msm_report
    assert c.last_msm_points() == points_report
    assert prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3)) == proof
    assert c.table_bytes() == (tables[0] + info["table_bytes"], tables[1]) and c.table_rows() == rows
    dom.close()
    assert c.table_bytes() == tables
    prover.close()
    c.close()
