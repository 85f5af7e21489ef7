"""GPU: KZG10 vector-commitment trees on a domain handle (plonk_kzg_tree_*), from the kernels up.

The three kernels of plonk_amd/csrc/kzg_tree.hip run alone through the door tests/csrc/dev_kzg_tree.hip: the map h against
oracle/merlin.py, the finish kernel over partial sums with known discrete logs (made by the sparse accumulation of kzg_many.hip
over TEST-OWNED points, through its own door), the delta kernel against subtraction mod q.  The calls are checked against the
big-int model tests/kzg_tree_model.py, which knows tau: every node of every level, after a build and after every update."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle import bls12_381 as E
from tests import kzg_many_model as MM
from tests import kzg_ref as K
from tests import kzg_tree_model as M
from tests import msm_tail_model as T
from tests.test_gpu_kzg_evals import Guarded, load_key

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_tree.so")
SO_MANY = os.path.join(HERE, "_build", "libdev_kzg_many.so")
Q = E.Q
OK, ERR_ARG, ERR_STATE, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -7, -9, -10, -12
ID48 = K.IDENTITY48
KEY_POINTS = 1 << 8
VDEC_OK, VDEC_IDENTITY = 0, 1
NOT_CANONICAL = Q.to_bytes(32, "little")            # q itself as four raw limbs


def mont(values):
    import plonk_amd
    return plonk_amd.fr_to_bytes_mont(values)


def unmont(raw):
    import plonk_amd
    return plonk_amd.fr_from_bytes_mont(raw)


def commit_of(scalar):
    return E.g1_compress(T.affine_g(scalar)) if scalar % Q else ID48


def raw96(scalar):
    import plonk_amd
    return plonk_amd.g1_to_raw96(T.affine_g(scalar)) if scalar % Q else bytes(96)


def code_of(call):
    import plonk_amd
    with pytest.raises(plonk_amd.PlonkError) as ei:
        call()
    return ei.value.code


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, KEY_POINTS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key(ctx):
    import plonk_amd
    k = plonk_amd.KzgKey(ctx, K.opening_key())
    yield k
    k.close()


@pytest.fixture(scope="module")
def door():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_tree.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dkt_map.argtypes = [vp, vp, vp, u64, vp]
    so.dkt_finish.argtypes = [vp, vp, u32, vp, u64, u64, ci, vp, vp, vp]
    so.dkt_delta.argtypes = [vp, vp, vp, u64, vp, vp]
    return so


@pytest.fixture(scope="module")
def door_many():
    so = ctypes.CDLL(SO_MANY)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    so.dkm_tables_fill.argtypes = [vp, vp, u32, u32, vp]
    so.dkm_sparse.argtypes = [vp, vp, u32, u32, vp, vp, vp, u64, vp, vp]
    return so


def domain_of(ctx, log_n):
    import plonk_amd
    d = plonk_amd.KzgDomain(ctx, log_n)
    assert d.build_many_tables(8)["built"] == 1
    return d


@pytest.fixture(scope="module")
def dom1(ctx):
    d = domain_of(ctx, 1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dom2(ctx):
    d = domain_of(ctx, 2)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dom8(ctx):
    d = domain_of(ctx, 8)
    yield d
    d.close()


def random_leaves(seed, count):
    rnd = random.Random(seed)
    return [rnd.randrange(Q) for _ in range(count)]


@pytest.fixture(scope="module")
def leaves43():
    return random_leaves(43, 64)


@pytest.fixture(scope="module")
def model43(leaves43):
    """the reference of (4, 3), computed once and left unchanged"""
    return M.Tree(2, 3, leaves43)


@pytest.fixture(scope="module")
def leaves82():
    out = random_leaves(82, 1 << 16)
    out[256 * 9:256 * 10] = [0] * 256             # an all-zero bottom node: the identity commitment, hashed as such
    return out


@pytest.fixture(scope="module")
def model82(leaves82):
    return M.Tree(8, 2, leaves82)


def all_nodes(tree):
    return [tree.nodes(l) for l in range(tree.depth)]


# ---- the map kernel alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65])
def test_map_kernel_against_the_oracle_transcript(ctx, door, count):
    rnd = random.Random(500 + count)
    comps = [ID48 if k % 7 == 0 else commit_of(rnd.randrange(1, Q)) for k in range(count)]
    src = ctx.alloc(max(48 * count, 48))
    if count:
        src.upload(b"".join(comps))
    out = Guarded(ctx, 32 * count)
    assert door.dkt_map(ctx.handle, src.ptr, None, count, out.ptr) == OK
    assert unmont(out.read()) == [M.h(c) for c in comps]
    if count:
        assert comps[0] == ID48 and M.h(ID48) != 0
    src.free()
    out.free()


def test_map_kernel_through_a_node_list(ctx, door):
    rnd = random.Random(77)
    comps = [commit_of(rnd.randrange(1, Q)) for _ in range(70)]
    picks = [69, 0, 64, 63, 5]
    src, lst = ctx.alloc(48 * 70), ctx.alloc(8 * len(picks))
    src.upload(b"".join(comps))
    lst.upload(np.array(picks, dtype=np.uint64).tobytes())
    out = Guarded(ctx, 32 * len(picks))
    assert door.dkt_map(ctx.handle, src.ptr, lst.ptr, len(picks), out.ptr) == OK
    assert unmont(out.read()) == [M.h(comps[k]) for k in picks]
    for b in (src, lst, out):
        b.free()


# ---- the finish kernel alone -----------------------------------------------------------------------------------------------------------------
class Partials:
    """partial sums with known discrete logs: one segment [(0, x)] of the sparse accumulation over a table whose point 0 has
    the discrete log `a` gives x a; an empty segment gives the identity"""

    def __init__(self, ctx, door_many):
        self.ctx, self.door, self.log_n, self.c = ctx, door_many, 1, 8
        self.a = 0x1234567 * K.G_SCALAR % Q
        lag = ctx.alloc(96 * 2)
        lag.upload(raw96(self.a) + raw96(3 * self.a))
        self.table = ctx.alloc(MM.table_bytes(1, 8))
        assert door_many.dkm_tables_fill(ctx.handle, lag.ptr, 1, 8, self.table.ptr) == OK
        lag.free()

    def make(self, scalars):
        """a device buffer of len(scalars) slots: slot j = [scalars[j]] G (scalars as multiples of a: pass x, get x a)"""
        count = len(scalars)
        offs, flat = [0], []
        for x in scalars:
            if x % Q:
                flat.append(x % Q)
            offs.append(len(flat))
        o, ix, dl = self.ctx.alloc(8 * len(offs)), self.ctx.alloc(4 * max(len(flat), 1)), self.ctx.alloc(32 * max(len(flat), 1))
        o.upload(np.array(offs, dtype=np.uint64).tobytes())
        ix.upload(np.zeros(max(len(flat), 1), dtype=np.uint32).tobytes())
        if flat:
            dl.upload(mont(flat))
        partial, out = Guarded(self.ctx, 256 * count), self.ctx.alloc(48 * count)
        assert self.door.dkm_sparse(self.ctx.handle, self.table.ptr, 1, 8, o.ptr, ix.ptr, dl.ptr, count, partial.ptr, out.ptr) == OK
        partial.read()
        for b in (o, ix, dl, out):
            b.free()
        return partial

    def free(self):
        self.table.free()


def split(rnd, total, parts):
    """`parts` scalars that add up to total, the identity among them where parts allow"""
    if parts == 1:
        return [total % Q]
    head = [rnd.randrange(1, Q) for _ in range(parts - 1)]
    if parts == 4:
        head[1] = 0                                   # an identity slice between finite ones
    return head + [(total - sum(head)) % Q]


class Level:
    """the stored arrays of a level, guarded"""

    def __init__(self, ctx, nodes):
        self.nodes = nodes
        self.pts, self.kind, self.comp = Guarded(ctx, 96 * nodes), Guarded(ctx, 4 * nodes), Guarded(ctx, 48 * nodes)

    def read(self):
        pts, kind, comp = self.pts.read(), self.kind.read(), self.comp.read()
        return ([pts[96 * k:96 * k + 96] for k in range(self.nodes)], list(np.frombuffer(kind, dtype=np.int32)),
                [comp[48 * k:48 * k + 48] for k in range(self.nodes)])

    def free(self):
        for b in (self.pts, self.kind, self.comp):
            b.free()


def want_node(scalar):
    return (raw96(scalar), VDEC_IDENTITY if scalar % Q == 0 else VDEC_OK, commit_of(scalar))


@pytest.mark.parametrize("slices", [1, 2, 4])
def test_finish_kernel_without_and_with_a_base(ctx, door, door_many, slices):
    rnd = random.Random(600 + slices)
    ps = Partials(ctx, door_many)
    a, nodes = ps.a, 70                                # more than one block of 64 lanes
    # ---- no base, dense stores from node `first` on: random sums, the identity as a sum of identities and of opposite slices ----
    first = 3
    sums = [rnd.randrange(1, Q) for _ in range(nodes - first)]
    sums[0] = 0
    parts = [split(rnd, s, slices) for s in sums]
    parts[1] = [0] * slices
    sums[1] = 0
    partial = ps.make([x for p in parts for x in p])
    lv = Level(ctx, nodes)
    assert door.dkt_finish(ctx.handle, partial.ptr, slices, None, first, nodes - first, 0, lv.pts.ptr, lv.kind.ptr, lv.comp.ptr) == OK
    pts, kind, comp = lv.read()
    for k in range(first, nodes):
        assert (pts[k], kind[k], comp[k]) == want_node(sums[k - first] * a), k
    assert kind[first] == kind[first + 1] == VDEC_IDENTITY and comp[first] == ID48
    assert all(p == b"\xA5" * 96 for p in pts[:first]) and all(c == b"\xA5" * 48 for c in comp[:first]), "dense stores begin at `first`"
    partial.free()
    # ---- with the stored point as base, scattered through a node list ----
    stored = {k: sums[k - first] for k in range(first, nodes)}
    picks = {first: rnd.randrange(1, Q),               # identity base + a sum
             first + 1: 0,                             # identity base + identity sum
             10: 0,                                    # a base + the identity sum: the base again
             69: stored[69],                           # the partial EQUALS the base: the doubling branch
             5: Q - stored[5],                         # the partial is its NEGATIVE: the cancelling branch
             64: rnd.randrange(1, Q), 63: rnd.randrange(1, Q)}
    order = [69, first, 64, 5, first + 1, 63, 10]
    partial = ps.make([x for k in order for x in split(rnd, picks[k], slices)])
    lst = ctx.alloc(8 * len(order))
    lst.upload(np.array(order, dtype=np.uint64).tobytes())
    before = lv.read()
    assert door.dkt_finish(ctx.handle, partial.ptr, slices, lst.ptr, 0, len(order), 1, lv.pts.ptr, lv.kind.ptr, lv.comp.ptr) == OK
    pts, kind, comp = lv.read()
    for k in range(nodes):
        if k in picks:
            assert (pts[k], kind[k], comp[k]) == want_node((stored[k] + picks[k]) * a), k
        else:
            assert (pts[k], kind[k], comp[k]) == (before[0][k], before[1][k], before[2][k]), "a node outside the list was touched"
    assert comp[69] == commit_of(2 * stored[69] * a) and comp[5] == ID48 and kind[5] == VDEC_IDENTITY and comp[10] == before[2][10]
    for b in (partial, lst, lv, ps):
        b.free()


def test_delta_kernel(ctx, door):
    rnd = random.Random(31)
    vals = [rnd.randrange(Q) for _ in range(600)]
    flat = rnd.sample(range(600), 300)
    fresh = [rnd.randrange(Q) for _ in flat]
    fresh[0], fresh[1] = vals[flat[0]], 0               # a value replaced by itself: delta 0
    v, f, x = Guarded(ctx, 32 * 600), ctx.alloc(8 * 300), ctx.alloc(32 * 300)
    v.buf.upload(mont(vals), 32)
    f.upload(np.array(flat, dtype=np.uint64).tobytes())
    x.upload(mont(fresh))
    d = Guarded(ctx, 32 * 300)
    assert door.dkt_delta(ctx.handle, x.ptr, f.ptr, 300, v.ptr, d.ptr) == OK
    assert unmont(d.read()) == [(a - vals[j]) % Q for a, j in zip(fresh, flat)]
    want = list(vals)
    for a, j in zip(fresh, flat):
        want[j] = a
    assert unmont(v.read()) == want
    for b in (v, f, x, d):
        b.free()


# ---- build -------------------------------------------------------------------------------------------------------------------------------------
def assert_last(tree, **want):
    last = tree.last()
    assert (last["log_n"], last["depth"], last["leaves"]) == (tree.log_n, tree.depth, 1 << (tree.log_n * tree.depth))
    assert last["device_bytes"] >= M.data_bytes(tree.log_n, tree.depth)
    for k, v in want.items():
        assert last[k] == v, (k, last[k], v)


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 3)])
def test_build_every_node_against_the_model(ctx, dom1, dom2, shape):
    import plonk_amd
    log_n, depth = shape
    dom = {1: dom1, 2: dom2}[log_n]
    leaves = random_leaves(10 * log_n + depth, 1 << (log_n * depth))
    model = M.Tree(log_n, depth, leaves)
    tree = plonk_amd.KzgTree(dom, depth)
    assert_last(tree, built=0, kind=M.NONE)
    tree.build(leaves)
    assert all_nodes(tree) == model.all_nodes() and tree.root() == model.root
    assert tree.root() == dom.commit_evals([model.vals[0]])[0]
    counts = M.build_counts(log_n, depth, 8)
    assert_last(tree, built=1, kind=M.BUILD, touched_nodes=counts["touched_nodes"], chunks=counts["chunks"], sparse_terms=0, items=0)
    assert tree.nodes(depth - 1, 1, 0) == [] and tree.nodes(0, 0, 1) == [model.root]
    for bad in ((depth, 0, 1), (0, 1, 1), (0, 0, 2), (depth - 1, 1 << (log_n * (depth - 1)), 1)):
        assert code_of(lambda: tree.nodes(*bad)) == ERR_ARG
    tree.close()


def test_build_across_chunk_boundaries_and_from_resident_leaves(ctx, dom2, leaves43, model43):
    import plonk_amd
    tree = plonk_amd.KzgTree(dom2, 3)
    cap = 5 * 304                                       # five nodes per chunk: the level of 16 crosses three boundaries
    dom2._set_workspace_cap(cap)
    try:
        tree.build(leaves43)
        counts = M.build_counts(2, 3, 8, cap)
        assert counts["chunks"] == 1 + 1 + 4
        assert_last(tree, built=1, kind=M.BUILD, touched_nodes=21, chunks=6)
        assert all_nodes(tree) == model43.all_nodes()
    finally:
        dom2._set_workspace_cap(0)
    buf = ctx.alloc(32 * 64)
    buf.upload(mont(leaves43))
    other = plonk_amd.KzgTree(dom2, 3)
    other.build_dev(buf.ptr)
    assert all_nodes(other) == all_nodes(tree) == model43.all_nodes()
    assert_last(other, built=1, kind=M.BUILD, touched_nodes=21, chunks=3)
    assert code_of(lambda: other.build_dev(buf.ptr + 8)) == ERR_ARG
    assert_last(other, built=0, kind=M.NONE)
    buf.free()
    tree.close()
    other.close()


def test_build_at_2_to_8_depth_2_with_an_all_zero_node(ctx, dom8, leaves82, model82):
    """257 nodes: a real wave per node (four slices of 64 values), 256 map lanes across four waves"""
    import plonk_amd
    tree = plonk_amd.KzgTree(dom8, 2)
    tree.build(mont(leaves82))
    got = all_nodes(tree)
    assert got == model82.all_nodes()
    assert got[1][9] == ID48 and model82.vals[0][9] == M.h(ID48)
    assert tree.root() == dom8.commit_evals([model82.vals[0]])[0]
    assert_last(tree, built=1, kind=M.BUILD, touched_nodes=257, chunks=2)
    assert tree.last()["device_bytes"] >= M.data_bytes(8, 2) == 32 * (65536 + 256) + 148 * 257
    tree.close()


# ---- update ----------------------------------------------------------------------------------------------------------------------------------------
def run_updates(ctx, dom, depth, leaves, steps):
    """every step on one tree; after each, ALL nodes against a fresh build from the new leaves and against the model"""
    import plonk_amd
    log_n = dom.log_n
    tree, fresh = plonk_amd.KzgTree(dom, depth), plonk_amd.KzgTree(dom, depth)
    leaves = list(leaves)
    model = M.Tree(log_n, depth, leaves)
    tree.build(mont(leaves))
    for name, idx, vals in steps(leaves):
        tree.update(idx, vals)
        for j, v in zip(idx, vals):
            leaves[j] = v
        model.update(idx, vals)
        fresh.build(mont(leaves))
        got = all_nodes(tree)
        assert got == all_nodes(fresh), name
        assert got == model.all_nodes(), name
        counts = M.update_counts(log_n, depth, idx)
        assert_last(tree, built=1, kind=M.UPDATE, touched_nodes=counts["touched_nodes"], sparse_terms=counts["sparse_terms"],
                    chunks=M.update_chunks(log_n, depth, idx, MM.WS_CAP_DEFAULT))
    # refused: each with its code, every stored byte as it was
    N, before = len(leaves), all_nodes(tree)
    assert code_of(lambda: tree.update([3, 5, 3], [1, 2, 3])) == ERR_ARG
    assert code_of(lambda: tree.update([3, N], [1, 2])) == ERR_ARG
    assert code_of(lambda: tree.update([], [])) == ERR_ARG
    assert code_of(lambda: tree.update([3, 4], [mont([1]), NOT_CANONICAL])) == ERR_DATA
    assert all_nodes(tree) == before
    values, path, proof = tree.prove([3])
    assert values == [leaves[3]], "and the leaves too"
    tree.close()
    fresh.close()
    return model


def steps_of(log_n):
    n = 1 << log_n

    def steps(leaves):
        rnd = random.Random(7000 + log_n)
        N = len(leaves)
        yield "one leaf", [N - 1], [rnd.randrange(Q)]
        yield "two in one node", [n + 1, n], [rnd.randrange(Q), rnd.randrange(Q)]
        yield "two nodes under one parent", [2 * n - 1, 0], [rnd.randrange(Q), rnd.randrange(Q)]
        node = 2
        yield "a whole node", list(range(node * n, (node + 1) * n)), [rnd.randrange(Q) for _ in range(n)]
        yield "a value replaced by itself", [5], [leaves[5]]
        yield "a value replaced by itself, beside one that changes", [n + 2, n + 3], [leaves[n + 2], rnd.randrange(Q)]
        yield "every value of a node doubled", list(range(node * n, (node + 1) * n)), [2 * leaves[j] % Q for j in range(node * n, (node + 1) * n)]
        kept = leaves[3 * n:4 * n]
        yield "a node set to zero", list(range(3 * n, 4 * n)), [0] * n
        yield "and set back", list(range(3 * n, 4 * n)), kept
        yield "leaves everywhere, the caller's order", rnd.sample(range(N), min(N, 40)), [rnd.randrange(Q) for _ in range(min(N, 40))]
    return steps


def test_updates_at_4_depth_3(ctx, dom2, leaves43):
    model = run_updates(ctx, dom2, 3, leaves43, steps_of(2))
    assert model.comp[2][3] != ID48


def test_updates_at_2_to_8_depth_2(ctx, dom8, leaves82):
    run_updates(ctx, dom8, 2, leaves82, steps_of(8))


def test_update_across_chunk_boundaries(ctx, dom2, leaves43):
    import plonk_amd
    tree = plonk_amd.KzgTree(dom2, 3)
    tree.build(leaves43)
    model = M.Tree(2, 3, leaves43)
    idx = list(range(64))
    vals = random_leaves(99, 64)
    cap = 3 * (304 + 4 * 36)                             # three bottom nodes per chunk
    dom2._set_workspace_cap(cap)
    try:
        tree.update(idx, vals)
    finally:
        dom2._set_workspace_cap(0)
    model.update(idx, vals)
    assert all_nodes(tree) == model.all_nodes()
    assert M.update_chunks(2, 3, idx, cap) == 6 + 2 + 1
    assert_last(tree, kind=M.UPDATE, touched_nodes=21, sparse_terms=84, chunks=9)
    tree.close()


# ---- prove and check -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree43(ctx, dom2, leaves43, model43):
    import plonk_amd
    t = plonk_amd.KzgTree(dom2, 3)
    t.build(leaves43)
    yield t
    t.close()


PROOF_CASES = {"one leaf": [37], "siblings": [9, 8], "different root children": [63, 0, 21], "all 64 leaves": list(range(63, -1, -1))}


@pytest.mark.parametrize("name", list(PROOF_CASES))
def test_prove_and_check_at_4_depth_3(ctx, key, dom2, tree43, leaves43, model43, name):
    idx = PROOF_CASES[name]
    label = b"tree " + name.encode()
    values, path, proof = tree43.prove(idx, label)
    plan = M.proof_plan(2, 3, idx)
    assert values == [leaves43[j] for j in idx]
    assert path == [model43.comp[l][k] for l, k in plan["path"]] and len(path) == tree43.proof_nodes(idx)
    assert_last(tree43, kind=M.PROVE, items=len(plan["items"]), vectors=len(plan["vectors"]), touched_nodes=len(plan["vectors"]))
    # the item order: the same proof verifies through the multiproof check over the model's items and values
    item_values = [model43.vals[plan["vectors"][v][0]][(plan["vectors"][v][1] << 2) + p] for v, p in plan["items"]]
    assert key.check_multi(2, [model43.root] + path, plan["items"], item_values, proof, label)
    multi = dom2.multi_last()
    assert (multi["items"], multi["vectors"]) == (len(plan["items"]), len(plan["vectors"]))
    assert key.check_tree(2, 3, model43.root, idx, values, path, proof, label)
    # what must not verify
    wrong = list(values)
    wrong[0] = (wrong[0] + 1) % Q
    assert not key.check_tree(2, 3, model43.root, idx, wrong, path, proof, label)
    assert not key.check_tree(2, 3, model43.comp[1][0], idx, values, path, proof, label), "another root"
    assert not key.check_tree(2, 3, model43.root, idx, values, path, proof, label + b"!"), "another label"
    swapped = list(path)
    swapped[-1] = ([c for c in model43.comp[2] if c not in path] + [K.scalar_commit(424242)])[0]
    assert not key.check_tree(2, 3, model43.root, idx, values, swapped, proof, label), "a path commitment swapped with another valid one"
    broken = list(path)
    broken[0] = bytes([0x9F]) + b"\xFF" * 47                            # x = 2^381 - 1 >= p: not a canonical coordinate
    assert key.check_tree_code(2, 3, model43.root, idx, values, broken, proof, label)[0] == ERR_POINT
    assert key.check_tree_code(2, 3, model43.root, idx, values, path, proof, label, nodes=len(path) - 1)[0] == ERR_ARG
    assert key.check_tree_code(2, 3, model43.root, idx, values, path + [path[0]], proof, label)[0] == ERR_ARG
    assert key.check_tree_code(2, 3, model43.root, idx, [NOT_CANONICAL] + values[1:], path, proof, label)[0] == ERR_DATA
    if len(idx) > 1:
        assert key.check_tree_code(2, 3, model43.root, [idx[0]] * len(idx), values, path, proof, label)[0] == ERR_ARG


def test_prove_refusals_leave_the_outputs_alone(ctx, tree43):
    for idx in ([], [5, 5], [64], [0, 1 << 40]):
        assert code_of(lambda: tree43.prove(idx)) == ERR_ARG
        assert code_of(lambda: tree43.proof_nodes(idx)) == ERR_ARG


def test_depth_1_proof_is_a_plain_multiproof(ctx, key, dom2):
    import plonk_amd
    leaves = random_leaves(5, 4)
    tree = plonk_amd.KzgTree(dom2, 1)
    tree.build(leaves)
    values, path, proof = tree.prove([3, 1], b"flat")
    assert path == [] and values == [leaves[3], leaves[1]] and tree.proof_nodes([3, 1]) == 0
    assert key.check_tree(2, 1, tree.root(), [3, 1], values, path, proof, b"flat")
    assert key.check_multi(2, [tree.root()], [(0, 1), (0, 3)], [leaves[1], leaves[3]], proof, b"flat")
    assert tree.root() == MM.commitment(leaves, 2)
    tree.close()


def test_a_proof_after_an_update_verifies_against_the_new_root_only(ctx, key, dom2, leaves43):
    import plonk_amd
    tree = plonk_amd.KzgTree(dom2, 3)
    tree.build(leaves43)
    old_root = tree.root()
    tree.update([20, 41], [111, 222])
    values, path, proof = tree.prove([41, 7], b"after")
    assert values == [222, leaves43[7]]
    new_root = tree.root()
    assert new_root != old_root
    assert key.check_tree(2, 3, new_root, [41, 7], values, path, proof, b"after")
    assert not key.check_tree(2, 3, old_root, [41, 7], values, path, proof, b"after")
    tree.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_tables_empty_trees_and_failed_builds(ctx, key, leaves43, model43):
    import plonk_amd
    dom = plonk_amd.KzgDomain(ctx, 2)
    tree = plonk_amd.KzgTree(dom, 3)
    # an empty tree: every call but build and last refuses
    for call in (tree.root, lambda: tree.nodes(1), lambda: tree.update([0], [1]), lambda: tree.prove([0])):
        assert code_of(call) == ERR_STATE
    assert_last(tree, built=0, kind=M.NONE)
    # no many-vector tables
    assert code_of(lambda: tree.build(leaves43)) == ERR_STATE
    assert_last(tree, built=0)
    dom.build_many_tables(4)
    tree.build(leaves43)
    assert tree.root() == model43.root
    # another window width than at the build is fine
    dom.build_many_tables(8)
    tree.update([1], [5])
    tree.update([1], [leaves43[1]])
    assert all_nodes(tree) == model43.all_nodes()
    # tables dropped under a live tree: update refuses and changes nothing, prove still works, build refuses and empties
    dom.drop_many_tables()
    assert code_of(lambda: tree.update([1], [5])) == ERR_STATE
    assert all_nodes(tree) == model43.all_nodes()
    values, path, proof = tree.prove([1], b"no tables")
    assert key.check_tree(2, 3, model43.root, [1], values, path, proof, b"no tables")
    assert code_of(lambda: tree.build(leaves43)) == ERR_STATE
    assert code_of(tree.root) == ERR_STATE
    # a failed build (a leaf >= q, both forms) leaves the tree empty
    dom.build_many_tables(8)
    tree.build(leaves43)
    bad = bytearray(mont(leaves43))
    bad[32 * 17:32 * 18] = NOT_CANONICAL
    assert code_of(lambda: tree.build(bytes(bad))) == ERR_DATA
    assert code_of(tree.root) == ERR_STATE and tree.last()["built"] == 0
    tree.build(leaves43)
    buf = ctx.alloc(32 * 64)
    buf.upload(bytes(bad))
    assert code_of(lambda: tree.build_dev(buf.ptr)) == ERR_DATA
    assert code_of(lambda: tree.prove([0])) == ERR_STATE
    buf.free()
    tree.build(leaves43)
    assert tree.root() == model43.root
    # shapes
    for depth in (0, 14, 1 << 31):
        assert code_of(lambda: plonk_amd.KzgTree(dom, depth)) == ERR_ARG
    # the domain closes its trees first
    dom.close()
    assert tree.handle is None


def test_tree_calls_leave_the_context_and_the_domain_reports_alone(ctx, dom2, leaves43):
    import plonk_amd
    ctx.msm([1, 2, 3, 4])
    dom2.commit_many([leaves43[:4]])
    before = (ctx.last_msm(), dom2.many_last(), ctx.table_bytes(), dom2.evals_last())
    tree = plonk_amd.KzgTree(dom2, 3)
    tree.build(leaves43)
    tree.update([0, 63], [9, 8])
    tree.nodes(2)
    assert (ctx.last_msm(), dom2.many_last(), ctx.table_bytes(), dom2.evals_last()) == before
    tree.prove([0])                                     # the multiproof's own MSMs: section 19 documents what they touch
    assert (dom2.many_last(), ctx.table_bytes()) == (before[1], before[2])
    tree.close()
    assert ctx.table_bytes() == before[2]


def test_a_reloaded_key_refuses_every_call_that_works_on_the_tree(leaves43):
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, 8)
    dom = plonk_amd.KzgDomain(c, 2)
    dom.build_many_tables(8)
    tree = plonk_amd.KzgTree(dom, 3)
    tree.build(leaves43)
    root = tree.root()
    load_key(c, 8)                                      # the same points, but no longer the key the handle was built on
    for call in (tree.root, lambda: tree.nodes(0), lambda: tree.update([0], [1]), lambda: tree.prove([0]),
                 lambda: plonk_amd.KzgTree(dom, 1)):
        assert code_of(call) == ERR_STATE
    assert tree.last()["built"] == 1
    assert code_of(lambda: tree.build(leaves43)) == ERR_STATE and tree.last()["built"] == 0
    assert len(root) == 48
    dom.close()
    c.close()
