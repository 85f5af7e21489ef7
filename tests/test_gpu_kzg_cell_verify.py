"""GPU: KZG10 cell verification (plonk_kzg_cell_verifier_create, plonk_kzg_verify_cells, plonk_kzg_verify_cells_each).  The
cells, proofs and commitments come from KzgDomain.open_cells on the device (and from the closed forms on the known-tau key for
the degenerate cases); the plan, the challenge and every kernel's output are compared with the big-int model
tests/kzg_cell_verify_model.py.  The kernels are also run on their own through tests/csrc/dev_kzg_cell_verify.hip with guard
bands around every output."""
import ctypes
import os
import random

import pytest

from oracle import bls12_381 as E
from tests import kzg_cell_verify_model as V
from tests import kzg_cells_model as M
from tests import kzg_ref as K
from tests.test_gpu_kzg_cells import cell_key, load_key, shaped

pytestmark = pytest.mark.gpu
Q = E.Q
OK, ERR_ARG, ERR_DEGREE, ERR_NO_SRS, ERR_STATE, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -3, -4, -7, -9, -10, -12
ID48 = K.IDENTITY48
BAD48 = b"\x9f" + b"\xff" * 47                     # compressed, x >= p: does not decode
KEY_POINTS = 1 << 12
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_cell_verify.so")
GUARD = b"\xA5" * 32


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, KEY_POINTS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rig(ctx):
    """domains by log_n, (key, verifier) pairs by (log_n, log_cell), opened blobs by (log_n, log_cell, tag)"""
    import plonk_amd

    class Rig:
        def __init__(self):
            self.doms, self.vers, self.opened = {}, {}, {}

        def dom(self, log_n):
            if log_n not in self.doms:
                self.doms[log_n] = plonk_amd.KzgDomain(ctx, log_n)
            return self.doms[log_n]

        def ver(self, log_n, log_cell):
            if (log_n, log_cell) not in self.vers:
                key = plonk_amd.KzgKey(ctx, cell_key(1 << log_cell))
                self.vers[log_n, log_cell] = (key, plonk_amd.KzgCellVerifier(key, log_n, log_cell))
            return self.vers[log_n, log_cell][1]

        def open(self, log_n, log_cell, polys):
            """(commitments, items of every cell of every polynomial)"""
            cells, proofs, cm = self.dom(log_n).open_cells(polys, log_cell)
            r = 1 << (log_n - log_cell)
            return cm, [(j, k, cells[j][k], proofs[j][k]) for j in range(len(polys)) for k in range(r)]

        def random_blobs(self, log_n, log_cell, count, seed=0):
            tag = (log_n, log_cell, count, seed)
            if tag not in self.opened:
                rnd = random.Random(1000 * log_n + 10 * log_cell + seed)
                self.opened[tag] = self.open(log_n, log_cell, [[rnd.randrange(Q) for _ in range(1 << log_n)] for _ in range(count)])
            return self.opened[tag]
    rig = Rig()
    yield rig
    for key, v in rig.vers.values():
        v.close()
        key.close()
    for d in rig.doms.values():
        d.close()


def assert_last(v, M_, K_, each, mins=(0, 0), key_checked=1):
    last, p = v.last(), V.plan(v.log_cell, M_, K_, each, *mins)
    assert (last["log_n"], last["log_cell"], last["key_checked"], last["path_each"]) == (v.log_n, v.log_cell, key_checked, int(each))
    assert (last["items"], last["commitments"]) == (K_, M_)
    for name in ("transforms", "msm_terms_left", "msm_terms_right", "msm_path_left", "msm_path_right", "scalar_muls"):
        assert last[name] == p[name], name
    l, r = 1 << v.log_cell, 1 << (v.log_n - v.log_cell)
    assert last["device_bytes"] >= 96 * l + 32 * (2 * r + l // 2)
    return last


def both(v, cm, items, want_each=None, label=b"t"):
    """the folded verdict and the per-item verdicts; checks them against each other and against want_each"""
    each = v.verify_each(cm, items)
    folded = v.verify(cm, items, label)
    assert folded == all(x == OK for x in each)
    if want_each is not None:
        assert each == want_each
    return folded, each


# ---- small sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_cell", [(a, b) for a in (3, 4, 6) for b in range(1, a)])
def test_small_sizes_all_cells_of_two_blobs_and_the_shaped_polynomials(rig, log_n, log_cell):
    v, r, l = rig.ver(log_n, log_cell), 1 << (log_n - log_cell), 1 << log_cell
    cm, items = rig.random_blobs(log_n, log_cell, 2)
    code, info = v.verify_code(cm, items, b"small")
    assert code == OK and (info["proofs"], info["msm_terms"], info["pairing_checks"], info["rejected"]) == (2 * r, 4 * r + 2 + l, 1, 0)
    assert_last(v, 2, 2 * r, False)
    verdicts, info = v.verify_each_info(cm, items)
    assert verdicts == [OK] * (2 * r)
    assert (info["proofs"], info["msm_terms"], info["pairing_checks"], info["rejected"]) == (2 * r, (l + 2) * 2 * r, 2 * r, 0)
    assert_last(v, 2, 2 * r, True)
    cm, items = rig.open(log_n, log_cell, shaped(log_n, log_cell))
    assert both(v, cm, items)[0]


def test_smallest_shape(rig):
    v = rig.ver(2, 1)
    cm, items = rig.random_blobs(2, 1, 2)
    assert both(v, cm, items, [OK] * 4)[0]
    bad = list(items)
    bad[3] = (bad[3][0], bad[3][1], [bad[3][2][0], (bad[3][2][1] + 1) % Q], bad[3][3])
    assert both(v, cm, bad, [OK, OK, OK, ERR_VERIFY])[0] is False


# ---- batch sizes around the path switches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 31, 32, 33, 63, 64, 70])
def test_batch_sizes_on_both_sides_of_the_msm_path_rule(rig, count):
    """(6, 3), 9 blobs: the left sum has K terms, the right one 9 + K + 8, so K = 32 / 33 ... 63 / 64 lie on both sides of
    msm_points' 64-term rule for the right sum (K >= 47) and for the left one (K >= 64)"""
    v = rig.ver(6, 3)
    cm, items = rig.random_blobs(6, 3, 9)
    items = items[:count]
    assert v.verify(cm, items, b"paths")
    last = assert_last(v, 9, count, False)
    assert (last["msm_path_left"], last["msm_path_right"]) == (int(count >= 64), int(count >= 47))
    rho = v._last_rho()
    bad = list(items)
    i = count // 2
    bad[i] = (bad[i][0], bad[i][1], bad[i][2][:7] + [(bad[i][2][7] + 1) % Q], bad[i][3])
    assert not v.verify(cm, bad, b"paths")
    for mins in ((1, 1), (1 << 30, 1 << 30), (1, 1 << 30), (1 << 30, 1)):      # buckets / per-term forced for each sum
        v._force_paths(*mins)
        try:
            assert v.verify(cm, items, b"paths") and v._last_rho() == rho
            last = assert_last(v, 9, count, False, mins)
            assert (last["msm_path_left"], last["msm_path_right"]) == (int(mins[0] == 1), int(mins[1] == 1))
            assert not v.verify(cm, bad, b"paths")
        finally:
            v._force_paths(0, 0)
    assert v.verify_each(cm, bad) == [OK if j != i else ERR_VERIFY for j in range(count)]


# ---- the sampler's shape, the largest cell ---------------------------------------------------------------------------------------
def test_sampler_shape_16_blobs_8_cells_each(rig):
    v = rig.ver(12, 6)
    rnd = random.Random(126)
    cm, items = rig.random_blobs(12, 6, 16)
    sampled = [it for j in range(16) for it in rnd.sample(items[64 * j:64 * (j + 1)], 8)]
    assert len(sampled) == 128
    assert both(v, cm, sampled, [OK] * 128)[0]
    assert_last(v, 16, 128, False)
    bad = list(sampled)
    bad[77] = (bad[77][0], (bad[77][1] + 1) % 64) + bad[77][2:]
    assert both(v, cm, bad, [OK] * 77 + [ERR_VERIFY] + [OK] * 50)[0] is False


def test_largest_cell(rig):
    v = rig.ver(12, 11)
    cm, items = rig.random_blobs(12, 11, 1)
    assert len(items) == 2 and both(v, cm, items, [OK, OK])[0]
    assert_last(v, 1, 2, False)
    bad = [items[0], (0, 1, items[1][2][:2047] + [(items[1][2][2047] + 1) % Q], items[1][3])]
    assert both(v, cm, bad, [OK, ERR_VERIFY])[0] is False


# ---- rejections --------------------------------------------------------------------------------------------------------------------
def test_rejections_name_exactly_the_bad_items(rig):
    v = rig.ver(6, 3)
    cm, items = rig.random_blobs(6, 3, 2)
    n = len(items)                                     # 16: blob 0 cells 0..7, blob 1 cells 0..7

    def one(i, item):
        return items[:i] + [item] + items[i + 1:]

    def only(*bad):
        return [ERR_VERIFY if j in bad else OK for j in range(n)]
    c, k, values, proof = items[5]
    plus = values[:7] + [(values[7] + 1) % Q]
    assert both(v, cm, one(5, (c, k, plus, proof)), only(5))[0] is False                   # one value + 1 in the last slot
    assert both(v, cm, one(5, (c, k, values, items[6][3])), only(5))[0] is False           # a neighbour's proof
    assert both(v, cm, one(5, (1, k, values, proof)), only(5))[0] is False                 # a wrong commitment index
    assert both(v, cm, one(5, (c, k + 1, values, proof)), only(5))[0] is False             # a cell index off by one
    assert both(v, cm, one(5, (c, k, values, ID48)), only(5))[0] is False                  # the identity in place of the proof
    two = one(5, (c, k, plus, proof))
    two[12] = (two[12][0], two[12][1], two[12][2], items[3][3])
    assert both(v, cm, two, only(5, 12))[0] is False                                       # two bad items in one batch
    # each verdict is the folded call's on that item alone
    for i in (5, 12, 0):
        assert v.verify(cm, [two[i]], b"x") == (i == 0)


def test_a_predictable_rho_voids_the_check(rig):
    """The same cell twice, + d on value j of the first copy and - d on the second.  The remainder is linear in the values, so
    with rho = 1 the two errors cancel in every R_j and the folded equation holds although neither item is valid: a caller
    who passes rho_override must draw it after every input is fixed.  With the derived rho the batch fails, and the per-item
    call rejects both copies."""
    v = rig.ver(6, 3)
    cm, items = rig.random_blobs(6, 3, 2)
    c, k, values, proof = items[11]
    d, j = 0x1234567, 2
    up, down = list(values), list(values)
    up[j], down[j] = (up[j] + d) % Q, (down[j] - d) % Q
    pair = [(c, k, up, proof), (c, k, down, proof)]
    assert v.verify(cm, pair, b"rho", rho=1)
    assert not v.verify(cm, pair, b"rho")
    assert v.verify_each(cm, pair) == [ERR_VERIFY, ERR_VERIFY]
    assert not v.verify(cm, pair, b"rho", rho=2)


# ---- degenerate data ---------------------------------------------------------------------------------------------------------------
def test_short_and_zero_polynomials_and_repeated_items(rig):
    log_n, log_cell, l, r = 6, 3, 8, 8
    v = rig.ver(log_n, log_cell)
    rnd = random.Random(63)
    short = [rnd.randrange(1, Q) for _ in range(l)]               # shorter than l + 1: identity proofs, c_j = f_j
    cm, items = rig.open(log_n, log_cell, [short, []])
    assert all(it[3] == ID48 for it in items) and cm[1] == ID48 and all(it[2] == [0] * l for it in items[r:])
    assert cm[0] == K.commit(short)
    assert both(v, cm, items, [OK] * (2 * r))[0]
    # the closed forms in place of the device's bytes
    w = M.root(log_n)
    closed = [(0, k, [K.evaluate(short, pow(w, k + r * i, Q)) for i in range(l)], ID48) for k in range(r)]
    assert closed == items[:r]
    assert both(v, cm, [items[2]] * 5, [OK] * 5)[0]               # the same item 5 times
    cm2, items2 = rig.random_blobs(log_n, log_cell, 2)
    assert both(v, cm2, [items2[9]] * 5, [OK] * 5)[0]
    wrong = (1, 0, items[0][2], ID48)                            # the short polynomial's cell under the zero commitment
    assert both(v, cm, [items[0], wrong], [OK, ERR_VERIFY])[0] is False


@pytest.mark.parametrize("log_n", [3, 4])
def test_degenerate_key(log_n):
    """tau = (2n-th root of unity)^3 (tests/test_gpu_kzg_cells.py test_degenerate_key): the key's points repeat with period 2n,
    identities, equal and opposite points enter every sum"""
    import plonk_amd
    n = 1 << log_n
    tau = pow(M.root(log_n + 1), 3, Q)
    c = plonk_amd.Context(0)
    load_key(c, n, tau)
    dom = plonk_amd.KzgDomain(c, log_n)
    rnd = random.Random(log_n)
    polys = [[rnd.randrange(Q) for _ in range(n)], [1] * n, [0] * (n - 1) + [1], [3, 1]]
    for log_cell in range(1, log_n):
        l, r = 1 << log_cell, 1 << (log_n - log_cell)
        key = plonk_amd.KzgKey(c, cell_key(l, tau))
        v = plonk_amd.KzgCellVerifier(key, log_n, log_cell)
        cells, proofs, cm = dom.open_cells(polys, log_cell)
        items = [(j, k, cells[j][k], proofs[j][k]) for j in range(len(polys)) for k in range(r)]
        assert both(v, cm, items, [OK] * len(items))[0]
        bad = list(items)
        bad[1] = (bad[1][0], bad[1][1], [(bad[1][2][0] + 1) % Q] + bad[1][2][1:], bad[1][3])
        assert both(v, cm, bad, [OK, ERR_VERIFY] + [OK] * (len(items) - 2))[0] is False
        v.close()
        key.close()
    dom.close()
    c.close()


# ---- the challenge -----------------------------------------------------------------------------------------------------------------
def test_challenge_equals_the_models_transcript_and_binds_every_input(rig):
    v = rig.ver(6, 3)
    key240 = cell_key(8)
    cm, items = rig.random_blobs(6, 3, 2)
    items = items[3:9]

    def rho(cm_, items_, label=b"lbl"):
        v.verify_code(cm_, items_, label)
        got = v._last_rho()
        assert got == V.challenge(label, 6, 3, key240, cm_, items_)
        return got
    seen = {rho(cm, items)}
    first = items[0]
    variants = [
        (cm, items, b"lbm"),
        ([cm[0], cm[0]], items, b"lbl"),
        (cm, [(1 - first[0],) + first[1:]] + items[1:], b"lbl"),
        (cm, [(first[0], first[1] ^ 1) + first[2:]] + items[1:], b"lbl"),
        (cm, [first[:2] + (first[2][:7] + [first[2][7] ^ 1], first[3])] + items[1:], b"lbl"),
        (cm, [first[:3] + (items[1][3],)] + items[1:], b"lbl"),
        (cm, items[:5], b"lbl"),
    ]
    for cm_, items_, label in variants:
        got = rho(cm_, items_, label)
        assert got not in seen
        seen.add(got)
    assert v.verify(cm, items, b"lbl", rho=12345) and v._last_rho() == 12345
    # K = 1 does not depend on rho: item 0 has weight 1
    assert v.verify(cm, items[:1], rho=1) and v.verify(cm, items[:1], rho=Q - 1)


# ---- key handling ------------------------------------------------------------------------------------------------------------------
def test_key_handling(ctx, rig):
    import plonk_amd
    cm, items = rig.random_blobs(6, 3, 2)
    ordinary = plonk_amd.KzgKey(ctx, K.opening_key())              # x_h = [tau] h: the commit key has more than l points
    with pytest.raises(plonk_amd.PlonkError) as ei:
        plonk_amd.KzgCellVerifier(ordinary, 6, 3)
    assert ei.value.code == ERR_VERIFY
    ordinary.close()
    other_g = plonk_amd.KzgKey(ctx, E.g1_compress(E.g1_mul(E.G1_GEN, 5)) + cell_key(8)[48:])
    with pytest.raises(plonk_amd.PlonkError) as ei:
        plonk_amd.KzgCellVerifier(other_g, 6, 3)                   # s_0 is not the key's g
    assert ei.value.code == ERR_VERIFY
    other_g.close()
    # exactly l points: the key cannot be checked, the verifier works
    c = plonk_amd.Context(0)
    load_key(c, 8)
    key = plonk_amd.KzgKey(c, cell_key(8))
    v = plonk_amd.KzgCellVerifier(key, 6, 3)
    assert both(v, cm, items, [OK] * 16)[0]
    assert_last(v, 2, 16, False, key_checked=0)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        plonk_amd.KzgCellVerifier(key, 6, 4)                       # fewer than l points
    assert ei.value.code == ERR_DEGREE
    # the handle keeps its copy of the key: another key on the context changes nothing
    load_key(c, 16, pow(K.TAU, 3, Q))
    assert both(v, cm, items, [OK] * 16)[0]
    bad = [(items[0][0], items[0][1], items[0][2], items[1][3])] + items[1:]
    assert both(v, cm, bad, [ERR_VERIFY] + [OK] * 15)[0] is False
    v.close()
    key.close()
    c.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_every_documented_error_in_the_documented_order(ctx, rig):
    import plonk_amd
    v = rig.ver(6, 3)
    key = rig.vers[6, 3][0]
    lib = ctx.lib
    cm, items = rig.random_blobs(6, 3, 2)
    items = items[:4]
    h = ctypes.c_void_p()
    for args in ((None, 6, 3, ctypes.byref(h)), (key.handle, 6, 3, None), (key.handle, 1, 1, ctypes.byref(h)), (key.handle, 21, 3, ctypes.byref(h)),
                 (key.handle, 6, 0, ctypes.byref(h)), (key.handle, 6, 6, ctypes.byref(h)), (key.handle, 13, 12, ctypes.byref(h))):
        assert lib.plonk_kzg_cell_verifier_create(*args) == ERR_ARG
    empty = plonk_amd.Context(0)
    k2 = plonk_amd.KzgKey(empty, cell_key(8))
    assert lib.plonk_kzg_cell_verifier_create(k2.handle, 6, 3, ctypes.byref(h)) == ERR_NO_SRS
    assert lib.plonk_kzg_cell_verifier_create(k2.handle, 6, 7, ctypes.byref(h)) == ERR_ARG      # the argument check comes first
    k2.close()
    empty.close()

    mont = plonk_amd.fr_to_bytes_mont
    noncanon = mont(items[1][2][:7]) + b"\xff" * 32
    bad_value = [items[0], items[1][:2] + (noncanon,) + items[1][3:]] + items[2:]
    bad_point = items[:2] + [items[2][:3] + (BAD48,)] + items[3:]
    bad_proof = items[:3] + [items[3][:3] + (items[0][3],)]

    def folded(cm_, items_, count=None, M_=None, rho=None, hdl=v.handle, drop=None):
        a = list(v._args(cm_, items_))
        a[0] = hdl
        if M_ is not None:
            a[2] = M_
        if count is not None:
            a[7] = count
        if drop is not None:
            a[drop] = None
        return lib.plonk_kzg_verify_cells(*a, b"e", 1, rho, None)

    def each(cm_, items_, count=None, hdl=v.handle, drop=None, no_verdicts=False):
        a = list(v._args(cm_, items_))
        a[0] = hdl
        if count is not None:
            a[7] = count
        if drop is not None:
            a[drop] = None
        verdicts = (ctypes.c_int32 * 8)(*([0x5A5A5A5A] * 8))
        return lib.plonk_kzg_verify_cells_each(*a, None if no_verdicts else verdicts, None), list(verdicts)
    untouched = [0x5A5A5A5A] * 8
    # PLONK_ERR_ARG
    assert folded(cm, items, hdl=None) == ERR_ARG and each(cm, items, hdl=None) == (ERR_ARG, untouched)
    for drop in (1, 3, 4, 5, 6):
        assert folded(cm, items, drop=drop) == ERR_ARG and each(cm, items, drop=drop) == (ERR_ARG, untouched)
    assert each(cm, items, no_verdicts=True)[0] == ERR_ARG
    assert folded(cm, [(2,) + items[0][1:]] + items[1:]) == ERR_ARG                 # a commitment index >= M
    assert each(cm, [(2,) + items[0][1:]] + items[1:]) == (ERR_ARG, untouched)
    assert folded(cm, [(0, 8) + items[0][2:]] + items[1:]) == ERR_ARG               # a cell index >= r
    assert each(cm, [(0, 8) + items[0][2:]] + items[1:]) == (ERR_ARG, untouched)
    assert folded(cm, items, count=(1 << 20) + 1) == ERR_ARG and each(cm, items, count=(1 << 20) + 1) == (ERR_ARG, untouched)
    assert folded(cm, items, M_=65537) == ERR_ARG
    assert each(cm, [], count=0) == (ERR_ARG, untouched)
    assert folded(cm, [], count=0) == ERR_VERIFY                                     # the empty batch
    assert v.verify(cm, []) is False
    # the order: ARG, DATA, POINT, VERIFY
    mixed = [bad_value[1], bad_point[2], bad_proof[3]]
    assert folded(cm, [(2,) + mixed[0][1:]] + mixed[1:]) == ERR_ARG
    assert folded(cm, mixed) == ERR_DATA
    assert folded(cm, mixed[1:]) == ERR_POINT
    assert folded(cm, mixed[2:]) == ERR_VERIFY
    assert folded(cm, items, rho=b"\xff" * 32) == ERR_DATA
    assert folded([cm[0], BAD48], items[:1]) == ERR_POINT                            # a commitment that does not decode
    assert folded([cm[0], ID48], items[:1]) == OK                                    # the compressed identity is legal
    # the per-item call: a malformed item never stops the others
    got = each(cm, [items[0]] + mixed)
    assert got == (ERR_VERIFY, [OK, ERR_DATA, ERR_POINT, ERR_VERIFY] + untouched[4:])
    both_bad = items[1][:2] + (noncanon, BAD48)
    assert v.verify_each(cm, [both_bad, items[0]]) == [ERR_DATA, OK]                 # the values are looked at first
    assert v.verify_each([BAD48, cm[1]], items) == [ERR_POINT] * 4 and v.verify_each([BAD48, cm[1]], [(1,) + it[1:] for it in items]) == [ERR_VERIFY] * 4
    info = plonk_amd._KzgCellVerifyInfo()
    assert lib.plonk_kzg_cell_verifier_last(v.handle, None) == ERR_ARG and lib.plonk_kzg_cell_verifier_last(None, ctypes.byref(info)) == ERR_ARG
    assert both(v, cm, items, [OK] * 4)[0]                                           # the handle still works


# ---- state -------------------------------------------------------------------------------------------------------------------------
def test_communicator_is_a_state_error(rig):
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, 16)
    key = plonk_amd.KzgKey(c, cell_key(8))
    c.comm_init(plonk_amd.Context.comm_unique_id(), 0, 1)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        plonk_amd.KzgCellVerifier(key, 6, 3)
    assert ei.value.code == ERR_STATE
    c.comm_destroy()
    v = plonk_amd.KzgCellVerifier(key, 6, 3)
    cm, items = rig.random_blobs(6, 3, 2)
    assert v.verify(cm, items)
    c.close()                                                    # closes the verifier before its key, the key before the context
    assert v.handle is None and key.handle is None


def test_context_left_as_found():
    """a proof, an opening and a cell call made on the same context before and after the two verification calls are
    byte-identical; plonk_ctx_last_msm_points and plonk_kzg_cells_last keep describing the caller's own last calls"""
    import plonk_amd
    from tests import circuits as C
    c = plonk_amd.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=78)()
    case = C.compile_fast(comp, b"kzg-cell-verify")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = plonk_amd.Prover.compile(c, b"kzg-cell-verify", cols["selectors"], cols["wires"], cols["witnesses"])
    rnd = random.Random(79)
    f = [rnd.randrange(Q) for _ in range(300)]
    z, w = rnd.randrange(Q), rnd.randrange(Q)
    proof = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    opening = c.kzg_open([f, f[:7]], z, w)
    pts = [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(70)]
    sc = [rnd.randrange(Q) for _ in range(70)]
    msm = c.msm_points(pts, sc)
    dom = plonk_amd.KzgDomain(c, 6)
    polys = [[rnd.randrange(Q) for _ in range(64)] for _ in range(10)]
    cells, proofs, cm = dom.open_cells(polys, 3)
    before = (c.last_msm_points(), dom.cells_last(), c.table_bytes(), c.table_rows())
    key = plonk_amd.KzgKey(c, cell_key(8))
    v = plonk_amd.KzgCellVerifier(key, 6, 3)
    items = [(j, k, cells[j][k], proofs[j][k]) for j in range(10) for k in range(8)]
    assert both(v, cm, items, [OK] * 80)[0]                      # both sums through the buckets
    assert both(v, cm, items[:3], [OK] * 3)[0]                   # both per term
    assert (c.last_msm_points(), dom.cells_last(), c.table_bytes(), c.table_rows()) == before
    assert prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3)) == proof
    assert c.kzg_open([f, f[:7]], z, w) == opening
    assert c.msm_points(pts, sc) == msm
    assert dom.open_cells(polys, 3) == (cells, proofs, cm)
    v.close()
    key.close()
    dom.close()
    prover.close()
    c.close()


# ---- the kernels on their own ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def doors():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_cell_verify.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    so.dkv_key_copy.argtypes = [vp, u64, vp]
    so.dkv_twist.argtypes = [vp, vp, vp, vp, u64, u32, vp, vp, vp, vp]
    so.dkv_colsum.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp]
    so.dkv_weights.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, u32, vp, vp]
    so.dkv_decode.argtypes = [vp, vp, u32, vp, vp, vp, u64]
    so.dkv_cell_sums.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64, u64, u32, vp, vp]
    return so


class Dev:
    """device buffers of a test: uploads with a 32-byte guard band on both sides of every buffer"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, data: bytes):
        b = self.ctx.alloc(len(data) + 64)
        b.upload(GUARD + data + GUARD)
        self.bufs.append(b)
        return b

    def out(self, nbytes: int):
        return self.put(b"\x5A" * nbytes)

    @staticmethod
    def ptr(b):
        return b.ptr + 32

    @staticmethod
    def get(b):
        raw = b.download()
        assert raw[:32] == GUARD and raw[-32:] == GUARD, "a kernel wrote outside its output"
        return raw[32:-32]

    def free(self):
        for b in self.bufs:
            b.free()


def u32bytes(xs):
    return b"".join(int(x).to_bytes(4, "little") for x in xs)


def words(raw):
    return [int.from_bytes(raw[i:i + 4], "little") for i in range(0, len(raw), 4)]


def canon(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.mark.parametrize("log_n,log_cell,count", [(3, 1, 5), (3, 1, 300), (8, 6, 1), (8, 6, 9), (9, 7, 3), (12, 11, 2)])
def test_twist_kernel_against_the_model(ctx, doors, log_n, log_cell, count):
    """l = 2, 64 (packed: 128 and 4 items per workgroup, a partly filled and several workgroups), 128 and 2048 (one item per
    workgroup); k = 0 and k = r - 1; with and without weights; a non-canonical value flags its item only"""
    import plonk_amd
    mont, unmont = plonk_amd.fr_to_bytes_mont, plonk_amd.fr_from_bytes_mont
    l, r = 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(log_cell * 1000 + count)
    kidx = [0, r - 1][:count] + [rnd.randrange(r) for _ in range(count - 2)]
    rows = [[rnd.randrange(Q) for _ in range(l)] for _ in range(count)]
    wts = [rnd.randrange(Q) for _ in range(count)]
    x, winv, itw = V.handle_tables(log_n, log_cell)
    d = Dev(ctx)
    values = bytearray(b"".join(mont(row) for row in rows))
    flagged = count - 1
    values[32 * (flagged * l + l - 1):32 * (flagged * l + l)] = b"\xff" * 32         # >= q
    bufs = [d.put(bytes(values)), d.put(u32bytes(kidx)), d.put(mont(wts)), d.put(mont(winv)), d.put(mont(itw))]
    for weights in (None, bufs[2]):
        out, flags = d.out(32 * l * count), d.put(bytes(4 * count))
        assert doors.dkv_twist(ctx.handle, d.ptr(bufs[0]), d.ptr(bufs[1]), d.ptr(weights) if weights else None, count, log_cell,
                               d.ptr(bufs[3]), d.ptr(bufs[4]), d.ptr(out), d.ptr(flags)) == 0
        got = unmont(d.get(out))
        assert words(d.get(flags)) == [0] * flagged + [1]
        for i in range(count):
            want = [0] * l if i == flagged else V.twist(rows[i], log_n, log_cell, kidx[i], wts[i] if weights else 1)
            assert got[i * l:(i + 1) * l] == want, i
        if count > 1 and not weights and l <= 128:                 # the quadratic closed form
            assert got[:l] == M.remainder_from_cell(rows[0], log_n, log_cell, 0)
    assert doors.dkv_twist(ctx.handle, d.ptr(bufs[0]), d.ptr(bufs[1]), None, count, 12, d.ptr(bufs[3]), d.ptr(bufs[4]), d.ptr(out), d.ptr(flags)) == ERR_ARG
    assert doors.dkv_twist(ctx.handle, d.ptr(bufs[0]), d.ptr(bufs[1]), None, 0, log_cell, d.ptr(bufs[3]), d.ptr(bufs[4]), d.ptr(out), d.ptr(flags)) == ERR_ARG
    d.free()


@pytest.mark.parametrize("count", [1, 2, 64, 65, 64 * 64 + 1])
def test_colsum_kernel(ctx, doors, count):
    """K = 1, 2, a full slice, one more than a slice, and more than a slice of slices (three passes); l = 8 and l = 128"""
    import plonk_amd
    mont = plonk_amd.fr_to_bytes_mont
    rnd = random.Random(count)
    for log_cell in (3, 7):
        l = 1 << log_cell
        rows = [[rnd.randrange(Q) for _ in range(l)] for _ in range(count)]
        d = Dev(ctx)
        src = d.put(b"".join(mont(r) for r in rows))
        s1 = V.colsum_slices(count)
        p0, p1 = d.out(32 * l * s1), d.out(32 * l * V.colsum_slices(s1))
        sc, ids = d.out(32 * l), d.out(4 * l)
        assert doors.dkv_colsum(ctx.handle, d.ptr(src), count, log_cell, d.ptr(p0), d.ptr(p1), d.ptr(sc), d.ptr(ids)) == 0
        assert canon(d.get(sc)) == [(-x) % Q for x in V.colsum(rows, l)]
        assert words(d.get(ids)) == list(range(l))
        d.get(p0), d.get(p1)
        d.free()


def test_weights_kernel(ctx, doors):
    """a commitment without items, all items on one commitment, a segment longer than a wave"""
    import plonk_amd
    mont = plonk_amd.fr_to_bytes_mont
    rnd = random.Random(4)
    log_n, log_cell = 6, 3
    l = 8
    x, _, _ = V.handle_tables(log_n, log_cell)
    for M_, cidx in ((4, [rnd.choice((0, 1, 3)) for _ in range(200)]), (1, [0] * 130), (3, [2])):
        K_ = len(cidx)
        kidx = [rnd.randrange(8) for _ in range(K_)]
        rho = rnd.randrange(Q)
        pw, W, px = V.weights(rho, cidx, kidx, M_, log_n, log_cell)
        perm, off = V.counting_sort(cidx, M_)
        lay = V.layout(log_cell, M_, K_)
        d = Dev(ctx)
        bufs = [d.put(mont(pw)), d.put(u32bytes(kidx)), d.put(mont(x)), d.put(u32bytes(perm)), d.put(u32bytes(off))]
        sc, ids = d.out(32 * lay["term_r"]), d.out(4 * lay["term_r"])
        assert doors.dkv_weights(ctx.handle, *[d.ptr(b) for b in bufs], K_, M_, log_cell, d.ptr(sc), d.ptr(ids)) == 0
        assert canon(d.get(sc)) == pw + W + px
        assert words(d.get(ids)) == [l + M_ + i for i in range(K_)] + [l + c for c in range(M_)] + [l + M_ + i for i in range(K_)]
        d.free()


def xyzz_compress(raw192):
    X, Y, ZZ, ZZZ = (int.from_bytes(raw192[48 * i:48 * (i + 1)], "little") for i in range(4))
    if ZZ == 0:
        return ID48
    return E.g1_compress((X * pow(ZZ, -1, E.P) % E.P, Y * pow(ZZZ, -1, E.P) % E.P))   # the Montgomery factors cancel


@pytest.mark.parametrize("log_cell", [1, 6, 7])
def test_cell_sums_kernel_against_the_exponent(ctx, doors, log_cell):
    """B_i compressed against [g (C + x_k pi - sum_j c_ij tau^j)] G of the model; l = 2, 64, 128 (fewer terms than lanes, one
    and two per lane); all-zero coefficients, the identity as C and as pi, a flagged item and one with a bad point"""
    import plonk_amd
    mont = plonk_amd.fr_to_bytes_mont
    log_n = log_cell + 2
    l, r = 1 << log_cell, 4
    rnd = random.Random(log_cell)
    x, _, _ = V.handle_tables(log_n, log_cell)
    cexp = [rnd.randrange(1, Q), 0, rnd.randrange(1, Q)]                       # commitment 1 is the identity
    comm = [K.scalar_commit(e) for e in cexp[:2]] + [BAD48]
    # (commitment, cell, coefficients, proof exponent or None for a bad point, flag)
    items = [(0, 0, [rnd.randrange(Q) for _ in range(l)], rnd.randrange(1, Q), 0),
             (0, r - 1, [0] * l, rnd.randrange(1, Q), 0),
             (1, 1, [rnd.randrange(Q) for _ in range(l)], 0, 0),
             (1, 2, [0] * l, 0, 0),
             (0, 1, [rnd.randrange(Q) for _ in range(l)], rnd.randrange(1, Q), 1),
             (2, 1, [1] * l, rnd.randrange(1, Q), 0),
             (0, 3, [0] * (l - 1) + [Q - 1], None, 0),
             (0, 2, [1] + [0] * (l - 1), rnd.randrange(1, Q), 0)]
    K_, M_ = len(items), len(comm)
    lay = V.layout(log_cell, M_, K_)
    proofs = [BAD48 if it[3] is None else K.scalar_commit(it[3]) for it in items]
    d = Dev(ctx)
    pts, kind, comp = d.out(96 * lay["points"]), d.put(bytes(4 * lay["points"])), d.out(48 * (M_ + K_))
    assert doors.dkv_key_copy(ctx.handle, l, d.ptr(pts)) == 0
    assert doors.dkv_decode(ctx.handle, b"".join(comm + proofs), M_ + K_, d.ptr(comp), d.ptr(pts), d.ptr(kind), l) == 0
    assert words(d.get(kind)) == [0] * l + [0, 1, 2] + [2 if it[3] is None else (1 if it[3] == 0 else 0) for it in items]
    bufs = [d.put(b"".join(mont(it[2]) for it in items)), d.put(u32bytes([it[0] for it in items])), d.put(u32bytes([it[1] for it in items])),
            d.put(mont(x)), d.put(u32bytes([it[4] for it in items]))]
    pairs, pre = d.out(192 * 2 * K_), d.out(4 * K_)
    assert doors.dkv_cell_sums(ctx.handle, *[d.ptr(b) for b in bufs], d.ptr(pts), d.ptr(kind), K_, M_, log_cell, d.ptr(pairs), d.ptr(pre)) == 0
    got_pre = [w - (1 << 32) if w >> 31 else w for w in words(d.get(pre))]
    assert got_pre == [0, 0, 0, 0, ERR_DATA, ERR_POINT, ERR_POINT, 0]
    raw = d.get(pairs)
    for i, (c, k, coeffs, pexp, _) in enumerate(items):
        a, b = raw[384 * i:384 * i + 192], raw[384 * i + 192:384 * (i + 1)]
        if got_pre[i]:
            assert a == b"\x5A" * 192 and b == b"\x5A" * 192                    # left alone
            continue
        want = (cexp[c] + x[k] * pexp - sum(cj * pow(K.TAU, j, Q) for j, cj in enumerate(coeffs))) % Q
        assert xyzz_compress(a) == K.scalar_commit(pexp), i
        assert xyzz_compress(b) == K.scalar_commit(want), i
    assert xyzz_compress(raw[384 * 3 + 192:384 * 4]) == ID48                     # nothing but identities and zeros
    d.free()
