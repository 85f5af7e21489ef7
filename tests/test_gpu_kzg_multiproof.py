"""GPU: KZG10 multiproofs (plonk_kzg_multiproof_open / _open_dev / _last / _check; plonk_amd/csrc/kzg_multiproof.hip).

The new kernels are tested on their own through tests/_build/libdev_kzg_multiproof.so (tests/csrc/dev_kzg_multiproof.hip, built by
build(): doors only, the kernels are libplonk_hip.so's) against the big-int model tests/kzg_multiproof_model.py — invd, the
gathered values, g after every chunk of groups and its fix-up, the weights in all three of their output forms — with guard words
around each output.  A wrong aggregation and a wrong MSM therefore fail different tests.

The calls are tested against closed forms: the commit key is the suite's synthetic known-tau key, so C_j = [p_j(tau) g] G,
D = [g(tau) g] G and pi = [((h - g)(tau) - y) / (tau - t) g] G, with r and t from the model's transcript: one big-int expression
and one oracle multiplication each.  Every comparison is exact, byte for byte; there is no tolerance anywhere.

Sizes: log_n 1, 2, 5, 6 (below one wave, one wave), 10 and 11 (one and two workgroups of kmp_aggregate_kernel's 256 x 4 values),
17 (512 partials per group: two strides of kmp_fix_kernel's 256 lanes), 7 with 64 and 65 point groups (one and two launches of the
aggregation), 3 with 63, 64 and 65 vectors (the fold's 64-vector groups)."""
import ctypes
import functools
import os
import random

import pytest

from oracle import bls12_381 as E
from tests import kzg_evals_model as EV
from tests import kzg_multiproof_model as M
from tests import kzg_ref as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_multiproof.so")
Q = E.Q
OK, ERR_ARG, ERR_STATE, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -7, -9, -10, -12
ID48 = K.IDENTITY48
TAU = K.TAU
KEY_POINTS = (1 << 12) + 3
GUARD = 32
R261 = pow(2, 261, Q)


def load_key(ctx, n, tau=TAU):
    buf = ctx.alloc(96 * n)
    ctx.srs_generate_dev(tau, K.G_SCALAR, n, buf.ptr)
    ctx.srs_load_dev(buf.ptr, n)
    ctx.sync()
    buf.free()


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
def domains(ctx):
    import plonk_amd
    made = {}

    def get(log_n):
        if log_n not in made:
            made[log_n] = plonk_amd.KzgDomain(ctx, log_n)
        return made[log_n]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def doors():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_multiproof.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dkm_invd.argtypes = [vp, u32, vp, vp]
    so.dkm_gather.argtypes = [vp, vp, vp, vp, u64, vp]
    so.dkm_aggregate.argtypes = [vp, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    so.dkm_weights.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp]
    so.dkm_const.argtypes = [ci]
    so.dkm_const.restype = u64
    return so


class Guarded:
    """a device buffer with GUARD bytes of 0xA5 on either side of `nbytes` of payload"""

    def __init__(self, ctx, nbytes):
        self.nbytes = nbytes
        self.buf = ctx.alloc(nbytes + 2 * GUARD)
        self.buf.upload(b"\xA5" * (nbytes + 2 * GUARD))
        self.ptr = self.buf.ptr + GUARD

    def read(self):
        raw = self.buf.download()
        assert raw[:GUARD] == b"\xA5" * GUARD and raw[-GUARD:] == b"\xA5" * GUARD, "a kernel wrote outside its output"
        return raw[GUARD:GUARD + self.nbytes]

    def free(self):
        self.buf.free()


def dev_u32(ctx, xs):
    b = ctx.alloc(4 * max(len(xs), 1))
    b.upload(b"".join(int(x).to_bytes(4, "little") for x in xs) or bytes(4))
    return b


def dev_vectors(ctx, vectors):
    import plonk_amd as P
    bufs = []
    for e in vectors:
        b = ctx.alloc(32 * len(e))
        b.upload(e if isinstance(e, (bytes, bytearray)) else P.fr_to_bytes_mont(e))
        bufs.append(b)
    table = ctx.alloc(8 * len(bufs))
    table.upload(b"".join(int(b.ptr).to_bytes(8, "little") for b in bufs))
    return bufs, table


_INVD = {}


def device_invd(ctx, doors, log_n):
    """the table the aggregation reads, made once per size by the door under test (the context frees it with everything else)"""
    import plonk_amd as P
    if (id(ctx), log_n) not in _INVD:
        n = 1 << log_n
        out, meta = Guarded(ctx, 32 * n), Guarded(ctx, 16)
        assert doors.dkm_invd(ctx.handle, log_n, out.ptr, meta.ptr) == 0
        raw = out.read()
        meta.read()
        meta.free()
        _INVD[(id(ctx), log_n)] = (out, P.fr_from_bytes_mont(raw))
    return _INVD[(id(ctx), log_n)]


# ---- the kernels on their own, through the doors ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 12])
def test_invd_against_the_model(ctx, doors, log_n):
    _, got = device_invd(ctx, doors, log_n)
    assert got == M.invd(log_n) and got[0] == 0


def run_aggregate(ctx, doors, log_n, vectors, items, r):
    """gather + the aggregation as the handle runs it -> (values, g)"""
    import plonk_amd as P
    n, Kc = 1 << log_n, len(items)
    perm, group_m, group_off = M.sort_points([m for _, m in items], n)
    groups = len(group_m)
    chunk, per_block, block = doors.dkm_const(0), doors.dkm_const(1), doors.dkm_const(2)
    nwaves = per_block * ((n + block - 1) // block)
    invd, _ = device_invd(ctx, doors, log_n)
    vbufs, table = dev_vectors(ctx, vectors)
    ins = [dev_u32(ctx, [j for j, _ in items]), dev_u32(ctx, [m for _, m in items]), dev_u32(ctx, perm), dev_u32(ctx, group_m),
           dev_u32(ctx, group_off)]
    vidx, midx, dperm, dgm, dgoff = ins
    yk, rpow, rtw = Guarded(ctx, 32 * Kc), Guarded(ctx, 32 * Kc), Guarded(ctx, 48 * Kc)
    ym, cw, negw = Guarded(ctx, 32 * groups), Guarded(ctx, 48 * groups), Guarded(ctx, 32 * groups)
    g, partial = Guarded(ctx, 32 * n), Guarded(ctx, 32 * min(groups, chunk) * nwaves)
    assert doors.dkm_gather(ctx.handle, table.ptr, vidx.ptr, midx.ptr, Kc, yk.ptr) == 0
    values = P.fr_from_bytes_mont(yk.read())
    assert doors.dkm_aggregate(ctx.handle, log_n, table.ptr, vidx.ptr, yk.ptr, Kc, P.fr_to_bytes_mont([r]), dperm.ptr, dgm.ptr, dgoff.ptr,
                               groups, invd.ptr, rpow.ptr, rtw.ptr, ym.ptr, cw.ptr, negw.ptr, g.ptr, partial.ptr) == 0
    got = P.fr_from_bytes_mont(g.read())
    assert P.fr_from_bytes_mont(rpow.read()) == M.powers(r, Kc)
    consts = M.group_constants(vectors, items, r, log_n)
    assert P.fr_from_bytes_mont(ym.read()) == [c[1] for c in consts]
    assert P.fr_from_bytes_mont(negw.read()) == [(-c[2]) % Q for c in consts]
    for x in (rtw, cw, partial, yk):
        x.read()
    for b in vbufs + [table] + ins:
        b.free()
    for x in (yk, rpow, rtw, ym, cw, negw, g, partial):
        x.free()
    return values, got


def item_sets(n, nv, rnd):
    """single, one point, one vector, every pair, duplicates, the edge indexes"""
    sets = {
        "single": [(nv - 1, rnd.randrange(n))],
        "one point": [(rnd.randrange(nv), n // 2) for _ in range(5)],
        "one vector": [(0, rnd.randrange(n)) for _ in range(6)],
        "duplicates": [(0, 1 % n), (nv - 1, 0), (0, 1 % n), (0, 1 % n), (nv - 1, 0)],
        "edges": [(0, 0), (nv - 1, n - 1), (0, n - 1), (nv - 1, 0)],
    }
    if n <= 64:
        sets["every pair"] = [(j, m) for j in range(nv) for m in range(n)]
    return sets


@pytest.mark.parametrize("log_n", [1, 2, 5, 6, 10, 11])
def test_aggregation_against_the_model(ctx, doors, log_n):
    n, nv = 1 << log_n, 3
    rnd = random.Random(log_n)
    vectors = [[rnd.randrange(Q) for _ in range(n)], [Q - 1] * n, [0] * (n - 1) + [9]]
    for name, items in item_sets(n, nv, rnd).items():
        r = rnd.randrange(Q)
        values, g = run_aggregate(ctx, doors, log_n, vectors, items, r)
        assert values == M.values_of(vectors, items), name
        assert g == M.aggregate(vectors, items, r, log_n), name


@pytest.mark.parametrize("groups", [63, 64, 65, 128])
def test_aggregation_on_both_sides_of_the_group_chunk(ctx, doors, groups):
    log_n, nv = 7, 2
    n = 1 << log_n
    assert doors.dkm_const(0) == M.GROUP_CHUNK == 64
    rnd = random.Random(groups)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(nv)]
    ms = rnd.sample(range(n), groups)
    items = [(rnd.randrange(nv), m) for m in ms] + [(1, ms[0]), (0, ms[-1])]
    rnd.shuffle(items)
    r = rnd.randrange(Q)
    assert run_aggregate(ctx, doors, log_n, vectors, items, r)[1] == M.aggregate(vectors, items, r, log_n)


def test_aggregation_with_two_strides_of_the_fix_kernel(ctx, doors):
    log_n = 17
    n = 1 << log_n
    assert doors.dkm_const(1) * (n // doors.dkm_const(2)) == 512
    rnd = random.Random(17)
    vectors = [[rnd.randrange(Q) for _ in range(n)]]
    items = [(0, 0), (0, n - 1), (0, n - 1)]
    r = rnd.randrange(Q)
    assert run_aggregate(ctx, doors, log_n, vectors, items, r)[1] == M.aggregate(vectors, items, r, log_n)


def slot29(raw48):
    """an Fr29Slot (9 limbs of 29 bits in 12 words, the value times 2^261) -> the value"""
    words = [int.from_bytes(raw48[4 * i:4 * i + 4], "little") for i in range(12)]
    assert words[9:] == [0, 0, 0] and all(w < (1 << 29) for w in words[:9])
    return sum(w << (29 * i) for i, w in enumerate(words[:9])) % Q * pow(R261, -1, Q) % Q


@pytest.mark.parametrize("Kc", [1, 63, 64, 65, 5000])
def test_weights_against_the_model(ctx, doors, Kc):
    import plonk_amd as P
    log_n, nv = 9, 4
    n = 1 << log_n
    rnd = random.Random(Kc)
    items = [(rnd.choice((0, 1, 3)), rnd.randrange(n)) for _ in range(Kc)]                    # vector 2 gets no item
    values = [rnd.randrange(Q) for _ in range(Kc)]
    r, t = rnd.randrange(Q), rnd.randrange(Q)
    perm, off = M.counting_sort([j for j, _ in items], nv)
    ins = [dev_u32(ctx, [m for _, m in items]), dev_u32(ctx, perm), dev_u32(ctx, off)]
    yk = ctx.alloc(32 * Kc)
    yk.upload(P.fr_to_bytes_mont(values))
    rpow, wt, stw, yout = Guarded(ctx, 32 * Kc), Guarded(ctx, 32 * Kc), Guarded(ctx, 48 * nv), Guarded(ctx, 32)
    sc, ids = Guarded(ctx, 32 * (nv + 3)), Guarded(ctx, 4 * (nv + 3))
    assert doors.dkm_weights(ctx.handle, log_n, P.fr_to_bytes_mont([r]), P.fr_to_bytes_mont([t]), ins[0].ptr, yk.ptr, ins[1].ptr, ins[2].ptr,
                             Kc, nv, rpow.ptr, wt.ptr, stw.ptr, yout.ptr, sc.ptr, ids.ptr) == 0
    want_wt, want_s, want_y = M.weights(items, values, r, t, log_n, nv)
    assert want_s[2] == 0
    assert P.fr_from_bytes_mont(wt.read()) == want_wt
    assert P.fr_from_bytes_mont(yout.read()) == [want_y]
    raw = stw.read()
    assert [slot29(raw[48 * j:48 * j + 48]) for j in range(nv)] == want_s
    raw = sc.read()
    assert [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(nv + 3)] == want_s + [Q - 1, t, (-want_y) % Q]
    raw = ids.read()
    assert [int.from_bytes(raw[4 * i:4 * i + 4], "little") for i in range(nv + 3)] == list(range(nv + 3))
    rpow.read()
    for b in ins + [yk]:
        b.free()
    for x in (rpow, wt, stw, yout, sc, ids):
        x.free()


# ---- the calls against the closed forms ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lagrange(log_n):
    return EV.lagrange_at(TAU, log_n)


def at_tau(e, log_n):
    return sum(a * b for a, b in zip(e, lagrange(log_n))) % Q


def expected(vectors, items, log_n, label=b"", commitments=None, challenges=None):
    """(values, commitments, proof96, r, t, s, y, D exponent) in closed form; r and t from the model's transcript"""
    values = M.values_of(vectors, items)
    cexp = [at_tau(e, log_n) for e in vectors]
    cm = [K.scalar_commit(x) for x in cexp] if commitments is None else [bytes(c) for c in commitments]
    tr, r = M.transcript_r(label, log_n, cm, items, values)
    if challenges is not None:
        r = challenges[0]
    d_exp = at_tau(M.aggregate(vectors, items, r, log_n), log_n)
    d48 = K.scalar_commit(d_exp)
    t = M.transcript_t(tr, d48) if challenges is None else challenges[1]
    _, s, y = M.weights(items, values, r, t, log_n, len(vectors))
    pi_exp = (sum(a * b for a, b in zip(s, cexp)) - d_exp - y) * pow((TAU - t) % Q, -1, Q) % Q
    return values, cm, d48 + K.scalar_commit(pi_exp), r, t, s, y, d_exp


def check_as_an_ordinary_opening(key, commitments, proof, s, y, t):
    """E - D opened at t with the value y and the witness pi, E = sum_j s_j C_j by the oracle's group law"""
    import plonk_amd as P
    acc = None
    for sj, c in zip(s, commitments):
        pt = E.g1_decompress(c)
        if sj and pt is not None:
            acc = E.g1_add(acc, E.g1_mul(pt, sj))
    d = E.g1_decompress(proof[:48])
    if d is not None:
        acc = E.g1_add(acc, E.g1_mul(d, Q - 1))
    opening = P.KzgProof.make(E.g1_compress(acc), y, proof[48:])
    assert key.check_each([t], [opening]) == [OK]


def assert_last(dom, nv, items, computed, host_form, built=None):
    last = dom.multi_last()
    groups = len({m for _, m in items})
    p = M.plan(dom.log_n, nv, len(items), groups, computed, host_form)
    assert (last["log_n"], last["items"], last["vectors"], last["point_groups"]) == (dom.log_n, len(items), nv, groups)
    assert (last["commitments_computed"], last["msm_launches"], last["msm_terms"], last["products"]) == \
        (p["commitments_computed"], p["msm_launches"], p["msm_terms"], p["products"])
    assert last["msm_launches"] == last["commitments_computed"] + 2 and last["msm_terms"] == dom.n
    assert last["device_bytes"] >= 32 * dom.n + 32 * p["stage_values"]
    if built is not None:
        assert last["built_points"] == built
    return last


CALLS = [(1, 1, 1), (1, 3, 5), (2, 1, 4), (2, 3, 9), (3, 1, 1), (3, 3, 40), (4, 3, 7), (5, 1, 33), (5, 3, 200), (6, 1, 64), (6, 3, 3000),
         (12, 3, 300), (3, 63, 70), (3, 64, 70), (3, 65, 70)]


@pytest.mark.parametrize("log_n,nv,Kc", CALLS)
def test_open_and_check_against_the_closed_form(domains, key, log_n, nv, Kc):
    dom, n = domains(log_n), 1 << log_n
    rnd = random.Random(100 * log_n + nv + Kc)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(nv)]
    items = [(rnd.randrange(nv), rnd.randrange(n)) for _ in range(Kc)]
    label = b"multi-%d" % log_n
    values, cm, proof, r, t, s, y, _ = expected(vectors, items, log_n, label)
    got = dom.open_multi(vectors, items, label)
    assert got == (values, cm, proof)
    assert dom._multi_last_challenges() == (r, t)                                  # the transcript challenges are the model's
    assert_last(dom, nv, items, True, True)
    assert key.check_multi(log_n, cm, items, values, proof, label)
    check_as_an_ordinary_opening(key, cm, proof, s, y, t)
    # the same commitments handed in: hashed as given, nothing computed
    assert dom.open_multi(vectors, items, label, commitments=cm) == got
    assert_last(dom, nv, items, False, True, built=0)


def test_given_commitments_are_hashed_not_decoded(domains, key):
    log_n, nv = 4, 2
    dom, n = domains(log_n), 16
    rnd = random.Random(44)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(nv)]
    items = [(0, 3), (1, 15), (1, 3)]
    wrong = [K.scalar_commit(5), b"\xff" * 48]                                     # one wrong point, one that does not decode
    values, cm, proof, *_ = expected(vectors, items, log_n, b"", commitments=wrong)
    assert dom.open_multi(vectors, items, commitments=wrong) == (values, wrong, proof)
    rc, _ = key.check_multi_code(log_n, wrong, items, values, proof)
    assert rc == ERR_POINT
    rc, _ = key.check_multi_code(log_n, [wrong[0], K.scalar_commit(at_tau(vectors[1], log_n))], items, values, proof)
    assert rc == ERR_VERIFY


def test_resident_form_gives_the_bytes_of_the_host_form(ctx, domains, key):
    import plonk_amd as P
    log_n, nv = 6, 5
    dom, n = domains(log_n), 64
    rnd = random.Random(606)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(nv)]
    items = [(rnd.randrange(nv), rnd.randrange(n)) for _ in range(77)]
    bufs, table = dev_vectors(ctx, vectors)
    ptrs = [b.ptr for b in bufs]
    want = dom.open_multi(vectors, items, b"dev")
    assert dom.open_multi_dev(ptrs, items, b"dev") == want == expected(vectors, items, log_n, b"dev")[:3]
    assert_last(dom, nv, items, True, False)
    assert dom.open_multi_dev(ptrs, items, b"dev", commitments=want[1]) == want
    assert key.check_multi(log_n, want[1], items, want[0], want[2], b"dev")
    for b, e in zip(bufs, vectors):
        assert b.download() == P.fr_to_bytes_mont(e)                               # the inputs are only read
        b.free()
    table.free()


def test_zero_vector_k1_relation_and_r_zero(domains, key):
    log_n = 5
    dom, n = domains(log_n), 32
    rnd = random.Random(55)
    vectors = [[0] * n, [rnd.randrange(Q) for _ in range(n)]]
    items = [(0, 7), (1, 7), (1, 31), (0, 0)]
    values, cm, proof, r, t, s, y, _ = expected(vectors, items, log_n)
    assert cm[0] == ID48 and values[0] == 0
    assert dom.open_multi(vectors, items) == (values, cm, proof)
    assert key.check_multi(log_n, cm, items, values, proof)
    check_as_an_ordinary_opening(key, cm, proof, s, y, t)
    # only the zero vector: g = 0, h = 0, D and pi are the identity
    got = dom.open_multi(vectors[:1], [(0, 3), (0, 4)])
    assert got == ([0, 0], [ID48], ID48 + ID48) and key.check_multi(log_n, [ID48], [(0, 3), (0, 4)], [0, 0], ID48 + ID48)
    # K = 1: item 0 has the weight r^0 = 1, so g = (p - y) / (X - w^m) and D is the witness plonk_kzg_open_evals gives at w^m
    # (with its evaluation y = e[m]); pi then opens h - g = p / (t - w^m) - g at t
    m = 19
    ev, cm1, wit = dom.open_evals(vectors[1:], EV.domain_points(log_n)[m])
    got = dom.open_multi(vectors[1:], [(0, m)])
    assert got[0] == ev == [vectors[1][m]] and got[1] == cm1 and got[2][:48] == wit
    assert key.check_multi(log_n, got[1], [(0, m)], got[0], got[2])
    # an override with r = 0: only item 0 counts (0^0 = 1); legal, and checked with the same override
    ch = (0, rnd.randrange(Q))
    want = expected(vectors, items, log_n, challenges=ch)
    got = dom.open_multi(vectors, items, challenges=ch)
    assert got == want[:3] and dom._multi_last_challenges() == ch
    assert got[2] == expected(vectors, items[:1], log_n, commitments=cm, challenges=ch)[2]
    assert key.check_multi(log_n, cm, items, values, got[2], challenges=ch)
    assert not key.check_multi(log_n, cm, items, values, got[2])                   # the transcript's challenges are others


# ---- rejections -----------------------------------------------------------------------------------------------------------------
def test_every_tampering_is_rejected(domains, key):
    import plonk_amd as P
    log_n, nv = 5, 3
    dom, n = domains(log_n), 32
    rnd = random.Random(9)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(nv)]
    items = [(rnd.randrange(nv), rnd.randrange(n)) for _ in range(12)]
    label = b"tamper"
    values, cm, proof = dom.open_multi(vectors, items, label)
    code = lambda **kw: key.check_multi_code(log_n, kw.get("cm", cm), kw.get("items", items), kw.get("values", values),
                                             kw.get("proof", proof), kw.get("label", label))[0]
    rc, info = key.check_multi_code(log_n, cm, items, values, proof, label)
    assert rc == OK and (info["proofs"], info["msm_terms"], info["pairing_checks"], info["rejected"]) == (12, nv + 3, 1, 0)
    assert code(values=values[:5] + [(values[5] + 1) % Q] + values[6:]) == ERR_VERIFY
    j, m = items[3]
    assert code(items=items[:3] + [(j, (m + 1) % n)] + items[4:]) == ERR_VERIFY
    assert code(items=items[:3] + [((j + 1) % nv, m)] + items[4:]) == ERR_VERIFY
    other = K.scalar_commit(12345)
    assert code(cm=[other] + cm[1:]) == ERR_VERIFY
    assert code(proof=other + proof[48:]) == ERR_VERIFY
    assert code(proof=proof[:48] + other) == ERR_VERIFY
    assert code(label=b"tampes") == ERR_VERIFY
    a, b = (0, 1) if items[0] != items[1] else (0, 2)
    sw_i, sw_v = list(items), list(values)
    sw_i[a], sw_i[b], sw_v[a], sw_v[b] = sw_i[b], sw_i[a], sw_v[b], sw_v[a]
    assert (sw_i, sw_v) != (items, values) and code(items=sw_i, values=sw_v) == ERR_VERIFY
    rc, info = key.check_multi_code(log_n, cm, items, values, proof[:48] + other, label)
    assert rc == ERR_VERIFY and info["rejected"] == 12
    # points that do not decode, and a point of the curve outside the subgroup
    flipped = bytes([cm[0][0] ^ 0x20]) + cm[0][1:]                                  # the other root: a valid point, a wrong commitment
    assert code(cm=[flipped] + cm[1:]) == ERR_VERIFY
    for bad in (b"\xff" * 48, outside_subgroup()):
        assert code(cm=[bad] + cm[1:]) == ERR_POINT
        assert code(proof=bad + proof[48:]) == ERR_POINT
        assert code(proof=proof[:48] + bad) == ERR_POINT
    assert not key.check_multi(log_n, cm, items, values, proof, b"other label")
    with pytest.raises(P.PlonkError) as ei:
        key.check_multi(log_n, [b"\xff" * 48] + cm[1:], items, values, proof, label)
    assert ei.value.code == ERR_POINT


@functools.lru_cache(maxsize=None)
def outside_subgroup() -> bytes:
    """a compressed point of the curve that is not in G1: the first x = 1, 2, ... with x^3 + 4 a square whose point does not
    vanish under the group order"""
    p = E.P
    x = 1
    while True:
        y2 = (x * x * x + 4) % p
        y = pow(y2, (p + 1) // 4, p)
        if y * y % p == y2 and E.g1_add(E.g1_mul((x, y), Q - 1), (x, y)) is not None:
            b = bytearray(x.to_bytes(48, "big"))
            b[0] |= 0x80
            if y > (p - y) % p:
                b[0] |= 0x20
            return bytes(b)
        x += 1


# ---- errors and state -------------------------------------------------------------------------------------------------------------
def test_errors_in_their_order_leave_the_outputs_untouched(ctx, domains, key):
    import plonk_amd as P
    log_n = 3
    dom, n = domains(log_n), 8
    lib = ctx.lib
    mont = P.fr_to_bytes_mont
    good, noncanon = mont(range(1, 9)), mont([1, 2]) + b"\xff" * 32 + mont([4, 5, 6, 7, 8])
    vals = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    cout = ctypes.create_string_buffer(b"\xA5" * 96, 96)
    proof = ctypes.create_string_buffer(b"\xA5" * 96, 96)
    w = EV.domain_points(log_n)
    in_domain = mont([5, w[3]])
    u32s = lambda xs: (ctypes.c_uint32 * max(len(xs), 1))(*xs)

    def open_(bufs, vi=(0, 1), mi=(7, 0), h=dom.handle, nv=None, count=None, label=b"x", label_len=1, ov=None, v=vals, p=proof, arr=None,
              fn=lib.plonk_kzg_multiproof_open, no_vi=False, no_mi=False):
        keep = [ctypes.create_string_buffer(b, len(b)) if b is not None else None for b in bufs]
        a = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.cast(k, ctypes.c_void_p).value if k is not None else None for k in keep])
        return fn(h, a if arr is None else arr, len(bufs) if nv is None else nv, None, None if no_vi else u32s(vi), None if no_mi else u32s(mi),
                  len(vi) if count is None else count, label, label_len, ov, v, cout, p)

    two = [good, good]
    for rc in (open_(two, h=None), open_(two, v=None), open_(two, p=None), open_(two, no_vi=True), open_(two, no_mi=True),
               open_(two, label=None), open_([good, None]), lib.plonk_kzg_multiproof_open(dom.handle, None, 2, None, u32s([0]), u32s([0]), 1,
                                                                                          b"", 0, None, vals, cout, proof),
               open_(two, vi=(), mi=()), open_(two, count=(1 << 20) + 1), open_([], vi=(0,), mi=(0,)), open_(two, nv=65537),
               open_(two, vi=(0, 2)), open_(two, mi=(8, 0))):
        assert rc == ERR_ARG
    # ARG before DATA before STATE
    assert open_([good, noncanon], vi=(0, 2)) == ERR_ARG
    assert open_([good, noncanon]) == ERR_DATA
    assert open_(two, ov=b"\xff" * 32 + mont([9])) == ERR_DATA
    assert open_(two, ov=mont([9]) + b"\xff" * 32) == ERR_DATA
    assert open_(two, ov=in_domain) == ERR_DATA                                     # an override t = w^3
    assert open_(two, ov=mont([5, 1])) == ERR_DATA
    # the resident form finds the value on the device
    bufs = [ctx.alloc(32 * n), ctx.alloc(32 * n)]
    bufs[0].upload(good)
    bufs[1].upload(noncanon)
    arr = (ctypes.c_void_p * 2)(bufs[0].ptr, bufs[1].ptr)
    assert open_(two, arr=arr, fn=lib.plonk_kzg_multiproof_open_dev) == ERR_DATA
    assert open_(two, arr=arr, vi=(0, 2), fn=lib.plonk_kzg_multiproof_open_dev) == ERR_ARG
    assert vals.raw == b"\xA5" * 64 and cout.raw == b"\xA5" * 96 and proof.raw == b"\xA5" * 96
    assert lib.plonk_kzg_multiproof_last(dom.handle, None) == ERR_ARG
    assert lib.plonk_kzg_multiproof_last(None, ctypes.byref(P._KzgMultiproofInfo())) == ERR_ARG
    # and the same buffers take a good call
    assert open_([good], arr=arr, nv=1, vi=(0, 0), fn=lib.plonk_kzg_multiproof_open_dev) == OK
    want = expected([list(range(1, 9))], [(0, 7), (0, 0)], log_n, b"x")
    assert vals.raw == mont(want[0]) and cout.raw[:48] == want[1][0] and proof.raw == want[2]
    assert cout.raw[48:] == b"\xA5" * 48
    for b in bufs:
        b.free()
    # the check: ARG, DATA, POINT, then the pairing
    values, cm, pr = want[:3]
    items = [(0, 7), (0, 0)]
    chk = lambda **kw: key.check_multi_code(kw.get("log_n", log_n), kw.get("cm", cm), kw.get("items", items), kw.get("values", values),
                                            kw.get("proof", pr), b"x", kw.get("ch"))[0]
    assert chk() == OK
    assert chk(log_n=0) == ERR_ARG and chk(log_n=21) == ERR_ARG
    assert chk(items=[(0, 8), (0, 0)]) == ERR_ARG and chk(items=[(1, 7), (0, 0)]) == ERR_ARG
    assert chk(cm=[], items=[(0, 7), (0, 0)]) == ERR_ARG
    assert chk(items=[], values=[]) == ERR_ARG
    assert lib.plonk_kzg_multiproof_check(key.handle, log_n, cm[0], 1, u32s([0]), u32s([0]), None, 1, pr, b"", 0, None, None) == ERR_ARG
    assert lib.plonk_kzg_multiproof_check(None, log_n, cm[0], 1, u32s([0]), u32s([0]), mont([1]), 1, pr, b"", 0, None, None) == ERR_ARG
    assert chk(values=[b"\xff" * 32, values[1]], items=[(0, 8), (0, 0)]) == ERR_ARG
    assert chk(values=[b"\xff" * 32, values[1]], cm=[b"\xff" * 48]) == ERR_DATA       # DATA before POINT
    assert chk(ch=b"\xff" * 32 + mont([9])) == ERR_DATA and chk(ch=in_domain) == ERR_DATA
    assert chk(cm=[b"\xff" * 48]) == ERR_POINT
    assert chk(ch=(5, 9)) == ERR_VERIFY


def test_state_errors_reloaded_key_and_communicator():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, 16)
    d = plonk_amd.KzgDomain(c, 3)
    e, items = [[1, 2, 3, 4, 5, 6, 7, 8]], [(0, 2), (0, 5)]
    before = d.open_multi(e, items)
    assert before == expected(e, items, 3)[:3]
    c.comm_init(plonk_amd.Context.comm_unique_id(), 0, 1)       # a communicator: the context holds only a range of the key
    with pytest.raises(plonk_amd.PlonkError) as ei:
        d.open_multi(e, items)
    assert ei.value.code == ERR_STATE
    c.comm_destroy()
    assert d.open_multi(e, items) == before
    load_key(c, 16)                                             # the same key again: still another generation
    for call in (lambda: d.open_multi(e, items), d.multi_last):
        with pytest.raises(plonk_amd.PlonkError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    # the order: an argument error and a data error come before the state error
    with pytest.raises(plonk_amd.PlonkError) as ei:
        d.open_multi(e, [(0, 8)])
    assert ei.value.code == ERR_ARG
    with pytest.raises(plonk_amd.PlonkError) as ei:
        d.open_multi(e, items, challenges=(5, 1))
    assert ei.value.code == ERR_DATA
    d.close()
    d2 = plonk_amd.KzgDomain(c, 3)
    assert d2.multi_last()["items"] == 0
    assert d2.open_multi(e, items) == before
    d2.close()
    c.close()


def test_context_left_as_found():
    """a proof, an opening, a plonk_msm_points report, plonk_kzg_domain_last and plonk_kzg_evals_last made on the same context
    before and after multiproof calls are identical; the tables stay"""
    import plonk_amd as P
    from tests import circuits as C
    c = P.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=78)()
    case = C.compile_fast(comp, b"kzg-multi")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = P.Prover.compile(c, b"kzg-multi", cols["selectors"], cols["wires"], cols["witnesses"])
    k = P.KzgKey(c, K.opening_key())
    rnd = random.Random(77)
    f = [rnd.randrange(Q) for _ in range(300)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    proof = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    opening = c.kzg_open([f, f[:7]], z, v)
    c.msm_points([E.g1_mul(E.G1_GEN, 3), E.g1_mul(E.G1_GEN, 5)], [2, 9])
    points_report = c.last_msm_points()
    dom = P.KzgDomain(c, 6)
    dom.open([[1, 2, 3]])
    domain_report = dom.last()
    e = [[rnd.randrange(Q) for _ in range(64)] for _ in range(3)]
    fresh = dom.evals_last()
    items = [(rnd.randrange(3), rnd.randrange(64)) for _ in range(20)]
    tables, rows = c.table_bytes(), c.table_rows()
    want = expected(e, items, 6, b"ctx")
    assert dom.open_multi(e, items, b"ctx") == want[:3]
    assert dom.multi_last()["built_points"] == 1
    # the Lagrange points are shared with the evaluation-form calls: their report shows them, and nothing else changed
    after = dom.evals_last()
    assert after["lagrange_bytes"] == 96 * 64 and {**after, "lagrange_bytes": fresh["lagrange_bytes"]} == fresh
    dom.open_evals(e, z, v)
    evals_report = dom.evals_last()
    assert evals_report["built_points"] == 0
    assert dom.open_multi(e, items, b"ctx") == want[:3] and k.check_multi(6, want[1], items, want[0], want[2], b"ctx")
    assert dom.multi_last()["built_points"] == 0
    assert dom.evals_last() == evals_report
    assert prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3)) == proof
    assert c.kzg_open([f, f[:7]], z, v) == opening
    assert (c.table_bytes(), c.table_rows()) == (tables, rows)
    assert c.last_msm_points() == points_report
    assert dom.last() == domain_report
    k.close()
    dom.close()
    prover.close()
    c.close()
