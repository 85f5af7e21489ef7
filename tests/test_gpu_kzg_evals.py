"""GPU: KZG10 in evaluation form (plonk_kzg_commit_evals / plonk_kzg_open_evals / _dev / plonk_kzg_evals_last;
plonk_amd/csrc/kzg_evals.hip).

The scalar stage is tested on its own through tests/_build/libdev_kzg_evals.so (tests/csrc/dev_kzg_evals.hip, built by
build(): doors only, the kernels are libplonk_hip.so's) against the big-int model tests/kzg_evals_model.py — the inverses, the
lane m, every y_j, F and q, with guard words around each output — and so is the Lagrange-point build.  A wrong quotient and a
wrong MSM therefore fail different tests.

The calls are tested against closed forms: the commit key is the suite's synthetic known-tau key, so commitment j is
[p_j(tau) g] G with p_j(tau) = sum_i e_j[i] L_i(tau), and the witness is [(F(tau) - Y) / (tau - z) g] G: one big-int expression
and one oracle multiplication each, at any size.  At 2^12 the bytes are those of plonk_kzg_open of plonk_ntt(inverse) of the
same vectors, and for z = w^m those of witness m of plonk_kzg_open_domain on the folded polynomial.  Every comparison is exact.

Sizes: log_n 1, 2, 5, 6 (5 and 6 straddle the 64 terms below which msm_points_run takes its per-term kernel), 8 and 9 (one
and two workgroups of the 64 x 4 batch inversion), 10 and 11 (one and two workgroups of the fold kernel's 256 x 4 values and
four and eight of the quotient kernel's 256), and 2^18 for the scalar stage (the 256 x 16 geometry of the inversion above
2^17).  Points: random, 0, w^0, w^(n-1), and w^m for m on both sides of those boundaries."""
import ctypes
import functools
import os
import random

import pytest

from oracle import bls12_381 as E
from tests import kzg_evals_model as M
from tests import kzg_ref as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_evals.so")
Q = E.Q
OK, ERR_ARG, ERR_STATE, ERR_DATA = 0, -1, -7, -9
ID48 = K.IDENTITY48
NONE = M.NONE
KEY_POINTS = (1 << 12) + 3
GUARD = 32                                                     # bytes of 0xA5 before and after every door output


def load_key(ctx, n, tau=K.TAU):
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
    assert os.path.exists(SO), "tests/_build/libdev_kzg_evals.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dke_inverses.argtypes = [vp, u32, vp, vp, vp, vp, u32]
    so.dke_fold_eval.argtypes = [vp, u32, vp, u32, vp, vp, vp, u64, vp, vp, vp, vp]
    so.dke_quotient.argtypes = [vp, u32, vp, vp, vp, u64, vp, vp]
    so.dke_lagrange_points.argtypes = [vp, u32, vp]
    so.dke_const.argtypes = [ci]
    so.dke_const.restype = u64
    return so


@functools.lru_cache(maxsize=None)
def lagrange(log_n, tau=K.TAU):
    return M.lagrange_at(tau, log_n)


def at_tau(e, log_n, tau=K.TAU):
    return sum(a * b for a, b in zip(e, lagrange(log_n, tau))) % Q


def expected(vectors, z, v, log_n, tau=K.TAU):
    """(evaluations, commitments, witness) in closed form"""
    s = M.scalar_stage(vectors, z, v, log_n)
    pt = [at_tau(e, log_n, tau) for e in vectors]
    ft, vp = 0, 1
    for x in pt:
        ft = (ft + vp * x) % Q
        vp = vp * v % Q
    assert (tau - z) % Q
    wit = K.scalar_commit((ft - s["Y"]) * pow((tau - z) % Q, -1, Q) % Q)
    return s["y"], [K.scalar_commit(x) for x in pt], wit


def assert_last(dom, count, m, commitments, witness, host_form, built=None):
    last = dom.evals_last()
    p = M.plan(dom.log_n, count, commitments, witness, host_form)
    assert (last["log_n"], last["count"], last["in_domain_index"]) == (dom.log_n, count, m)
    assert (last["msm_launches"], last["msm_terms"]) == (p["msm_launches"], p["msm_terms"])
    if built is not None:
        assert last["built_points"] == built
    if p["msm_launches"]:
        assert last["lagrange_bytes"] == 96 * dom.n
    return last


def boundary_indices(n):
    """m on both sides of every block boundary of the inversion (256 at these sizes), the quotient kernel (256) and the fold
    kernel (lanes 256 apart, workgroups of 1024), inside n"""
    return sorted({m for m in (0, n - 1, 63, 64, 255, 256, 1023, 1024) if m < n})


# ---- the scalar stage on its own, through the doors ---------------------------------------------------------------------------
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


def run_stage(ctx, doors, log_n, vectors, z, v):
    """the three doors in the order the handle runs them -> dict like M.scalar_stage's (Y from the device's own y)"""
    import plonk_amd as P
    n, count = 1 << log_n, len(vectors)
    vbufs = []
    for e in vectors:
        b = ctx.alloc(32 * n)
        b.upload(P.fr_to_bytes_mont(e))
        vbufs.append(b)
    table = ctx.alloc(8 * count)
    table.upload(b"".join(int(b.ptr).to_bytes(8, "little") for b in vbufs))
    nwaves = doors.dke_const(1) * ((n + doors.dke_const(2) - 1) // doors.dke_const(2))
    qblocks = (n + doors.dke_const(3) - 1) // doors.dke_const(3)
    inv, meta, fold, q = Guarded(ctx, 32 * n), Guarded(ctx, 16), Guarded(ctx, 32 * n), Guarded(ctx, 32 * n)
    partial, evals = Guarded(ctx, 32 * nwaves * min(count, doors.dke_const(0))), Guarded(ctx, 32 * count)
    vpow, qpart = Guarded(ctx, 48 * count), Guarded(ctx, 32 * qblocks)
    zb, vb = P.fr_to_bytes_mont([z]), P.fr_to_bytes_mont([v])
    assert doors.dke_inverses(ctx.handle, log_n, zb, inv.ptr, meta.ptr, table.ptr, count) == 0
    mraw = meta.read()
    m, bad = int.from_bytes(mraw[:8], "little"), int.from_bytes(mraw[8:], "little")
    out = {"inv": P.fr_from_bytes_mont(inv.read()), "m": m, "bad": bad}
    assert doors.dke_fold_eval(ctx.handle, log_n, table.ptr, count, zb, vb, inv.ptr, m, vpow.ptr, fold.ptr, partial.ptr, evals.ptr) == 0
    out["y"] = P.fr_from_bytes_mont(evals.read())
    out["F"] = P.fr_from_bytes_mont(fold.read())
    partial.read(), vpow.read()
    Y, vp = 0, 1
    for yj in out["y"]:
        Y = (Y + vp * yj) % Q
        vp = vp * v % Q
    out["Y"] = Y
    assert doors.dke_quotient(ctx.handle, log_n, fold.ptr, inv.ptr, P.fr_to_bytes_mont([Y]), m, q.ptr, qpart.ptr) == 0
    out["q"] = P.fr_from_bytes_mont(q.read())
    qpart.read(), inv.read(), fold.read()
    for b in vbufs + [table]:
        b.free()
    for g in (inv, meta, fold, q, partial, evals, vpow, qpart):
        g.free()
    return out


@pytest.mark.parametrize("log_n", [1, 2, 5, 6, 8, 9, 10, 11])
def test_scalar_stage_against_the_model(ctx, doors, log_n):
    n = 1 << log_n
    rnd = random.Random(log_n)
    pts = M.domain_points(log_n)
    single = [0] * n
    single[n - 1] = 9
    vectors = [[rnd.randrange(Q) for _ in range(n)], [Q - 1] * n, single]
    v = rnd.randrange(Q)
    for z in [rnd.randrange(Q), 0] + [pts[m] for m in boundary_indices(n)]:
        got = run_stage(ctx, doors, log_n, vectors, z, v)
        want = M.scalar_stage(vectors, z, v, log_n)
        assert got["bad"] == 0
        for k in ("m", "inv", "y", "F", "Y", "q"):
            assert got[k] == want[k], (k, z)


def test_scalar_stage_of_more_vectors_than_one_fold_launch(ctx, doors):
    log_n, n, count = 5, 32, M.GROUP + 1
    rnd = random.Random(65)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(count)]
    v = rnd.randrange(Q)
    for z in (rnd.randrange(Q), M.domain_points(log_n)[17]):
        got, want = run_stage(ctx, doors, log_n, vectors, z, v), M.scalar_stage(vectors, z, v, log_n)
        for k in ("m", "y", "F", "q"):
            assert got[k] == want[k], k


def test_scalar_stage_flags_a_non_canonical_resident_value(ctx, doors):
    import plonk_amd as P
    n = 64
    b = ctx.alloc(32 * n)
    b.upload(P.fr_to_bytes_mont([1] * n))
    b.upload(b"\xff" * 32, offset=32 * 63)
    table, inv, meta = ctx.alloc(8), ctx.alloc(32 * n), ctx.alloc(16)
    table.upload(int(b.ptr).to_bytes(8, "little"))
    assert doors.dke_inverses(ctx.handle, 6, P.fr_to_bytes_mont([5]), inv.ptr, meta.ptr, table.ptr, 1) == 0
    raw = meta.download()
    assert int.from_bytes(raw[:8], "little") == NONE and int.from_bytes(raw[8:], "little") == 1
    for x in (b, table, inv, meta):
        x.free()


def test_scalar_stage_at_2_to_18_sampled(ctx, doors):
    """the 256 x 16 geometry of the batch inversion (above 2^17 values), 256 workgroups of the fold kernel; z = w^m with m in
    the last workgroup.  The model runs in full, the comparison is sampled."""
    log_n, n = 18, 1 << 18
    rnd = random.Random(18)
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    import plonk_amd as P
    e = P.fr_from_bytes_mont(bytes(raw))
    m = n - 4096 + 5
    z = M.domain_points(log_n)[m]
    got, want = run_stage(ctx, doors, log_n, [e], z, 1), M.scalar_stage([e], z, 1, log_n)
    assert got["m"] == want["m"] == m and got["y"] == want["y"] == [e[m]]
    idx = [0, 1, 4095, 4096, m - 1, m, m + 1, n - 1] + rnd.sample(range(n), 24)
    for k in ("inv", "F", "q"):
        assert [got[k][i] for i in idx] == [want[k][i] for i in idx], k
    z = rnd.randrange(Q)
    got, want = run_stage(ctx, doors, log_n, [e], z, 1), M.scalar_stage([e], z, 1, log_n)
    assert got["m"] == NONE and got["y"] == want["y"]
    for k in ("inv", "F", "q"):
        assert [got[k][i] for i in idx] == [want[k][i] for i in idx], k


@pytest.mark.parametrize("log_n", [1, 3, 6])
def test_lagrange_points_against_the_oracle(ctx, doors, log_n):
    import plonk_amd as P
    n = 1 << log_n
    out = Guarded(ctx, 96 * n)
    assert doors.dke_lagrange_points(ctx.handle, log_n, out.ptr) == 0
    raw = out.read()
    for i, s in enumerate(lagrange(log_n)):
        assert raw[96 * i:96 * i + 96] == P.g1_to_raw96(E.g1_mul(E.G1_GEN, s * K.G_SCALAR % Q)), i
    out.free()


# ---- the calls against the closed forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 5, 6, 8, 9, 10, 11])
@pytest.mark.parametrize("count", [0, 1, 3])
def test_commit_and_open_against_the_closed_form(domains, log_n, count):
    dom, n = domains(log_n), 1 << log_n
    rnd = random.Random(10 * log_n + count)
    pts = M.domain_points(log_n)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(count)]
    v = rnd.randrange(Q) if count != 1 else None
    if count == 0:
        assert dom.commit_evals([]) == []
        assert dom.open_evals([], 5, None) == ([], [], ID48)
        assert_last(dom, 0, NONE, True, True, True)
        return
    first = True
    for z in [rnd.randrange(Q), 0] + [pts[m] for m in boundary_indices(n)]:
        ev, cm, wit = dom.open_evals(vectors, z, v, commitments=first)
        want = expected(vectors, z, v if v is not None else 1, log_n)
        assert ev == want[0], z
        assert wit == want[2], z
        if first:
            assert cm == want[1]
            assert dom.commit_evals(vectors) == want[1]
            assert_last(dom, count, NONE, True, False, True)
            ev, cm, wit = dom.open_evals(vectors, z, v, commitments=False)
        assert_last(dom, count, pts.index(z) if z in pts else NONE, False, True, True, built=0)
        first = False


@pytest.mark.parametrize("log_n", [5, 6])
def test_more_vectors_than_one_fold_launch(domains, log_n):
    dom, n, count = domains(log_n), 1 << log_n, M.GROUP + 1
    rnd = random.Random(650 + log_n)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(count)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    want = expected(vectors, z, v, log_n)
    assert dom.open_evals(vectors, z, v) == want
    assert_last(dom, count, NONE, True, True, True)
    zm = M.domain_points(log_n)[n - 2]
    ev, cm, wit = dom.open_evals(vectors, zm, v, commitments=False)
    assert (ev, wit) == (expected(vectors, zm, v, log_n)[0], expected(vectors, zm, v, log_n)[2])
    assert ev == [e[n - 2] for e in vectors]


@pytest.mark.parametrize("log_n", [2, 6])
def test_shaped_vectors(domains, log_n):
    dom, n = domains(log_n), 1 << log_n
    pts = M.domain_points(log_n)
    rnd = random.Random(log_n)
    for m in (0, n - 1):
        single = [0] * n
        single[m] = 11
        for z in (pts[m], rnd.randrange(Q)):
            for e in ([0] * n, [7] * n, [Q - 1] * n, single):
                got = dom.open_evals([e], z)
                assert got == expected([e], z, 1, log_n), (m, z)
                if len(set(e)) == 1:
                    assert got[2] == ID48 and got[0] == [e[0]]          # a constant: the quotient is zero
                if e[0] == 0 and len(set(e)) == 1:
                    assert got[1] == [ID48]
    # the four together, folded
    v = rnd.randrange(Q)
    vs = [[0] * n, [7] * n, [Q - 1] * n, single]
    assert dom.open_evals(vs, pts[n - 1], v) == expected(vs, pts[n - 1], v, log_n)


def test_evaluate_only_runs_no_msm_and_builds_no_points(ctx):
    import plonk_amd
    dom = plonk_amd.KzgDomain(ctx, 7)
    rnd = random.Random(7)
    e = [[rnd.randrange(Q) for _ in range(128)] for _ in range(2)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    assert dom.evals_last()["count"] == 0 and dom.evals_last()["lagrange_bytes"] == 0
    before = dom.last()
    ev, cm, wit = dom.open_evals(e, z, v, commitments=False, witness=False)
    assert (ev, cm, wit) == (expected(e, z, v, 7)[0], None, None)
    last = assert_last(dom, 2, NONE, False, False, True, built=0)
    assert (last["msm_launches"], last["lagrange_bytes"]) == (0, 0)
    assert dom.open_evals(e, z, v) == expected(e, z, v, 7)
    assert assert_last(dom, 2, NONE, True, True, True, built=1)["msm_launches"] == 3
    assert dom.commit_evals(e) == expected(e, z, v, 7)[1]
    assert_last(dom, 2, NONE, True, False, True, built=0)
    assert dom.last() == before                                  # plonk_kzg_domain_last does not see these calls
    dom.close()


def test_point_equal_to_tau_against_plonk_kzg_open(ctx, domains):
    """the closed form's denominator is zero there; the coefficient route has no such problem"""
    dom, n = domains(6), 64
    rnd = random.Random(66)
    vectors = [[rnd.randrange(Q) for _ in range(n)] for _ in range(2)]
    v = rnd.randrange(Q)
    coeffs = [ctx.ntt(e, 6, inverse=True) for e in vectors]
    assert dom.open_evals(vectors, K.TAU, v) == ctx.kzg_open(coeffs, K.TAU, v)


# ---- byte identity with the coefficient route ------------------------------------------------------------------------------------
def random_raw(rnd, n):
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    return bytes(raw)


def test_4096_points_count_2_equals_the_coefficient_route(ctx, domains, key):
    import plonk_amd as P
    log_n, n = 12, 1 << 12
    dom = domains(log_n)
    rnd = random.Random(12)
    raws = [random_raw(rnd, n) for _ in range(2)]
    coeff_raws = [ctx.ntt_bytes(r, log_n, True, False, n) for r in raws]
    v = rnd.randrange(Q)
    pts = M.domain_points(log_n)
    m = 256
    folded = None
    for z in (rnd.randrange(Q), 0, pts[m]):
        got = dom.open_evals(raws, z, v)
        assert got == ctx.kzg_open(coeff_raws, z, v), z
        proof = ctx.kzg_flatten(got[1], got[0], v, got[2])
        assert key.check_each([z], [proof]) == [OK]
        bad = P.KzgProof.make(bytes(proof.commitment), (proof.value + 1) % Q, bytes(proof.witness))
        assert key.check_each([z], [bad]) != [OK]
    assert_last(dom, 2, m, True, True, True)
    vectors = [P.fr_from_bytes_mont(r) for r in raws]
    assert got[0] == [vectors[0][m], vectors[1][m]]
    # the witness at w^m is witness m of the whole-domain opening of the folded polynomial
    cs = [P.fr_from_bytes_mont(r) for r in coeff_raws]
    folded = [(a + v * b) % Q for a, b in zip(*cs)]
    ev, wit, cm = dom.open([folded], commitments=False)
    assert wit[0][m] == got[2]
    assert got == expected(vectors, pts[m], v, log_n)


def test_65536_points_count_2_sampled():
    import plonk_amd as P
    log_n, n = 16, 1 << 16
    c = P.Context(0)
    load_key(c, n)                                              # exactly n points
    k = P.KzgKey(c, K.opening_key())
    dom = P.KzgDomain(c, log_n)
    rnd = random.Random(16)
    raws = [random_raw(rnd, n) for _ in range(2)]
    vectors = [P.fr_from_bytes_mont(r) for r in raws]
    v = rnd.randrange(Q)
    m = n - 300
    for z in (rnd.randrange(Q), M.domain_points(log_n)[m]):
        got = dom.open_evals(raws, z, v)
        assert got == expected(vectors, z, v, log_n)
        assert k.check_each([z], [c.kzg_flatten(got[1], got[0], v, got[2])]) == [OK]
    assert_last(dom, 2, m, True, True, True, built=0)
    dom.close()
    k.close()
    c.close()


# ---- the resident form ---------------------------------------------------------------------------------------------------
def test_resident_form_gives_the_bytes_of_the_host_form(ctx, domains):
    import plonk_amd as P
    dom, n = domains(6), 64
    rnd = random.Random(606)
    count = 5
    raws = [random_raw(rnd, n) for _ in range(count)]
    bufs = []
    for r in raws:
        b = ctx.alloc(32 * n)
        b.upload(r)
        bufs.append(b)
    ptrs = [b.ptr for b in bufs]
    v = rnd.randrange(Q)
    for z in (rnd.randrange(Q), M.domain_points(6)[63]):
        assert dom.open_evals_dev(ptrs, z, v) == dom.open_evals(raws, z, v)
        assert dom.open_evals_dev(ptrs[:1], z) == dom.open_evals(raws[:1], z)
    dom.open_evals_dev(ptrs, 0, v)
    assert_last(dom, count, NONE, True, True, False)
    assert dom.commit_evals_dev(ptrs) == dom.commit_evals(raws)
    for b in bufs:
        assert b.download() == raws[bufs.index(b)]               # the inputs are only read
        b.free()


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(ctx, domains):
    import plonk_amd as P
    dom, n = domains(3), 8
    lib = ctx.lib
    mont = P.fr_to_bytes_mont
    good, noncanon = mont(range(1, 9)), mont([1, 2]) + b"\xff" * 32 + mont([4, 5, 6, 7, 8])
    ev = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    cm = ctypes.create_string_buffer(b"\xA5" * 96, 96)
    wit = ctypes.create_string_buffer(b"\xA5" * 48, 48)
    point, v = mont([5]), mont([6])

    def table(bufs):
        keep = [ctypes.create_string_buffer(b, len(b)) if b is not None else None for b in bufs]
        arr = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.cast(k, ctypes.c_void_p).value if k is not None else None for k in keep])
        return keep, arr

    def open_(bufs, count=None, h=dom.handle, p=point, vv=v, e=ev, arr=None, fn=lib.plonk_kzg_open_evals):
        keep, a = table(bufs)
        return fn(h, a if arr is None else arr, len(bufs) if count is None else count, p, vv, e, cm, wit)

    def commit(bufs, count=None, h=dom.handle, out=cm, fn=lib.plonk_kzg_commit_evals):
        keep, a = table(bufs)
        return fn(h, a, len(bufs) if count is None else count, out)

    assert open_([good], h=None) == ERR_ARG
    assert open_([good], p=None) == ERR_ARG
    assert open_([good], e=None) == ERR_ARG
    assert open_([good, None]) == ERR_ARG
    assert open_([good, good], vv=None) == ERR_ARG               # count > 1 needs the challenge
    assert open_([good], count=65537) == ERR_ARG
    assert lib.plonk_kzg_open_evals(dom.handle, None, 1, point, v, ev, cm, wit) == ERR_ARG
    assert open_([good, noncanon]) == ERR_DATA
    assert open_([good], p=b"\xff" * 32) == ERR_DATA
    assert open_([good, good], vv=b"\xff" * 32) == ERR_DATA
    assert commit([good], h=None) == ERR_ARG
    assert commit([good], out=None) == ERR_ARG
    assert commit([good], count=65537) == ERR_ARG
    assert commit([good, noncanon]) == ERR_DATA
    # the resident form finds the value on the device
    bufs = [ctx.alloc(32 * n), ctx.alloc(32 * n)]
    bufs[0].upload(good)
    bufs[1].upload(noncanon)
    arr = (ctypes.c_void_p * 2)(bufs[0].ptr, bufs[1].ptr)
    assert lib.plonk_kzg_open_evals_dev(dom.handle, arr, 2, point, v, ev, cm, wit) == ERR_DATA
    assert lib.plonk_kzg_commit_evals_dev(dom.handle, arr, 2, cm) == ERR_DATA
    assert lib.plonk_kzg_open_evals_dev(dom.handle, arr, 2, point, None, ev, cm, wit) == ERR_ARG
    assert ev.raw == b"\xA5" * 64 and cm.raw == b"\xA5" * 96 and wit.raw == b"\xA5" * 48
    assert lib.plonk_kzg_evals_last(dom.handle, None) == ERR_ARG
    assert lib.plonk_kzg_evals_last(None, ctypes.byref(P._KzgEvalsInfo())) == ERR_ARG
    # and the same buffers take a good call
    assert lib.plonk_kzg_open_evals_dev(dom.handle, arr, 1, point, None, ev, cm, wit) == OK
    want = expected([list(range(1, 9))], 5, 1, 3)
    assert ev.raw[:32] == mont(want[0]) and cm.raw[:48] == want[1][0] and wit.raw == want[2]
    assert ev.raw[32:] == b"\xA5" * 32 and cm.raw[48:] == b"\xA5" * 48
    for b in bufs:
        b.free()


def test_state_error_after_the_key_is_reloaded():
    import plonk_amd as P
    c = P.Context(0)
    load_key(c, 16)
    d = P.KzgDomain(c, 3)
    e = [[1, 2, 3, 4, 5, 6, 7, 8]]
    before = d.open_evals(e, 9)
    load_key(c, 16)                                             # the same key again: still another generation
    for call in (lambda: d.open_evals(e, 9), lambda: d.commit_evals(e), d.evals_last, lambda: d.open_evals([], 9)):
        with pytest.raises(P.PlonkError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    d.close()
    d2 = P.KzgDomain(c, 3)
    assert d2.open_evals(e, 9) == before == expected(e, 9, 1, 3)
    d2.close()
    c.close()


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def test_a_key_of_exactly_n_points():
    import plonk_amd as P
    c = P.Context(0)
    load_key(c, 8)
    d = P.KzgDomain(c, 3)
    rnd = random.Random(8)
    e = [[rnd.randrange(Q) for _ in range(8)] for _ in range(2)]
    for z in (rnd.randrange(Q), M.domain_points(3)[5]):
        assert d.open_evals(e, z, 3) == expected(e, z, 3, 3)
    assert d.commit_evals(e) == [P.g1_compress(c.commit(c.ntt(x, 3, inverse=True))) for x in e]
    d.close()
    c.close()


@pytest.mark.parametrize("log_n", [3, 4])
def test_degenerate_key(log_n):
    """tau = (2n-th root of unity)^3: the key's points repeat with period 2n and tau^n = -1, so the group transform meets
    equal and opposite points; tau is not a domain point, so the closed form still holds"""
    import plonk_amd as P
    n = 1 << log_n
    tau = pow(M.root(log_n + 1), 3, Q)
    assert pow(tau, n, Q) == Q - 1 and tau not in M.domain_points(log_n)
    c = P.Context(0)
    load_key(c, n, tau)
    dom = P.KzgDomain(c, log_n)
    rnd = random.Random(log_n)
    e = [[rnd.randrange(Q) for _ in range(n)], [1] * n, [0] * (n - 1) + [1]]
    v = rnd.randrange(Q)
    for z in (rnd.randrange(Q), M.domain_points(log_n)[n - 1], 0):
        assert dom.open_evals(e, z, v) == expected(e, z, v, log_n, tau)
    dom.close()
    c.close()


# ---- the context is left as it was found -----------------------------------------------------------------------------------
def test_context_left_as_found():
    """a proof, an opening and a plonk_msm_points report made on the same context before and after evaluation-form calls are
    identical; the tables stay; plonk_kzg_domain_last is unchanged"""
    import plonk_amd as P
    from tests import circuits as C
    c = P.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=78)()
    case = C.compile_fast(comp, b"kzg-evals")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = P.Prover.compile(c, b"kzg-evals", cols["selectors"], cols["wires"], cols["witnesses"])
    rnd = random.Random(77)
    f = [rnd.randrange(Q) for _ in range(300)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    proof = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    assert len(proof) == 1008
    opening = c.kzg_open([f, f[:7]], z, v)
    pts = [E.g1_mul(E.G1_GEN, 3), E.g1_mul(E.G1_GEN, 5)]
    c.msm_points(pts, [2, 9])
    points_report = c.last_msm_points()
    dom = P.KzgDomain(c, 6)
    dom.open([[1, 2, 3]])
    domain_report = dom.last()
    tables, rows = c.table_bytes(), c.table_rows()
    e = [[rnd.randrange(Q) for _ in range(64)] for _ in range(3)]
    for zz in (z, M.domain_points(6)[9]):
        assert dom.open_evals(e, zz, v) == expected(e, zz, v, 6)
    assert dom.commit_evals(e) == expected(e, z, v, 6)[1]
    assert prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3)) == proof
    assert c.kzg_open([f, f[:7]], z, v) == opening
    assert (c.table_bytes(), c.table_rows()) == (tables, rows)
    assert c.last_msm_points() == points_report
    assert dom.last() == domain_report
    dom.close()
    prover.close()
    c.close()
