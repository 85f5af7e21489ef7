"""GPU: KZG10 openings over a whole domain (plonk_kzg_domain_create / _points / plonk_kzg_open_domain / _dev / _last;
plonk_amd/csrc/kzg_domain.hip) against the closed form of tests/kzg_ref.py.  The commit key is the suite's synthetic known-tau
key, so witness i of f is [g (f(tau) - f(w^i)) / (tau - w^i)] G and exists as bytes at every size; evaluations are Horner
values (the C oracle's NTT at 2^12).  Every comparison is exact.  At n <= 8 each opening is also compared with plonk_kzg_open at
that point, and at 2^8 and 2^12 ALL openings go through plonk_kzg_check_each with the handle's own points."""
import ctypes
import random

import pytest

from oracle import bls12_381 as E
from oracle import cbind
from tests import kzg_domain_model as M
from tests import kzg_ref as K

pytestmark = pytest.mark.gpu
Q = E.Q
OK, ERR_ARG, ERR_DEGREE, ERR_NO_SRS, ERR_STATE, ERR_DATA, ERR_VERIFY = 0, -1, -3, -4, -7, -9, -12
ID48 = K.IDENTITY48
KEY_POINTS = (1 << 12) + 3


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


def witness48(f, z, tau=K.TAU):
    return K.scalar_commit(K.witness_scalar([f], z, 1, tau))


def check_all(dom, polys, tau=K.TAU, indices=None):
    """every (or the listed) evaluation and witness of every polynomial against the closed form, the commitments too"""
    ev, wit, cm = dom.open(polys)
    pts = M.domain_points(dom.log_n)
    for j, f in enumerate(polys):
        assert cm[j] == K.commit(f, tau), j
        for i in (range(dom.n) if indices is None else indices):
            assert ev[j][i] == K.evaluate(f, pts[i]), (j, i)
            assert wit[j][i] == witness48(f, pts[i], tau), (j, i)
    return ev, wit, cm


def assert_last(dom, count, cap=M.WS_CAP_DEFAULT):
    last, p = dom.last(), M.plan(dom.log_n, count, cap)
    assert (last["log_n"], last["count"], last["workspace_cap_bytes"]) == (dom.log_n, count, cap)
    assert (last["chunks"], last["chunk_polys"], last["stage_launches"], last["scalar_muls"]) == \
        (p["chunks"], p["chunk_polys"], p["stage_launches"], p["scalar_muls"])
    n = dom.n
    assert last["device_bytes"] >= 2 * n * 256 + n * 32 + p["ws_bytes"]
    return last


# ---- facts about the inputs -----------------------------------------------------------------------------------------------
def test_points_are_the_domain_plonk_ntt_uses(ctx, domains):
    for log_n in (1, 3, 8):
        dom = domains(log_n)
        pts = dom.points()
        assert pts == M.domain_points(log_n)
        rnd = random.Random(log_n)
        f = [rnd.randrange(Q) for _ in range(dom.n)]
        assert ctx.ntt(f, log_n) == [K.evaluate(f, z) for z in pts]
    assert dom.last()["count"] == 0 and dom.last()["device_bytes"] >= 2 * 256 * 256 + 256 * 32


# ---- small sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 3, 6])
def test_small_sizes_every_witness_and_evaluation(ctx, domains, log_n):
    import plonk_amd
    dom, n = domains(log_n), 1 << log_n
    rnd = random.Random(log_n)
    lengths = sorted({0, 1, 2, n - 1, n})
    polys = [[rnd.randrange(1, Q) for _ in range(m)] for m in lengths]
    ev, wit, cm = check_all(dom, polys)
    assert_last(dom, len(polys))
    for j, m in enumerate(lengths):
        if m <= 1:
            assert wit[j] == [ID48] * n                       # zero and constant polynomials: n identities
    assert cm[0] == ID48 and ev[0] == [0] * n
    if n <= 8:
        pts = dom.points()
        for j, f in enumerate(polys):
            assert cm[j] == plonk_amd.g1_compress(ctx.commit(f))
            for i, z in enumerate(pts):
                e1, c1, w1 = ctx.kzg_open([f], z, None)
                assert (e1[0], c1[0], w1) == (ev[j][i], cm[j], wit[j][i]), (j, i)
    # without the commitments
    ev2, wit2, cm2 = dom.open(polys, commitments=False)
    assert (ev2, wit2, cm2) == (ev, wit, None)


@pytest.mark.parametrize("log_n", [2, 3, 6])
def test_shaped_polynomials(domains, log_n):
    dom, n = domains(log_n), 1 << log_n
    polys = [[0] * (n - 1) + [1],                             # X^(n-1) alone
             [Q - 1, 1],                                      # X - 1: evaluation 0 at w^0
             [0] * (n - 3) + [Q - 1, 0, 1],                   # X^(n-1) - X^(n-3): G_0 = G_n = 0, identities enter the inverse transform
             [5, 7] + [0] * (n - 2),                          # trailing zeros
             [Q - 1] * n]                                     # the coefficient q - 1
    ev, wit, cm = check_all(dom, polys)
    assert ev[1][0] == 0
    import plonk_amd
    padded = dom.open_bytes([plonk_amd.fr_to_bytes_mont([5, 7] + [0] * (3 * n))])       # longer than n, trimmed length 2
    assert padded[1] == b"".join(wit[3]) and padded[2] == cm[3]


@pytest.mark.parametrize("log_n", [3, 4])
def test_degenerate_key(log_n):
    """tau = (2n-th root of unity)^3: the key's points repeat with period 2n and tau^n = -1, so the transforms meet equal and
    opposite points; tau is not a domain point, so the closed form still holds"""
    import plonk_amd
    n = 1 << log_n
    tau = pow(M.root(log_n + 1), 3, Q)
    assert pow(tau, n, Q) == Q - 1 and tau not in M.domain_points(log_n)
    c = plonk_amd.Context(0)
    load_key(c, n, tau)
    dom = plonk_amd.KzgDomain(c, log_n)
    rnd = random.Random(log_n)
    polys = [[rnd.randrange(Q) for _ in range(n)], [1] * n, [0] * (n - 1) + [1], [3, 1]]
    check_all(dom, polys, tau)
    dom.close()
    c.close()


# ---- n = 256 --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def polys256():
    rnd = random.Random(256)
    lens = [256, 255, 1, 200, 0, 256, 17, 2, 129, 128, 256, 64, 3, 250, 256, 100, 256]
    return [[rnd.randrange(1, Q) for _ in range(m)] for m in lens]


@pytest.mark.parametrize("count", [1, 3, 17])
def test_256_points_sampled_witnesses_and_every_opening_through_check_each(domains, key, polys256, count):
    import plonk_amd
    dom, n = domains(8), 256
    polys = polys256[:count]
    ev, wit, cm = dom.open(polys)
    assert_last(dom, count)
    pts = dom.points()
    sample = [0, 1, n // 2, n - 1] + random.Random(count).sample(range(2, n - 1), 12)
    for j, f in enumerate(polys):
        assert cm[j] == K.commit(f)
        assert ev[j] == [K.evaluate(f, z) for z in pts]
        for i in (range(n) if j == 0 and count == 3 else sample):         # all 256 witnesses of one polynomial, once
            assert wit[j][i] == witness48(f, pts[i]), (j, i)
    proofs = [plonk_amd.KzgProof.make(cm[j], ev[j][i], wit[j][i]) for j in range(count) for i in range(n)]
    assert key.check_each(pts * count, proofs) == [OK] * (count * n)
    # corrupting one evaluation flips exactly that verdict
    bad = (count - 1) * n + 77
    proofs[bad] = plonk_amd.KzgProof.make(cm[count - 1], (ev[count - 1][77] + 1) % Q, wit[count - 1][77])
    assert key.check_each(pts * count, proofs) == [OK] * bad + [ERR_VERIFY] + [OK] * (count * n - bad - 1)


# ---- n = 2^12 -------------------------------------------------------------------------------------------------------------
def test_4096_points_count_2(domains, key):
    import plonk_amd
    dom, n = domains(12), 1 << 12
    rnd = random.Random(12)
    raws = []
    for m in (n, n - 5):
        raw = bytearray(rnd.randbytes(32 * m))
        for i in range(31, 32 * m, 32):
            raw[i] &= 0x3F
        raws.append(bytes(raw))
    polys = [plonk_amd.fr_from_bytes_mont(r) for r in raws]
    ev, wit, cm = dom.open_bytes(raws)
    assert_last(dom, 2)
    for j in range(2):
        assert ev[32 * n * j:32 * n * (j + 1)] == cbind.ntt_bytes(raws[j], 12, False, False, len(polys[j]))
        assert cm[48 * j:48 * j + 48] == K.commit(polys[j])
    pts = dom.points()
    evs = plonk_amd.fr_from_bytes_mont(ev)
    for j in range(2):
        ft = K.evaluate(polys[j], K.TAU)
        for i in [0, 1, n // 2, n - 1] + rnd.sample(range(2, n - 1), 12):
            want = K.scalar_commit((ft - evs[j * n + i]) * pow((K.TAU - pts[i]) % Q, -1, Q) % Q)
            assert wit[48 * (j * n + i):48 * (j * n + i + 1)] == want, (j, i)
    proofs = [plonk_amd.KzgProof.make(cm[48 * j:48 * j + 48], evs[j * n + i], wit[48 * (j * n + i):48 * (j * n + i + 1)])
              for j in range(2) for i in range(n)]
    assert key.check_each(pts * 2, proofs) == [OK] * (2 * n)


def test_65536_points_count_2_sampled():
    """2^16: 1024 workgroups per stage and polynomial; the commitments, sampled evaluations and witnesses by closed form and
    the sampled openings through plonk_kzg_check_each (the whole range 2^17..2^20 of log_n runs the same code: 2^20 was
    checked this way once)"""
    import plonk_amd
    log_n, n = 16, 1 << 16
    c = plonk_amd.Context(0)
    load_key(c, n)
    k = plonk_amd.KzgKey(c, K.opening_key())
    dom = plonk_amd.KzgDomain(c, log_n)
    rnd = random.Random(16)
    raws = []
    for m in (n, n // 2 + 1):
        raw = bytearray(rnd.randbytes(32 * m))
        for i in range(31, 32 * m, 32):
            raw[i] &= 0x3F
        raws.append(bytes(raw))
    ev, wit, cm = dom.open_bytes(raws)
    assert_last(dom, 2)
    w = M.root(log_n)
    idx = [0, 1, n // 2, n - 1] + rnd.sample(range(2, n - 1), 12)
    zs = [pow(w, i, Q) for i in idx]
    points, proofs = [], []
    for j, raw in enumerate(raws):
        f = plonk_amd.fr_from_bytes_mont(raw)
        ft = K.evaluate(f, K.TAU)
        assert cm[48 * j:48 * j + 48] == K.scalar_commit(ft)
        for t, i in enumerate(idx):
            at = j * n + i
            e = plonk_amd.fr_from_bytes_mont(ev[32 * at:32 * at + 32])[0]
            if t < 4:
                assert e == K.evaluate(f, zs[t]), (j, i)
                assert wit[48 * at:48 * at + 48] == K.scalar_commit((ft - e) * pow((K.TAU - zs[t]) % Q, -1, Q) % Q), (j, i)
            points.append(zs[t])
            proofs.append(plonk_amd.KzgProof.make(cm[48 * j:48 * j + 48], e, wit[48 * at:48 * at + 48]))
    assert k.check_each(points, proofs) == [OK] * len(proofs)
    dom.close()
    k.close()
    c.close()


# ---- chunking, the resident form ------------------------------------------------------------------------------------------
def test_forced_chunking_gives_the_same_bytes(domains):
    """the handle's test-only cap setter (KzgDomain._set_workspace_cap -> plonk_test_kzg_domain_set_cap): room for two
    polynomials of n = 64, so five run as three chunks"""
    import plonk_amd
    dom, n = domains(6), 64
    rnd = random.Random(6)
    raws = [plonk_amd.fr_to_bytes_mont([rnd.randrange(Q) for _ in range(m)]) for m in (64, 10, 0, 63, 64)]
    whole = dom.open_bytes(raws)
    assert_last(dom, 5)
    assert dom.last()["chunks"] == 1
    cap = 2 * (2 * n * 256)
    dom._set_workspace_cap(cap)
    try:
        assert dom.open_bytes(raws) == whole
        last = assert_last(dom, 5, cap)
        assert (last["chunks"], last["chunk_polys"]) == (3, 2)
        dom._set_workspace_cap(1)                              # below one polynomial: a one-polynomial chunk is always allowed
        assert dom.open_bytes(raws) == whole
        assert assert_last(dom, 5, 1)["chunks"] == 5
    finally:
        dom._set_workspace_cap(0)
    assert dom.last()["workspace_cap_bytes"] == M.WS_CAP_DEFAULT


def test_resident_form_gives_the_bytes_of_the_host_form(ctx, domains):
    import plonk_amd
    dom, n = domains(6), 64
    rnd = random.Random(66)
    lens = [64, 0, 5, 64, 1]
    raws = [plonk_amd.fr_to_bytes_mont([rnd.randrange(Q) for _ in range(m)]) for m in lens]
    raws[2] += bytes(32 * 100)                                  # trailing zeros beyond n: trimmed length 5
    whole = dom.open_bytes(raws)
    bufs = []
    for r in raws:
        b = ctx.alloc(max(len(r), 32))
        b.upload(r)
        bufs.append(b)
    count = len(raws)
    ev, wit, cm = ctx.alloc(32 * n * count), ctx.alloc(48 * n * count), ctx.alloc(48 * count)
    dom.open_dev([b.ptr for b in bufs], [len(r) // 32 for r in raws], ev.ptr, wit.ptr, cm.ptr)
    assert (ev.download(), wit.download(), cm.download()) == whole
    assert_last(dom, count)
    wit.upload(b"\xA5" * wit.nbytes)
    dom.open_dev([b.ptr for b in bufs], [len(r) // 32 for r in raws], ev.ptr, wit.ptr, None)
    assert wit.download() == whole[1]
    # errors of the resident form leave the outputs untouched
    ev.upload(b"\xA5" * ev.nbytes)
    wit.upload(b"\xA5" * wit.nbytes)
    bad = ctx.alloc(32 * 65)
    bad.upload(plonk_amd.fr_to_bytes_mont([1] * 65))
    with pytest.raises(plonk_amd.PolynomialDegreeTooLarge):
        dom.open_dev([bufs[0].ptr, bad.ptr], [64, 65], ev.ptr, wit.ptr, None)
    bad.upload(b"\xff" * 32, offset=32 * 3)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        dom.open_dev([bufs[0].ptr, bad.ptr], [64, 64], ev.ptr, wit.ptr, None)
    assert ei.value.code == ERR_DATA
    assert ev.download() == b"\xA5" * ev.nbytes and wit.download() == b"\xA5" * wit.nbytes
    for b in bufs + [ev, wit, cm, bad]:
        b.free()


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors_of_create(ctx):
    import plonk_amd
    lib = ctx.lib
    h = ctypes.c_void_p()
    for log_n in (0, 21, 32):
        assert lib.plonk_kzg_domain_create(ctx.handle, log_n, ctypes.byref(h)) == ERR_ARG and not h.value
    assert lib.plonk_kzg_domain_create(None, 3, ctypes.byref(h)) == ERR_ARG
    assert lib.plonk_kzg_domain_create(ctx.handle, 3, None) == ERR_ARG
    assert lib.plonk_kzg_domain_create(ctx.handle, 13, ctypes.byref(h)) == ERR_DEGREE and not h.value     # the key holds 2^12 + 3 points
    fresh = plonk_amd.Context(0)
    assert lib.plonk_kzg_domain_create(fresh.handle, 3, ctypes.byref(h)) == ERR_NO_SRS
    load_key(fresh, 8)
    assert lib.plonk_kzg_domain_create(fresh.handle, 4, ctypes.byref(h)) == ERR_DEGREE
    d = plonk_amd.KzgDomain(fresh, 3)                           # exactly n points are enough
    check_all(d, [[1, 2, 3, 4, 5, 6, 7, 8]])
    d.close()
    fresh.close()


def test_a_context_with_a_communicator_is_refused():
    import plonk_amd
    fresh = plonk_amd.Context(0)
    load_key(fresh, 8)
    lib, h = fresh.lib, ctypes.c_void_p()
    d = plonk_amd.KzgDomain(fresh, 3)
    fresh.comm_init(plonk_amd.Context.comm_unique_id(), 0, 1)   # a communicator: the context holds only a range of the key
    assert lib.plonk_kzg_domain_create(fresh.handle, 3, ctypes.byref(h)) == ERR_STATE
    with pytest.raises(plonk_amd.PlonkError) as ei:
        d.open([[1, 2]])
    assert ei.value.code == ERR_STATE
    fresh.comm_destroy()
    check_all(d, [[1, 2]])
    d.close()
    fresh.close()


def test_errors_of_open_leave_the_outputs_untouched(ctx, domains):
    import plonk_amd
    dom, n = domains(3), 8
    lib = ctx.lib
    mont = plonk_amd.fr_to_bytes_mont
    good, long_, noncanon = mont([1] * 8), mont([1] * 9), mont([1, 2]) + b"\xff" * 32 + mont([3])
    ev = ctypes.create_string_buffer(b"\xA5" * (32 * n * 2), 32 * n * 2)
    wit = ctypes.create_string_buffer(b"\xA5" * (48 * n * 2), 48 * n * 2)
    cm = ctypes.create_string_buffer(b"\xA5" * 96, 96)

    def call(bufs, count=None, h=dom.handle, e=ev, w=wit):
        keep = [ctypes.create_string_buffer(b, len(b)) for b in bufs]
        parr = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.cast(k, ctypes.c_void_p).value for k in keep])
        larr = (ctypes.c_uint64 * max(len(bufs), 1))(*[len(b) // 32 for b in bufs])
        return lib.plonk_kzg_open_domain(h, parr, larr, len(bufs) if count is None else count, e, w, cm)

    assert call([good, long_]) == ERR_DEGREE
    assert call([good, noncanon]) == ERR_DATA
    assert call([good], count=65537) == ERR_ARG
    assert call([good], h=None) == ERR_ARG
    assert call([good], e=None) == ERR_ARG
    assert call([good], w=None) == ERR_ARG
    assert call([], count=0) == OK                              # count == 0 writes nothing
    assert ev.raw == b"\xA5" * len(ev.raw) and wit.raw == b"\xA5" * len(wit.raw) and cm.raw == b"\xA5" * 96
    assert lib.plonk_kzg_domain_points(dom.handle, None) == ERR_ARG and lib.plonk_kzg_domain_last(dom.handle, None) == ERR_ARG
    assert lib.plonk_kzg_domain_points(None, ev) == ERR_ARG
    assert lib.plonk_kzg_domain_last(None, ctypes.byref(plonk_amd._KzgDomainInfo())) == ERR_ARG
    assert call([good, mont([0] * 20)]) == OK                   # twenty zeros trim to the zero polynomial
    assert wit.raw[48 * n:] == ID48 * n and cm.raw[48:] == ID48


def test_state_error_after_the_key_is_reloaded():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, 16)
    d = plonk_amd.KzgDomain(c, 3)
    before = d.open([[1, 2, 3]])
    load_key(c, 16)                                             # the same key again: still another generation
    for call in (lambda: d.open([[1, 2, 3]]), d.points, d.last, lambda: d.open([])):
        with pytest.raises(plonk_amd.PlonkError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    d.close()
    d2 = plonk_amd.KzgDomain(c, 3)
    assert d2.open([[1, 2, 3]]) == before
    d2.close()
    c.close()


# ---- the context is left as it was found -----------------------------------------------------------------------------------
def test_context_left_as_found():
    """a proof and an opening made on the same context before and after a domain call are byte-identical; the tables stay"""
    import plonk_amd
    from tests import circuits as C
    c = plonk_amd.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=78)()
    case = C.compile_fast(comp, b"kzg-domain")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = plonk_amd.Prover.compile(c, b"kzg-domain", cols["selectors"], cols["wires"], cols["witnesses"])
    rnd = random.Random(77)
    f = [rnd.randrange(Q) for _ in range(300)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    proof = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    opening = c.kzg_open([f, f[:7]], z, v)
    tables, rows = c.table_bytes(), c.table_rows()
    dom = plonk_amd.KzgDomain(c, 6)
    check_all(dom, [[rnd.randrange(Q) for _ in range(64)], [4, 5, 6]], indices=[0, 1, 32, 63])
    assert prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3)) == proof
    assert c.kzg_open([f, f[:7]], z, v) == opening
    assert (c.table_bytes(), c.table_rows()) == (tables, rows)
    dom.close()
    prover.close()
    c.close()
