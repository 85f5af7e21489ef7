"""GPU: the KZG10 opening layer (plonk_kzg_open / _open_dev / _flatten / _key_create / _batch_check, plonk_srs_check;
plonk_amd/csrc/kzg.hip and the fold / evaluate kernels of poly.hip) against the plain-Python yardstick tests/kzg_ref.py.
The commit key is the suite's synthetic known-tau key and the opening key is built from the same tau, so the expected
evaluations, commitments and witnesses exist as bytes at every size; all comparisons are exact."""
import ctypes
import random

import pytest

from oracle import bls12_381 as E
from oracle.merlin import Transcript
from tests import circuits as C
from tests import kzg_ref as K

pytestmark = pytest.mark.gpu
Q = E.Q
OK, ERR_ARG, ERR_DEGREE, ERR_NO_SRS, ERR_STATE, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -3, -4, -7, -9, -10, -12
BIG = (1 << 20) + 7        # points of the large key
ID48 = K.IDENTITY48


def rand_poly(rnd, n):
    """n coefficients: (ints, Montgomery bytes) — the bytes are drawn, the ints derived, so 2^20 coefficients stay cheap"""
    import plonk_amd
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F                      # < 2^254 < q: canonical limbs
    return plonk_amd.fr_from_bytes_mont(bytes(raw)), bytes(raw)


def load_big_key(ctx, n=BIG):
    buf = ctx.alloc(96 * n)
    ctx.srs_generate_dev(K.TAU, K.G_SCALAR, n, buf.ptr)
    ctx.srs_load_dev(buf.ptr, n)
    ctx.sync()
    buf.free()


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_big_key(c)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key(ctx):
    import plonk_amd
    k = plonk_amd.KzgKey(ctx, K.opening_key())
    yield k
    k.close()


def check_open(ctx, polys_int, polys_bytes, z, v, commitments=True):
    ev, cm, wit = ctx.kzg_open(polys_bytes, z, v, commitments=commitments)
    e_ev, e_cm, e_wit = K.open_expected(polys_int, z, 1 if v is None else v)
    assert ev == e_ev
    if commitments:
        assert cm == e_cm
    else:
        assert cm is None
    assert wit == e_wit
    return ev, cm, wit


# ---- facts about the inputs: a silent yardstick must not pass -------------------------------------------------------
def test_yardstick_commitments_equal_context_commit_and_its_witness_satisfies_the_pairing_equation(ctx):
    import plonk_amd
    rnd = random.Random(11)
    p = [rnd.randrange(Q) for _ in range(5)]
    assert K.commit(p) == plonk_amd.g1_compress(ctx.commit(p)) != ID48
    assert K.commit([0, 0]) == ID48
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    polys = [p, [rnd.randrange(Q) for _ in range(3)]]
    evals, comms, wit = K.open_expected(polys, z, v)
    # the MSM over the explicit key agrees with the closed form of the witness
    q = K.ruffini(K.fold(polys, v), z)
    assert plonk_amd.g1_compress(ctx.commit(q)) == wit
    # e(C - [e] g, h) == e(W, x_h - [z] h) for the flattened proof, through the suite's own pairing
    flat = K.flatten(comms, evals, v, wit)
    assert K.batch_check([z], [flat], u=1)
    bad = (flat[0], (flat[1] + 1) % Q, flat[2])
    assert not K.batch_check([z], [bad], u=1)


# ---- open -------------------------------------------------------------------------------------------------------------
SMALL = [1, 2, 5, 1024, 1025]


@pytest.mark.parametrize("count", [1, 3, 15, 40])
def test_open_small_lengths_every_count(ctx, count):
    rnd = random.Random(100 + count)
    for n in SMALL:
        polys = [rand_poly(rnd, n) for _ in range(count)]
        check_open(ctx, [p[0] for p in polys], [p[1] for p in polys], rnd.randrange(Q), rnd.randrange(Q) if count > 1 else None)


@pytest.mark.parametrize("n,count", [((1 << 16) + 3, 1), ((1 << 16) + 3, 3), ((1 << 16) + 3, 15), ((1 << 16) + 3, 40),
                                     (1 << 20, 1), (1 << 20, 3), (1 << 20, 15)])
def test_open_large(ctx, n, count):
    """evaluations, EVERY commitment and the witness at the large lengths, through the host form and the resident form: at
    (2^20, 15) that is four grouped commitment launches of 2^20-term sets in a row, per form"""
    rnd = random.Random(n + count)
    polys = [rand_poly(rnd, n) for _ in range(count)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    staged = check_open(ctx, [p[0] for p in polys], [p[1] for p in polys], z, v)
    bufs = []
    for _, raw in polys:
        b = ctx.alloc(len(raw))
        b.upload(raw)
        bufs.append(b)
    assert ctx.kzg_open_dev([b.ptr for b in bufs], [n] * count, z, v) == staged
    for b in bufs:
        b.free()


def test_open_2p20_count_40(ctx):
    """40 crosses both existing term caps (poly_lincomb 24, poly_eval 16) at the flagship length, with all 40 commitments,
    resident and staged.  Four distinct polynomials, each used ten times, keep the yardstick cheap."""
    rnd = random.Random(40)
    n, count = 1 << 20, 40
    base = [rand_poly(rnd, n) for _ in range(4)]
    bufs = []
    for ints, raw in base:
        b = ctx.alloc(len(raw))
        b.upload(raw)
        bufs.append(b)
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    base_ev = [K.evaluate(p[0], z) for p in base]
    base_tau = [K.evaluate(p[0], K.TAU) for p in base]
    base_cm = [K.scalar_commit(t) for t in base_tau]
    ft = sum(pow(v, i, Q) * base_tau[i % 4] for i in range(count)) % Q
    fz = sum(pow(v, i, Q) * base_ev[i % 4] for i in range(count)) % Q
    expected = ([base_ev[i % 4] for i in range(count)], [base_cm[i % 4] for i in range(count)],
                K.scalar_commit((ft - fz) * pow((K.TAU - z) % Q, -1, Q) % Q))
    assert ctx.kzg_open_dev([bufs[i % 4].ptr for i in range(count)], [n] * count, z, v) == expected
    assert ctx.kzg_open([base[i % 4][1] for i in range(count)], z, v) == expected
    assert ctx.kzg_open_dev([bufs[i % 4].ptr for i in range(count)], [n] * count, z, v, commitments=False) == (expected[0], None, expected[2])
    for b in bufs:
        b.free()


def test_open_mixed_lengths_empty_polynomials_and_trailing_zeros(ctx):
    rnd = random.Random(7)
    lens = [0, 5, 1, 0, 1025, 3, 70000, 2, 0, 64, 1024, 7]
    polys = [[rnd.randrange(Q) for _ in range(n)] for n in lens]
    polys[4] = polys[4][:1000] + [0] * 25            # trailing zeros inside a polynomial
    polys[9] = [0] * 64                              # a zero polynomial with a length
    polys[6][-1] = 0
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    import plonk_amd
    ev, cm, wit = check_open(ctx, polys, [plonk_amd.fr_to_bytes_mont(p) for p in polys], z, v)
    assert cm[0] == cm[3] == cm[9] == ID48 and ev[0] == ev[9] == 0


def test_open_special_points(ctx):
    import plonk_amd
    rnd = random.Random(8)
    n = 1024
    polys = [[rnd.randrange(Q) for _ in range(n)] for _ in range(3)]
    raw = [plonk_amd.fr_to_bytes_mont(p) for p in polys]
    omega = pow(7, (Q - 1) // n, Q)                  # a root of unity of the size
    assert pow(omega, n, Q) == 1 and pow(omega, n // 2, Q) != 1
    for z in (0, 1, omega, pow(omega, 5, Q), rnd.randrange(Q)):
        check_open(ctx, polys, raw, z, rnd.randrange(Q))
    check_open(ctx, polys[:1], raw[:1], 0, None)     # open_single at zero: the quotient is a shift
    check_open(ctx, polys, raw, rnd.randrange(Q), 0)  # v = 0: only the first polynomial counts
    check_open(ctx, polys, raw, rnd.randrange(Q), 1)


def test_open_constant_empty_and_no_polynomials(ctx):
    import plonk_amd
    ev, cm, wit = check_open(ctx, [[5]], [plonk_amd.fr_to_bytes_mont([5])], 12345, None)
    assert wit == ID48 and ev == [5]
    ev, cm, wit = ctx.kzg_open([b"", b"", b""], 3, 9)
    assert ev == [0, 0, 0] and cm == [ID48] * 3 and wit == ID48
    ev, cm, wit = ctx.kzg_open([], 3, None)
    assert ev == [] and cm == [] and wit == ID48
    ev, cm, wit = ctx.kzg_open_dev([], [], 3, None)
    assert ev == [] and wit == ID48


def test_open_resident_and_staged_agree_and_the_grouped_accumulation_runs(ctx):
    """count x length larger than a staging buffer (max(longest, 2^16) coefficients): the host form takes several groups"""
    rnd = random.Random(9)
    lens = [(1 << 16) - 5, 40000, (1 << 16), 1000, 30000, 65000, 12, 50000, 60000, 9]
    assert sum(lens) > 4 * (1 << 16)
    polys = [rand_poly(rnd, n) for n in lens]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    staged = check_open(ctx, [p[0] for p in polys], [p[1] for p in polys], z, v)
    bufs = []
    for _, raw in polys:
        b = ctx.alloc(len(raw))
        b.upload(raw)
        bufs.append(b)
    resident = ctx.kzg_open_dev([b.ptr for b in bufs], lens, z, v)
    assert resident == staged
    # more than one launch group of the resident form too (KZG_GROUP = 64 polynomials per launch)
    many = [rand_poly(rnd, 1 + (i * 37) % 300) for i in range(150)]
    check_open(ctx, [p[0] for p in many], [p[1] for p in many], z, v)
    for b in bufs:
        b.free()


def test_open_errors(ctx):
    import plonk_amd
    one = plonk_amd.fr_to_bytes_mont([1])
    fresh = plonk_amd.Context(0)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        fresh.kzg_open([one], 1, None)
    assert ei.value.code == ERR_NO_SRS
    with pytest.raises(plonk_amd.PlonkError) as ei:
        fresh.kzg_open([b""], 1, None)
    assert ei.value.code == ERR_NO_SRS
    assert fresh.kzg_open([], 1, None) == ([], [], ID48)
    srs = C.synthetic_srs(64)
    fresh.srs_load_bytes(srs, 64)
    ok = plonk_amd.fr_to_bytes_mont([3] * 64)
    fresh.kzg_open([ok], 5, None)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        fresh.kzg_open([plonk_amd.fr_to_bytes_mont([3] * 65)], 5, None)
    assert ei.value.code == ERR_DEGREE
    # the degree is that of the TRIMMED polynomial: 70 coefficients, the last 6 zero, fit a 64-point key
    padded = [rnd_c for rnd_c in range(1, 65)] + [0] * 6
    ev, cm, wit = fresh.kzg_open([plonk_amd.fr_to_bytes_mont(padded)], 5, None)
    assert (ev, cm, wit) == K.open_expected([padded], 5)
    buf = fresh.alloc(32 * 70)
    buf.upload(plonk_amd.fr_to_bytes_mont(padded))
    assert fresh.kzg_open_dev([buf.ptr], [70], 5, None) == (ev, cm, wit)
    buf.upload(plonk_amd.fr_to_bytes_mont([1] * 70))
    with pytest.raises(plonk_amd.PlonkError) as ei:
        fresh.kzg_open_dev([buf.ptr], [70], 5, None)
    assert ei.value.code == ERR_DEGREE
    # NULLs
    lib, h = fresh.lib, fresh.handle
    z = plonk_amd.fr_to_bytes_mont([5])
    out, wit48 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(48)
    ptrs, lens = (ctypes.c_void_p * 2)(None, None), (ctypes.c_uint64 * 2)(1, 1)
    assert lib.plonk_kzg_open(h, ptrs, lens, 1, z, None, out, None, wit48) == ERR_ARG        # polys[0] NULL with a length
    keep = ctypes.create_string_buffer(ok, len(ok))
    ptrs[0] = ptrs[1] = ctypes.cast(keep, ctypes.c_void_p).value
    assert lib.plonk_kzg_open(h, ptrs, lens, 1, None, None, out, None, wit48) == ERR_ARG     # point
    assert lib.plonk_kzg_open(h, ptrs, lens, 1, z, None, None, None, wit48) == ERR_ARG       # evaluations
    assert lib.plonk_kzg_open(h, ptrs, lens, 1, z, None, out, None, None) == ERR_ARG         # witness
    assert lib.plonk_kzg_open(h, ptrs, lens, 2, z, None, out, None, wit48) == ERR_ARG        # two polynomials need v
    assert lib.plonk_kzg_open(None, ptrs, lens, 1, z, None, out, None, wit48) == ERR_ARG
    assert lib.plonk_kzg_open(h, ptrs, lens, 65537, z, z, out, None, wit48) == ERR_ARG
    assert lib.plonk_kzg_open(h, ptrs, lens, 1, z, None, out, None, wit48) == OK
    # a context with a communicator holds only a range of the key
    uid = plonk_amd.Context.comm_unique_id()
    fresh.comm_init(uid, 0, 1)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        fresh.kzg_open([ok], 5, None)
    assert ei.value.code == ERR_STATE
    k = plonk_amd.KzgKey(fresh, K.opening_key())
    with pytest.raises(plonk_amd.PlonkError) as ei:
        k.srs_check(bytes(32))
    assert ei.value.code == ERR_STATE
    k.close()
    fresh.comm_destroy()
    fresh.kzg_open([ok], 5, None)
    buf.free()
    fresh.close()


def test_open_leaves_the_prover_of_the_context_untouched():
    import plonk_amd
    c = plonk_amd.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=77)()
    case = C.compile_fast(comp, b"kzg")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = plonk_amd.Prover.compile(c, b"kzg", cols["selectors"], cols["wires"], cols["witnesses"])
    before = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    rnd = random.Random(5)
    polys = [[rnd.randrange(Q) for _ in range(700)] for _ in range(20)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    assert c.kzg_open(polys, z, v) == K.open_expected(polys, z, v)
    after = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    assert before == after
    prover.close()
    c.close()


# ---- batch check -------------------------------------------------------------------------------------------------------
def make_proof(comm, e, wit):
    import plonk_amd
    return plonk_amd.KzgProof.make(comm, e, wit)


def opened(ctx, rnd, n, z):
    """one honest opening of a random polynomial of n coefficients at z, from kzg_open"""
    p = [rnd.randrange(Q) for _ in range(n)]
    ev, cm, wit = ctx.kzg_open([p], z, None)
    return make_proof(cm[0], ev[0], wit)


def scalar_proofs(rnd, count, points):
    """honest openings made in the exponent (no polynomial): commitment [c] g, evaluation e, witness [(c - e) / (tau - z)] g"""
    proofs, logs = [], []
    for k in range(count):
        c, e = rnd.randrange(Q), rnd.randrange(Q)
        w = (c - e) * pow((K.TAU - points[k]) % Q, -1, Q) % Q
        logs.append((c, e, w))
        proofs.append(make_proof(K.scalar_commit(c), e, K.scalar_commit(w)))
    return proofs, logs


def test_batch_verification_port(ctx, key):
    """key.rs test_batch_verification: two polynomials opened at two different points, checked together"""
    rnd = random.Random(21)
    za, zb = rnd.randrange(Q), rnd.randrange(Q)
    pa, pb = opened(ctx, rnd, 30, za), opened(ctx, rnd, 30, zb)
    assert key.batch_check([za], [pa]) and key.batch_check([zb], [pb])
    assert key.batch_check([za, zb], [pa, pb], label=b"")
    assert not key.batch_check([zb, za], [pa, pb])
    ref = [(bytes(p.commitment), p.value, bytes(p.witness)) for p in (pa, pb)]
    assert K.batch_check([za, zb], ref) and not K.batch_check([zb, za], ref)


def test_aggregate_witness_port(ctx, key):
    """key.rs test_aggregate_witness: three polynomials at one point, v from a transcript, flattened, checked singly"""
    rnd = random.Random(22)
    polys = [[rnd.randrange(Q) for _ in range(n)] for n in (28, 28, 29)]
    z = rnd.randrange(Q)
    v = Transcript(b"").challenge_scalar(b"v_challenge")
    ev, cm, wit = ctx.kzg_open(polys, z, v)
    flat = ctx.kzg_flatten(cm, ev, v, wit)
    assert (bytes(flat.commitment), flat.value, bytes(flat.witness)) == K.flatten(cm, ev, v, wit)
    assert key.batch_check([z], [flat])
    wrong = ctx.kzg_flatten(cm, ev, (v + 1) % Q, wit)
    assert not key.batch_check([z], [wrong])


def test_batch_with_aggregation_port(ctx, key):
    """key.rs test_batch_with_aggregation: an aggregated opening of three polynomials at one point and a single opening at
    another, in one batch; the transcript that gave v continues into the batch challenge, so the caller passes its own u"""
    rnd = random.Random(23)
    polys = [[rnd.randrange(Q) for _ in range(n)] for n in (28, 28, 28)]
    za, zb = rnd.randrange(Q), rnd.randrange(Q)
    single = opened(ctx, rnd, 28, zb)
    t = Transcript(b"agg_batch")
    v = t.challenge_scalar(b"v_challenge")
    ev, cm, wit = ctx.kzg_open(polys, za, v)
    flat = ctx.kzg_flatten(cm, ev, v, wit)
    points, proofs = [za, zb], [flat, single]
    u = K.batch_challenge(t, points, [(bytes(p.commitment), p.value, bytes(p.witness)) for p in proofs])
    assert key.batch_check(points, proofs, u=u)
    assert key._last_challenges()[0] == u
    assert not key.batch_check(points, [flat, opened(ctx, rnd, 28, za)], u=u)


@pytest.mark.parametrize("count,repeat", [(1, False), (2, False), (2, True), (64, False), (64, True), (1024, False), (1500, True)])
def test_batch_check_sizes(key, count, repeat):
    rnd = random.Random(300 + count)
    zs = [rnd.randrange(Q) for _ in range(3)]
    points = [zs[k % 3] if repeat else rnd.randrange(Q) for k in range(count)]
    proofs, logs = scalar_proofs(rnd, count, points)
    rc, info = key.batch_check_code(points, proofs, label=b"sizes")
    u = key._last_challenges()[0]
    assert u == K.batch_challenge(Transcript(b"sizes"), points, [(bytes(p.commitment), p.value, bytes(p.witness)) for p in proofs])
    assert K.batch_check_scalar(points, logs, u)
    assert rc == OK
    assert info["proofs"] == count and info["msm_terms"] == 3 * count + 1 and info["pairing_checks"] == 1 and info["rejected"] == 0


def test_batch_check_identity_commitments(key):
    rnd = random.Random(31)
    z = rnd.randrange(Q)
    zero_poly = make_proof(ID48, 0, ID48)                               # the zero polynomial opens to zero anywhere
    constant = make_proof(K.scalar_commit(9), 9, ID48)                  # a constant: identity witness
    through_zero = make_proof(ID48, (-(K.TAU - z) * 4) % Q, K.scalar_commit(4))   # c = 0 = e + w (tau - z)
    assert key.batch_check([z], [zero_poly]) and key.batch_check([z], [constant]) and key.batch_check([z], [through_zero])
    assert key.batch_check([z, z, 5], [zero_poly, constant, zero_poly])
    assert not key.batch_check([z], [make_proof(ID48, 1, ID48)])


def test_batch_check_tamper_sweep(key):
    rnd = random.Random(32)
    count = 64
    points = [rnd.randrange(Q) for _ in range(count)]
    proofs, _ = scalar_proofs(rnd, count, points)
    assert key.batch_check(points, proofs)
    other = K.scalar_commit(rnd.randrange(Q))
    for k in (0, 17, 63):
        p = proofs[k]
        bad_points = list(points)
        bad_points[k] = (points[k] + 1) % Q
        cases = [(bad_points, proofs),
                 (points, proofs[:k] + [make_proof(bytes(p.commitment), (p.value + 1) % Q, bytes(p.witness))] + proofs[k + 1:]),
                 (points, proofs[:k] + [make_proof(other, p.value, bytes(p.witness))] + proofs[k + 1:]),
                 (points, proofs[:k] + [make_proof(bytes(p.commitment), p.value, other)] + proofs[k + 1:])]
        for pts, prs in cases:
            rc, info = key.batch_check_code(pts, prs)
            assert rc == ERR_VERIFY and info["rejected"] == count


def test_batch_check_malformed_input(ctx, key):
    rnd = random.Random(33)
    points = [rnd.randrange(Q) for _ in range(4)]
    proofs, _ = scalar_proofs(rnd, 4, points)
    x = 1
    while pow((x ** 3 + 4) % E.P, (E.P - 1) // 2, E.P) == 1:
        x += 1
    not_a_point = bytearray(x.to_bytes(48, "big"))
    not_a_point[0] |= 0x80
    for field in ("commitment", "witness"):
        bad = make_proof(bytes(proofs[2].commitment), proofs[2].value, bytes(proofs[2].witness))
        ctypes.memmove(getattr(bad, field), bytes(not_a_point), 48)
        assert key.batch_check_code(points, proofs[:2] + [bad] + proofs[3:])[0] == ERR_POINT
    uncompressed = make_proof(bytes(47) + b"\x01", proofs[0].value, bytes(proofs[0].witness))     # no compression flag
    assert key.batch_check_code(points, [uncompressed] + proofs[1:])[0] == ERR_POINT
    # non-canonical scalars: the limbs of q itself, as an evaluation, as a point and as u
    noncanon = make_proof(bytes(proofs[1].commitment), 0, bytes(proofs[1].witness))
    ctypes.memmove(noncanon.evaluation, Q.to_bytes(32, "little"), 32)
    assert key.batch_check_code(points, [proofs[0], noncanon] + proofs[2:])[0] == ERR_DATA
    arr = (type(proofs[0]) * 4)(*proofs)
    import plonk_amd
    pts = bytearray(plonk_amd.fr_to_bytes_mont(points))
    lib = ctx.lib
    assert lib.plonk_kzg_batch_check(key.handle, bytes(pts), arr, 4, b"", 0, None, None) == OK
    assert lib.plonk_kzg_batch_check(key.handle, bytes(pts), arr, 4, b"", 0, (Q + 5).to_bytes(32, "little"), None) == ERR_DATA
    pts[32:64] = (2 ** 256 - 1).to_bytes(32, "little")
    assert lib.plonk_kzg_batch_check(key.handle, bytes(pts), arr, 4, b"", 0, None, None) == ERR_DATA
    # the bool form tells malformed input from a failing batch
    with pytest.raises(plonk_amd.PointMalformed):
        key.batch_check(points, [uncompressed] + proofs[1:])
    with pytest.raises(plonk_amd.InvalidData):
        key.batch_check(points, [proofs[0], noncanon] + proofs[2:])
    # count == 0 (key.rs:667) and NULLs
    assert key.batch_check_code([], [])[0] == ERR_VERIFY and key.batch_check([], []) is False
    assert lib.plonk_kzg_batch_check(None, bytes(pts), arr, 4, b"", 0, None, None) == ERR_ARG
    assert lib.plonk_kzg_batch_check(key.handle, None, arr, 4, b"", 0, None, None) == ERR_ARG
    assert lib.plonk_kzg_batch_check(key.handle, bytes(pts), None, 4, b"", 0, None, None) == ERR_ARG


def test_batch_challenge_binding(key):
    """the u the library derived equals the restatement, for several labels and batch lengths"""
    rnd = random.Random(34)
    for label, count in ((b"", 1), (b"x", 3), (b"a longer transcript label", 17)):
        points = [rnd.randrange(Q) for _ in range(count)]
        proofs, _ = scalar_proofs(rnd, count, points)
        assert key.batch_check(points, proofs, label=label)
        ref = [(bytes(p.commitment), p.value, bytes(p.witness)) for p in proofs]
        assert key._last_challenges()[0] == K.batch_challenge(Transcript(label), points, ref)


def test_flatten_errors(ctx):
    import plonk_amd
    with pytest.raises(plonk_amd.PlonkError) as ei:
        ctx.kzg_flatten([], [], 7, ID48)
    assert ei.value.code == ERR_ARG
    with pytest.raises(plonk_amd.PlonkError) as ei:
        ctx.kzg_flatten([bytes(48)], [1], 7, ID48)
    assert ei.value.code == ERR_POINT


def test_key_create_validates_the_opening_key(ctx):
    import plonk_amd
    good = K.opening_key()
    with pytest.raises(ValueError):
        plonk_amd.KzgKey(ctx, good[:239])
    out = ctypes.c_void_p()
    assert ctx.lib.plonk_kzg_key_create(ctx.handle, None, ctypes.byref(out)) == ERR_ARG
    for bad in (ID48 + good[48:], good[:48] + bytes([0xC0]) + bytes(95) + good[144:], good[:47] + bytes([good[47] ^ 1]) + good[48:],
                good[:239] + bytes([good[239] ^ 1])):
        with pytest.raises(plonk_amd.PlonkError) as ei:
            plonk_amd.KzgKey(ctx, bad)
        assert ei.value.code in (ERR_DATA,), bad[:4]


# ---- srs_check ---------------------------------------------------------------------------------------------------------
def test_srs_check_passes_on_the_large_key_and_derives_r_as_restated(ctx, key):
    seed = bytes(range(32))
    assert key.srs_check(seed)
    assert key._last_challenges()[1] == K.srs_challenge(seed, BIG, K.opening_key())
    assert key.srs_check(bytes(32))


def test_srs_check_small_key_and_every_kind_of_wrong_key():
    import plonk_amd
    c = plonk_amd.Context(0)
    n = 1 << 10
    srs = C.synthetic_srs(n)
    seed = b"\x5a" * 32
    k = plonk_amd.KzgKey(c, K.opening_key())
    with pytest.raises(plonk_amd.PlonkError) as ei:
        k.srs_check(seed)
    assert ei.value.code == ERR_NO_SRS
    c.srs_load_bytes(srs, n)
    assert k.srs_check(seed)
    assert k._last_challenges()[1] == K.srs_challenge(seed, n, K.opening_key())
    # one point replaced by another valid point of the subgroup
    other = E.g1_to_raw96(E.g1_mul(E.G1_GEN, 123456789))
    for i in (1, 500, n - 1):
        c.srs_load_bytes(srs[:96 * i] + other + srs[96 * (i + 1):], n)
        assert not k.srs_check(seed)
    # two points swapped
    i, j = 3, 700
    swapped = srs[:96 * i] + srs[96 * j:96 * (j + 1)] + srs[96 * (i + 1):96 * j] + srs[96 * i:96 * (i + 1)] + srs[96 * (j + 1):]
    c.srs_load_bytes(swapped, n)
    assert not k.srs_check(seed)
    # the first point is not g
    c.srs_load_bytes(other + srs[96:], n)
    assert not k.srs_check(seed)
    c.srs_load_bytes(srs, n)
    assert k.srs_check(seed)
    # x_h of another tau; another g
    k2 = plonk_amd.KzgKey(c, K.opening_key(tau=(K.TAU + 1) % Q))
    assert not k2.srs_check(seed)
    k3 = plonk_amd.KzgKey(c, K.opening_key(g=K.G_SCALAR + 1))
    assert not k3.srs_check(seed)
    # a key of one point and of two
    c.srs_load_bytes(srs[:96], 1)
    assert k.srs_check(seed) and not k3.srs_check(seed)
    c.srs_load_bytes(srs[:192], 2)
    assert k.srs_check(seed) and not k2.srs_check(seed)
    for kk in (k, k2, k3):
        kk.close()
    c.close()
