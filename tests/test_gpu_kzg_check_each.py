"""GPU: OpeningKey::check of every opening on its own in one pass (plonk_kzg_check_each; kzg.hip, pairing.hip).  Every
verdict equals plonk_kzg_batch_check with count == 1 on that item; a tampered item changes its own verdict only; two
tampers that cancel under a fixed batch challenge — which the folded check cannot see — are both flagged."""
import ctypes
import random

import pytest

from oracle import bls12_381 as E
from tests import circuits as C
from tests import kzg_ref as K

pytestmark = pytest.mark.gpu
Q = E.Q
OK, ERR_ARG, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -9, -10, -12
ID48 = K.IDENTITY48


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    srs = C.synthetic_srs(64)
    c.srs_load_bytes(srs, 64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key(ctx):
    import plonk_amd
    k = plonk_amd.KzgKey(ctx, K.opening_key())
    yield k
    k.close()


def make_proof(comm, e, wit):
    import plonk_amd
    return plonk_amd.KzgProof.make(comm, e, wit)


def opened(ctx, poly, z):
    ev, cm, wit = ctx.kzg_open([poly], z, None)
    return make_proof(cm[0], ev[0], wit)


def openings(ctx, rnd, count):
    """`count` openings of short polynomials at distinct points; item 0 at the point 0, item 1 (if any) of the zero
    polynomial (identity commitment and witness)"""
    points = [0] + [rnd.randrange(1, Q) for _ in range(count - 1)]
    assert len(set(points)) == count
    proofs = []
    for k, z in enumerate(points):
        poly = [0, 0, 0] if k == 1 else [rnd.randrange(Q) for _ in range(2 + k % 5)]
        proofs.append(opened(ctx, poly, z))
    if count > 1:
        assert bytes(proofs[1].commitment) == ID48 and bytes(proofs[1].witness) == ID48
    return points, proofs


def singles(key, points, proofs):
    return [key.batch_check_code([z], [p])[0] for z, p in zip(points, proofs)]


@pytest.mark.parametrize("count", [1, 3, 65])
def test_honest_openings_and_a_tamper_sweep_equal_the_single_calls(ctx, key, count):
    rnd = random.Random(3000 + count)
    points, proofs = openings(ctx, rnd, count)
    verdicts, info = key.check_each_info(points, proofs)
    assert verdicts == [OK] * count == singles(key, points, proofs)
    assert info["proofs"] == count and info["pairing_checks"] == count and info["msm_terms"] == 4 * count and info["rejected"] == 0
    other = K.scalar_commit(rnd.randrange(1, Q))
    k = count - 1
    p = proofs[k]
    bad_points = list(points)
    bad_points[k] = (points[k] + 1) % Q
    cases = [(points, proofs[:k] + [make_proof(other, p.value, bytes(p.witness))]),                       # commitment
             (points, proofs[:k] + [make_proof(bytes(p.commitment), (p.value + 1) % Q, bytes(p.witness))]),   # evaluation
             (points, proofs[:k] + [make_proof(bytes(p.commitment), p.value, other)]),                   # witness
             (bad_points, proofs)]                                                                       # point
    for pts, prs in cases:
        verdicts, info = key.check_each_info(pts, prs)
        assert verdicts == [OK] * k + [ERR_VERIFY]
        assert verdicts[k] == key.batch_check_code([pts[k]], [prs[k]])[0]
        assert info["rejected"] == 1 and info["pairing_checks"] == count


def test_tampers_that_cancel_under_a_fixed_challenge_are_both_flagged(ctx, key):
    rnd = random.Random(3010)
    points, proofs = openings(ctx, rnd, 4)
    d = rnd.randrange(1, Q)
    plus, minus = K.g_point(K.G_SCALAR * d % Q), K.g_point(K.G_SCALAR * (Q - d) % Q)
    bad = list(proofs)
    for k, delta in ((0, plus), (3, minus)):
        c = E.g1_add(E.g1_decompress(bytes(proofs[k].commitment)), delta)
        bad[k] = make_proof(E.g1_compress(c), proofs[k].value, bytes(proofs[k].witness))
    assert key.batch_check_code(points, bad, u=1)[0] == OK                # C_0 + D + C_3 - D: the folded check passes
    assert singles(key, points, bad) == [ERR_VERIFY, OK, OK, ERR_VERIFY]
    assert key.check_each(points, bad) == [ERR_VERIFY, OK, OK, ERR_VERIFY]


def test_malformed_items_get_their_own_verdict(ctx, key):
    import plonk_amd
    rnd = random.Random(3020)
    points, proofs = openings(ctx, rnd, 5)
    noncanon = make_proof(bytes(proofs[1].commitment), 0, bytes(proofs[1].witness))
    ctypes.memmove(noncanon.evaluation, Q.to_bytes(32, "little"), 32)
    off = make_proof(bytes([0x80]) + (1).to_bytes(47, "big"), proofs[3].value, bytes(proofs[3].witness))   # x = 1: off the curve
    items = [proofs[0], noncanon, proofs[2], off, proofs[4]]
    verdicts, info = key.check_each_info(points, items)
    assert verdicts == [OK, ERR_DATA, OK, ERR_POINT, OK] == singles(key, points, items)
    assert info["pairing_checks"] == 3 and info["msm_terms"] == 12 and info["rejected"] == 2
    # a non-canonical point, and both at once (the scalars are looked at first)
    pts = [plonk_amd.fr_to_bytes_mont([z]) for z in points]
    pts[3] = (2 ** 256 - 1).to_bytes(32, "little")
    assert key.check_each(pts, items) == [OK, ERR_DATA, OK, ERR_DATA, OK]
    # argument errors
    lib = ctx.lib
    arr = (type(proofs[0]) * 5)(*proofs)
    raw = plonk_amd.fr_to_bytes_mont(points)
    v = (ctypes.c_int32 * 5)()
    assert lib.plonk_kzg_check_each(None, raw, arr, 5, v, None) == ERR_ARG
    assert lib.plonk_kzg_check_each(key.handle, None, arr, 5, v, None) == ERR_ARG
    assert lib.plonk_kzg_check_each(key.handle, raw, None, 5, v, None) == ERR_ARG
    assert lib.plonk_kzg_check_each(key.handle, raw, arr, 5, None, None) == ERR_ARG
    assert lib.plonk_kzg_check_each(key.handle, raw, arr, 0, v, None) == ERR_ARG
    assert lib.plonk_kzg_check_each(key.handle, raw, arr, (1 << 24) + 1, v, None) == ERR_ARG
    assert lib.plonk_kzg_check_each(key.handle, raw, arr, 5, v, None) == OK and list(v) == [OK] * 5
