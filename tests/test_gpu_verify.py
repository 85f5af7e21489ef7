"""GPU: proof verification (plonk_verifier_from_bytes / plonk_verify, plonk_amd/csrc/verify.hip) — honest proofs of the GPU
prover verify and agree with the known-tau verifier of oracle/verifier.py, tampered proofs are rejected with the right
per-proof code, a batch takes one pairing check when valid and finds exactly its bad proofs by bisection, and a verifier
leaves its context's prover alone."""
import os
import random
import sys

import pytest

from oracle import bls12_381 as E
from oracle.verifier import verify_with_tau
from tests import circuits as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g2_ref as G2   # noqa: E402

pytestmark = pytest.mark.gpu
Q, P = E.Q, E.P
TAU = 0x5EED0000 * 0x9E3779B97F4A7C15 % Q          # circuits.synthetic_srs's defaults
G_SCALAR = 0xA5A5A5A5DEADBEEF
OK, ERR_ARG, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -9, -10, -12


def opening_key():
    return (E.g1_compress(E.g1_mul(E.G1_GEN, G_SCALAR)) + G2.g2_compress(G2.G2_GEN)
            + G2.g2_compress(G2.g2_mul(G2.G2_GEN, TAU)))


class Setup:
    def __init__(self, ctx, log_n, seed, label=b"verify"):
        import plonk_amd
        comp = C.big_widget_circuit(1 << log_n, seed=seed)()
        case = C.compile_fast(comp, label)
        srs = C.synthetic_srs(case["size"] + 7)
        ctx.srs_load_bytes(srs, len(srs) // 96)
        cols = C.circuit_columns(comp)
        self.prover = plonk_amd.Prover.compile(ctx, label, cols["selectors"], cols["wires"], cols["witnesses"])
        self.values, self.case, self.label = cols["values"], case, label
        self.pi_idx = case["pi_idx"]
        self.pis = [case["pi"][i] for i in self.pi_idx]
        self.blob = self.prover.verifier_to_bytes(opening_key(), self.pi_idx)
        raw = self.prover.vk_commitments()
        self.vk = {name: E.g1_decompress(raw[48 * k:48 * k + 48]) for k, name in enumerate(plonk_amd.POLY_ORDER)}

    def prove(self, seed):
        return self.prover.prove_witnesses(self.values, self.case["pi"], C.blinders(seed))

    def tau_ok(self, proof, pis=None):
        pi = dict(zip(self.pi_idx, pis if pis is not None else self.pis))
        return verify_with_tau(proof, self.vk, self.label, self.case["constraints"], pi, TAU, E.g1_mul(E.G1_GEN, G_SCALAR))


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def s10(ctx):
    return Setup(ctx, 10, 401)


@pytest.fixture(scope="module")
def verifier(ctx, s10):
    import plonk_amd
    v = plonk_amd.Verifier(ctx, s10.blob)
    yield v
    v.close()


@pytest.fixture(scope="module")
def proofs(s10):
    return [s10.prove(5000 + k) for k in range(64)]


def test_honest_proofs_verify_like_the_known_tau_verifier(ctx, s10, verifier, proofs):
    assert s10.pis, "the circuit has public inputs"
    for proof in proofs[:3]:
        assert s10.tau_ok(proof)
        assert verifier.verify(proof, s10.pis)
        info = verifier.last()
        assert info["proofs"] == 1 and info["pairing_checks"] == 1 and info["msm_terms"] == 13 + 16


def test_2p12_proof_verifies(ctx):
    import plonk_amd
    s = Setup(ctx, 12, 402, label=b"verify-2p12")
    v = plonk_amd.Verifier(ctx, s.blob)
    proof = s.prove(1)
    assert s.tau_ok(proof) and v.verify(proof, s.pis)
    bad = bytearray(proof)
    bad[528] ^= 1
    assert not s.tau_ok(bytes(bad)) and not v.verify(bytes(bad), s.pis)
    v.close()


def non_square_x():
    x = 1
    while pow((x ** 3 + 4) % P, (P - 1) // 2, P) == 1:
        x += 1
    return x


def on_curve_outside_g1():
    x = 1
    while True:
        y2 = (x ** 3 + 4) % P
        if pow(y2, (P - 1) // 2, P) == 1:
            y = pow(y2, (P + 1) // 4, P)
            acc = E.to_jac(None)
            for bit in bin(Q)[2:]:                                        # [q] P without jac_mul's reduction mod q
                acc = E.jac_double(acc)
                if bit == "1":
                    acc = E.jac_add(acc, E.to_jac((x, y)))
            if E.to_affine(acc) is not None:
                return (x, y)
        x += 1


def with_comm(proof, k, enc48):
    b = bytearray(proof)
    b[48 * k:48 * k + 48] = enc48
    return bytes(b)


def with_eval(proof, k, value_int):
    b = bytearray(proof)
    b[528 + 32 * k:528 + 32 * k + 32] = value_int.to_bytes(32, "little")
    return bytes(b)


def test_tampered_proofs_are_rejected_with_the_right_code(ctx, s10, verifier, proofs):
    import plonk_amd
    proof = proofs[0]
    ev0 = int.from_bytes(proof[528:560], "little")
    off = bytearray(non_square_x().to_bytes(48, "big"))
    off[0] |= 0x80
    cases = [
        (with_eval(proof, 0, Q), ERR_DATA),                                   # non-canonical scalar
        (with_comm(proof, 2, bytes(off)), ERR_POINT),                         # x^3 + 4 not a square
        (with_comm(proof, 3, E.g1_compress(on_curve_outside_g1())), ERR_POINT),
        (with_eval(proof, 5, (int.from_bytes(proof[528 + 160:528 + 192], "little") + 1) % Q), ERR_VERIFY),
        (with_eval(proof, 0, (ev0 + 1) % Q), ERR_VERIFY),
        (with_comm(proof, 9, E.g1_compress(None)), ERR_VERIFY),               # W_z swapped for the identity
        (with_comm(proof, 4, proof[0:48]), ERR_VERIFY),                       # z swapped for another valid point
    ]
    got = verifier.verify_batch([p for p, _ in cases], [s10.pis] * len(cases))
    assert got == [code for _, code in cases]
    for p, code in cases:                                                      # the same verdicts one at a time
        assert verifier.verify_batch([p], [s10.pis]) == [code]
        if code == ERR_VERIFY:
            assert not s10.tau_ok(p)
    wrong = list(s10.pis)
    wrong[0] = (wrong[0] + 1) % Q
    assert not verifier.verify(proof, wrong) and not s10.tau_ok(proof, wrong)
    with pytest.raises(plonk_amd.PlonkError) as e:                            # Error::InconsistentPublicInputsLen
        verifier.verify(proof, s10.pis[:-1])
    assert e.value.code == ERR_ARG


def test_other_circuit_and_version_mismatch_are_rejected(ctx, s10, verifier, proofs):
    import plonk_amd
    other = Setup(ctx, 10, 403)
    assert not verifier.verify(other.prove(7), s10.pis)
    # V2 proof against a V3 verifier and the reverse
    s10b = Setup(ctx, 10, 401)
    s10b.prover.set_version(2)
    v2proof = s10b.prove(5000)
    assert not verifier.verify(v2proof, s10.pis)
    v2 = plonk_amd.Verifier(ctx, s10.blob)
    v2.set_version(2)
    assert v2.verify(v2proof, s10.pis)
    assert not v2.verify(proofs[0], s10.pis)
    with pytest.raises(plonk_amd.PlonkError):
        v2.set_version(1)
    v2.close()


def test_batch_of_64_takes_one_pairing_check(verifier, s10, proofs):
    assert len(set(proofs)) == 64
    assert verifier.verify_batch(proofs, [s10.pis] * 64) == [OK] * 64
    info = verifier.last()
    assert info["pairing_checks"] == 1 and info["msm_terms"] == 13 * 64 + 16 and info["rejected"] == 0


@pytest.mark.parametrize("nbad", [1, 3])
def test_batch_finds_exactly_its_bad_proofs(verifier, s10, proofs, nbad):
    rnd = random.Random(nbad)
    bad = sorted(rnd.sample(range(64), nbad))
    batch = list(proofs)
    for k in bad:
        batch[k] = with_eval(batch[k], 14, (int.from_bytes(batch[k][528 + 448:560 + 448], "little") + 1) % Q)
    got = verifier.verify_batch(batch, [s10.pis] * 64)
    assert [k for k, v in enumerate(got) if v != OK] == bad and all(got[k] == ERR_VERIFY for k in bad)
    info = verifier.last()
    assert info["rejected"] == nbad
    assert info["pairing_checks"] <= 1 + 2 * nbad * 6                        # O(b log K), K = 64


def test_opposite_shifts_do_not_cancel(verifier, s10, proofs):
    """W_z of proof k moved by +D and of proof k' by -D: an unweighted sum of the checks would accept both"""
    d = E.g1_mul(E.G1_GEN, 0xD317A)
    batch = list(proofs[:8])
    for k, sgn in ((2, 1), (5, Q - 1)):
        wz = E.g1_decompress(batch[k][9 * 48:10 * 48])
        batch[k] = with_comm(batch[k], 9, E.g1_compress(E.g1_add(wz, E.g1_mul(d, sgn))))
    got = verifier.verify_batch(batch, [s10.pis] * 8)
    assert got == [OK, OK, ERR_VERIFY, OK, OK, ERR_VERIFY, OK, OK]


def test_verifier_leaves_the_prover_alone(ctx):
    """prove, verify (a batch, then one proof), prove again on one context: same bytes, same MSM plan, same prover"""
    import plonk_amd
    s = Setup(ctx, 10, 404)   # (the other setups of this module loaded their own commit keys on ctx)
    v = plonk_amd.Verifier(ctx, s.blob)
    before = s.prove(777)
    desc = s.prover.describe()
    msm = ctx.last_msm()
    assert v.verify_batch([before] * 3, [s.pis] * 3) == [OK] * 3
    assert v.verify(before, s.pis)
    assert ctx.last_msm() == msm
    assert s.prove(777) == before
    assert s.prover.describe() == desc
    v.close()


def test_malformed_verifier_blobs_are_refused(ctx, s10):
    import plonk_amd
    blob = s10.blob
    with pytest.raises(plonk_amd.NotEnoughBytes):
        plonk_amd.Verifier(ctx, blob[:40])
    with pytest.raises(plonk_amd.NotEnoughBytes):
        plonk_amd.Verifier(ctx, blob[:-1])
    big = bytearray(blob)
    big[24:32] = (1 << 62).to_bytes(8, "big")                                  # pi count whose byte length overflows
    with pytest.raises(plonk_amd.NotEnoughBytes):
        plonk_amd.Verifier(ctx, bytes(big))
    ok_off = 48 + len(s10.label) + 968
    for off, enc in ((ok_off, E.g1_compress(None)), (ok_off + 48, bytes([0xC0]) + bytes(95)),
                     (ok_off + 144, bytes([0xC0]) + bytes(95)), (ok_off + 48, bytes([0x80]) + bytes([0xFF]) * 95)):
        b = bytearray(blob)
        b[off:off + len(enc)] = enc
        with pytest.raises(plonk_amd.InvalidData):
            plonk_amd.Verifier(ctx, bytes(b))


# ---- every single-field tamper through the device path, both transcript versions -----------------------------------------
@pytest.mark.parametrize("version", [3, 2])
def test_every_single_field_tamper_is_rejected(ctx, version):
    """each of the 11 commitments replaced by another valid point and each of the 15 evaluations + 1 (the selector
    evaluations q_arith, q_c, q_l, q_r included: the opening binds them through [F]): one batch, and one at a time"""
    import plonk_amd
    s = Setup(ctx, 10, 405, label=b"tamper-v%d" % version)
    s.prover.set_version(version)
    v = plonk_amd.Verifier(ctx, s.blob)
    v.set_version(version)
    proof = s.prove(31)
    cases = []
    for c in range(11):
        cases.append(with_comm(proof, c, E.g1_compress(E.g1_mul(E.G1_GEN, 0xC0FFEE + c))))
    for k in range(15):
        cases.append(with_eval(proof, k, (int.from_bytes(proof[528 + 32 * k:560 + 32 * k], "little") + 1) % Q))
    got = v.verify_batch([proof] + cases, [s.pis] * (1 + len(cases)))
    assert got == [OK] + [ERR_VERIFY] * len(cases)
    for i, bad in enumerate(cases):
        assert v.verify_batch([bad], [s.pis]) == [ERR_VERIFY], i
        if version == 3:
            assert not s.tau_ok(bad), i
    v.close()


# ---- the device MSM against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 2, 31, 1000, 1 << 16])
def test_device_msm_matches_the_oracle(ctx, size):
    """verify_msm_kernel through the binding's test hook: identity points, repeated points, P with -P, zero scalars,
    q - 1 and random full-width scalars"""
    rnd = random.Random(size)
    pool = [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(24)]
    pool += [E.g1_mul(p, Q - 1) for p in pool[:8]]          # -P next to P
    pool.append(None)                                        # the identity
    pts, sc = [], []
    special = [0, 1, Q - 1, 2, Q - 2]
    for i in range(size):
        pts.append(pool[rnd.randrange(len(pool))] if size > 2 else pool[i])
        sc.append(special[i % len(special)] if i % 3 == 0 else rnd.randrange(Q))
    if size >= 31:
        pts[5], sc[5] = pts[4], sc[4]                        # the same term twice: a doubling inside one lane's sum
        pts[7], sc[7] = E.g1_mul(pts[6], Q - 1) if pts[6] else None, sc[6]   # P and -P with equal scalars: cancel
    got = ctx._verify_msm(pts, sc)
    if size <= 1000:
        assert got == E.msm_pippenger(pts, sc) == E.msm_naive(pts, sc)
    else:   # the same sum with the scalars of equal points added first (the pool is small)
        agg = {}
        for p, s in zip(pts, sc):
            if p is not None:
                agg[p] = (agg.get(p, 0) + s) % Q
        assert got == E.msm_naive(list(agg), list(agg.values()))
    # sums that cancel exactly: P [s] + P [q - s] = O, and the whole of it as the identity
    p = pool[0]
    assert ctx._verify_msm([p, p], [12345, Q - 12345]) is None
    assert ctx._verify_msm([None, p], [7, 0]) is None


# ---- larger circuits: the bench workloads ----------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,profile", [(16, "widgets"), (20, "dense")])
def test_bench_circuit_proof_verifies(log_n, profile):
    import bench
    import plonk_amd
    c = plonk_amd.Context(0)
    prover, wbuf, _ = bench.build_prover(c, log_n, 0, 1, None, profile=profile)
    pi = prover.public_inputs
    if profile == "widgets":
        assert pi, "the widget profile has public inputs"
    idx = sorted(pi)
    ok = (E.g1_compress(E.g1_mul(E.G1_GEN, bench.G_SCALAR)) + G2.g2_compress(G2.G2_GEN)
          + G2.g2_compress(G2.g2_mul(G2.G2_GEN, bench.TAU)))
    v = plonk_amd.Verifier(c, prover.verifier_to_bytes(ok, idx))
    bl = plonk_amd.fr_to_bytes_mont([(0xB11D0000 + i) * 0x9E3779B97F4A7C15 % Q for i in range(14)])
    proof = prover.prove_dev(wbuf.ptr, pi, bl)
    raw = prover.vk_commitments()
    vk = {name: E.g1_decompress(raw[48 * k:48 * k + 48]) for k, name in enumerate(plonk_amd.POLY_ORDER)}
    assert verify_with_tau(proof, vk, b"bench", 1 << log_n, pi, bench.TAU, E.g1_mul(E.G1_GEN, bench.G_SCALAR))
    vals = [pi[i] for i in idx]
    assert v.verify(proof, vals)
    bad = bytearray(proof)
    bad[530] ^= 4
    assert not v.verify(bytes(bad), vals)
    v.close()
    prover.close()
    wbuf.free()
    c.close()
