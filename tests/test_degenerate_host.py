"""The reference pinned at the edges of tests/degenerate_cases.py — CPU only.  For every case of the corpus the C restatement
of the reference prover (oracle/c/oracle_prove.c) returns a proof or CircuitUnsatisfied as the case expects; the big-int
verifier with the known trapdoor (oracle/verifier.py) accepts each proof under the C prover's VerifierKey and refuses it with
one evaluation byte changed; the proof is as degenerate as the case claims (identity commitments counted); the wire-index
form of the case reproduces its sigma; and the circuit a Composer can express — the empty one — is proved by the big-int
oracle (oracle/plonk.py) to the same 1008 bytes.  tests/test_gpu_degenerate.py compares the library with these proofs."""
import pytest

from oracle import bls12_381 as E
from oracle import cbind
from oracle import plonk as O
from oracle.verifier import verify_with_tau
from tests import degenerate_cases as D
from tests import diagnose_ref as DR

SRS_G = E.g1_mul(E.G1_GEN, D.G_SCALAR)
_ran = set()


def vk_points(vk48: bytes) -> dict:
    return {name: E.g1_decompress(vk48[48 * k:48 * k + 48]) for k, name in enumerate(cbind.POLY_ORDER)}


def tau_ok(case, vk, proof) -> bool:
    return verify_with_tau(proof, vk, D.LABEL, case.constraints, case.pi, D.TAU, SRS_G)


@pytest.mark.parametrize("name", [c.name for c in D.corpus()])
def test_c_oracle_proves_verifies_and_is_degenerate(name):
    case = D.by_name(name)
    got = D.oracle(name)
    _ran.add(name)
    # the wire-index form realises the case's sigma (what Prover.compile is given on the device)
    idx, values = D.unsat_witness_form(case) if case.expect == "unsat" else D.witness_form(case)
    assert D.sigma_from_indices(idx, case.n) == case.sigma
    assert [[values[idx[col][i]] for i in range(case.constraints)] for col in range(4)] == [w[:case.constraints] for w in case.wires]
    # the yardstick of the diagnosis agrees with the expected outcome
    shim = type("Rows", (), {"constraints": D.gates(case), "public_inputs": case.pi})()
    report = DR.report(shim, case.n, case.wires, pi=case.pi, sigma=case.sigma)
    if case.expect == "unsat":
        assert got["proofs"] == {"random": "unsat", "zero": "unsat"}
        assert report == [(case.changed_row, 1, 0)]
        return
    assert report == []
    vk = vk_points(got["vk"])
    if case.family == "no-selectors":
        assert sum(got["vk"][48 * k:48 * k + 48] == bytes([0xC0]) + bytes(47) for k in range(15)) == 11
    for kind in ("random", "zero"):
        proof = got["proofs"][kind]
        assert isinstance(proof, bytes) and len(proof) == 1008, (kind, proof)
        assert tau_ok(case, vk, proof), kind
        bad = bytearray(proof)
        bad[528 + 32 * 14] ^= 1                       # z_eval: bound by every proof, whatever else is zero
        assert not tau_ok(case, vk, bytes(bad)), kind
    # the degeneracy is real: a later edit cannot quietly turn the corpus into ordinary circuits
    assert D.identity_commitments(got["proofs"]["random"]) == 0
    assert D.identity_commitments(got["proofs"]["zero"]) >= case.identity_floor()
    assert got["proofs"]["zero"] != got["proofs"]["random"]


def test_every_case_of_the_corpus_ran():
    """(runs after the parametrised test above: same module, definition order)"""
    names = [c.name for c in D.corpus()]
    assert len(names) == 9 * 5 + 1 + 6 and _ran == set(names)
    # both sides of every threshold the issue names are there
    assert {(c.n, c.constraints) for c in D.corpus() if c.family == "zero-witness"} == {
        (2, 2), (4, 4), (4, 3), (8, 8), (8, 5), (16, 16), (16, 9), (64, 64), (64, 33), (4096, 4096), (4096, 2049)}


class Replay:
    def __init__(self, vals):
        self.vals = list(vals)

    def random_scalar(self):
        return self.vals.pop(0)


@pytest.mark.parametrize("kind", ["random", "zero"])
def test_empty_composer_through_the_bigint_oracle(kind):
    """Composer() with nothing appended, proved by oracle/plonk.py: the same VerifierKey and the same 1008 bytes as the C
    restatement — which is thereby pinned where the device is compared with it (n = 4, below the 4n quotient path)."""
    case = D.by_name("empty-composer-n4-c4")
    raw = D.srs(16)                                    # compile_circuit trims to next_pow2(4 + 6) + 6 + 1 = 23 points
    pp = [E.g1_from_raw96(raw[96 * i:96 * i + 96]) for i in range(len(raw) // 96)]
    assert raw[:len(D.srs(4))] == D.srs(4)
    oprover = O.compile_circuit(pp, D.LABEL, O.Composer(), msm=E.msm_pippenger)
    assert oprover.size == 4 and oprover.constraints == 4
    got = D.oracle(case.name)
    assert got["vk"] == b"".join(E.g1_compress(oprover.vk[name]) for name in cbind.POLY_ORDER)
    rng = Replay(D.BLINDERS[kind])
    proof, pis = O.prove(oprover, rng, O.Composer(), msm=E.msm_pippenger)
    assert not rng.vals and pis == []
    assert proof == got["proofs"][kind]
