"""GPU: the library on the degenerate corpus of tests/degenerate_cases.py — domains of 2 and 4 rows (the n < 8 fallback to
the 8n quotient domain), identically zero wire and quotient polynomials, zero blinders, q - 1 on every wire of one
permutation cycle, a public input on every row, no selector at all, the empty Composer — against the C restatement of the
reference prover, whose proofs tests/test_degenerate_host.py pins on the CPU.

Every case runs under both quotient domains and both wire-commitment modes.  In each configuration a prover created from
the coefficient forms and one compiled on the device from gate columns must give the C oracle's VerifierKey commitments and,
through prove / prove_dev / prove_witnesses and for random and for zero blinders, its 1008 proof bytes; diagnose must agree
with the yardstick of tests/diagnose_ref.py; a Verifier built from the prover must accept the proofs — with up to nine of
their eleven commitments the identity, and a key whose selector commitments all are — and refuse them with one byte changed.
The unsatisfied cases must raise CircuitUnsatisfied from every entry point and leave the prover able to prove the honest
assignment bit-exactly.

The n = 2 cases with non-zero blinders are the regression tests of blind_kernel (poly.hip): with three blinders on a domain
of two rows, b0 X^n and -b2 X^2 are the same coefficient, and the kernel used to store one over the other — every such
proof came back as CircuitUnsatisfied."""
import os
import sys

import pytest

from conftest import configure
from oracle import bls12_381 as E
from tests import circuits as C
from tests import degenerate_cases as D
from tests import diagnose_ref as DR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g2_ref as G2   # noqa: E402

pytestmark = pytest.mark.gpu
OK, ERR_POINT, ERR_VERIFY = 0, -10, -12
CONFIGS = [(domain, wire_commit) for domain in (4, 8) for wire_commit in (0, 1)]   # wire_commit 0: values, 1: coefficient form
_ran = set()
_opening_key = []


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    yield c
    c.close()


def opening_key():
    if not _opening_key:
        _opening_key.append(E.g1_compress(E.g1_mul(E.G1_GEN, D.G_SCALAR)) + G2.g2_compress(G2.G2_GEN)
                            + G2.g2_compress(G2.g2_mul(G2.G2_GEN, D.TAU)))
    return _opening_key[0]


def tampered(proof: bytes) -> bytes:
    bad = bytearray(proof)
    bad[528 + 32 * 14] ^= 1                      # z_eval (the same byte tests/test_degenerate_host.py changes)
    return bytes(bad)


def check_diagnosis(d, want, n):
    assert d.ok == (not want)
    assert d.rows == want
    assert d.info == DR.info(want, n)


def build_provers(ctx, circuit, want_vk, domain, wire_commit):
    """the two provers of one configuration, each checked for the mode it was built in and for its VerifierKey"""
    import plonk_amd
    n = circuit.n
    configure(ctx, quotient_domain=domain, wire_commit=wire_commit)
    idx, values = D.witness_form(circuit)
    created = plonk_amd.Prover(ctx, circuit.constraints, D.LABEL, D.polys(circuit))
    compiled = plonk_amd.Prover.compile(ctx, D.LABEL, {k: C.fr_bytes(v) for k, v in circuit.selectors.items()}, idx, len(values))
    for gp in (created, compiled):
        info = gp.describe()
        assert gp.size == n == info["size"]
        assert info["quotient_domain"] == (domain if n >= 8 else 8)      # below 8 rows the 4n de-aliasing does not apply
        assert info["wire_commit_values"] == (1 if wire_commit == 0 else 0)
        assert gp.vk_commitments() == want_vk
    return created, compiled, values


def run_case(ctx, name):
    import plonk_amd
    case = D.by_name(name)
    circuit = case.honest if case.expect == "unsat" else case
    n = case.n
    want = D.oracle(circuit.name)
    assert D.oracle(name)["proofs"] == ({"random": "unsat", "zero": "unsat"} if case.expect == "unsat" else want["proofs"])
    srs = D.srs(n)
    ctx.srs_load_bytes(srs, len(srs) // 96)
    rows = type("Rows", (), {"constraints": D.gates(case), "public_inputs": case.pi})()
    report = DR.report(rows, n, case.wires, pi=case.pi, sigma=case.sigma)
    assert report == ([(case.changed_row, 1, 0)] if case.expect == "unsat" else [])
    raw = D.wire_bytes(case)
    honest_raw = D.wire_bytes(circuit)
    pis = [case.pi[i] for i in case.pi_idx]
    wbuf = ctx.alloc(4 * 32 * n)

    def resident(cols):
        for k in range(4):
            wbuf.upload(cols[k], 32 * n * k)
        return wbuf.ptr

    for domain, wire_commit in CONFIGS:
        created, compiled, honest_values = build_provers(ctx, circuit, want["vk"], domain, wire_commit)
        values = D.unsat_witness_form(case)[1] if case.expect == "unsat" else honest_values
        # ---- diagnosis through the three entry points
        check_diagnosis(created.diagnose(raw, case.pi, cap=n), report, n)
        check_diagnosis(created.diagnose_dev(resident(raw), case.pi, cap=n), report, n)
        check_diagnosis(compiled.diagnose_witnesses(values, case.pi, cap=n), report, n)
        if case.expect == "unsat":
            for kind, bl in D.BLINDERS.items():
                with pytest.raises(plonk_amd.CircuitUnsatisfied):
                    created.prove(case.wires, case.pi, bl)
                with pytest.raises(plonk_amd.CircuitUnsatisfied):
                    created.prove_dev(resident(raw), case.pi, C.fr_bytes(bl))
                with pytest.raises(plonk_amd.CircuitUnsatisfied):
                    compiled.prove_witnesses(values, case.pi, bl)
        # ---- the three proving entry points, both blinder sets (unsat: the same provers on the honest assignment, afterwards)
        for kind, bl in D.BLINDERS.items():
            expected = want["proofs"][kind]
            assert created.prove(circuit.wires, circuit.pi, bl) == expected, (kind, domain, wire_commit)
            assert created.prove_dev(resident(honest_raw), circuit.pi, C.fr_bytes(bl)) == expected, (kind, domain, wire_commit)
            assert compiled.prove_witnesses(honest_values, circuit.pi, bl) == expected, (kind, domain, wire_commit)
        # ---- verification on the device: honest proofs with identity commitments, under a key that may hold some
        v = plonk_amd.Verifier(ctx, created.verifier_to_bytes(opening_key(), case.pi_idx))
        good = [want["proofs"]["random"], want["proofs"]["zero"]]
        for proof in good:
            assert v.verify(proof, pis)
            assert not v.verify(tampered(proof), pis)
        assert v.verify_batch(good + [tampered(good[1])], [pis] * 3) == [OK, OK, ERR_VERIFY]
        v.close()
        created.close()
        compiled.close()
    wbuf.free()
    _ran.add(name)


@pytest.mark.parametrize("name", D.small_names())
def test_small_domains(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", D.large_names())
def test_scan_and_batch_inverse_over_several_workgroups(ctx, name):
    """n = 4096: the 4n domain of 2^14 spans several workgroups of the product scan and of batch_inverse"""
    run_case(ctx, name)


def test_every_case_of_the_corpus_ran():
    """(runs after the parametrised tests above: same module, definition order)"""
    assert len(_ran) == len(D.corpus()) == 52


def test_malformed_identity_encodings_are_refused(ctx):
    """The reference decodes every commitment of a Proof and of a VerifierKey with G1Affine::from_slice
    (commitment_scheme/kzg10/commitment.rs:52-55; widget.rs:113-134): the identity is the compression and the infinity flag
    and nothing else (0xC0, then zeros — the tests above verify honest proofs and keys that hold it); an infinity flag with
    any other bit, or without the compression flag, is no point.  In a proof: that proof's verdict is PLONK_ERR_POINT and
    its neighbours in the batch keep theirs.  In a verifier blob: InvalidData."""
    import plonk_amd
    configure(ctx, quotient_domain=4, wire_commit=0)
    case = D.by_name("no-selectors-n8-c8")
    want = D.oracle(case.name)
    srs = D.srs(case.n)
    ctx.srs_load_bytes(srs, len(srs) // 96)
    gp = plonk_amd.Prover(ctx, case.constraints, D.LABEL, D.polys(case))
    blob = gp.verifier_to_bytes(opening_key(), [])
    gp.close()
    v = plonk_amd.Verifier(ctx, blob)
    proof = want["proofs"]["zero"]
    ident = bytes([0xC0]) + bytes(47)
    at = [k for k in range(11) if proof[48 * k:48 * k + 48] == ident]
    assert len(at) >= 4
    malformed = [bytes([0xC0]) + bytes(46) + b"\x01",       # infinity flag, x not zero
                 bytes([0xC0, 0x01]) + bytes(46),
                 bytes([0xE0]) + bytes(47),                 # infinity flag with the sign flag
                 bytes([0x40]) + bytes(47),                 # infinity flag without the compression flag
                 bytes([0xDF]) + bytes([0xFF]) * 47]        # infinity flag, every x bit set
    for enc in malformed:
        for k in (at[0], at[-1]):
            bad = proof[:48 * k] + enc + proof[48 * k + 48:]
            assert v.verify_batch([proof, bad, want["proofs"]["random"]], [[]] * 3) == [OK, ERR_POINT, OK], (enc[:2], k)
            assert not v.verify(bad, [])
    v.close()
    vk_off = 48 + len(D.LABEL) + 8
    assert blob[vk_off:vk_off + 48] == ident                # q_m of a circuit without selectors
    for enc in malformed:
        for j in (0, 10):
            bad = blob[:vk_off + 48 * j] + enc + blob[vk_off + 48 * j + 48:]
            with pytest.raises(plonk_amd.InvalidData):
                plonk_amd.Verifier(ctx, bad)
