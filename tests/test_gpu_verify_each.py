"""GPU: every proof checked on its own in one pass (plonk_verify_each, plonk_amd.verify_each; verify.hip, pairing.hip).
Two circuits compiled from one SRS (versions 3 and 2), interleaved: the verdict vector equals the list of count == 1
plonk_verify codes whatever is wrong with a proof, an all-bad batch costs no more checks than it has proofs, every
PLONK_ERR_ARG case is refused, and the call leaves plonk_verify_mixed and the provers of the context as it found them."""
import ctypes
import random

import pytest

from oracle import bls12_381 as E
from tests import circuits as C
from tests.test_gpu_verify_mixed import Circ, opening_key, TAU
from tests.test_verify_host import arithmetic_circuit

pytestmark = pytest.mark.gpu
Q = E.Q
OK, ERR_ARG, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -9, -10, -12


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    srs = C.synthetic_srs(64)                       # one SRS for both circuits, loaded before either is compiled
    c.srs_load_bytes(srs, len(srs) // 96)
    yield c
    c.close()


@pytest.fixture(scope="module")
def circs(ctx):
    cs = {"b": Circ(ctx, arithmetic_circuit(14, 502), b"each-b"),                     # 2^4, no public input, V3
          "c": Circ(ctx, C.big_widget_circuit(16, seed=503)(), b"each-c", 2)}         # 2^4, 1 input, V2
    yield cs
    for c in cs.values():
        c.verifier.close()
        c.prover.close()


@pytest.fixture(scope="module")
def proofs(circs):
    return {k: [c.prove(8000 + 31 * i + ord(k)) for i in range(3)] for k, c in circs.items()}


_single = {}


def single(v, proof, pis):
    """the count == 1 plonk_verify code of this proof with its own verifier"""
    key = (id(v), proof, tuple(pis))
    if key not in _single:
        _single[key] = v.verify_batch([proof], [pis])[0]
    return _single[key]


def interleaved(circs, proofs, count):
    return [(circs["bc"[k % 2]].verifier, proofs["bc"[k % 2]][(k // 2) % 3], circs["bc"[k % 2]].pis) for k in range(count)]


def flipped(item, k=14):
    v, p, pis = item
    b = bytearray(p)
    b[528 + 32 * k:560 + 32 * k] = ((int.from_bytes(b[528 + 32 * k:560 + 32 * k], "little") + 1) % Q).to_bytes(32, "little")
    return v, bytes(b), pis


def swapped(item):
    v, p, pis = item
    return v, p[48:96] + p[0:48] + p[96:], pis


def wrong_input(item):
    v, p, pis = item
    assert pis
    return v, p, [(pis[0] + 1) % Q] + list(pis[1:])


def undecodable(item):
    v, p, pis = item
    return v, p[:96] + bytes([0x80]) + (1).to_bytes(47, "big") + p[144:], pis


def noncanonical(item):
    v, p, pis = item
    return v, p[:528 + 64] + Q.to_bytes(32, "little") + p[560 + 64:], pis


@pytest.mark.parametrize("count", [1, 5, 66])
def test_verdicts_equal_the_single_calls(circs, proofs, count):
    import plonk_amd
    items = interleaved(circs, proofs, count)
    verdicts, info = plonk_amd.verify_each_info(items)
    assert verdicts == [OK] * count == [single(*it) for it in items]
    assert info["proofs"] == count and info["pairing_checks"] == count and info["msm_terms"] == 29 * count and info["rejected"] == 0
    assert plonk_amd.verify_each(items) == verdicts
    # one bad proof of every kind, spread over the batch (at count == 1 one after the other)
    makers = [flipped, swapped, wrong_input, undecodable, noncanonical]
    want_codes = [ERR_VERIFY, ERR_VERIFY, ERR_VERIFY, ERR_POINT, ERR_DATA]
    if count == 1:
        for make, code in zip(makers, want_codes):
            it = make(interleaved(circs, proofs, 2)[1])                      # circuit c: it has a public input
            verdicts, info = plonk_amd.verify_each_info([it])
            assert verdicts == [code] == [single(*it)]
            assert info["rejected"] == 1 and info["pairing_checks"] <= 1
        return
    pos = [0, 4, 1, 3, 2] if count == 5 else [1, 63, 65, 0, 64]
    bad = list(items)
    for p, make in zip(pos, makers):
        if make is wrong_input:
            assert bad[p][0] is circs["c"].verifier
        bad[p] = make(bad[p])
    verdicts, info = plonk_amd.verify_each_info(bad)
    want = [single(*it) for it in bad]
    assert verdicts == want
    assert [want[p] for p in pos] == want_codes and sum(1 for w in want if w != OK) == 5
    assert info["rejected"] == 5 and info["pairing_checks"] <= count - 2 and info["msm_terms"] == 29 * info["pairing_checks"]


def test_an_all_bad_batch_costs_no_more_checks_than_proofs(circs, proofs):
    import plonk_amd
    items = [flipped(it, k % 15) for k, it in enumerate(interleaved(circs, proofs, 66))]
    verdicts, info = plonk_amd.verify_each_info(items)
    assert verdicts == [ERR_VERIFY] * 66
    assert info["pairing_checks"] <= 66 and info["rejected"] == 66          # bisection reports 131 checks here


def test_the_single_circuit_form(circs, proofs):
    c = circs["c"]
    ps = [proofs["c"][i % 3] for i in range(5)]
    assert c.verifier.verify_each(ps, [c.pis] * 5) == [OK] * 5
    ps[2] = flipped((None, ps[2], None))[1]
    pis = [c.pis] * 4 + [[(c.pis[0] + 5) % Q]]
    before = c.verifier.last()
    assert c.verifier.verify_each(ps, pis) == [OK, OK, ERR_VERIFY, OK, ERR_VERIFY]
    assert c.verifier.last() == before                                      # plonk_verifier_last is not written


def raw_call(lib, handles, circuit, proofs_blob, pi, pi_total, count, verdicts=True):
    hv = (ctypes.c_void_p * max(len(handles), 1))(*handles) if handles is not None else None
    cv = (ctypes.c_uint32 * max(len(circuit), 1))(*circuit) if circuit is not None else None
    out = (ctypes.c_int32 * max(count, 1))() if verdicts else None
    return lib.plonk_verify_each(hv, len(handles or []), cv, proofs_blob, pi, pi_total, count, out, None)


def test_argument_errors_are_refused(ctx, circs, proofs):
    import plonk_amd
    lib = ctx.lib
    b, c = circs["b"], circs["c"]
    pb, pc = proofs["b"][0], proofs["c"][0]
    pi_c = plonk_amd.fr_to_bytes_mont(c.pis)
    hs = [c.verifier.handle.value, b.verifier.handle.value]
    assert raw_call(lib, hs, [0, 1], pc + pb, pi_c, 1, 2) == OK
    assert raw_call(lib, hs, None, pc + pc, pi_c + pi_c, 2, 2) == OK          # circuit == NULL: all of verifiers[0]

    def refused(rc, text):
        assert rc == ERR_ARG
        assert text in (lib.plonk_last_error() or b"").decode()

    refused(raw_call(lib, None, [0], pc, pi_c, 1, 1), "NULL")
    refused(raw_call(lib, hs, [0], None, pi_c, 1, 1), "NULL")
    refused(raw_call(lib, hs, [0], pc, None, 1, 1), "NULL")
    refused(raw_call(lib, [hs[0], None], [0], pc, pi_c, 1, 1), "NULL verifier")
    refused(raw_call(lib, [], [0], pc, pi_c, 1, 1), "nverifiers == 0")
    refused(raw_call(lib, hs, [0], pc, pi_c, 1, 0), "count")
    refused(raw_call(lib, hs, None, pc, pi_c, 1, 0), "count")
    refused(raw_call(lib, hs, [0], pc, pi_c, 1, (1 << 24) + 1, verdicts=False), "count")
    refused(raw_call(lib, hs, None, pc, pi_c, 1, (1 << 24) + 1, verdicts=False), "count")
    refused(raw_call(lib, hs, [0], pc, pi_c, 1, 1, verdicts=False), "verdicts")     # there is no NULL form
    refused(raw_call(lib, hs, [0, 2], pc + pb, pi_c, 1, 2), "circuit[k] >= nverifiers")
    refused(raw_call(lib, hs, [0, 1], pc + pb, pi_c, 2, 2), "pi_total")
    refused(raw_call(lib, hs, None, pc + pc, pi_c, 1, 2), "pi_total")
    ctx2 = plonk_amd.Context(0)
    other = plonk_amd.Verifier(ctx2, b.blob)
    try:
        refused(raw_call(lib, [hs[0], other.handle.value], [0, 1], pc + pb, pi_c, 1, 2), "different contexts")
    finally:
        other.close()
        ctx2.close()
    tau2 = plonk_amd.Verifier(ctx, b.blob_with(ok=opening_key(TAU + 1)))
    try:
        refused(raw_call(lib, [hs[0], tau2.handle.value], [0, 1], pc + pb, pi_c, 1, 2), "opening keys")
        with pytest.raises(plonk_amd.PlonkError) as e:
            plonk_amd.verify_each([(c.verifier, pc, c.pis), (tau2, pb, [])])
        assert e.value.code == ERR_ARG
    finally:
        tau2.close()
    with pytest.raises(ValueError):
        plonk_amd.verify_each([])


def test_the_call_leaves_the_context_as_it_found_it(circs, proofs):
    import plonk_amd
    items = interleaved(circs, proofs, 12)
    items[5] = flipped(items[5])
    items[8] = undecodable(items[8])
    seed = 8888
    proof_before = circs["b"].prove(seed)
    mixed_before = plonk_amd.verify_mixed(items)
    verdicts = plonk_amd.verify_each(items)
    assert verdicts == mixed_before[0] and [k for k, v in enumerate(verdicts) if v != OK] == [5, 8]
    mixed_after = plonk_amd.verify_mixed(items)
    assert mixed_after[0] == mixed_before[0]
    for field in ("proofs", "msm_terms", "pairing_checks", "rejected"):
        assert mixed_after[1][field] == mixed_before[1][field]
    assert circs["b"].prove(seed) == proof_before
