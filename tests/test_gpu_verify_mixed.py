"""GPU: mixed-circuit batch verification (plonk_verify_mixed, plonk_amd.verify_mixed; verify.hip).  Proofs of several
circuits compiled from one SRS verify in one pairing check; every verdict equals plonk_verify on that proof alone and the
known-tau verifier of oracle/verifier.py; a proof filed under the wrong circuit, label, public-input indexes or version is
rejected alone; bisection finds exactly the bad proofs; the device replay equals the host harness
(tests/csrc/host_verify_mixed.cpp) bit for bit; every PLONK_ERR_ARG case is refused."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from oracle import bls12_381 as E
from oracle.serialize import verifier_to_bytes
from oracle.verifier import verify_with_tau
from tests import circuits as C
from tests.test_verify_host import arithmetic_circuit, tampers

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g2_ref as G2   # noqa: E402

pytestmark = pytest.mark.gpu
Q = E.Q
TAU = 0x5EED0000 * 0x9E3779B97F4A7C15 % Q          # circuits.synthetic_srs's defaults
G_SCALAR = 0xA5A5A5A5DEADBEEF
OK, ERR_ARG, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -9, -10, -12
HERE = os.path.dirname(os.path.abspath(__file__))


def opening_key(tau=TAU):
    return (E.g1_compress(E.g1_mul(E.G1_GEN, G_SCALAR)) + G2.g2_compress(G2.G2_GEN)
            + G2.g2_compress(G2.g2_mul(G2.G2_GEN, tau)))


class Circ:
    """a circuit compiled on the GPU prover against the module's one SRS, and its verifier"""

    def __init__(self, ctx, comp, label, version=3):
        import plonk_amd
        case = C.compile_fast(comp, label)
        cols = C.circuit_columns(comp)
        self.prover = plonk_amd.Prover.compile(ctx, label, cols["selectors"], cols["wires"], cols["witnesses"])
        self.prover.set_version(version)
        self.values, self.case, self.label, self.version = cols["values"], case, label, version
        self.pi_idx = case["pi_idx"]
        self.pis = [case["pi"][i] for i in self.pi_idx]
        self.blob = self.prover.verifier_to_bytes(opening_key(), self.pi_idx)
        raw = self.prover.vk_commitments()
        self.vk = {name: E.g1_decompress(raw[48 * k:48 * k + 48]) for k, name in enumerate(plonk_amd.POLY_ORDER)}
        self.verifier = plonk_amd.Verifier(ctx, self.blob)
        self.verifier.set_version(version)

    def prove(self, seed):
        return self.prover.prove_witnesses(self.values, self.case["pi"], C.blinders(seed))

    def blob_with(self, label=None, pi_idx=None, ok=None):
        return verifier_to_bytes(label or self.label, dict(self.vk, n=self.case["constraints"]), ok or opening_key(),
                                 self.pi_idx if pi_idx is None else pi_idx, self.case["size"], self.case["constraints"])

    def tau_ok(self, proof, label=None):
        try:
            return verify_with_tau(proof, self.vk, label or self.label, self.case["constraints"],
                                   dict(zip(self.pi_idx, self.pis)), TAU, E.g1_mul(E.G1_GEN, G_SCALAR))
        except AssertionError:
            return False

    def single(self, proof):   # plonk_verify on this proof alone
        return self.verifier.verify_batch([proof], [self.pis])[0]


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    srs = C.synthetic_srs((1 << 12) + 7)            # one SRS for every circuit, loaded before any is compiled
    c.srs_load_bytes(srs, len(srs) // 96)
    yield c
    c.close()


@pytest.fixture(scope="module")
def circs(ctx):
    cs = {"a": Circ(ctx, C.big_widget_circuit(1 << 12, seed=501)(), b"mixed-a"),     # 2^12, every widget, 6 inputs
          "b": Circ(ctx, arithmetic_circuit(14, 502), b"mixed-b"),                    # 2^4, no public input
          "c": Circ(ctx, C.big_widget_circuit(16, seed=503)(), b"mixed-c", 2),        # 2^4, 1 input, V2
          "d": Circ(ctx, C.big_widget_circuit(1 << 10, seed=504)(), b"mixed-d")}      # 2^10, 6 inputs
    yield cs
    for c in cs.values():
        c.verifier.close()
        c.prover.close()


@pytest.fixture(scope="module")
def proofs(circs):
    return {k: [c.prove(7000 + 31 * i + ord(k)) for i in range(3)] for k, c in circs.items()}


def items_of(circs, proofs, order="abcd"):
    out = []
    for i in range(3):
        for k in order:
            out.append((circs[k].verifier, proofs[k][i], circs[k].pis))
    return out


def test_valid_mixed_batch_takes_one_check_and_is_order_free(circs, proofs):
    import plonk_amd
    assert len({len(c.pis) for c in circs.values()}) == 3 and circs["c"].version == 2
    items = items_of(circs, proofs)
    verdicts, info = plonk_amd.verify_mixed(items)
    assert verdicts == [OK] * 12
    assert info["pairing_checks"] == 1 and info["msm_terms"] == 13 * 12 + 15 * 4 + 1 and info["rejected"] == 0
    rnd = random.Random(5)
    for _ in range(2):
        shuffled = list(items)
        rnd.shuffle(shuffled)
        assert plonk_amd.verify_mixed(shuffled)[0] == [OK] * 12
    # two circuits only: C = 2
    verdicts, info = plonk_amd.verify_mixed([it for it in items if it[0] in (circs["b"].verifier, circs["d"].verifier)])
    assert verdicts == [OK] * 6 and info["msm_terms"] == 13 * 6 + 15 * 2 + 1
    # one proof: weight 1, the plonk_verify shape
    verdicts, info = plonk_amd.verify_mixed(items[:1])
    assert verdicts == [OK] and info["msm_terms"] == 13 + 15 + 1 and info["pairing_checks"] == 1


def test_tamper_sweep_matches_single_calls_and_the_known_tau_verifier(circs, proofs):
    import plonk_amd
    honest = items_of(circs, proofs)
    for key in ("d", "c"):
        c = circs[key]
        bad = [p for _, p in tampers(proofs[key][0])]
        b = bytearray(proofs[key][1])
        b[528:560] = Q.to_bytes(32, "little")
        bad.append(bytes(b))                                               # non-canonical: PLONK_ERR_DATA
        b = bytearray(proofs[key][2])
        b[0:48] = bytes([0x80]) + (1).to_bytes(47, "big")
        bad.append(bytes(b))                                               # off the curve: PLONK_ERR_POINT
        items = []
        for i, p in enumerate(bad):
            items.append((c.verifier, p, c.pis))
            items.append(honest[i % len(honest)])
        verdicts, info = plonk_amd.verify_mixed(items)
        want = []
        for v, p, _ in items:
            if v is c.verifier:
                want.append(c.single(p))
            else:
                want.append(OK)
        assert verdicts == want
        assert want[-4] == ERR_DATA and want[-2] == ERR_POINT and want[:52:2] == [ERR_VERIFY] * 26
        assert info["rejected"] == len(bad)
        if c.version == 3:
            assert not any(c.tau_ok(p) for p in bad[:26])


def test_cross_circuit_substitution_rejects_exactly_the_affected_proof(ctx, circs, proofs):
    import plonk_amd
    a, b, d = circs["a"], circs["b"], circs["d"]
    base = items_of(circs, proofs)
    # a valid proof of A filed under verifier B (with B's public inputs)
    items = list(base)
    items[4] = (b.verifier, proofs["a"][1], b.pis)
    verdicts, _ = plonk_amd.verify_mixed(items)
    assert [k for k, v in enumerate(verdicts) if v != OK] == [4]
    # equal VK, another label / other public-input indexes
    relabel = plonk_amd.Verifier(ctx, d.blob_with(label=b"mixed-e"))
    moved = plonk_amd.Verifier(ctx, d.blob_with(pi_idx=[(i + 1) % d.case["size"] for i in d.pi_idx]))
    try:
        for other in (relabel, moved):
            items = list(base)
            items[7] = (other, items[7][1], d.pis)
            assert items[7][1] in proofs["d"]
            verdicts, _ = plonk_amd.verify_mixed(items)
            assert [k for k, v in enumerate(verdicts) if v != OK] == [7]
        assert not d.tau_ok(proofs["d"][0], label=b"mixed-e")
    finally:
        relabel.close()
        moved.close()
    # the same circuit at V2 and V3 with the proofs swapped
    c = circs["c"]
    v3 = plonk_amd.Verifier(ctx, c.blob)
    try:
        c.prover.set_version(3)
        p3 = c.prove(9100)
        c.prover.set_version(2)
        p2 = c.prove(9101)
        ok_items = [(v3, p3, c.pis), (c.verifier, p2, c.pis)] + base[:4]
        assert plonk_amd.verify_mixed(ok_items)[0] == [OK] * 6
        swapped = [(v3, p2, c.pis), (c.verifier, p3, c.pis)] + base[:4]
        assert plonk_amd.verify_mixed(swapped)[0] == [ERR_VERIFY, ERR_VERIFY] + [OK] * 4
    finally:
        v3.close()


def test_bisection_finds_bad_proofs_in_different_circuits(circs, proofs):
    import plonk_amd
    pool = items_of(circs, proofs)
    items = [pool[k % len(pool)] for k in range(3000)]
    bad = [17, 1234, 2999]
    for k in bad:
        v, p, pis = items[k]
        b = bytearray(p)
        b[528 + 448:560 + 448] = ((int.from_bytes(b[528 + 448:560 + 448], "little") + 1) % Q).to_bytes(32, "little")
        items[k] = (v, bytes(b), pis)
    assert len({items[k][0] for k in bad}) == 3                              # three different circuits
    verdicts, info = plonk_amd.verify_mixed(items)
    assert [k for k, v in enumerate(verdicts) if v != OK] == bad
    assert all(verdicts[k] == ERR_VERIFY for k in bad)
    assert info["rejected"] == 3 and 1 < info["pairing_checks"] <= 1 + 2 * 3 * 12
    assert info["msm_terms"] == 13 * 3000 + 15 * 4 + 1


# ---- the device replay against the host harness ------------------------------------------------------------------------------
def host_lib():
    so = os.path.join(HERE, "_build", "libhost_verify_mixed.so")
    src = os.path.join(HERE, "csrc", "host_verify_mixed.cpp")
    csrc = os.path.join(HERE, "..", "plonk_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", so])
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.hm_replay.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, vp, vp, vp, vp, vp]
    return lib


def test_device_replay_equals_the_host_harness(ctx, circs, proofs):
    lib = host_lib()
    rnd = random.Random(9)
    items = []
    for k in range(288):
        key = "abcd"[k % 4]
        c = circs[key]
        p = proofs[key][k % 3]
        if k % 3 == 1:
            p = rnd.choice(tampers(p))[1]
        elif k % 17 == 0:
            b = bytearray(p)
            b[528 + 64:560 + 64] = Q.to_bytes(32, "little")
            p = bytes(b)
        items.append((c.verifier, p, c.pis))
    got = ctx._verify_replay(items)
    statuses = set()
    for (v, p, pis), (st, sc, dg) in zip(items, got):
        c = next(x for x in circs.values() if x.verifier is v)
        st_a, st_b = ctypes.c_int32(), ctypes.c_int32()
        sa, sb, hd = ctypes.create_string_buffer(896), ctypes.create_string_buffer(896), ctypes.create_string_buffer(32)
        vals = b"".join((x * E.FR_R % Q).to_bytes(32, "little") for x in pis) or b"\0" * 32
        assert lib.hm_replay(c.blob, len(c.blob), c.version, p, vals, ctypes.byref(st_a), sa, hd, ctypes.byref(st_b), sb) == 0
        assert st == st_a.value == st_b.value
        assert b"".join(sc) == sa.raw
        assert dg == hd.raw
        statuses.add(st)
    assert statuses == {0, 2}


# ---- argument errors -----------------------------------------------------------------------------------------------------
def raw_call(lib, handles, circuit, proofs_blob, pi, pi_total, count, verdicts=True):
    hv = (ctypes.c_void_p * max(len(handles), 1))(*handles) if handles is not None else None
    cv = (ctypes.c_uint32 * max(len(circuit), 1))(*circuit) if circuit is not None else None
    out = (ctypes.c_int32 * max(count, 1))() if verdicts else None
    return lib.plonk_verify_mixed(hv, len(handles or []), cv, proofs_blob, pi, pi_total, count, out, None)


def test_argument_errors_are_refused(ctx, circs, proofs):
    import plonk_amd
    lib = ctx.lib
    a, b = circs["a"], circs["b"]
    pa, pb = proofs["a"][0], proofs["b"][0]
    pi_a = plonk_amd.fr_to_bytes_mont(a.pis)
    hs = [a.verifier.handle.value, b.verifier.handle.value]
    assert raw_call(lib, hs, [0, 1], pa + pb, pi_a, len(a.pis), 2) == OK

    def refused(rc, text):
        assert rc == ERR_ARG
        assert text in (lib.plonk_last_error() or b"").decode()

    refused(raw_call(lib, None, [0], pa, pi_a, 6, 1), "NULL")
    refused(raw_call(lib, hs, None, pa, pi_a, 6, 1), "NULL")
    refused(raw_call(lib, hs, [0], None, pi_a, 6, 1), "NULL")
    refused(raw_call(lib, hs, [0], pa, None, 6, 1), "NULL")
    refused(raw_call(lib, [hs[0], None], [0], pa, pi_a, 6, 1), "NULL verifier")
    refused(raw_call(lib, [], [0], pa, pi_a, 6, 1), "nverifiers == 0")
    refused(raw_call(lib, hs, [0], pa, pi_a, 6, 0), "count")
    refused(raw_call(lib, hs, [0], pa, pi_a, 6, (1 << 24) + 1, verdicts=False), "count")
    refused(raw_call(lib, hs, [0, 1], pa + pb, pi_a, len(a.pis), 2, verdicts=False), "verdicts")
    refused(raw_call(lib, hs, [0, 2], pa + pb, pi_a, len(a.pis), 2), "circuit[k] >= nverifiers")
    refused(raw_call(lib, hs, [0, 1], pa + pb, pi_a, len(a.pis) + 1, 2), "pi_total")
    refused(raw_call(lib, hs, [1, 1], pa + pb, pi_a, len(a.pis), 2), "pi_total")
    # a verifier of another context, and an opening key with another tau
    ctx2 = plonk_amd.Context(0)
    other = plonk_amd.Verifier(ctx2, b.blob)
    try:
        refused(raw_call(lib, [hs[0], other.handle.value], [0, 1], pa + pb, pi_a, len(a.pis), 2), "different contexts")
    finally:
        other.close()
        ctx2.close()
    tau2 = plonk_amd.Verifier(ctx, b.blob_with(ok=opening_key(TAU + 1)))
    try:
        refused(raw_call(lib, [hs[0], tau2.handle.value], [0, 1], pa + pb, pi_a, len(a.pis), 2), "opening keys")
        with pytest.raises(plonk_amd.PlonkError) as e:
            plonk_amd.verify_mixed([(a.verifier, pa, a.pis), (tau2, pb, [])])
        assert e.value.code == ERR_ARG
    finally:
        tau2.close()
    with pytest.raises(ValueError):
        plonk_amd.verify_mixed([])
    # the same handle twice is two slots, and a verifier's own plonk_verifier_last is untouched
    before = a.verifier.last()
    assert raw_call(lib, [hs[0], hs[0]], [1, 0], pa + pa, pi_a + pi_a, 2 * len(a.pis), 2) == OK
    assert a.verifier.last() == before
