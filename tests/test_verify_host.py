"""CPU: the host half of proof verification — the pairing of plonk_amd/csrc/hostpairing.hpp against the independent
plain-Python one of tests/pairing_ref.py, its algebraic properties, and the barycentric evaluation of verify_core.hpp
(tests/csrc/host_verify.cpp, built with g++ like tests/csrc/host_arith.cpp)."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from oracle import bls12_381 as E

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import g2_ref as G2          # noqa: E402
import pairing_ref as PR     # noqa: E402

SO = os.path.join(HERE, "_build", "libhost_verify.so")
Q, P = E.Q, E.P


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_verify.cpp")
    csrc = os.path.join(HERE, "..", "plonk_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    lib.hv_multi_pairing.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p]
    lib.hv_pairing_pow_q_is_one.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.hv_parse.argtypes = [ctypes.c_char_p, ctypes.c_uint64]
    lib.hv_verify.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]
    lib.hv_barycentric.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.c_void_p, ctypes.c_void_p]
    return lib


def cpp_pairing(lib, pairs):
    out = (ctypes.c_uint64 * 72)()
    g1 = b"".join(E.g1_compress(p) for p, _ in pairs)
    g2 = b"".join(G2.g2_compress(q) for _, q in pairs)
    assert lib.hv_multi_pairing(len(pairs), g1, g2, out) == 0
    return [sum(int(out[6 * i + k]) << (64 * k) for k in range(6)) for i in range(12)]


def f12_is_one(c):
    return c == [1] + [0] * 11


def f12_tower_mul(lib_vals_a, lib_vals_b):
    return PR.f12_mul(PR.from_tower(lib_vals_a), PR.from_tower(lib_vals_b))


def test_pairing_equals_the_python_pairing(lib):
    rnd = random.Random(11)
    for _ in range(2):
        p = E.g1_mul(E.G1_GEN, rnd.randrange(1, Q))
        q = G2.g2_mul(G2.G2_GEN, rnd.randrange(1, Q))
        assert PR.from_tower(cpp_pairing(lib, [(p, q)])) == PR.pairing(p, q)


def test_bilinearity_and_non_degeneracy(lib):
    rnd = random.Random(12)
    a, b = rnd.randrange(1, Q), rnd.randrange(1, Q)
    e1 = cpp_pairing(lib, [(E.G1_GEN, G2.G2_GEN)])
    assert not f12_is_one(e1)                                              # non-degenerate
    eab = cpp_pairing(lib, [(E.g1_mul(E.G1_GEN, a), G2.g2_mul(G2.G2_GEN, b))])
    assert PR.from_tower(eab) == PR.f12_pow(PR.from_tower(e1), a * b % Q)   # e([a]P, [b]Q) = e(P, Q)^(ab)


def test_order_and_inverse(lib):
    p = E.g1_mul(E.G1_GEN, 0x1234567)
    assert lib.hv_pairing_pow_q_is_one(E.g1_compress(p), G2.g2_compress(G2.G2_GEN)) == 1   # e(P, Q)^q = 1
    neg = E.g1_mul(p, Q - 1)
    assert f12_is_one(cpp_pairing(lib, [(neg, G2.G2_GEN), (p, G2.G2_GEN)]))               # e(-P, Q) e(P, Q) = 1


def test_multi_miller_loop_is_the_product_of_pairings(lib):
    rnd = random.Random(13)
    pairs = [(E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)), G2.g2_mul(G2.G2_GEN, rnd.randrange(1, Q))) for _ in range(3)]
    prod = PR.ONE
    for pq in pairs:
        prod = PR.f12_mul(prod, PR.from_tower(cpp_pairing(lib, [pq])))
    assert PR.from_tower(cpp_pairing(lib, pairs)) == prod
    # the KZG shape of the verification equation: e(-[tau] W, h) e(W, [tau] h) = 1, and not for a wrong tau
    tau, w = rnd.randrange(1, Q), E.g1_mul(E.G1_GEN, rnd.randrange(1, Q))
    xh = G2.g2_mul(G2.G2_GEN, tau)
    assert f12_is_one(cpp_pairing(lib, [(E.g1_mul(w, Q - 1), xh), (E.g1_mul(w, tau), G2.G2_GEN)]))
    assert not f12_is_one(cpp_pairing(lib, [(E.g1_mul(w, Q - 1), xh), (E.g1_mul(w, tau + 1), G2.G2_GEN)]))
    # an identity on the G1 side contributes 1
    assert cpp_pairing(lib, [(None, xh), pairs[0]]) == cpp_pairing(lib, [pairs[0]])


def fr_mont(x):
    return (x * E.FR_R % Q).to_bytes(32, "little")


def fr_from_mont(buf):
    return int.from_bytes(bytes(buf), "little") * E.FR_RINV % Q


def bary(lib, n, pis, z):
    idx = (ctypes.c_uint64 * max(len(pis), 1))(*[i for i, _ in pis])
    vals = b"".join(fr_mont(v) for _, v in pis) or b"\0" * 32
    l1, pe = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    ok = lib.hv_barycentric(n, len(pis), idx, vals, fr_mont(z), l1, pe)
    return (fr_from_mont(l1.raw), fr_from_mont(pe.raw)) if ok else None


def test_barycentric_evaluation_and_its_edge_cases(lib):
    from oracle.fft import EvaluationDomain
    n = 16
    d = EvaluationDomain(n)
    pis = [(0, 5), (3, 7), (9, 0), (15, Q - 1)]
    z = 0x1234567890ABCDEF
    zh = (pow(z, n, Q) - 1) % Q
    want_l1 = zh * pow(n * (z - 1) % Q, -1, Q) % Q
    want_pi = sum(v * pow((pow(d.group_gen_inv, i, Q) * z - 1) % Q, -1, Q) for i, v in pis) % Q * zh % Q * d.size_inv % Q
    assert bary(lib, n, pis, z) == (want_l1, want_pi)
    assert bary(lib, n, [], z) == (want_l1, 0)
    assert bary(lib, n, pis, 1) is None                                    # z = 1: L1's denominator vanishes
    root = pow(d.group_gen, 3, Q)                                          # z = omega^3: the root of public input 3
    assert bary(lib, n, pis, root) is None
    assert bary(lib, n, pis, pow(d.group_gen, 9, Q)) is not None           # the root of a ZERO input is skipped


# ---- the verification core (verify_core.hpp + a naive host MSM) against oracle/verifier.py --------------------------------
TAU = 0x5EED0000 * 0x9E3779B97F4A7C15 % Q        # circuits.synthetic_srs's defaults
G_SCALAR = 0xA5A5A5A5DEADBEEF
OK, ERR_BYTES, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -8, -9, -10, -12


def opening_key():
    return (E.g1_compress(E.g1_mul(E.G1_GEN, G_SCALAR)) + G2.g2_compress(G2.G2_GEN)
            + G2.g2_compress(G2.g2_mul(G2.G2_GEN, TAU)))


def arithmetic_circuit(ngates, seed):
    """arithmetic gates only, no public input (the unused selectors commit to the identity)"""
    from oracle import plonk as O
    r = random.Random(seed)
    c = O.Composer()
    ws = [c.append_witness(r.randrange(Q)) for _ in range(4)]
    while len(c.constraints) < ngates:
        ws.append(c.gate_add(r.choice(ws), r.choice(ws), r.choice(ws), q_l=r.randrange(Q), q_r=r.randrange(Q), q_f=1,
                             q_c=r.randrange(Q)))
    return c


class OracleCase:
    """a circuit proved by the C oracle prover (oracle/c) and its Verifier::to_bytes blob"""

    def __init__(self, comp, label, version):
        from oracle import cbind
        from oracle.serialize import verifier_to_bytes
        from tests import circuits as C
        import plonk_amd
        self.case = C.compile_fast(comp, label)
        self.label, self.version = label, version
        srs = C.synthetic_srs(self.case["size"] + 7)
        cp = cbind.CProver(self.case["constraints"], label, self.case["polys"], srs)
        cp.set_version(version)
        raw = cp.vk()
        self.vk = {name: E.g1_decompress(raw[48 * k:48 * k + 48]) for k, name in enumerate(plonk_amd.POLY_ORDER)}
        self.proof = cp.prove(self.case["wires"], self.case["pi_idx"], self.case["pi_val"], C.blinders(len(label) + version))
        cp.close()
        self.pis = [self.case["pi"][i] for i in self.case["pi_idx"]]
        self.blob = verifier_to_bytes(label, dict(self.vk, n=self.case["constraints"]), opening_key(), self.case["pi_idx"],
                                      self.case["size"], self.case["constraints"])

    def host(self, lib, proof, pis=None, blob=None, version=None):
        pis = self.pis if pis is None else pis
        b = self.blob if blob is None else blob
        vals = b"".join(fr_mont(v) for v in pis) or b"\0" * 32
        return lib.hv_verify(b, len(b), self.version if version is None else version, proof, vals)

    def tau(self, proof, pis=None, label=None):
        from oracle.verifier import verify_with_tau
        pi = dict(zip(self.case["pi_idx"], self.pis if pis is None else pis))
        try:
            return verify_with_tau(proof, self.vk, label or self.label, self.case["constraints"], pi, TAU,
                                   E.g1_mul(E.G1_GEN, G_SCALAR))
        except AssertionError:   # parse_proof refuses a non-canonical scalar / a point off the curve
            return False


def tampers(proof):
    """every single-field tamper: each commitment replaced by another valid point, each evaluation + 1"""
    out = []
    for c in range(11):
        b = bytearray(proof)
        b[48 * c:48 * c + 48] = E.g1_compress(E.g1_mul(E.G1_GEN, 0xC0FFEE + c))
        out.append((f"commitment {c}", bytes(b)))
    for k in range(15):
        b = bytearray(proof)
        v = (int.from_bytes(b[528 + 32 * k:560 + 32 * k], "little") + 1) % Q
        b[528 + 32 * k:560 + 32 * k] = v.to_bytes(32, "little")
        out.append((f"evaluation {k}", bytes(b)))
    return out


def oracle_cases():
    from tests import circuits as C
    return [("2^4, no public input", lambda: arithmetic_circuit(14, 1)),
            ("2^4, public input", lambda: C.big_widget_circuit(16, seed=2)()),
            ("2^8, public inputs", lambda: C.big_widget_circuit(256, seed=3)()),
            ("2^12, every widget, public inputs", lambda: C.big_widget_circuit(1 << 12, seed=4)())]


@pytest.mark.parametrize("version", [3, 2])
@pytest.mark.parametrize("name,build", oracle_cases(), ids=[n for n, _ in oracle_cases()])
def test_host_core_matches_the_known_tau_verifier(lib, name, build, version):
    oc = OracleCase(build(), b"host-core", version)
    assert oc.host(lib, oc.proof) == OK
    assert oc.host(lib, oc.proof, version=5 - version) == ERR_VERIFY            # the other version's seeding
    if version == 3:
        assert oc.tau(oc.proof)
    for what, bad in tampers(oc.proof):
        got = oc.host(lib, bad)
        assert got == ERR_VERIFY, what
        if version == 3:
            assert not oc.tau(bad), what
    # a wrong label
    from oracle.serialize import verifier_to_bytes
    other = verifier_to_bytes(b"host-corf", dict(oc.vk, n=oc.case["constraints"]), opening_key(), oc.case["pi_idx"],
                              oc.case["size"], oc.case["constraints"])
    assert oc.host(lib, oc.proof, blob=other) == ERR_VERIFY
    if version == 3:
        assert not oc.tau(oc.proof, label=b"host-corf")
    # wrong public-input values
    if oc.pis:
        for i in range(len(oc.pis)):
            wrong = list(oc.pis)
            wrong[i] = (wrong[i] + 1) % Q
            assert oc.host(lib, oc.proof, pis=wrong) == ERR_VERIFY
            if version == 3:
                assert not oc.tau(oc.proof, wrong)
    # non-canonical scalar, point off the curve
    b = bytearray(oc.proof)
    b[528:560] = Q.to_bytes(32, "little")
    assert oc.host(lib, bytes(b)) == ERR_DATA
    b = bytearray(oc.proof)
    b[0:48] = bytes([0x80]) + (1).to_bytes(47, "big")                         # x = 1: 1 + 4 is not a square mod p
    assert oc.host(lib, bytes(b)) == ERR_POINT


# ---- Verifier::try_from_bytes on the host -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_case():
    return OracleCase(arithmetic_circuit(14, 9), b"blob", 3)


def parse(lib, blob):
    return lib.hv_parse(blob, len(blob))


def test_blob_parser_accepts_the_blob_and_refuses_truncations(lib, blob_case):
    blob = blob_case.blob
    assert parse(lib, blob) == OK
    for cut in (0, 8, 40, 47, 48, 60, len(blob) - 241, len(blob) - 1):
        assert parse(lib, blob[:cut]) == ERR_BYTES, cut


def set_be(blob, field, value):
    b = bytearray(blob)
    b[8 * field:8 * field + 8] = value.to_bytes(8, "big")
    return bytes(b)


def test_blob_parser_refuses_inconsistent_and_overflowing_lengths(lib, blob_case):
    blob = blob_case.blob
    assert parse(lib, set_be(blob, 0, len(blob))) == ERR_BYTES                  # label longer than the blob
    assert parse(lib, set_be(blob, 1, 100)) == ERR_BYTES                        # verifier key shorter than its 968 bytes
    assert parse(lib, set_be(blob, 2, 239)) in (ERR_BYTES, ERR_DATA)            # opening key shorter than 240 bytes
    assert parse(lib, set_be(blob, 3, 1)) == ERR_BYTES                          # one public-input index more than present
    assert parse(lib, set_be(blob, 3, 1 << 61)) == ERR_BYTES                    # 8 x count overflows
    assert parse(lib, set_be(blob, 0, (1 << 64) - 1)) == ERR_BYTES              # label + vk overflows
    assert parse(lib, set_be(blob, 4, 24)) == ERR_DATA                          # size not a power of two
    assert parse(lib, set_be(blob, 5, 15)) == ERR_DATA                          # constraints != vk.n


def opening_key_offset(case):
    return 48 + len(case.label) + 968


def with_bytes(blob, off, enc):
    b = bytearray(blob)
    b[off:off + len(enc)] = enc
    return bytes(b)


def test_blob_parser_refuses_bad_opening_keys(lib, blob_case):
    blob, off = blob_case.blob, opening_key_offset(blob_case)
    ident2 = bytes([0xC0]) + bytes(95)
    assert parse(lib, with_bytes(blob, off, E.g1_compress(None))) == ERR_DATA           # identity g
    assert parse(lib, with_bytes(blob, off + 48, ident2)) == ERR_DATA                   # identity h
    assert parse(lib, with_bytes(blob, off + 144, ident2)) == ERR_DATA                  # identity x_h
    noncanon = bytes([0x80 | (P >> 376)]) + (P % (1 << 376)).to_bytes(47, "big")        # x.c1 = p
    assert parse(lib, with_bytes(blob, off + 48, noncanon + bytes(48))) == ERR_DATA
    # an x whose x^3 + 4 (1 + u) is not a square in Fp2: off the twist
    x = 1
    while G2.f2_sqrt(G2.f2_add(G2.f2_mul(G2.f2_sqr((x, 0)), (x, 0)), G2.B2)) is not None:
        x += 1
    off_curve = bytes([0x80]) + bytes(47) + x.to_bytes(48, "big")
    assert parse(lib, with_bytes(blob, off + 48, off_curve)) == ERR_DATA
    # on the twist but outside the order-q subgroup
    x = 1
    while True:
        y = G2.f2_sqrt(G2.f2_add(G2.f2_mul(G2.f2_sqr((x, 0)), (x, 0)), G2.B2))
        if y is not None and G2.g2_mul((( x, 0), y), Q) is not None:
            break
        x += 1
    assert parse(lib, with_bytes(blob, off + 144, G2.g2_compress(((x, 0), y)))) == ERR_DATA
    assert parse(lib, with_bytes(blob, off + 48, b"\x00" + G2.g2_compress(G2.G2_GEN)[1:])) == ERR_DATA   # no compression flag
    # a verifier-key commitment off the curve
    assert parse(lib, with_bytes(blob, 48 + len(blob_case.label) + 8, bytes([0x80]) + (1).to_bytes(47, "big"))) == ERR_DATA
