"""CPU: the host half of mixed-circuit batch verification (plonk_verify_mixed).  tests/csrc/host_verify_mixed.cpp (g++)
drives verify_core.hpp's replay the way the replay kernel does — from a per-circuit POD and a pre-seeded transcript —
and must agree with verify_scalars; the proof digest, the verifier digest and rho are restated here with oracle/merlin.py;
a fold of three circuits with a naive MSM and one pairing accepts honest proofs and rejects every single-field tamper."""
import ctypes
import os
import subprocess

import pytest

from oracle import bls12_381 as E
from tests.test_verify_host import OracleCase, arithmetic_circuit, fr_mont, tampers

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhost_verify_mixed.so")
Q = E.Q
OK, REJECT, DATA = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_verify_mixed.cpp")
    csrc = os.path.join(HERE, "..", "plonk_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.hm_replay.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, vp, vp, vp, vp, vp]
    lib.hm_verifier_digest.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, vp]
    lib.hm_rho.argtypes = [vp, u64, ctypes.c_char_p, vp, ctypes.c_char_p, vp, u64, vp]
    lib.hm_fold.argtypes = [ctypes.c_uint32, ctypes.c_char_p, vp, vp, u64, vp, ctypes.c_char_p, ctypes.c_char_p]
    return lib


def pi_bytes(pis):
    return b"".join(fr_mont(v) for v in pis) or b"\0" * 32


def replay(lib, oc, proof, pis=None):
    """(core status, core scalars, digest, reference status, reference scalars)"""
    st_a, st_b = ctypes.c_int32(), ctypes.c_int32()
    sa, sb, dg = ctypes.create_string_buffer(896), ctypes.create_string_buffer(896), ctypes.create_string_buffer(32)
    rc = lib.hm_replay(oc.blob, len(oc.blob), oc.version, bytes(proof), pi_bytes(oc.pis if pis is None else pis),
                       ctypes.byref(st_a), sa, dg, ctypes.byref(st_b), sb)
    assert rc == 0
    return st_a.value, sa.raw, dg.raw, st_b.value, sb.raw


def cases():
    from tests import circuits as C
    return [("2^4, no public input", lambda: arithmetic_circuit(14, 21)),
            ("2^4, public input", lambda: C.big_widget_circuit(16, seed=22)()),
            ("2^8, public inputs", lambda: C.big_widget_circuit(256, seed=23)()),
            ("2^10, every widget, public inputs", lambda: C.big_widget_circuit(1 << 10, seed=24)())]


@pytest.mark.parametrize("version", [3, 2])
@pytest.mark.parametrize("name,build", cases(), ids=[n for n, _ in cases()])
def test_kernel_shaped_replay_equals_verify_scalars(lib, name, build, version):
    oc = OracleCase(build(), b"mixed-core", version)
    probes = [("honest", oc.proof, None)] + [(w, p, None) for w, p in tampers(oc.proof)]
    b = bytearray(oc.proof)
    b[528 + 32 * 3:560 + 32 * 3] = Q.to_bytes(32, "little")
    probes.append(("non-canonical", bytes(b), None))
    if oc.pis:
        probes.append(("wrong public input", oc.proof, [(oc.pis[0] + 1) % Q] + oc.pis[1:]))
    digests = set()
    for what, proof, pis in probes:
        st_a, sa, dg, st_b, sb = replay(lib, oc, proof, pis)
        assert st_a == st_b, what
        assert sa == sb, what
        if st_a == DATA:
            assert dg == bytes(32), what
        else:
            digests.add(dg)
    assert replay(lib, oc, oc.proof)[0] == OK
    assert replay(lib, oc, b)[0] == DATA
    assert len(digests) == len(probes) - 1                          # every tamper changes the proof digest


# ---- the three transcripts, restated with oracle/merlin.py ------------------------------------------------------------------
def py_proof_digest(oc, proof):
    """the replayed transcript (V3) up to u_challenge, then challenge_bytes("batch digest", 32)"""
    from oracle.plonk import seed_transcript_v3
    tr = seed_transcript_v3(oc.label, dict(oc.vk, n=oc.case["constraints"]), oc.case["constraints"])
    for v in oc.pis:
        tr.append_scalar(b"pi", v)
    cm = [proof[48 * i:48 * i + 48] for i in range(11)]
    ev = [int.from_bytes(proof[528 + 32 * i:560 + 32 * i], "little") for i in range(15)]
    for lab, i in ((b"a_comm", 0), (b"b_comm", 1), (b"c_comm", 2), (b"d_comm", 3)):
        tr.append_message(lab, cm[i])
    tr.append_scalar(b"beta", tr.challenge_scalar(b"beta"))
    tr.challenge_scalar(b"gamma")
    tr.append_message(b"z_comm", cm[4])
    for lab in (b"alpha", b"range separation challenge", b"logic separation challenge", b"fixed base separation challenge",
                b"variable base separation challenge"):
        tr.challenge_scalar(lab)
    for lab, i in ((b"t_low_comm", 5), (b"t_mid_comm", 6), (b"t_high_comm", 7), (b"t_fourth_comm", 8)):
        tr.append_message(lab, cm[i])
    tr.challenge_scalar(b"z_challenge")
    # Proof::to_bytes evaluation order: a b c d a_w b_w d_w q_arith q_c q_l q_r s1 s2 s3 z
    for lab, i in ((b"a_eval", 0), (b"b_eval", 1), (b"c_eval", 2), (b"d_eval", 3), (b"s_sigma_1_eval", 11),
                   (b"s_sigma_2_eval", 12), (b"s_sigma_3_eval", 13), (b"z_eval", 14), (b"a_w_eval", 4), (b"b_w_eval", 5),
                   (b"d_w_eval", 6), (b"q_arith_eval", 7), (b"q_c_eval", 8), (b"q_l_eval", 9), (b"q_r_eval", 10)):
        tr.append_scalar(lab, ev[i])
    tr.challenge_scalar(b"v_challenge")
    tr.challenge_scalar(b"v_w_challenge")
    tr.append_message(b"w_z_chall_comm", cm[9])
    tr.append_message(b"w_z_chall_w_comm", cm[10])
    tr.challenge_scalar(b"u_challenge")
    return tr.challenge_bytes(b"batch digest", 32)


def py_verifier_digest(oc, version):
    from oracle.merlin import Transcript
    blob, L = oc.blob, len(oc.label)
    vk = blob[48 + L + 8:48 + L + 8 + 15 * 48]                            # VerifierKey::to_bytes order
    ok = blob[48 + L + 968:48 + L + 968 + 240]
    tr = Transcript(b"plonk-verifier-digest-v1")
    tr.append_message(b"label", oc.label)
    tr.append_u64(b"version", version)
    tr.append_u64(b"size", oc.case["size"])
    tr.append_u64(b"constraints", oc.case["constraints"])
    for j in range(15):
        tr.append_message(b"vk", vk[48 * j:48 * j + 48])
    tr.append_message(b"opening key", ok)
    tr.append_u64(b"public inputs", len(oc.case["pi_idx"]))
    for i in oc.case["pi_idx"]:
        tr.append_u64(b"public input index", i)
    return tr.challenge_bytes(b"circuit digest", 32)


def py_rho(used, slot_digest, circuit, proof_digest, which):
    from oracle.merlin import Transcript
    tr = Transcript(b"plonk-batch-verify-mixed-v1")
    tr.append_u64(b"batch length", len(which))
    for s in used:
        tr.append_u64(b"slot", s)
        tr.append_message(b"circuit", slot_digest[s])
    for k in which:
        tr.append_u64(b"circuit", circuit[k])
        tr.append_message(b"proof", proof_digest[k])
    return tr.challenge_scalar(b"rho")


def test_digests_and_rho_match_their_restatement(lib):
    from tests import circuits as C
    a = OracleCase(C.big_widget_circuit(256, seed=31)(), b"digest-a", 3)
    b = OracleCase(arithmetic_circuit(14, 32), b"digest-b", 3)
    assert a.pis
    for oc in (a, b):
        for proof in (oc.proof, tampers(oc.proof)[3][1], tampers(oc.proof)[20][1]):
            assert replay(lib, oc, proof)[2] == py_proof_digest(oc, proof)
        for version in (3, 2):
            out = ctypes.create_string_buffer(32)
            assert lib.hm_verifier_digest(oc.blob, len(oc.blob), version, out) == 0
            assert out.raw == py_verifier_digest(oc, version)
    out2, out3 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    lib.hm_verifier_digest(a.blob, len(a.blob), 2, out2)
    lib.hm_verifier_digest(a.blob, len(a.blob), 3, out3)
    assert out2.raw != out3.raw                                           # the version is bound
    # rho over slots {0, 2} of three (slot 1 unused by this sub-batch) and four proofs, and over a sub-batch of two
    slot_digest = [bytes([s]) * 32 for s in range(3)]
    circuit = [2, 0, 2, 0]
    proof_digest = [bytes([0x40 + k]) * 32 for k in range(4)]
    for used, which in (([0, 2], [0, 1, 2, 3]), ([2], [0, 2]), ([0, 2], [1, 2])):
        u = (ctypes.c_uint32 * len(used))(*used)
        w = (ctypes.c_uint32 * len(which))(*which)
        out = ctypes.create_string_buffer(32)
        assert lib.hm_rho(u, len(used), b"".join(slot_digest), (ctypes.c_uint32 * 4)(*circuit), b"".join(proof_digest), w,
                          len(which), out) == 0
        assert int.from_bytes(out.raw, "little") == py_rho(used, slot_digest, circuit, proof_digest, which)


# ---- a fold of three circuits --------------------------------------------------------------------------------------------
def fold(lib, cases_, items):
    """items: [(slot, proof, pis)]"""
    blobs = b"".join(c.blob for c in cases_)
    lens = (ctypes.c_uint64 * len(cases_))(*[len(c.blob) for c in cases_])
    vers = (ctypes.c_int32 * len(cases_))(*[c.version for c in cases_])
    circ = (ctypes.c_uint32 * len(items))(*[s for s, _, _ in items])
    proofs = b"".join(bytes(p) for _, p, _ in items)
    pis = b"".join(fr_mont(v) for _, _, ps in items for v in ps) or b"\0" * 32
    return lib.hm_fold(len(cases_), blobs, lens, vers, len(items), circ, proofs, pis)


def test_fold_of_three_circuits_accepts_and_rejects_every_tamper(lib):
    from tests import circuits as C
    cs = [OracleCase(arithmetic_circuit(30, 41), b"fold-a", 3),
          OracleCase(C.big_widget_circuit(16, seed=42)(), b"fold-b", 2),
          OracleCase(C.big_widget_circuit(1 << 10, seed=43)(), b"fold-c", 3)]
    assert len({len(c.pis) for c in cs}) == 3 and len({c.case["size"] for c in cs}) == 3
    items = [(2, cs[2].proof, cs[2].pis), (0, cs[0].proof, cs[0].pis), (1, cs[1].proof, cs[1].pis)]
    assert fold(lib, cs, items) == 1
    assert fold(lib, cs, items[1:]) == 1                                   # slot 2 unused
    for i in range(len(items)):
        s, proof, pis = items[i]
        for what, bad in tampers(proof):
            t = list(items)
            t[i] = (s, bad, pis)
            assert fold(lib, cs, t) == 0, (i, what)
    # a proof filed under another circuit, and a wrong public input
    assert fold(lib, cs, [(1, cs[2].proof, cs[1].pis)] + items[1:]) == 0
    wrong = [(cs[2].pis[0] + 1) % Q] + cs[2].pis[1:]
    assert fold(lib, cs, [(2, cs[2].proof, wrong)] + items[1:]) == 0
