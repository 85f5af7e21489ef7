"""CPU: the host-callable half of the KZG10 opening checks — plonk_amd/csrc/kzg_core.hpp (the batch challenge, the 3K + 1
terms of OpeningKey::batch_check, the scalars of AggregateProof::flatten, the challenge of plonk_srs_check) compiled with g++
(tests/csrc/host_kzg.cpp, like tests/csrc/host_verify.cpp) against the plain-Python yardstick tests/kzg_ref.py; a whole
batch check through the host core with a naive MSM and the host pairing; the layout of plonk_kzg_proof."""
import ctypes
import os
import random
import subprocess

import pytest

import plonk_amd
from oracle import bls12_381 as E
from oracle.merlin import Transcript
from tests import kzg_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_kzg.so")
Q = E.Q
OK, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -9, -10, -12


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_kzg.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.hk_proof_size.restype = u64
    lib.hk_batch_challenge.argtypes = [ctypes.c_char_p, u64, vp, vp, u64, vp]
    lib.hk_batch_terms.argtypes = [vp, vp, vp, u64, vp, vp]
    lib.hk_batch_check.argtypes = [vp, vp, vp, u64, ctypes.c_char_p, u64, vp]
    lib.hk_flatten_scalars.argtypes = [vp, vp, u64, vp, vp]
    lib.hk_srs_challenge.argtypes = [vp, u64, vp, vp]
    lib.hk_srs_challenge.restype = None
    lib.hk_opening_key_valid.argtypes = [vp]
    return lib


def mont(vals):
    return plonk_amd.fr_to_bytes_mont(vals)


def proof_array(proofs):
    """proofs: (commitment48, evaluation, witness48)"""
    return (plonk_amd.KzgProof * max(len(proofs), 1))(*[plonk_amd.KzgProof.make(c, e, w) for c, e, w in proofs])


def honest(rnd, count, points=None):
    """honest openings made in the exponent: ([c] g, e, [(c - e) / (tau - z)] g)"""
    points = points or [rnd.randrange(Q) for _ in range(count)]
    out = []
    for z in points:
        c, e = rnd.randrange(Q), rnd.randrange(Q)
        out.append((K.scalar_commit(c), e, K.scalar_commit((c - e) * pow((K.TAU - z) % Q, -1, Q) % Q)))
    return points, out


def host_u(lib, label, points, proofs):
    out = ctypes.create_string_buffer(32)
    assert lib.hk_batch_challenge(label, len(label), mont(points), proof_array(proofs), len(proofs), out) == 0
    return plonk_amd.fr_from_bytes_mont(out.raw)[0]


def test_proof_layout_matches_the_ctypes_mirror_and_a_c99_compile(lib, tmp_path):
    P = plonk_amd.KzgProof
    assert ctypes.sizeof(P) == 128 == lib.hk_proof_size()
    assert (P.commitment.offset, P.evaluation.offset, P.witness.offset) == (0, 48, 80)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "plonk_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(plonk_kzg_proof), offsetof(plonk_kzg_proof, commitment),\n'
                   '  offsetof(plonk_kzg_proof, evaluation), offsetof(plonk_kzg_proof, witness)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [128, 0, 48, 80]
    p = P.make(K.scalar_commit(3), 12345, K.IDENTITY48)
    assert p.value == 12345 and bytes(p.commitment) == K.scalar_commit(3) and bytes(p.witness) == K.IDENTITY48


@pytest.mark.parametrize("label,count", [(b"", 1), (b"", 2), (b"kzg", 5), (b"a much longer label for the transcript " * 5, 33)])
def test_batch_challenge_equals_the_merlin_restatement(lib, label, count):
    rnd = random.Random(len(label) + count)
    points, proofs = honest(rnd, count)
    assert host_u(lib, label, points, proofs) == K.batch_challenge(Transcript(label), points, proofs)


def test_batch_challenge_binds_every_input(lib):
    """the reference's binding test: the point, either commitment, the evaluation or the batch length changes u"""
    rnd = random.Random(2)
    points, proofs = honest(rnd, 3)
    base = host_u(lib, b"bind", points, proofs)
    assert base == K.batch_challenge(Transcript(b"bind"), points, proofs)
    other = K.scalar_commit(rnd.randrange(Q))
    c, e, w = proofs[1]
    variants = [([points[0], (points[1] + 1) % Q, points[2]], proofs),
                (points, [proofs[0], (other, e, w), proofs[2]]),
                (points, [proofs[0], (c, (e + 1) % Q, w), proofs[2]]),
                (points, [proofs[0], (c, e, other), proofs[2]]),
                (points[:2], proofs[:2]),
                (points + [points[0]], proofs + [proofs[0]])]
    seen = {base}
    for pts, prs in variants:
        u = host_u(lib, b"bind", pts, prs)
        assert u == K.batch_challenge(Transcript(b"bind"), pts, prs)
        assert u not in seen
        seen.add(u)
    assert host_u(lib, b"bind2", points, proofs) not in seen


@pytest.mark.parametrize("count", [1, 2, 7])
def test_terms_equal_a_naive_sum_with_the_python_group_law(lib, count):
    rnd = random.Random(30 + count)
    points, proofs = honest(rnd, count)
    u = rnd.randrange(Q)
    n = 3 * count + 1
    sc, ids = (ctypes.c_uint32 * (8 * n))(), (ctypes.c_uint32 * n)()
    assert lib.hk_batch_terms(mont([u]), mont(points), proof_array(proofs), count, sc, ids) == 0
    got = [(int.from_bytes(bytes(sc)[32 * t:32 * t + 32], "little"), ids[t]) for t in range(n)]
    tw, tc = K.batch_terms(u, points, proofs)
    assert got[:count] == tw and got[count:] == tc
    # and the sums are what key.rs:681-692 accumulates, term by term
    table = [K.g_point()]
    for c, _, w in proofs:
        table += [E.g1_decompress(c), E.g1_decompress(w)]
    total_w = total_c = None
    gm, pw = 0, 1
    for z, (c, e, w) in zip(points, proofs):
        cp, wp = E.g1_decompress(c), E.g1_decompress(w)
        item = E.g1_add(cp, E.g1_mul(wp, z))
        total_c = E.g1_add(total_c, E.g1_mul(item, pw))
        total_w = E.g1_add(total_w, E.g1_mul(wp, pw))
        gm = (gm + pw * e) % Q
        pw = pw * u % Q
    total_c = E.g1_add(total_c, E.g1_mul(K.g_point(), (-gm) % Q))
    assert K.group_sum(got[:count], table) == total_w and K.group_sum(got[count:], table) == total_c


def test_valid_and_tampered_batches_through_the_host_core(lib):
    rnd = random.Random(4)
    ok_key = K.opening_key()
    assert lib.hk_opening_key_valid(ok_key) == 1
    assert lib.hk_opening_key_valid(K.IDENTITY48 + ok_key[48:]) == 0
    points, proofs = honest(rnd, 4, [rnd.randrange(Q), 0, 1, rnd.randrange(Q)])
    pts = mont(points)
    assert lib.hk_batch_check(ok_key, pts, proof_array(proofs), 4, b"t", 1, None) == OK
    assert K.batch_check(points, proofs, label=b"t")
    assert lib.hk_batch_check(ok_key, pts, proof_array(proofs[:1]), 1, b"", 0, None) == OK      # the reference's single check
    c, e, w = proofs[2]
    other = K.scalar_commit(77)
    for bad in ((c, (e + 1) % Q, w), (other, e, w), (c, e, other)):
        tampered = proofs[:2] + [bad] + proofs[3:]
        assert lib.hk_batch_check(ok_key, pts, proof_array(tampered), 4, b"t", 1, None) == ERR_VERIFY
    assert not K.batch_check(points, proofs[:2] + [(c, (e + 1) % Q, w)] + proofs[3:], label=b"t")
    assert lib.hk_batch_check(ok_key, mont([points[0], 5, points[2], points[3]]), proof_array(proofs), 4, b"t", 1, None) == ERR_VERIFY
    assert lib.hk_batch_check(K.opening_key(tau=K.TAU + 1), pts, proof_array(proofs), 4, b"t", 1, None) == ERR_VERIFY
    # a caller-supplied u; the identity as a commitment; count == 0; malformed input
    assert lib.hk_batch_check(ok_key, pts, proof_array(proofs), 4, b"", 0, mont([12345])) == OK
    zero = (K.IDENTITY48, 0, K.IDENTITY48)
    assert lib.hk_batch_check(ok_key, mont([9]), proof_array([zero]), 1, b"", 0, None) == OK
    assert lib.hk_batch_check(ok_key, pts, proof_array([]), 0, b"", 0, None) == ERR_VERIFY
    assert lib.hk_batch_check(ok_key, pts, proof_array(proofs), 4, b"", 0, (Q + 1).to_bytes(32, "little")) == ERR_DATA
    assert lib.hk_batch_check(ok_key, pts, proof_array([(bytes(48), e, w)] + proofs[1:]), 4, b"", 0, None) == ERR_POINT


def test_flatten_on_the_reference_case(lib):
    """proof.rs tests: commitments 2G, 3G, 5G, evaluations 11, 13, 17, v = 7"""
    comms = [E.g1_compress(E.g1_mul(E.G1_GEN, k)) for k in (2, 3, 5)]
    evals, v = [11, 13, 17], 7
    sc, e_out = (ctypes.c_uint32 * 24)(), ctypes.create_string_buffer(32)
    assert lib.hk_flatten_scalars(mont([v]), mont(evals), 3, sc, e_out) == 0
    powers = [int.from_bytes(bytes(sc)[32 * i:32 * i + 32], "little") for i in range(3)]
    assert powers == [1, 7, 49]
    e = plonk_amd.fr_from_bytes_mont(e_out.raw)[0]
    assert e == 11 + 7 * 13 + 49 * 17
    got_c, got_e, got_w = K.flatten(comms, evals, v, K.IDENTITY48)
    assert got_c == E.g1_compress(E.g1_mul(E.G1_GEN, 2 + 7 * 3 + 49 * 5)) and got_e == e and got_w == K.IDENTITY48


def test_srs_challenge_equals_the_restatement(lib):
    out = ctypes.create_string_buffer(32)
    for seed, n in ((bytes(32), 1), (bytes(range(32)), (1 << 20) + 7)):
        lib.hk_srs_challenge(seed, n, K.opening_key(), out)
        assert plonk_amd.fr_from_bytes_mont(out.raw)[0] == K.srs_challenge(seed, n, K.opening_key())
    lib.hk_srs_challenge(bytes(32), 2, K.opening_key(), out)
    assert plonk_amd.fr_from_bytes_mont(out.raw)[0] != K.srs_challenge(bytes(32), 1, K.opening_key())


def test_yardstick_closed_forms_agree_with_the_explicit_polynomial_arithmetic():
    """facts about the yardstick itself: the closed-form witness equals the commitment of the explicit Ruffini quotient"""
    rnd = random.Random(6)
    polys = [[rnd.randrange(Q) for _ in range(n)] for n in (4, 0, 6, 1)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    f = K.fold(polys, v)
    q = K.ruffini(f, z)
    # q (X - z) + f(z) == f
    back = [0] * len(f)
    for i, c in enumerate(q):
        back[i + 1] = (back[i + 1] + c) % Q
        back[i] = (back[i] - z * c) % Q
    back[0] = (back[0] + K.evaluate(f, z)) % Q
    assert back == f
    assert K.commit(q) == K.scalar_commit(K.witness_scalar(polys, z, v))
    assert K.ruffini([1, 2, 3], 0) == [2, 3] and K.ruffini([5], 9) == [] and K.ruffini([0, 0], 3) == []
