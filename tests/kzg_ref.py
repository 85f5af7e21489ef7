"""Plain-Python yardstick of the KZG10 opening layer (reference src/commitment_scheme/kzg10/key.rs:394-417, 571-591,
661-707; proof.rs:69-109), over oracle/bls12_381.py, oracle/merlin.py, tests/pairing_ref.py and tests/g2_ref.py.

With a KNOWN tau the commit key is [g tau^i] G, so commit(p) = [g p(tau)] G and the aggregate witness of f = sum v^i p_i at
z is [g (f(tau) - f(z)) / (tau - z)] G: expected bytes exist at any size without an MSM on the CPU.  (tau == z never
happens for the points the tests use; `witness_scalar` asserts it.)"""
import os
import sys

from oracle import bls12_381 as E
from oracle.merlin import Transcript

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g2_ref as G2        # noqa: E402
import pairing_ref as PR   # noqa: E402

Q = E.Q
TAU = 0x5EED0000 * 0x9E3779B97F4A7C15 % Q          # tests/circuits.synthetic_srs's defaults
G_SCALAR = 0xA5A5A5A5DEADBEEF
IDENTITY48 = bytes([0xC0]) + bytes(47)


def g_point(g=G_SCALAR):
    return E.g1_mul(E.G1_GEN, g)


def opening_key(tau=TAU, g=G_SCALAR) -> bytes:
    return E.g1_compress(g_point(g)) + G2.g2_compress(G2.G2_GEN) + G2.g2_compress(G2.g2_mul(G2.G2_GEN, tau))


def trimmed(p):
    n = len(p)
    while n and p[n - 1] % Q == 0:
        n -= 1
    return n


def evaluate(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % Q
    return acc


def scalar_commit(s, g=G_SCALAR) -> bytes:
    """48 bytes of [g s] G (the identity for s == 0)"""
    s = s * g % Q
    return E.g1_compress(E.g1_mul(E.G1_GEN, s)) if s else IDENTITY48


def commit(p, tau=TAU, g=G_SCALAR) -> bytes:
    return scalar_commit(evaluate(p, tau), g)


def fold(polys, v):
    """compute_aggregate_witness' sum: coefficients of sum_i v^i p_i (key.rs:403-414)"""
    out = [0] * max((len(p) for p in polys), default=0)
    w = 1
    for p in polys:
        for j, c in enumerate(p):
            out[j] = (out[j] + c * w) % Q
        w = w * v % Q
    return out


def ruffini(f, z):
    """Polynomial::ruffini: the quotient of f by (X - z), remainder dropped"""
    n = trimmed(f)
    if n <= 1:
        return []
    q = [0] * (n - 1)
    acc = 0
    for i in range(n - 1, 0, -1):
        acc = (acc * z + f[i]) % Q
        q[i - 1] = acc
    return q


def witness_scalar(polys, z, v, tau=TAU):
    """w(tau) for w = (f - f(z)) / (X - z), f = sum v^i p_i"""
    assert (tau - z) % Q, "the opening point equals tau"
    ft = fz = 0
    w = 1
    for p in polys:
        ft = (ft + w * evaluate(p, tau)) % Q
        fz = (fz + w * evaluate(p, z)) % Q
        w = w * v % Q
    return (ft - fz) * pow((tau - z) % Q, -1, Q) % Q


def open_expected(polys, z, v=1, tau=TAU, g=G_SCALAR):
    """(evaluations, commitments, witness) of plonk_kzg_open"""
    return ([evaluate(p, z) for p in polys], [commit(p, tau, g) for p in polys], scalar_commit(witness_scalar(polys, z, v, tau), g))


def batch_challenge(transcript, points, proofs):
    """key.rs:571-591; proofs: (commitment48, evaluation, witness48)"""
    transcript.append_message(b"dom-sep", b"kzg10-batch-check-v1")
    transcript.append_u64(b"batch-len", len(proofs))
    for z, (c, e, w) in zip(points, proofs):
        transcript.append_scalar(b"batch-point", z)
        transcript.append_message(b"batch-polynomial-commitment", bytes(c))
        transcript.append_scalar(b"batch-evaluation", e)
        transcript.append_message(b"batch-witness-commitment", bytes(w))
    return transcript.challenge_scalar(b"batch-challenge")


def batch_terms(u, points, proofs):
    """the 3K + 1 (scalar, point index) terms over the table [g | C_0 W_0 | C_1 W_1 ...]: K of total_w, then 2K + 1 of total_c"""
    K = len(proofs)
    tw, tc1, tc2 = [], [], []
    gm, w = 0, 1
    for k, (z, (_, e, _)) in enumerate(zip(points, proofs)):
        tw.append((w, 2 + 2 * k))
        tc1.append((w, 1 + 2 * k))
        tc2.append((w * z % Q, 2 + 2 * k))
        gm = (gm + w * e) % Q
        w = w * u % Q
    assert len(tw) == K
    return tw, tc1 + tc2 + [((-gm) % Q, 0)]


def group_sum(terms, table):
    acc = None
    for s, i in terms:
        if table[i] is not None and s % Q:
            acc = E.g1_add(acc, E.g1_mul(table[i], s % Q))
    return acc


def pairing_is_one(neg_left, right, h, x_h):
    """e(-neg_left, x_h) e(right, h) == 1 with tests/pairing_ref.py"""
    pairs = []
    if neg_left is not None:
        pairs.append(((neg_left[0], (-neg_left[1]) % E.P), x_h))
    if right is not None:
        pairs.append((right, h))
    return PR.multi_pairing(pairs) == PR.ONE


def batch_check(points, proofs, label=b"", u=None, tau=TAU, g=G_SCALAR):
    """OpeningKey::batch_check (key.rs:661-707) by the group law and the pairing of the test suite: slow, small batches only"""
    if not proofs or len(points) != len(proofs):
        return False
    if u is None:
        u = batch_challenge(Transcript(label), points, proofs)
    table = [g_point(g)]
    for c, _, w in proofs:
        table += [E.g1_decompress(bytes(c)), E.g1_decompress(bytes(w))]
    tw, tc = batch_terms(u, points, proofs)
    return pairing_is_one(group_sum(tw, table), group_sum(tc, table), G2.G2_GEN, G2.g2_mul(G2.G2_GEN, tau))


def batch_check_scalar(points, proofs_scalar, u, tau=TAU):
    """the same statement in the exponent, for proofs given as DISCRETE LOGS (c, e, w) to the base g: sum u^k (c_k + z_k w_k
    - e_k) == tau sum u^k w_k — what lets a test know the right answer at any batch size"""
    lhs = rhs = 0
    w = 1
    for z, (c, e, wt) in zip(points, proofs_scalar):
        lhs = (lhs + w * (c + z * wt - e)) % Q
        rhs = (rhs + w * wt) % Q
        w = w * u % Q
    return lhs == rhs * tau % Q


def flatten(commitments, evaluations, v, witness):
    """AggregateProof::flatten (proof.rs:69-109) -> (commitment48, evaluation, witness48)"""
    acc, e, w = None, 0, 1
    for c, ev in zip(commitments, evaluations):
        pt = E.g1_decompress(bytes(c))
        if pt is not None and w:
            acc = E.g1_add(acc, E.g1_mul(pt, w))
        e = (e + w * ev) % Q
        w = w * v % Q
    return (E.g1_compress(acc) if acc is not None else IDENTITY48), e, bytes(witness)


def srs_challenge(seed32: bytes, npoints: int, opening_key240: bytes) -> int:
    t = Transcript(b"plonk-srs-check-v1")
    t.append_message(b"seed", seed32)
    t.append_u64(b"points", npoints)
    t.append_message(b"opening key", opening_key240)
    return t.challenge_scalar(b"r")
