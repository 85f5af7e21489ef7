"""Big-int model of what a KZG domain handle with Lagrange-basis tables adds (plonk_amd/csrc/kzg_evals_core.hpp
kze_tables_plan, kzg_evals_finish.cuh kze_finish_chain, g1codec.cuh g1r_compress48_words): the plan of the grouped table
launches of a call, and the finishing of a commitment from its bit sums — the Horner chain of hostg1.hpp finish_bit_sums on
POINTS, with the oracle's group law, and the 48-byte encoding.  tests/msm_tail_model.py::finish_scalar is the same chain on
scalars; the two are pinned to each other and to the oracle's compression by tests/test_kzg_evals_tables_host.py."""
from oracle import bls12_381 as E
from tests.msm_tail_model import finish_scalar

P, Q = E.P, E.Q
TABLE_GROUP = 4
FINISH_CHUNK = 4096
BIT_SUMS = 21
SLOT_BYTES = 192


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def plan(commitments, group_vectors, joined, separate):
    """commitments grouped inside groups of `group_vectors` vectors; `joined` MSMs in the same run, one launch each;
    `separate` MSMs a run of their own each"""
    run = joined
    first = 0
    while first < commitments:
        cnt = min(group_vectors, commitments - first)
        run += -(-cnt // TABLE_GROUP)
        first += cnt
    device = run > 1
    entries = commitments + joined
    chunks = []
    if device:
        left = entries
        while left:
            chunks.append(min(left, FINISH_CHUNK))
            left -= chunks[-1]
    return {"msms": commitments + joined + separate, "group_launches": run + separate, "device_finished": int(device),
            "finish_launches": len(chunks), "last_chunk": chunks[-1] if chunks else 0}


def evals_plan(group_vectors, count, commitments, witness):
    """an evaluation-form call: group_vectors is KzePlan::group_vectors (tests/kzg_evals_model.py plan)"""
    if not count:
        return plan(0, 1, 0, 0)
    return plan(count if commitments else 0, group_vectors, 1 if witness else 0, 0)


def multiproof_plan(computed):
    """a multiproof: `computed` commitments in one run, then D and pi on their own"""
    return plan(computed, max(computed, 1), 0, 2)


# ---- the chain on points ----------------------------------------------------------------------------------------------------
def finish_point(u, rb, bitpos):
    """u: rb + 9 affine points (None: the identity) -> the commitment, an affine point or None"""
    U = list(u[rb:rb + 7]) + [E.g1_add(u[rb + 7], u[0])] + list(u[1:rb])
    acc = E.to_jac(U[6 + rb])
    for j in range(5 + rb, -1, -1):
        acc = E.jac_add(E.jac_double(acc), E.to_jac(U[j]))
    if bitpos:
        acc = E.jac_add(E.jac_double(acc), E.jac_neg(E.to_jac(u[rb + 8])))
    return E.to_affine(acc)


def compress48(pt):
    """G1Affine::to_bytes as the device writes it: twelve 32-bit words, word k the byte-swapped word 11 - k of x, the flags in
    the low byte of word 0"""
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    x, y = pt
    words = [(x >> (32 * k)) & 0xFFFFFFFF for k in range(12)]
    out = bytearray()
    for k in range(12):
        out += int.from_bytes(words[11 - k].to_bytes(4, "little"), "big").to_bytes(4, "little")
    out[0] |= 0x80 | (0x20 if y > P >> 1 else 0)
    return bytes(out)


def finish_bytes_of_scalars(k, rb, bitpos, g=E.G1_GEN):
    """the 48 bytes for bit sums [k_j] g: one multiplication by the scalar chain's result"""
    s = finish_scalar(list(k), rb, bitpos)
    return compress48(E.g1_mul(g, s))


# ---- bit sums as the device holds them ---------------------------------------------------------------------------------------
def fp_mont48(a):
    return (a * E.FP_R % P).to_bytes(48, "little")


def slot_bytes(pt, z=1):
    """an XYZZ slot (X, Y, ZZ, ZZZ: canonical Montgomery, 48 bytes each) of the affine point pt scaled by z: X = x z^2,
    Y = y z^3, ZZ = z^2, ZZZ = z^3; None: the identity as G1::identity() writes it"""
    if pt is None:
        return fp_mont48(1) * 2 + bytes(96)
    z2, z3 = z * z % P, z * z * z % P
    return fp_mont48(pt[0] * z2 % P) + fp_mont48(pt[1] * z3 % P) + fp_mont48(z2) + fp_mont48(z3)


def commitment_bytes(points, rb, zs=None, filler=0xEE):
    """the BIT_SUMS slots of one commitment: rb + 9 of them from `points`, the rest filler bytes no chain may read"""
    assert len(points) == rb + 9
    out = b"".join(slot_bytes(p, zs[i] if zs else 1) for i, p in enumerate(points))
    return out + bytes([filler]) * (SLOT_BYTES * (BIT_SUMS - rb - 9))


# ---- operand families -------------------------------------------------------------------------------------------------------
def u_index(rb, j):
    """the slot that is U_j of the Horner chain, j = 0 .. 6 + rb (U_7 is slot rb + 7 plus slot 0: this returns rb + 7)"""
    return rb + j if j <= 7 else j - 7


def special_scalars(rb, bitpos):
    """name -> the rb + 9 scalars of bit sums [k_j] G that walk the chain through its branches"""
    top = 6 + rb
    zero = [0] * (rb + 9)

    def put(**at):
        k = list(zero)
        for j, v in at.items():
            k[u_index(rb, int(j[1:]))] = v % Q
        return k
    fam = {
        "all identity": list(zero),
        "one slot": put(**{"U%d" % top: 5}),
        "only the lowest": put(U0=3),
        "doubling: 2 acc == addend": put(**{"U%d" % top: 1, "U%d" % (top - 1): 2, "U3": 9}),
        "opposite: 2 acc == -addend": put(**{"U%d" % top: 1, "U%d" % (top - 1): -2, "U2": 7}),
        "opposite then identity addends": put(**{"U%d" % top: 3, "U%d" % (top - 1): -6}),
        "C_128 and T_0 equal": None, "C_128 and T_0 opposite": None,
    }
    k = list(zero)
    k[rb + 7], k[0], k[rb] = 11, 11, 1
    fam["C_128 and T_0 equal"] = k
    k = list(zero)
    k[rb + 7], k[0], k[rb + 1] = 11, Q - 11, 4
    fam["C_128 and T_0 opposite"] = k
    if bitpos:
        w = put(U0=5)
        k = list(w)
        k[rb + 8] = 10                      # S == 2 W: the identity
        fam["S == 2 W"] = k
        k = list(w)
        k[rb + 8] = Q - 10                  # -S == 2 W: the doubling branch of the last step
        fam["S == -2 W"] = k
        k = list(zero)
        k[rb + 8] = 6                       # W the identity
        fam["only S"] = k
    return fam
