"""Executable statement of what the kernels of plonk_amd/csrc/msm.hip that FOLLOW the bucket sort must write, given the arrays
tests/msm_sort_model.py says they read: slice partials, buckets, the row / column sums in `chunk`, and the bit sums.  Big
integers and numpy.  Not product code.

Every point a test handles is [k]G with k known (bookkeeping by scalars): a table point, a crafted bucket, and therefore every
sum of them.  An expected result is [sum of +-k mod Q]G — one fixed-base multiplication per compared point however many
buckets fed it (mul_g: 8-bit windows over a table of 32 x 255 multiples of G, built once).

The slot codec
  G1RSlot     4 coordinates (X, Y, ZZ, ZZZ) of 16 words: 14 limbs of 28 bits + 2 zero words, Montgomery radix 2^392, value
              x * 2^392 mod p + k p with k free inside the contract X < 16p, Y < 8p, ZZ, ZZZ < 2p; ZZ all zero = the identity
  G1AffineR   2 coordinates (x, y < 2p): a table entry of 128 bytes
  G1          4 coordinates of 12 words, radix 2^384, canonical: an output slot of 192 bytes

The membership sets of the reduction tail, bucket index b = 128 h + (l - 1) with weight b + 1 = 128 h + l, from the comments
of msm.hip and hostg1.hpp (finish_bit_sums):
  outputs     slots [0, rb): rows h with bit j of h set; [rb, rb + 7): columns of weight l < 128 with bit j of l set; rb + 7:
              C_128; rb + 8: S, every bucket (written for bit-position rows only).  rb = 8 over 2^15 buckets, 12 over 2^19.
  2^15        rcq: 256 R_h, then 2 x 128 half-columns C'[half][l] (rows 128 half .. 128 half + 127)   msm_rowcol_quad_kernel
              rc:  256 R_h, then 128 C_l                                                            msm_rowcol_kernel
  2^19        rc1: 4096 R_h, then 32 x 128 CP[p][l] (rows 128 p .. 128 p + 127)                     msm_rowcol_tp_kernel
              rc2: 256 G_g (rows 16 g .. 16 g + 15), 128 C_l, 128 identities, 256 P[sg][r] (rows h with h % 16 = r and
                   h // 256 = sg)                                                                   msm_fold_quad_kernel

and the launch rule of msm_batch_device_v restated (launch_rule): slice length, heavy threshold, lanes per bucket sum, dense
quad / list mode / direct writes, fused segment workers."""
import functools

import numpy as np

from arith_vectors import FP28_R, FP28_RINV, limbs28, value28
from oracle import bls12_381 as E

P, Q = E.P, E.Q
W = 16                              # entries per scalar at most (MSM_W)
HEAVY_SEG = 128                     # slices per segment of a heavy bucket
SLOT_WORDS, OUT_WORDS = 64, 48      # G1RSlot, G1 in 32-bit words
MAX_BATCH = 4
BIT_SUMS = 21                       # output slots per commitment (MSM_BIT_SUMS)
BOUNDS = (16, 8, 2, 2)              # the contract of a stored point: X < 16p, Y < 8p, ZZ < 2p, ZZZ < 2p


def rowbits(bits):
    return bits - 7


def fused_workers(bits):
    return 512 if bits > 15 else 128


# ---- [k]G ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g_table():
    rows, base = [], E.to_jac(E.G1_GEN)
    for _ in range(32):
        acc, row = E.JAC_ID, [None]
        for _ in range(255):
            acc = E.jac_add(acc, base)
            row.append(acc)
        rows.append([None] + [E.to_affine(p) for p in row[1:]])
        base = E.jac_add(row[255], base)
    return rows


def _madd(p, a):
    """Jacobian p + affine a (a never the identity): jac_add of the oracle with Z2 = 1"""
    X1, Y1, Z1 = p
    if Z1 == 0:
        return (a[0], a[1], 1)
    zz = Z1 * Z1 % P
    U2, S2 = a[0] * zz % P, a[1] * Z1 * zz % P
    if U2 == X1:
        return E.jac_add(p, (a[0], a[1], 1))
    H = (U2 - X1) % P
    I = 4 * H * H % P
    J = H * I % P
    r = 2 * (S2 - Y1) % P
    V = X1 * I % P
    X3 = (r * r - J - 2 * V) % P
    return X3, (r * (V - X3) - 2 * Y1 * J) % P, 2 * Z1 * H % P


_mul_memo = {}


def mul_g(k):
    """[k mod Q]G as a Jacobian triple (E.JAC_ID for 0)"""
    k %= Q
    got = _mul_memo.get(k)
    if got is None:
        got, t = E.JAC_ID, _g_table()
        for w in range(32):
            d = (k >> (8 * w)) & 255
            if d:
                got = _madd(got, t[w][d])
        if len(_mul_memo) < (1 << 17):
            _mul_memo[k] = got
    return got


def affine_g(k):
    return E.to_affine(mul_g(k))


# ---- the slot codec ---------------------------------------------------------------------------------------------------------
def coord28(v, mult=0):
    """the 16 words of a coordinate of value v (mod p) stored as v * 2^392 mod p + mult * p"""
    x = v % P * FP28_R % P + mult * P
    assert x < (1 << 392)
    return limbs28(x) + [0, 0]


IDENTITY_SLOT = coord28(1) + coord28(1) + [0] * 32          # G1R::identity(): X = Y = 1, ZZ = ZZZ = 0


def encode_slot(pt, z=1, mult=(0, 0, 0, 0)):
    """pt: affine (x, y) or None; the point as (x z^2, y z^3, z^2, z^3), every coordinate + mult[i] p"""
    if pt is None:
        return list(IDENTITY_SLOT)
    assert z % P and all(0 <= m < b for m, b in zip(mult, BOUNDS))
    zz, zzz = z * z % P, z * z * z % P
    return coord28(pt[0] * zz, mult[0]) + coord28(pt[1] * zzz, mult[1]) + coord28(zz, mult[2]) + coord28(zzz, mult[3])


def encode_affine(pt, mult=(0, 0)):
    """a table entry: x, y < 2p"""
    assert all(0 <= m < 2 for m in mult)
    return coord28(pt[0], mult[0]) + coord28(pt[1], mult[1])


def raw_coords(words):
    """the stored integers of the 4 (or 2) coordinates of a slot, limbs and pad words checked"""
    w = [int(x) for x in words]
    assert len(w) % 16 == 0
    out = []
    for c in range(len(w) // 16):
        ls = w[16 * c:16 * c + 14]
        assert all(x < (1 << 28) for x in ls), "a limb of coordinate %d has more than 28 bits: %s" % (c, [hex(x) for x in ls])
        assert w[16 * c + 14] == 0 and w[16 * c + 15] == 0, "the pad words of coordinate %d are not zero" % c
        out.append(value28(ls))
    return out


def decode_slot(words):
    """G1RSlot -> None (ZZ all zero) or (X, Y, ZZ, ZZZ) mod p out of Montgomery form, a point of the curve"""
    w = [int(x) for x in words]
    if not any(w[32:46]):
        return None
    X, Y, ZZ, ZZZ = (v * FP28_RINV % P for v in raw_coords(w))
    return _on_curve(X, Y, ZZ, ZZZ)


def _on_curve(X, Y, ZZ, ZZZ):
    assert ZZ and pow(ZZ, 3, P) == ZZZ * ZZZ % P, "ZZ^3 != ZZZ^2"
    assert (Y * Y - X * X * X - 4 * ZZZ * ZZZ) % P == 0, "Y^2 != X^3 + 4 ZZZ^2"
    return X, Y, ZZ, ZZZ


def decode_out(words):
    """G1 (48 words, radix 2^384, canonical) -> None or (X, Y, ZZ, ZZZ)"""
    w = [int(x) for x in words]
    v = [sum(w[12 * c + i] << (32 * i) for i in range(12)) for c in range(4)]
    assert all(x < P for x in v), "an output coordinate is not canonical"
    if v[2] == 0:
        return None
    return _on_curve(*(x * E.FP_RINV % P for x in v))


def same_point(xyzz, jac):
    """xyzz: a decoded slot; jac: a Jacobian triple of the oracle"""
    if xyzz is None or jac[2] == 0:
        return xyzz is None and jac[2] == 0
    X, Y, ZZ, ZZZ = xyzz
    Xe, Ye, Ze = jac
    z2 = Ze * Ze % P
    return (X * z2 - Xe * ZZ) % P == 0 and (Y * z2 * Ze - Ye * ZZZ) % P == 0


def to_affine(xyzz):
    if xyzz is None:
        return None
    X, Y, ZZ, ZZZ = xyzz
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


# ---- membership sets ----------------------------------------------------------------------------------------------------------
def set_ids(bits, name):
    """(ids, nsets): ids has one row per way a bucket belongs to the sums of `name`; ids[r][b] = the sum bucket b feeds in that
    way, or -1"""
    nb = 1 << bits
    b = np.arange(nb, dtype=np.int64)
    h, l0 = b >> 7, b & 127
    none = np.full(nb, -1, dtype=np.int64)
    if name == "rcq":
        assert bits == 15
        return [h, 256 + 128 * (h >> 7) + l0], 512
    if name == "rc":
        assert bits == 15
        return [h, 256 + l0], 384
    if name == "rc1":
        assert bits == 19
        return [h, 4096 + 128 * (h >> 7) + l0], 8192
    if name == "rc2":                                   # [384, 512) stay empty: the identities
        assert bits == 19
        return [h >> 4, 256 + l0, 512 + 16 * (h >> 8) + (h & 15)], 768
    assert name == "out"
    rb = rowbits(bits)
    ids = [np.where((h >> j) & 1, j, none) for j in range(rb)]
    ids += [np.where((((l0 + 1) >> j) & 1) & (l0 < 127), rb + j, none) for j in range(7)]
    ids += [np.where(l0 == 127, rb + 7, none), np.full(nb, rb + 8, dtype=np.int64)]
    return ids, rb + 9


def set_scalars(ids, nsets, idx, sgn, pool_k, weights=None):
    """bucket b holds sgn[b] * [pool_k[idx[b]]]G (idx[b] < 0: empty).  The scalar of every sum of (ids, nsets), by counting the
    pool members per sum (np.add.at) — one big-int product per (sum, member)"""
    full = np.nonzero(idx >= 0)[0]
    wt = sgn[full].astype(np.int64) * (1 if weights is None else weights[full])
    out = [0] * nsets
    k = np.array([int(x) for x in pool_k], dtype=object)
    counts = np.zeros((nsets, len(pool_k)), dtype=np.int64)
    for row in ids:
        s = row[full]
        keep = s >= 0
        np.add.at(counts, (s[keep], idx[full][keep]), wt[keep])
    tot = counts.astype(object).dot(k)
    return [int(t) % Q for t in tot]


def finish_scalar(u, rb, bitpos):
    """finish_bit_sums (hostg1.hpp) on scalars: u = the rb + 9 bit sums"""
    U = list(u[rb:rb + 7]) + [u[rb + 7] + u[0]] + list(u[1:rb])
    acc = U[6 + rb]
    for j in range(5 + rb, -1, -1):
        acc = 2 * acc + U[j]
    if bitpos:
        acc = 2 * acc - u[rb + 8]
    return acc % Q


# ---- the launch rule ----------------------------------------------------------------------------------------------------
class Rule:
    pass


def launch_rule(bits, mmax, ksl=0, order=-1, acc_lds=False, bsum_lane=False, tail_serial=False):
    """what msm_batch_device_v decides for a launch of at most mmax terms over 2^bits buckets under these switches"""
    nb = 1 << bits
    r = Rule()
    if ksl in (4, 8, 16, 32, 64, 128):
        r.ksl = ksl
    elif bits > 15:
        expect = 13 * mmax // nb
        r.ksl = 32 if expect <= 24 else (64 if expect <= 49 else 128)
    else:
        r.ksl = 4
        while r.ksl < 32 and r.ksl * nb < 3 * mmax:
            r.ksl *= 2
    r.avg = W * mmax // r.ksl // nb
    r.heavy_thresh = max(2 * r.avg, 16)
    acc_ordered = order == 1 if order >= 0 else r.ksl >= 16
    r.ordered = r.direct = acc_ordered and not acc_lds
    tail_quad = not tail_serial
    r.fused = fused_workers(bits) if (tail_quad or bits > 15) else 0
    r.list_mode = bits > 15 and r.ordered
    r.dense_quad = (not r.list_mode) and tail_quad and (not bsum_lane) and r.avg <= 8
    r.bsum = 1 if (r.dense_quad or r.avg <= 4) else (2 if r.avg <= 16 else (4 if r.avg <= 32 else 8))
    r.lanes = 4 if (r.dense_quad or r.list_mode) else r.bsum          # lanes that share a bucket
    r.empty = "zero" if r.list_mode else "identity"                   # what an empty bucket holds after phase 1
    return r


# ---- phase 1: partials and buckets from the sort model -----------------------------------------------------------------------
def entry_scalar(md, table_k, e):
    """the scalar of entry e (sign << 31 | table index) of the sort model md over a table whose entry t is [table_k[t]]G"""
    e = int(e)
    k = table_k[e & 0x7FFFFFFF]
    return (Q - k) % Q if e >> 31 else k


def bucket_scalars(md, table_k):
    """{bucket: scalar} of every non-empty bucket"""
    out = {}
    for b, e in zip(md.bucket_of.tolist(), md.entries.tolist()):
        out[b] = (out.get(b, 0) + entry_scalar(md, table_k, e)) % Q
    return out


# ---- the pool of the crafted bucket arrays ----------------------------------------------------------------------------------
NPOOL, NREP = 64, 4
_pool_rnd = __import__("random").Random(64)
POOL_K = [_pool_rnd.randrange(1, Q) for _ in range(NPOOL)]       # random 255-bit scalars


@functools.lru_cache(maxsize=None)
def pool_slots():
    """[sign][member][representation] -> the 64 words of a slot.  Representations: 0 affine (Z = 1), canonical; 1 a random Z,
    canonical; 2 a random Z, random admissible multiples of p; 3 a random Z, the largest admissible multiples (X + 15p, Y + 7p,
    ZZ + p, ZZZ + p).  Member NPOOL: the identity as G1R::identity(), as an all-zero slot (the sort's fill), with X, Y of a point
    left behind, and G1R::identity() again."""
    rnd = __import__("random").Random(65)
    out = np.zeros((2, NPOOL + 1, NREP, SLOT_WORDS), dtype=np.uint32)
    top = tuple(b - 1 for b in BOUNDS)
    for j, k in enumerate(POOL_K):
        for sign, kk in enumerate((k, Q - k)):
            pt = affine_g(kk)
            out[sign, j, 0] = encode_slot(pt)
            out[sign, j, 1] = encode_slot(pt, rnd.randrange(2, P))
            out[sign, j, 2] = encode_slot(pt, rnd.randrange(2, P), tuple(rnd.randrange(b) for b in BOUNDS))
            out[sign, j, 3] = encode_slot(pt, rnd.randrange(2, P), top)
    for sign in (0, 1):
        out[sign, NPOOL, 0] = IDENTITY_SLOT
        out[sign, NPOOL, 2] = coord28(rnd.randrange(P), 3) + coord28(rnd.randrange(P), 2) + [0] * 32
        out[sign, NPOOL, 3] = IDENTITY_SLOT
    return out


# ---- phase 1: the test-owned table and the designed inputs ---------------------------------------------------------------
import random as _random                                          # noqa: E402

import msm_sort_model as S                                        # noqa: E402

_table_rnd = _random.Random(24)
_half = [_table_rnd.randrange(1, Q) for _ in range(10)] + [1, 2]
TABLE_K = _half + [Q - k for k in _half]      # 24 multiples of G: every point has its opposite in the set, G and 2G are among them
NT = len(TABLE_K)


def table_choice(t):
    """(point, representation) of table entry t (numpy or int): a hash of the index, so that equal and opposite points sit at
    unrelated indices; representation bit 0: x + p, bit 1: y + p"""
    t = np.asarray(t, dtype=np.uint64)
    hsh = (t * np.uint64(0x9E3779B1) + (t >> np.uint64(7))) & np.uint64(0xFFFFFFFF)
    return (hsh >> np.uint64(8)) % np.uint64(NT), (hsh >> np.uint64(3)) & np.uint64(3)


class Table:
    """entry t holds TABLE_K[point] in representation rep, by table_choice unless `special` says otherwise"""

    def __init__(self, special=None):
        self.special = dict(special or {})

    def points(self, t):
        t = np.asarray(t, dtype=np.int64)
        j, rep = table_choice(t)
        j, rep = j.astype(np.int64), rep.astype(np.int64)
        for i, (pj, prep) in self.special.items():
            hit = t == i
            j[hit], rep[hit] = pj, prep
        return j, rep

    def entry_words(self, t):
        """(len(t), 32) uint32: the 128-byte entries"""
        j, rep = self.points(t)
        return _affine_words()[j, rep]


@functools.lru_cache(maxsize=None)
def _affine_words():
    out = np.zeros((NT, 4, 32), dtype=np.uint32)
    for j, k in enumerate(TABLE_K):
        pt = affine_g(k)
        for rep in range(4):
            out[j, rep] = encode_affine(pt, (rep & 1, rep >> 1))
    return out


def entry_terms(table, entries):
    """(point index, sign) per entry word"""
    e = np.asarray(entries, dtype=np.int64)
    j, _ = table.points(e & 0x7FFFFFFF)
    return j, np.where(e >> 31, -1, 1).astype(np.int64)


def sums_by(table, entries, ids, nsets):
    """the scalars of nsets sums over entries: ids = rows of (sum index per entry, or -1)"""
    j, sgn = entry_terms(table, entries)
    return set_scalars(ids, nsets, j, sgn, TABLE_K)


def chain_events(terms):
    """what one lane of msm_accumulate[_ordered]_kernel meets on the signed scalars `terms` of its slice, in order; returns
    (sum, events): 'pair' a first pair with equal x, 'double' acc = the next point, 'cancel+' acc = -next with the chain
    continuing from the identity, 'identity' a chain that ends in the identity"""
    ev, acc, i = set(), 0, 0
    terms = [t % Q for t in terms]
    if len(terms) >= 2:
        if terms[0] == terms[1] or (terms[0] + terms[1]) % Q == 0:
            ev.add("pair")
        else:
            acc, i = (terms[0] + terms[1]) % Q, 2
    for n in range(i, len(terms)):
        s = terms[n]
        if acc and acc == s and n > 0:
            ev.add("double")
        if acc and (acc + s) % Q == 0 and n + 1 < len(terms):
            ev.add("cancel+")
        acc = (acc + s) % Q
    if acc == 0:
        ev.add("identity")
    return acc, ev


def multi_scalar(bits, rows, bucket, n):
    """one scalar with n <= 10 digits, all in `bucket` (rows apart by one digit width), under the recoding of `rows` (the last two
    digits of a bit-position recoding share what is left of the 256 bits: no digit up there)"""
    assert 1 <= n <= 10
    if rows == S.ROWS_WINDOW:
        assert bits == 15 and bucket + 1 < (1 << 15)
        return (bucket + 1) * sum(1 << (16 * w) for w in range(n))
    if rows == S.ROWS_BITPOS:
        return (2 * bucket + 1) * sum(1 << ((bits + 2) * w) for w in range(n))
    assert rows == S.ROWS_QUARTERPOS and bucket + 1 < (1 << (bits - 1)) and (bucket + 1) & 15      # a digit starts at a non-zero nibble
    return (bucket + 1) * sum(1 << (S.digit_width(rows, bits) * w) for w in range(n))


def one_scalar(bits, rows, bucket):
    return multi_scalar(bits, rows, bucket, 1)


def slice_plan(bits, lanes, heavy_thresh, big):
    """{bucket: slices}: 1, 2, G - 1, G, G + 1, 2 G + 1 slices for the launch's G lanes per bucket, heavy_thresh and one more, 128,
    129 and 257 (one, two, three segments) — at the low end of the bucket range, where skewed digits put them, and at the high
    end; big: two buckets of 64 * 128 + 1 slices (65 segments each: the k += 64 loop of msm_heavy_bucket_quad_kernel, and with
    the others more segments than the 128 fused workers of the 2^15-bucket variant)"""
    nb = 1 << bits
    ns = [1, 2, max(lanes - 1, 1), lanes, lanes + 1, 2 * lanes + 1, heavy_thresh, heavy_thresh + 1, HEAVY_SEG, HEAVY_SEG + 1, 2 * HEAVY_SEG + 1]
    plan = {}
    for j, n in enumerate(ns):
        plan[j + 1 if j < 8 else j + 2] = n                # bucket 0 takes the carries of the negative digits, bucket 9 stays empty
        plan[nb // 2 - 2 - 16 * j] = n
    if big:
        plan[20] = plan[nb // 2 - 100] = 64 * HEAVY_SEG + 1
    return plan


CHAIN_FIRST = 3000                                          # buckets [CHAIN_FIRST, ...) hold the designed chains


def chain_plan(nrandom=40):
    """[(signed members of TABLE_K as (point, sign bit), ...)] per chain bucket: every slice of at most 4 entries"""
    r = _random.Random(5)
    out = [((0, 0), (0, 0)), ((0, 0), (0 + NT // 2, 0)), ((1, 0), (1, 1)), ((2, 0), (2, 0), (2, 0)), ((3, 0), (3, 1), (3, 0), (3, 1))]
    for _ in range(nrandom):                                # P, -P and a third point in the order the sort leaves them in
        p, o = r.randrange(NT), r.randrange(NT)
        out.append(tuple(r.sample([(p, 0), (p, 1) if r.random() < 0.5 else ((p + NT // 2) % NT, 0), (o, r.randrange(2))], 3)))
    for _ in range(nrandom // 2):                           # P, P and a third point
        p, o = r.randrange(NT), r.randrange(NT)
        out.append(tuple(r.sample([(p, 0), (p, 0), (o, 0)], 3)))
    return out


class Phase1Input:
    pass


def phase1_input(bits, rows, m, ksl, plan, seed, chains=40):
    """Sparse scalars of length m whose buckets hold plan[b] slices of ksl entries (the last slice partly filled), the chain
    buckets on top, and the table whose special entries make the chains"""
    r = _random.Random(seed)
    free = list(range(1, m - 1))
    r.shuffle(free)
    free = [0, m - 1] + free
    items, special, pos = {}, {}, 0
    inp = Phase1Input()
    inp.entries_of = {}
    for b, ns in sorted(plan.items()):
        n = (ns - 1) * ksl + 1 + (b % ksl)
        inp.entries_of[b] = n
        while n:
            take = min(n, 10) if rows == S.ROWS_WINDOW and b + 1 < (1 << 15) or rows != S.ROWS_WINDOW else 1
            items[free[pos]] = multi_scalar(bits, rows, b, take)
            pos += 1
            n -= take
    inp.chains = {}
    if chains:
        for c, members in enumerate(chain_plan(chains)):
            b = CHAIN_FIRST + 2 * c
            assert b not in plan
            inp.chains[b] = members
            inp.entries_of[b] = len(members)
            for pj, sign in members:
                i = free[pos]
                pos += 1
                s = one_scalar(bits, rows, b)
                if sign:                                    # 2^width - s: the digit -s in row 0 and a carry digit + 1, which falls into bucket 0
                    s = (1 << S.digit_width(rows, bits)) - s
                    inp.entries_of[0] = inp.entries_of.get(0, 0) + 1
                items[i] = s
                special[i] = (pj, r.randrange(4))
    assert pos <= m
    inp.scalars, inp.table, inp.m = S.Sparse(m, items), Table(special), m
    return inp


# (name, bits, rows, mmax, switches, big) — the launches of phase 1; ksl = 4 forced over 2^15 buckets
PHASE1_LAUNCHES = [
    ("dense quad", 15, 16, 300, dict(ksl=4), False),
    ("BSUM(1) by lanes", 15, 16, 300, dict(ksl=4, bsum_lane=1), False),
    ("BSUM(2)", 15, 16, 73728, dict(ksl=4), True),
    ("BSUM(4)", 15, 16, 139264, dict(ksl=4), False),
    ("BSUM(8)", 15, 16, 270336, dict(ksl=4), False),
    ("order 0", 15, 16, 300, dict(ksl=4, order=0), False),
    ("order 1", 15, 16, 300, dict(ksl=4, order=1), False),
    ("order 1, BSUM(2)", 15, 16, 73728, dict(ksl=4, order=1), False),
    ("acc_lds", 15, 16, 300, dict(ksl=4, acc_lds=1), False),
    ("acc_wg 64", 15, 16, 300, dict(ksl=4, order=1, acc_wg=64), False),
    ("tail_serial", 15, 16, 73728, dict(ksl=4, tail_serial=1), True),
    ("2^19 list mode", 19, 256, 6000, dict(), False),
    ("2^19 list mode, quarter rows", 19, 64, 6000, dict(), False),
    ("2^19 list mode, short slices, many segments", 19, 256, 60000, dict(ksl=4, order=1), True),
    ("2^19 dense quad", 19, 256, 300, dict(order=0, ksl=4), False),
]


def phase1_case(name):
    """(bits, rows, mmax, switches, rule, input) of a launch of PHASE1_LAUNCHES"""
    for i, (n, bits, rows, mmax, sw, big) in enumerate(PHASE1_LAUNCHES):
        if n == name:
            rule = launch_rule(bits, mmax, **{k: v for k, v in sw.items() if k in ("ksl", "order", "acc_lds", "bsum_lane", "tail_serial")})
            plan = slice_plan(bits, rule.lanes, rule.heavy_thresh, big)
            if bits == 19 and big:                          # more segments than the 512 fused workers: eight buckets of 65
                for j in range(6):
                    plan[40 + 5 * j] = 64 * HEAVY_SEG + 1
            if mmax == 300:                                 # what 300 scalars can hold
                plan = {b: ns for b, ns in plan.items() if ns <= HEAVY_SEG + 1 and b < 64}
            return bits, rows, mmax, sw, rule, phase1_input(bits, rows, mmax, rule.ksl, plan, 100 + i, chains=40 if mmax > 300 else 10)
    raise KeyError(name)
