"""One set of arithmetic edge-case vectors for two back ends.

The operand lists and the expected values of every family of tests/csrc/arith_cases.hpp, built from oracle.bls12_381 and
Python integers only.  tests/test_field_host.py runs them through the g++ build of the product's __host__ __device__ headers
(h_case_<family>), tests/test_gpu_field_device.py through the hipcc build of the same bodies on the device (d_case_<family>).

A family is a list of cases in a fixed order: the packed input record, and either the exact output record or a predicate on
it (the raw Fp28 products promise a range and a residue, not a representative).  Cases are NOT grouped by kind: edge values
sit beside random ones, so that the lanes of one wave take different paths.

The pairing tower of pairing28.cuh (the last section) has a reference of its own, tests/pairing_tower_model.py, and two of
its routines read the 47 KB PairingTables28: a family may name one blob of bytes (`shared`) that the harness turns into a
read-only buffer once, before the cases run."""
import functools
import random
import struct

from oracle import bls12_381 as E

Q, P = E.Q, E.P
M28 = (1 << 28) - 1
FP28_R = 1 << 392                     # Fp28's Montgomery radix (14 x 28 bits)
FP28_RINV = pow(FP28_R, -1, P)

# ---- values -> limbs ----------------------------------------------------------------------------------------------------


def words(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def fr_mont(x):
    return words(x * E.FR_R % Q, 8)


def fp_mont(x):
    return words(x * E.FP_R % P, 12)


def point_words(pt):
    """affine x || y as 2 x 12 Montgomery limbs (the 96-byte raw form); None (the identity) -> zeros"""
    if pt is None:
        return [0] * 24
    return list(struct.unpack("<24I", E.g1_to_raw96(pt)))


def limbs28(v):
    return [(v >> (28 * i)) & M28 for i in range(14)]


def value28(ls):
    return sum(int(x) << (28 * i) for i, x in enumerate(ls))


# ---- operand classes ------------------------------------------------------------------------------------------------------


def edge_values(mod, rnd, n=60):
    vals = [0, 1, 2, mod - 1, mod - 2, (mod - 1) // 2, (1 << 32) - 1, 1 << 32, (1 << 255) % mod]
    return vals + [rnd.randrange(mod) for _ in range(n)]


# (limb width, limbs, Montgomery radix bits) of every representation a value of the field is computed in
FR_VIEWS = [(32, 8, 256), (29, 9, 261)]
FP_VIEWS = [(32, 12, 384), (28, 14, 392)]


def saturated_values(m, views):
    """values whose limbs are all saturated below the top one and that are still below the modulus, in each view: as the
    plain integer and as the value whose Montgomery representation in that view has those limbs"""
    out = []
    for width, limbs, rbits in views:
        k = width * (limbs - 1)
        pattern = (((m >> k) - 1) << k) | ((1 << k) - 1)
        assert pattern < m and all((pattern >> (width * i)) & ((1 << width) - 1) == (1 << width) - 1 for i in range(limbs - 1))
        out += [pattern, pattern * pow(1 << rbits, -1, m) % m]
    return out


def sum_edge_pairs(m, views, rnd):
    """a + b in {m - 1, m, m + 1}: the conditional subtraction of an addition on both sides of its threshold — as values,
    and as the Montgomery residues a R, b R the limbs actually hold in each view (a R + b R = m - 1, m, m + 1 as integers)"""
    out = []
    for rbits in [0] + [r for _, _, r in views]:
        rinv = pow(1 << rbits, -1, m)
        for s in (m - 1, m, m + 1):
            for a in (1, 2, (m - 1) // 2, (m + 1) // 2, m - 2, m - 1, rnd.randrange(2, m - 2), rnd.randrange(2, m - 2)):
                b = s - a
                if 0 <= b < m:
                    out.append((a * rinv % m, b * rinv % m))
    return out


def new_binary_pairs(m, views, rnd):
    """the operand classes beyond edge x edge: sums at the modulus, a = b, a = m - 1 against {1, 2, m - 1}, saturated limbs"""
    sat = saturated_values(m, views)
    pairs = sum_edge_pairs(m, views, rnd)
    pairs += [(v, v) for v in (0, 1, (m - 1) // 2, (m + 1) // 2, m - 1, rnd.randrange(m), rnd.randrange(m))]
    pairs += [(m - 1, b) for b in (1, 2, m - 1)]
    pairs += [(s, t) for s in sat for t in (s, sat[0], 1, m - 1, m - s, m - 1 - s, rnd.randrange(m))]
    pairs += [(rnd.randrange(m), s) for s in sat]
    return pairs


@functools.lru_cache(None)
def fr_binary_pairs():
    rnd = random.Random(1)
    vals = edge_values(Q, rnd)
    pairs = [(a, b) for a in vals for b in vals[:12] + [rnd.randrange(Q)]]
    return pairs, new_binary_pairs(Q, FR_VIEWS, random.Random(1001))


def fr_inv_values():
    return edge_values(Q, random.Random(1))[1:20]


@functools.lru_cache(None)
def fp_binary_pairs():
    rnd = random.Random(2)
    vals = edge_values(P, rnd, 40)
    pairs = [(a, b) for a in vals for b in vals[:10] + [rnd.randrange(P)]]
    return pairs, new_binary_pairs(P, FP_VIEWS, random.Random(1002))


def fp_inv_values():
    return edge_values(P, random.Random(2), 40)[1:8]


@functools.lru_cache(None)
def g1_points():
    rnd = random.Random(3)
    return [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(6)]


G1_MUL_SCALARS = (1, 2, 3, 0xFFFF, 0x80000001)


@functools.lru_cache(None)
def fp28_cases():
    """(values a, for each a the list of b): the old edge x edge list, then the new operand classes as single pairs"""
    rnd = random.Random(9)
    vals = edge_values(P, rnd, 60)
    per_a = [(a, vals[:9] + [rnd.randrange(P), rnd.randrange(P)]) for a in vals]
    return per_a, new_binary_pairs(P, FP_VIEWS, random.Random(1009))


# the lazy paddings of fp28.cuh (K p with every limb but the top >= 2^29 - 2), restated: sub_lazy<K>(a, b) = a + PAD_K - b limb by limb
FP28_PAD16 = [0x2ffaaab0, 0x2efffffd, 0x2ffffb9d, 0x2ffeb151, 0x2241eabd, 0x20f6b0f4, 0x26730d28,
              0x238512bd, 0x2774b84d, 0x2bacd762, 0x2a7b6432, 0x269a4b19, 0x2ea397fc, 0x001a010f]
FP28_PAD32 = [0x2ff55560, 0x2dfffffd, 0x2ffff73d, 0x2ffd62a5, 0x2483d57d, 0x21ed61ea, 0x2ce61a52,
              0x270a257c, 0x2ee9709c, 0x2759aec6, 0x24f6c867, 0x2d349635, 0x2d472ffa, 0x00340221]
assert value28(FP28_PAD16) == 16 * P and value28(FP28_PAD32) == 32 * P
assert all(x >= (1 << 29) - 2 for x in FP28_PAD16[:13] + FP28_PAD32[:13])

FP28_ONES = [M28] * 13 + [0x1a010]            # < p, every low limb saturated


@functools.lru_cache(None)
def fp28_raw_operands():
    rnd = random.Random(28)
    norm = [limbs28(rnd.randrange(2 * P)) for _ in range(6)] + [FP28_ONES, limbs28(0), limbs28(1), limbs28(P - 1), limbs28(2 * P - 1)]
    assert value28(FP28_ONES) < P
    return norm


@functools.lru_cache(None)
def g1r_points():
    rnd = random.Random(12)
    return [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(40)]


@functools.lru_cache(None)
def g1r_accumulate_cases():
    """(points, sign flags): chains of mixed additions"""
    rnd = random.Random(12)
    pts = [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(40)]
    assert pts == g1r_points()
    cases = []
    for n in (1, 2, 3, 17, 40):
        cases.append((pts[:n], [rnd.randrange(2) for _ in range(n)]))
    # same point repeatedly: first mixed add hits the doubling branch, then generic adds; P + (-P) + P; P + (-P)
    return cases + [([pts[0]] * 9, [0] * 9), ([pts[0]] * 3, [0, 1, 0]), ([pts[0]] * 2, [0, 1])]


@functools.lru_cache(None)
def g1r_tree_cases():
    """(points, k, expected [2 k] sum)"""
    pts = g1r_points()[:20]
    s = None
    for p in pts:
        s = E.g1_add(s, p)
    return [(pts, k, E.g1_mul(s, 2 * k)) for k in (1, 2, 16 * 2047, 0xFFFF)]


@functools.lru_cache(None)
def g1r_pair_cases():
    """(points, sign flags) for the affine-pair first step: every sign combination, then equal and opposite first points"""
    rnd = random.Random(6201)
    pts = [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(24)]
    cases = []
    for trial in range(40):
        n = [2, 2, 2, 2, 3, 8, 24][trial % 7]
        sel = [pts[rnd.randrange(len(pts))] for _ in range(n)]
        if trial % 7 == 0:
            sel[1] = pts[(pts.index(sel[0]) + 1) % len(pts)]
        neg = [(trial >> 0) & 1, (trial >> 1) & 1] + [rnd.randrange(2) for _ in range(n - 2)]
        cases.append((sel, neg))
    return cases + [([pts[0]] * 5, [0] * 5), ([pts[0]] * 5, [0, 1, 0, 0, 0])]


def g1r_sum(pts, neg):
    exp = None
    for p, s in zip(pts, neg):
        exp = E.g1_add(exp, (p[0], (P - p[1]) % P) if s else p)
    return exp


@functools.lru_cache(None)
def fr29_cases():
    rnd = random.Random(29)
    vals = edge_values(Q, rnd, 40)
    old = []
    for a in vals:
        for b in vals[:10] + [rnd.randrange(Q)]:
            old.append((a, b, rnd.choice(vals)))
    rnd2 = random.Random(1029)
    new = [(a, b, rnd2.choice(vals)) for a, b in new_binary_pairs(Q, FR_VIEWS, rnd2)]
    return old, new


@functools.lru_cache(None)
def fr29_sub_reduce_pairs():
    rnd = random.Random(31)
    vals = edge_values(Q, rnd, 60)
    pairs = [(a, b) for a in vals for b in vals[:12] + [rnd.randrange(Q)]]
    return pairs, new_binary_pairs(Q, FR_VIEWS, random.Random(1031))


def safegcd_fp_values():
    rnd = random.Random(381)
    return edge_values(P, rnd, 150) + [(1 << k) % P for k in (1, 29, 30, 31, 59, 60, 380)] + [P - (1 << 30), (P + 1) // 2, 3, P - 3]


def safegcd_fr_values():
    rnd = random.Random(255)
    return edge_values(Q, rnd, 200) + [Q - (1 << 30), (Q + 1) // 2, 7, pow(7, (Q - 1) >> 32, Q)]


def safegcd_fr_mont_values():
    r = random.Random(92)
    return [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, 1 << 254] + [r.randrange(Q) for _ in range(300)]


def safegcd_cg_values():
    """the composer's out-of-line inversion: the Fr inversion lists, the 2^k boundaries of the 30-bit limbs included"""
    r = random.Random(93)
    return [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, Q - (1 << 30), (1 << 30) - 1] + \
        [(1 << k) % Q for k in (1, 29, 30, 31, 59, 60, 254)] + saturated_values(Q, FR_VIEWS) + [r.randrange(Q) for _ in range(60)]


@functools.lru_cache(None)
def decompress_cases():
    """(48-byte encoding, return code, point or None when the output is not specified beyond the code)"""
    rnd = random.Random(11)
    pts = [E.G1_GEN] + [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(24)]
    pts += [(x, (P - y) % P) for x, y in pts[:8]]                      # the other root / sign flag
    good = [(E.g1_compress(pt), 0, pt) for pt in pts]
    g = E.g1_compress(E.G1_GEN)
    bad = [(bytes([g[0] & 0x7F]) + g[1:], 1),                           # compression flag missing
           (bytes([0xC0]) + bytes(47), 2),                              # the identity
           (bytes([0xE0]) + bytes(47), 1),                              # identity with the sort flag
           (bytes([0xC0]) + bytes(46) + b"\x01", 1),                    # identity with x != 0
           (bytes([0x80 | (P >> 376)]) + (P & ((1 << 376) - 1)).to_bytes(47, "big"), 1)]   # x = p
    for x in (P + 1, P + 2, (1 << 381) - 1):                             # x > p that still fits the 381 bits
        bad.append((bytes([0x80 | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big"), 1))
    small = []
    for x in range(1, 40):                                               # x^3 + 4 a non-residue for about half of them
        rhs = (x ** 3 + 4) % P
        on_curve = pow(rhs, (P - 1) // 2, P) == 1
        pt = None
        if on_curve:                                                     # smaller root requested (flag clear)
            y = pow(rhs, (P + 1) // 4, P)
            pt = (x, min(y, P - y))
        small.append((bytes([0x80]) + x.to_bytes(47, "big"), 0 if on_curve else 1, pt))
    assert sum(1 for _, rc, _ in small if rc) > 5
    # interleave: valid points, malformed encodings and small x side by side
    out, bad3 = [], [(e, rc, None) for e, rc in bad]
    for i in range(max(len(good), len(bad3), len(small))):
        for lst in (good, bad3, small):
            if i < len(lst):
                out.append(lst[i])
    return out


def recode_scalars(r):
    return [0, 1, 2, 3, 4, 0xffff, 0x10000, 0x10001, 0x1ffff, 0x20000, Q - 1, Q - 2, (Q - 1) // 2, (1 << 254) + 1,
            (1 << 254) - 1, int("5" * 63, 16), int("a" * 62, 16), int("f" * 60, 16) << 8, sum(1 << (17 * k + 16) for k in range(14)),
            (1 << 239) - 1, ((1 << 16) - 1) << 238, 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000] + \
           [r.randrange(Q) for _ in range(400)] + [r.randrange(1 << r.randrange(1, 255)) for _ in range(200)]


RECODE_MODES = (1, 2, 21, 0, 120, 116)      # every mode h_msm_recode takes

GLV_LAMBDA = 0xac45a4010001a40200000000ffffffff


@functools.lru_cache(None)
def glv_cases():
    """(k, base point, pre-doublings)"""
    lam = GLV_LAMBDA
    rnd = random.Random(6202)
    ks = [0, 1, 2, lam - 1, lam, lam + 1, 2 * lam, lam * lam, Q - 1, Q - lam, (1 << 128) - 1, 1 << 128, (1 << 254) + 1]
    ks += [rnd.randrange(Q) for _ in range(40)] + [rnd.randrange(1 << 64) for _ in range(4)] + [rnd.randrange(1 << 64) * lam % Q for _ in range(4)]
    return [(k, E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)), i % 3) for i, k in enumerate(ks)]


# merlin 3.0 transcript::tests::equivalence_simple
MERLIN_SIMPLE = "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"

# ---- families -----------------------------------------------------------------------------------------------------------------


NEW_CLASS = " [new operand class]"     # label of the cases beyond the lists the host test always had


class Family:
    """cases of one kernel: in_fmt / out_fmt are struct formats of the C records (little endian, no padding)"""

    def __init__(self, name, in_fmt, out_fmt):
        self.name = name
        self.in_struct = struct.Struct("<" + in_fmt)
        self.out_struct = struct.Struct("<" + out_fmt)
        self.inputs = []
        self.expect = []      # a tuple (the exact record) or a predicate on the unpacked record
        self.labels = []
        self.shared = None    # bytes every case of the family reads beside its own record (handed over once, before the cases)

    def add(self, fields, expect, label=""):
        self.inputs.append(self.in_struct.pack(*fields))
        if not callable(expect):
            expect = self.out_struct.pack(*expect)
        self.expect.append(expect)
        self.labels.append(label)

    def __len__(self):
        return len(self.inputs)

    def input_bytes(self):
        return b"".join(self.inputs)

    def check(self, out_bytes):
        """every output record against its expectation: bit for bit, or through the case's predicate"""
        size = self.out_struct.size
        assert len(out_bytes) == size * len(self)
        for i, exp in enumerate(self.expect):
            rec = out_bytes[size * i:size * (i + 1)]
            if callable(exp):
                exp(self.out_struct.unpack(rec), (self.name, i, self.labels[i]))
            else:
                assert rec == exp, (self.name, i, self.labels[i], self.out_struct.unpack(rec), self.out_struct.unpack(exp))

    def failures(self, out_bytes):
        """(index, label) of every case whose record is wrong (check() stops at the first)"""
        size, bad = self.out_struct.size, []
        for i, exp in enumerate(self.expect):
            rec = out_bytes[size * i:size * (i + 1)]
            try:
                if callable(exp):
                    exp(self.out_struct.unpack(rec), i)
                else:
                    assert rec == exp
            except AssertionError:
                bad.append((i, self.labels[i]))
        return bad

    def run(self, lib, prefix):
        """through `<prefix>case_<name>` of a loaded library (h_: the host build, d_: the device build); returns its code"""
        import ctypes
        for which, st in ((0, self.in_struct), (1, self.out_struct)):
            size = getattr(lib, f"{prefix}record_size_{self.name}")(which)
            assert size == st.size, (self.name, which, size, st.size)
        if self.shared is not None:          # the harness turns the blob into its read-only buffer (the device twin uploads it)
            share = getattr(lib, f"{prefix}shared_tables")
            share.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
            share.restype = ctypes.c_int
            rc = share(self.shared, len(self.shared))
            if rc:
                return rc, b""
        fn = getattr(lib, f"{prefix}case_{self.name}")
        fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
        fn.restype = ctypes.c_int
        data = self.input_bytes()
        out = ctypes.create_string_buffer(self.out_struct.size * len(self))
        rc = fn(data, len(data), out, len(out.raw), len(self))
        return rc, out.raw


FR_MUL, FR_ADD, FR_SUB, FR_INV, FR_FROM_MONT, FR_GENERATOR, FR_ROOT, FR_ONE = range(8)
FP_MUL, FP_ADD, FP_SUB, FP_INV = range(4)
G1_ADD_AFF, G1_NEG_ADD, G1_MUL_U32 = range(3)
FP28_ROUNDTRIP, FP28_MUL, FP28_CHAIN, FP28_ZERO_TEST = range(4)
RAW_MUL, RAW_SQR, RAW_MUL2, RAW_SUB_LAZY32, RAW_NEG_LAZY16, RAW_ADD_LAZY = range(6)
G1R_ACCUMULATE, G1R_TREE, G1R_PAIR_FIRST, G1R_AFFINE_ROUNDTRIP = range(4)
GLV_MUL, GLV_SPLIT = range(2)
FR29_BUTTERFLY, FR29_CHAIN, FR29_MUL2, FR29_SUB_REDUCE = range(4)
GCD_FP28, GCD_FP28_LAZY, GCD_FR29_TW, GCD_FR_MONT, GCD_CG_INV = range(5)
G1R_MAX_POINTS = 40

# the canonical limbs of 0 - 1 in Fr: identical to the reference's BlsScalar.0 (fully reduced output)
FR_MINUS_ONE_LIMBS64 = [0xfffffffd00000003, 0xfb38ec08fffb13fc, 0x99ad88181ce5880f, 0x5bc8f5f97cd877d8]


def _fr():
    f = Family("fr", "I8I8I", "8I")
    old, new = fr_binary_pairs()
    inv = fr_inv_values()
    for i, (a, b) in enumerate(old + new):
        tag = "" if i < len(old) else NEW_CLASS
        f.add([FR_MUL] + fr_mont(a) + fr_mont(b), fr_mont(a * b % Q), "mul" + tag)
        f.add([FR_ADD] + fr_mont(a) + fr_mont(b), fr_mont((a + b) % Q), "add" + tag)
        f.add([FR_SUB] + fr_mont(a) + fr_mont(b), fr_mont((a - b) % Q), "sub" + tag)
        if i % 40 == 7 and inv:                              # the Fermat inversions spread among the cheap cases
            v = inv.pop()
            f.add([FR_INV] + fr_mont(v) + [0] * 8, fr_mont(pow(v, -1, Q)), "inv")
    assert not inv
    f.add([FR_INV] + [0] * 16, [0] * 8, "inv 0")             # a^(q-2) of 0
    f.add([FR_FROM_MONT] + fr_mont(12345) + [0] * 8, words(12345, 8), "from_mont")
    # canonical limbs: 0 - 1 is q - 1 in Montgomery form, limb for limb the reference's
    f.add([FR_SUB] + fr_mont(0) + fr_mont(1), [w for l in FR_MINUS_ONE_LIMBS64 for w in (l & 0xFFFFFFFF, l >> 32)], "canonical")
    f.add([FR_GENERATOR] + [0] * 16, fr_mont(7), "generator")
    f.add([FR_ROOT] + [0] * 16, fr_mont(E.ROOT_OF_UNITY), "root of unity")
    f.add([FR_ONE] + [0] * 16, fr_mont(1), "one")
    return f


def _fp():
    f = Family("fp", "I12I12I", "12I")
    old, new = fp_binary_pairs()
    inv = fp_inv_values()
    for i, (a, b) in enumerate(old + new):
        tag = "" if i < len(old) else NEW_CLASS
        f.add([FP_MUL] + fp_mont(a) + fp_mont(b), fp_mont(a * b % P), "mul" + tag)
        f.add([FP_ADD] + fp_mont(a) + fp_mont(b), fp_mont((a + b) % P), "add" + tag)
        f.add([FP_SUB] + fp_mont(a) + fp_mont(b), fp_mont((a - b) % P), "sub" + tag)
        if i % 40 == 7 and inv:
            v = inv.pop()
            f.add([FP_INV] + fp_mont(v) + [0] * 12, fp_mont(pow(v, -1, P)), "inv")
    assert not inv
    f.add([FP_INV] + [0] * 24, [0] * 12, "inv 0")
    return f


def _g1():
    f = Family("g1", "II24I24I", "I24I")
    pts = g1_points()
    zero = [0] * 24
    for a in pts:
        for b in pts:                                            # includes a == b (doubling branch)
            s = E.g1_add(a, b)
            f.add([G1_ADD_AFF, 0] + point_words(a) + point_words(b), [1] + point_words(s), "add_affine")
        f.add([G1_NEG_ADD, 0] + point_words(a) + zero, [0] + zero, "P + (-P)")
        for k in G1_MUL_SCALARS:
            f.add([G1_MUL_U32, k] + point_words(a) + zero, [1] + point_words(E.g1_mul(a, k)), "mul_u32")
        f.add([G1_MUL_U32, 0] + point_words(a) + zero, [0] + zero, "mul_u32 0")
    return f


def _g1_full():
    f = Family("g1_full", "24I24I", "I24I")
    pts = g1_points()
    for a in pts:
        for b in pts:                                            # a == b: the doubling branch of the general addition
            f.add(point_words(a) + point_words(b), [1] + point_words(E.g1_add(a, b)), "add")
        f.add(point_words(a) + point_words((a[0], P - a[1])), [0] + [0] * 24, "P + (-P)")
    return f


def _fp28():
    f = Family("fp28", "I12I12I", "I12I")
    per_a, new = fp28_cases()
    z = [0] * 12
    for a, bs in per_a:
        f.add([FP28_ROUNDTRIP] + fp_mont(a) + z, [0] + fp_mont(a), "roundtrip")
        for b in bs:
            f.add([FP28_MUL] + fp_mont(a) + fp_mont(b), [0] + fp_mont(a * b % P), "mul")
            f.add([FP28_CHAIN] + fp_mont(a) + fp_mont(b), [0] + fp_mont(a * b % P), "chain")
        f.add([FP28_ZERO_TEST] + fp_mont(a) + z, [3 | (4 if a == 0 else 0)] + z, "zero_test")
    for a, b in new:
        f.add([FP28_MUL] + fp_mont(a) + fp_mont(b), [0] + fp_mont(a * b % P), "mul" + NEW_CLASS)
        f.add([FP28_CHAIN] + fp_mont(a) + fp_mont(b), [0] + fp_mont(a * b % P), "chain" + NEW_CLASS)
    for a in saturated_values(P, FP_VIEWS):
        f.add([FP28_ROUNDTRIP] + fp_mont(a) + z, [0] + fp_mont(a), "roundtrip" + NEW_CLASS)
        f.add([FP28_ZERO_TEST] + fp_mont(a) + z, [3] + z, "zero_test" + NEW_CLASS)
    return f


def _raw_product(residue):
    """a raw Montgomery product: normalised limbs, value below 2p, and the residue"""
    def check(rec, where):
        assert all(x <= M28 for x in rec[:13]), ("result not normalised", where)
        r = value28(rec)
        assert r < 2 * P and r % P == residue, where
    return check


def _fp28_raw():
    f = Family("fp28_raw", "I14I14I14I14I", "14I")
    norm = fp28_raw_operands()
    zero = limbs28(0)

    def prod(x, y):
        return value28(x) * value28(y) * FP28_RINV % P

    for a in norm:
        for b in norm:
            # lazy minuend/subtrahend combos (values: a - b + 32p < 34p needs b < 16p: ok, b < 2p)
            la = [x + p - y for x, p, y in zip(a, FP28_PAD32, b)]
            assert max(la) < (1 << 30) and min(la) >= 0 and value28(la) == value28(a) + 32 * P - value28(b)
            nb = [p - y for p, y in zip(FP28_PAD16, b)]
            assert min(nb) >= 0 and value28(nb) == 16 * P - value28(b)
            f.add([RAW_SUB_LAZY32] + a + b + zero + zero, la, "sub_lazy<32>")
            f.add([RAW_NEG_LAZY16] + zero + b + zero + zero, nb, "neg_lazy<16>")
            f.add([RAW_SQR] + la + zero + zero + zero, _raw_product(prod(la, la)), "sqr lazy")      # value < 34p
            f.add([RAW_MUL] + la + la + zero + zero, _raw_product(prod(la, la)), "mul lazy x lazy")
            f.add([RAW_SQR] + a + zero + zero + zero, _raw_product(prod(a, a)), "sqr")
            # mul2 as the point formulas use it: (norm x lazy) + (norm x lazy)
            f.add([RAW_MUL2] + a + la + b + nb, _raw_product((prod(a, la) + prod(b, nb)) % P), "mul2")
            f.add([RAW_ADD_LAZY] + b + b + zero + zero, [2 * y for y in b], "add_lazy")
            f.add([RAW_MUL] + a + b + zero + zero, _raw_product(prod(a, b)), "mul")
    return f


def _signed(p, s):
    return (p[0], (P - p[1]) % P) if s else p


def _g1r_record(op, pts, neg=None, k=0):
    n = len(pts)
    assert n <= G1R_MAX_POINTS
    flat = [w for p in pts for w in point_words(p)] + [0] * (24 * (G1R_MAX_POINTS - n))
    flags = list(neg or []) + [0] * (G1R_MAX_POINTS - len(neg or []))
    return [op, n, k] + flat + flags


def _g1r():
    f = Family("g1r", "III%dI%dB" % (24 * G1R_MAX_POINTS, G1R_MAX_POINTS), "II24I")
    pts = g1r_points()

    def out(pt, used=0):
        return [0 if pt is None else 1, used] + point_words(pt)

    acc, tree, pair = g1r_accumulate_cases(), g1r_tree_cases(), g1r_pair_cases()
    pair = pair + [([pair[0][0][0]], [1]), ([pair[0][0][0], _signed(pair[0][0][0], 1)], [0, 0])]   # a single negated entry; P, -P unsigned
    # interleaved: chains of different length and kind side by side in a wave
    for i in range(max(len(acc), len(tree), len(pair))):
        if i < len(acc):
            p, neg = acc[i]
            f.add(_g1r_record(G1R_ACCUMULATE, p, neg), out(g1r_sum(p, neg)), "accumulate")
        if i < len(tree):
            p, k, want = tree[i]
            f.add(_g1r_record(G1R_TREE, p, None, k), out(want), "tree")
        if i < len(pair):
            p, neg = pair[i]
            used = 1 if len(p) >= 2 and p[0][0] != p[1][0] else 0
            f.add(_g1r_record(G1R_PAIR_FIRST, p, neg), out(g1r_sum(p, neg), used), "pair_first")
        if i in (3, 11):
            f.add(_g1r_record(G1R_AFFINE_ROUNDTRIP, [pts[i]]), out(E.g1_mul(pts[i], 4)), "affine_roundtrip")
    return f


def _glv():
    f = Family("glv", "II8I24I", "I24I8I")
    lam = GLV_LAMBDA
    assert lam * lam + lam + 1 == Q
    for k, base, pre in glv_cases():
        k1, k2 = k % lam, k // lam
        f.add([GLV_SPLIT, 0] + words(k, 8) + [0] * 24, [0] + [0] * 24 + words(k1, 4) + words(k2, 4), "split %x" % k)
        exp = E.g1_mul(base, k * (1 << pre) % Q) if k else None
        f.add([GLV_MUL, pre] + words(k, 8) + point_words(base), [0 if exp is None else 1] + point_words(exp) + [0] * 8, "mul %x" % k)
    return f


def _fr29():
    f = Family("fr29", "II8I8I8I", "8I8I")
    z = [0] * 8
    old, new = fr29_cases()
    for i, (a, b, w) in enumerate(old + new):
        tag = "" if i < len(old) else NEW_CLASS
        ins = fr_mont(a) + fr_mont(b) + fr_mont(w)
        f.add([FR29_BUTTERFLY, 0] + ins, fr_mont((a + b) % Q) + fr_mont((a - b) * w % Q), "butterfly" + tag)   # canonical limbs
        x, y = a, b
        for _ in range(9):
            x, y = (x + y) % Q, (x - y) * w % Q
        f.add([FR29_CHAIN, 9] + ins, fr_mont(x) + fr_mont(y), "chain")
        f.add([FR29_MUL2, 0] + ins, fr_mont(a * b * w % Q) + z, "mul2")
    old, new = fr29_sub_reduce_pairs()
    for i, (a, b) in enumerate(old + new):
        f.add([FR29_SUB_REDUCE, 0] + fr_mont(a) + fr_mont(b) + z, fr_mont((2 * a - 2 * b) % Q) + z, "sub_reduce" + ("" if i < len(old) else NEW_CLASS))
    return f


def _safegcd():
    f = Family("safegcd", "I12I", "12I")
    z4 = [0] * 4
    fpv, frv, frm, cgv = safegcd_fp_values(), safegcd_fr_values(), safegcd_fr_mont_values(), safegcd_cg_values()
    for i in range(max(len(fpv), len(frv), len(frm), len(cgv))):          # the five instances side by side
        if i < len(fpv):
            a = fpv[i]
            f.add([GCD_FP28] + fp_mont(a), fp_mont(pow(a, -1, P) if a else 0), "fp28_inv_gcd %x" % a)
            f.add([GCD_FP28_LAZY] + fp_mont(a), fp_mont(pow(8 * a % P, -1, P) if a else 0), "fp28_inv_gcd 8x %x" % a)
        if i < len(frv):
            a = frv[i]
            f.add([GCD_FR29_TW] + fr_mont(a) + z4, fr_mont(pow(a, -1, Q) if a else 0) + z4, "fr29_inv_gcd_tw %x" % a)
        if i < len(frm):
            a = frm[i]
            f.add([GCD_FR_MONT] + fr_mont(a) + z4, fr_mont(pow(a, -1, Q) if a else 0) + z4, "fr_inv_gcd %x" % a)
        if i < len(cgv):
            a = cgv[i]
            f.add([GCD_CG_INV] + fr_mont(a) + z4, fr_mont(pow(a, -1, Q) if a else 0) + z4, "cg_inv %x" % a)
    return f


def _decompress():
    f = Family("decompress", "48B", "I24I")
    for enc, rc, pt in decompress_cases():
        if rc == 0:
            assert E.g1_decompress(enc) == pt
            f.add(list(enc), [0] + point_words(pt), enc.hex())
        else:
            def code_only(rec, where, rc=rc):
                assert rec[0] == rc, where
            f.add(list(enc), code_only, enc.hex())
    return f


def recode_expected(s, mode):
    """(n, [slot, row, bucket, sign] per digit) of msm_recode.cuh in `mode`, from the big-int models"""
    from msm_wide_model import bitpos_digits, even_digits, signed_digits
    if mode == 0:
        return [(w, w, abs(d) - 1, 1 if d < 0 else 0) for w, d in enumerate(signed_digits(s, 16)) if d]   # slot = row
    if mode in (1, 2, 21):
        dg = bitpos_digits(s, 21) if mode == 21 else bitpos_digits(s)
        return [(j, row, abs(d) >> 1, 1 if d < 0 else 0) for j, (row, d) in enumerate(dg)]
    dg = even_digits(s, 20 if mode == 120 else 16)
    return [(j, row, abs(d) - 1, 1 if d < 0 else 0) for j, (row, d) in enumerate(dg)]


def _recode():
    f = Family("recode", "I8I", "I64I")
    scalars = recode_scalars(random.Random(99))
    for s in scalars:
        for mode in RECODE_MODES:                 # neighbouring lanes recode the same scalar differently
            dg = recode_expected(s, mode)
            assert len(dg) <= 16
            flat = [v for d in dg for v in d]
            f.add([mode] + words(s, 8), [len(dg)] + flat + [0] * (64 - len(flat)), "mode %d %x" % (mode, s))
    return f


def _merlin():
    from oracle.merlin import Transcript
    f = Family("merlin", "I", "32B")
    t = Transcript(b"test protocol")
    t.append_message(b"some label", b"some data")
    assert t.challenge_bytes(b"challenge", 32).hex() == MERLIN_SIMPLE
    f.add([0], list(bytes.fromhex(MERLIN_SIMPLE)), "equivalence_simple")
    return f


# ---- the pairing tower of pairing28.cuh against tests/pairing_tower_model.py ------------------------------------------------
# Records are raw Fp28 limbs (14 words a coordinate, Montgomery with R' = 2^392); a raw value v stands for the residue
# v / R'.  Every output coordinate must be normalised, below 2p (the header's contract) and of the model's residue.

P28_RED, P28_ADD, P28_SUB, P28_NEG = range(4)
F2R_ADD, F2R_SUB, F2R_NEG, F2R_CONJ, F2R_MUL_XI, F2R_MUL, F2R_SQR, F2R_MUL_FP, F2R_INV = range(9)
F6R_ADD, F6R_SUB, F6R_NEG, F6R_MUL_V, F6R_MUL, F6R_INV, F6R_MUL_01, F6R_MUL_1 = range(8)
F12R_MUL, F12R_SQR, F12R_CONJ, F12R_INV, F12R_MUL_014, F12R_MUL_LINE, F12R_MUL_LINE_GENERIC, F12R_IS_ONE, F12R_PUT = range(9)
CYC_F4_SQR, CYC_SQR, CYC_POW_X = range(3)
STAGE_AFF, STAGE_MILLER, STAGE_FINAL_EXP = range(3)
PTOP = P >> (28 * 13)                   # p's top limb


def mont28(x):
    return x * FP28_R % P


def res28(v):
    return v * FP28_RINV % P


@functools.lru_cache(None)
def tower_coords():
    """the operand class of one coordinate, as raw values below 2p: every residue in both representatives the contract
    allows (x R' mod p, and that + p), the saturated-limb patterns, 2p - 1"""
    rnd = random.Random(2800)
    residues = [0, 1, 2, P - 1, P - 2, (P - 1) // 2] + [rnd.randrange(P) for _ in range(6)]
    out = []
    for x in residues:
        out += [mont28(x), mont28(x) + P]
    out += [value28(FP28_ONES)] + saturated_values(P, FP_VIEWS) + [2 * P - 1]
    assert all(0 <= v < 2 * P for v in out)
    return tuple(out)


def _tm():
    import pairing_tower_model as TM
    return TM


def _level(n):
    """(nested model value of n residues, its residues, product, inverse, negation, conjugation or None) of Fp2 / Fp6 / Fp12"""
    TM = _tm()
    return {2: (tuple, list, TM.f2_mul, TM.f2_inv, TM.f2_neg, TM.f2_conj),
            6: (TM.f6_of_coords, TM.f6_coords, TM.f6_mul, TM.f6_inv, TM.f6_neg, None),
            12: (TM.f12_of_coords, TM.f12_coords, TM.f12_mul, TM.f12_inv, TM.f12_neg, TM.f12_conj)}[n]


def tower_value(raw, n):
    """the model's element for n raw coordinates"""
    assert len(raw) == n
    return _level(n)[0]([res28(v) for v in raw])


def tower_raw(x, n, reps=0):
    """raw coordinates of a model element: Montgomery form, coordinate i in its upper representative when bit i of reps is set"""
    return [mont28(v) + (P if (reps >> i) & 1 else 0) for i, v in enumerate(_level(n)[1](x))]


def tower_limbs(raw):
    return [w for v in raw for w in limbs28(v)]


@functools.lru_cache(None)
def tower_elements(n):
    """elements of n coordinates (2, 6, 12) as raw values: zero, one, one non-zero coordinate in each position, every
    coordinate 2p - 1, the coordinate class dealt out n at a time (each of its values somewhere), and random ones"""
    rnd = random.Random(2800 + n)
    cs = list(tower_coords())
    nonzero = [c for c in cs if c % P]
    els = [[0] * n, [mont28(1)] + [0] * (n - 1), [2 * P - 1] * n]
    for i in range(n):
        els.append([0] * i + [nonzero[(5 * i + n) % len(nonzero)]] + [0] * (n - 1 - i))
    deal = cs[:]
    rnd.shuffle(deal)
    for k in range(0, len(deal), n):
        els.append([deal[(k + i) % len(deal)] for i in range(n)])
    els += [[rnd.randrange(2 * P) for _ in range(n)] for _ in range(3)]
    rnd.shuffle(els)                   # structured elements between random ones
    return tuple(tuple(e) for e in els)


@functools.lru_cache(None)
def tower_mul_pairs(n):
    """the operand pairs of the multiplicative routines beyond element x element: (x, x), (x, -x), (x, 1 / x) and, where the
    level has one, (x, conj x) whose product lies in the field below; the second operand in mixed representatives"""
    _, flat, _, inv, neg, conj = _level(n)
    out = []
    for j, x in enumerate(tower_elements(n)):
        xm = tower_value(x, n)
        out.append((x, x, "(x, x)"))
        out.append((x, tuple(tower_raw(neg(xm), n, 0x555 * (j & 3))), "(x, -x)"))
        if any(v % P for v in x):
            out.append((x, tuple(tower_raw(inv(xm), n, 0xA5A >> (j % 5))), "(x, 1/x)"))
        if conj:
            out.append((x, tuple(tower_raw(conj(xm), n, j)), "(x, conj x)"))
    return tuple(out)


def tower_out(expect, offset=0):
    """the predicate of an output of len(expect) coordinates from word `offset` of the record"""
    expect = list(expect)

    def check(rec, where):
        for j, e in enumerate(expect):
            ls = rec[offset + 14 * j:offset + 14 * j + 14]
            assert all(x <= M28 for x in ls), ("coordinate not normalised", where, j)
            v = value28(ls)
            assert v < 2 * P, ("coordinate not below 2p", where, j)
            assert res28(v) == e, ("wrong residue", where, j)
    return check


def _pick(seq, i, k):
    """k entries of seq from a position that moves with i"""
    return [seq[(7 * i + 3 * t) % len(seq)] for t in range(k)]


def p28_red_inputs():
    """normalised values below 64p around every threshold of the quotient estimate floor(top limb / (ptop + 1)), and around
    multiples of p"""
    vals = []
    for q in range(64):
        for top in (q * (PTOP + 1) - 1, q * (PTOP + 1), q * (PTOP + 1) + 1):
            for low in (0, (1 << 364) - 1):
                v = (top << 364) | low
                if top >= 0 and v < 64 * P:
                    vals.append(v)
    for k in (1, 2, 4, 6, 63, 64):
        vals += [v for v in (k * P - 1, k * P, k * P + 1) if v < 64 * P]
    assert 64 * P - 1 in vals          # the largest normalised value of the range
    return vals


def _p28_red():
    f = Family("p28_red", "I14I14I", "14I")
    rnd = random.Random(2801)
    cs = tower_coords()
    z = [0] * 14
    red = p28_red_inputs()
    ends = [0, 2 * P - 1]              # both ends of the wrappers' operand range (normalised, below 2p)
    pairs = [(a, b) for a in ends for b in ends] + [(a, b) for i, a in enumerate(cs) for b in _pick(cs, i, 2) + [ends[i & 1]]]
    for i in range(max(len(red), len(pairs))):
        if i < len(red):
            f.add([P28_RED] + limbs28(red[i]) + z, tower_out([res28(red[i])]), "p28_red %x" % red[i])
            v = rnd.randrange(64 * P)
            f.add([P28_RED] + limbs28(v) + z, tower_out([res28(v)]), "p28_red random")
        if i < len(pairs):
            a, b = pairs[i]
            f.add([P28_ADD] + limbs28(a) + limbs28(b), tower_out([res28(a + b)]), "p28_add")
            f.add([P28_SUB] + limbs28(a) + limbs28(b), tower_out([res28(a - b)]), "p28_sub")
            f.add([P28_NEG] + limbs28(a) + z, tower_out([res28(-a)]), "p28_neg")
    # 64 quotients x 3 top limbs (q = 0 has no top limb below it) x 2 fillings of the low limbs, and 3 values around each of
    # p, 2p, 4p, 6p, 63p and 64p less the two that are not below 64p: every one of them is below 64p and stays
    assert len(f) == 2 * len(red) + 3 * len(pairs) and len(red) == (64 * 3 - 1) * 2 + (6 * 3 - 2)
    return f


def _f2r():
    TM = _tm()
    f = Family("f2r", "I28I28I14I", "28I")
    els, cs = tower_elements(2), tower_coords()
    z2, z1 = [0] * 28, [0] * 14
    n0 = 0

    def binary(op, x, y, fn, label):
        f.add([op] + tower_limbs(x) + tower_limbs(y) + z1, tower_out(fn(tower_value(x, 2), tower_value(y, 2))), label)

    for i, x in enumerate(els):
        xm = tower_value(x, 2)
        for y in _pick(els, i, 4):
            binary(F2R_ADD, x, y, TM.f2_add, "add")
            binary(F2R_MUL, x, y, TM.f2_mul, "mul")
            binary(F2R_SUB, x, y, TM.f2_sub, "sub")
        for op, fn, label in ((F2R_NEG, TM.f2_neg, "neg"), (F2R_CONJ, TM.f2_conj, "conj"), (F2R_MUL_XI, TM.f2_mul_xi, "mul_xi"), (F2R_SQR, TM.f2_sqr, "sqr")):
            f.add([op] + tower_limbs(x) + z2 + z1, tower_out(fn(xm)), label)
        for k in _pick(cs, i, 3):
            f.add([F2R_MUL_FP] + tower_limbs(x) + z2 + limbs28(k), tower_out(TM.f2_mul_fp(xm, res28(k))), "mul_fp")
        if any(v % P for v in x):          # the inverse of 0 is not specified
            f.add([F2R_INV] + tower_limbs(x) + z2 + z1, tower_out(TM.f2_inv(xm)), "inv")
            n0 += 1
    # a^2 + b^2 with one of the two zero, in either representative of zero
    one_zero = [(c, zero) for c in _pick([c for c in cs if c % P], 1, 6) for zero in (0, P)]
    for a, zero in one_zero:
        for x in ((a, zero), (zero, a)):
            f.add([F2R_INV] + tower_limbs(x) + z2 + z1, tower_out(TM.f2_inv(tower_value(x, 2))), "inv, one coordinate zero")
    pairs = tower_mul_pairs(2)
    for x, y, label in pairs:
        binary(F2R_MUL, x, y, TM.f2_mul, "mul " + label)
        binary(F2R_ADD, x, y, TM.f2_add, "add " + label)
        binary(F2R_SUB, x, y, TM.f2_sub, "sub " + label)
    assert len(f) == len(els) * (12 + 4 + 3) + n0 + 2 * len(one_zero) + 3 * len(pairs) and n0 >= len(els) - 3
    return f


def _f6r():
    TM = _tm()
    f = Family("f6r", "II84I84I28I28I", "84I")
    els, e2 = tower_elements(6), tower_elements(2)
    z6, z2 = [0] * 84, [0] * 28
    n0 = 0

    def case(op, alias, x, y, a0, a1, want, label):
        f.add([op, alias] + tower_limbs(x) + (tower_limbs(y) if y else z6) + (tower_limbs(a0) if a0 else z2) + (tower_limbs(a1) if a1 else z2),
              tower_out(TM.f6_coords(want)), label + (" r == x", " r == y")[alias - 1] * (alias > 0))

    for i, x in enumerate(els):
        xm = tower_value(x, 6)
        for t, y in enumerate(_pick(els, i, 3)):
            ym = tower_value(y, 6)
            case(F6R_MUL, (i + t) % 3, x, y, None, None, TM.f6_mul(xm, ym), "mul")
            case(F6R_ADD, (i + t) & 1, x, y, None, None, TM.f6_add(xm, ym), "add")      # in place as f12r_mul calls them
            case(F6R_SUB, (i + t + 1) & 1, x, y, None, None, TM.f6_sub(xm, ym), "sub")
        case(F6R_NEG, 0, x, None, None, None, TM.f6_neg(xm), "neg")
        case(F6R_MUL_V, i & 1, x, None, None, None, TM.f6_mul_v(xm), "mul_v")
        for t, (a0, a1) in enumerate(zip(_pick(e2, i, 2), _pick(e2, i + 1, 2))):
            am0, am1 = tower_value(a0, 2), tower_value(a1, 2)
            case(F6R_MUL_01, (i + t) & 1, x, None, a0, a1, TM.f6_mul(xm, (am0, am1, TM.F2_ZERO)), "mul_01")
            case(F6R_MUL_1, (i + t + 1) & 1, x, None, None, a1, TM.f6_mul(xm, (TM.F2_ZERO, am1, TM.F2_ZERO)), "mul_1")
        if any(v % P for v in x):
            case(F6R_INV, i & 1, x, None, None, None, TM.f6_inv(xm), "inv")                # in place as f12r_inv calls it
            n0 += 1
    pairs = tower_mul_pairs(6)
    for j, (x, y, label) in enumerate(pairs):
        case(F6R_MUL, j % 3, x, y, None, None, TM.f6_mul(tower_value(x, 6), tower_value(y, 6)), "mul " + label)
    assert len(f) == len(els) * (9 + 2 + 4) + n0 + len(pairs) and n0 >= len(els) - 2
    return f


def _f12r_expect(residues, flag=0, put=None):
    coords = tower_out(residues, 1)
    put = list(put) if put else [0] * 144

    def check(rec, where):
        assert rec[0] == flag, ("flag", where)
        coords(rec, where)
        assert list(rec[169:]) == put, ("f12r_put", where)
    return check


def _f12r():
    TM = _tm()
    f = Family("f12r", "II168I168I84I14I14I", "I168I144I")
    els, e2, cs = tower_elements(12), tower_elements(2), tower_coords()
    z12, z3, z1 = [0] * 168, [0] * 84, [0] * 14
    n0 = 0

    def case(op, alias, x, y, want, label, line=None, px=0, py=0, flag=0, put=None):
        ll = tower_limbs([c for c2 in line for c in c2]) if line else z3
        f.add([op, alias] + tower_limbs(x) + (tower_limbs(y) if y else z12) + ll + limbs28(px) + limbs28(py),
              _f12r_expect(TM.f12_coords(want), flag, put), label + (" r == x", " r == y")[alias - 1] * (alias > 0))

    for i, x in enumerate(els):
        xm = tower_value(x, 12)
        for t, y in enumerate(_pick(els, i, 3)):
            case(F12R_MUL, (i + t) % 3, x, y, TM.f12_mul(xm, tower_value(y, 12)), "mul")
        case(F12R_SQR, i & 1, x, None, TM.f12_sqr(xm), "sqr")
        case(F12R_CONJ, (i + 1) & 1, x, None, TM.f12_conj(xm), "conj")
        if any(v % P for v in x):
            case(F12R_INV, i & 1, x, None, TM.f12_inv(xm), "inv")
            n0 += 1
        # the sparse products against the model's DENSE product of the line element
        for t in range(2):
            line = _pick(e2, 3 * i + t, 3)
            a0, a1, b1 = (tower_value(c, 2) for c in line)
            case(F12R_MUL_014, (i + t) & 1, x, None, TM.f12_mul(xm, TM.sparse_014(a0, a1, b1)), "mul_014", line)
            px, py = _pick(cs, 2 * i + t, 2)
            want = TM.f12_mul(xm, TM.line_element(a0, a1, b1, res28(px), res28(py)))
            case(F12R_MUL_LINE, 1, x, None, want, "mul_line", line, px, py)
            case(F12R_MUL_LINE_GENERIC, 1, x, None, want, "mul_line_generic", line, px, py)
        case(F12R_IS_ONE, 1, x, None, xm, "is_one", flag=1 if xm == TM.F12_ONE else 0)
        case(F12R_PUT, 1, x, None, xm, "put", put=[w for c in TM.f12_coords(xm) for w in words(c, 12)])
    pairs = tower_mul_pairs(12)
    for j, (x, y, label) in enumerate(pairs):
        case(F12R_MUL, j % 3, x, y, TM.f12_mul(tower_value(x, 12), tower_value(y, 12)), "mul " + label)
    # is_one: 1 in both representatives, 1 with one coordinate stored as p, 1 with one other coordinate not 0 modulo p
    one = [mont28(1)] + [0] * 11
    ones = [(one, 1), ([mont28(1) + P] + [0] * 11, 1), ([1] + [0] * 11, 0), ([mont28(2)] + [0] * 11, 0), ([mont28(1) + 1] + [0] * 11, 0)]
    for i in range(12):
        ones.append((one[:i] + [one[i] + P] + one[i + 1:], 1))
        if i:
            ones.append((one[:i] + [(1, P - 1, P + 1, mont28(1), 2 * P - 1)[i % 5]] + one[i + 1:], 0))
    for x, flag in ones:
        case(F12R_IS_ONE, 1, x, None, tower_value(x, 12), "is_one: 1 and its neighbours", flag=flag)
    assert len(f) == len(els) * (3 + 2 + 6 + 2) + n0 + len(pairs) + len(ones) and n0 >= len(els) - 1 and len(ones) == 5 + 12 + 11
    return f


@functools.lru_cache(None)
def pairing_shared_blob():
    """the compressed x_h || h of tests/kzg_ref.py, from which the harness fills the PairingTables28 the table families read"""
    import g2_ref as G2
    import kzg_ref as K
    return G2.g2_compress(G2.g2_mul(G2.G2_GEN, K.TAU)) + G2.g2_compress(G2.G2_GEN)


def _f12r_frob():
    """expected values: the model's x^(p^k) as a power, never a table"""
    TM = _tm()
    f = Family("f12r_frob", "II168I", "168I")
    f.shared = pairing_shared_blob()
    els = tower_elements(12)
    n = len(els[0])
    structured = [e for e in els if sum(1 for v in e if v) == 1]
    sel = [[mont28(1)] + [0] * 11, structured[0], structured[7], [2 * P - 1] * 12] + [e for e in els if all(v not in (0, 2 * P - 1) for v in e)][:3]
    assert n == 12 and len(sel) == 7
    for i, x in enumerate(sel):
        for k in (1, 2, 3):
            alias = (i + k) & 1
            f.add([k, alias] + tower_limbs(x), tower_out(TM.f12_coords(TM.frobenius(tower_value(x, 12), k))), "frob %d%s" % (k, " r == x" * alias))
    assert len(f) == 21
    return f


@functools.lru_cache(None)
def cyclotomic_elements():
    """(raw element, model element) of the cyclotomic subgroup: edge and random elements mapped there BY THE MODEL, their
    conjugates, and 1; the raw forms in mixed representatives"""
    TM = _tm()
    els = tower_elements(12)
    src = [e for e in els if sum(1 for v in e if v) == 1][:2] + [[2 * P - 1] * 12] + [e for e in els if all(v not in (0, 2 * P - 1) for v in e)][:3]
    out = [([mont28(1)] + [0] * 11, TM.F12_ONE), ([mont28(1) + P] + [P] * 11, TM.F12_ONE)]
    for j, x in enumerate(src):
        m = TM.to_cyclotomic(tower_value(x, 12))
        assert TM.f12_mul(m, TM.f12_conj(m)) == TM.F12_ONE
        out.append((tower_raw(m, 12, 0x3C5 * j), m))
        out.append((tower_raw(TM.f12_conj(m), 12, 0xC3A >> j), TM.f12_conj(m)))
    return tuple(out)


def _f12r_cyc():
    TM = _tm()
    f = Family("f12r_cyc", "II168I", "168I")
    e2 = tower_elements(2)
    cyc = cyclotomic_elements()
    pow_cases = [cyc[0], cyc[2], cyc[3], cyc[-2]]                     # 1, m and conj(m), one more
    for i in range(max(len(e2), len(cyc))):
        if i < len(e2):
            for b in _pick(e2, i, 2) + [e2[i]]:
                c0, c1 = TM.f4_sqr(tower_value(e2[i], 2), tower_value(b, 2))
                f.add([CYC_F4_SQR, 0] + tower_limbs(e2[i]) + tower_limbs(b) + [0] * 112,
                      tower_out(list(c0) + list(c1) + [0] * 8), "f4r_sqr")      # the case body zeroes the rest
        if i < len(cyc):
            x, m = cyc[i]
            f.add([CYC_SQR, i & 1] + tower_limbs(x), tower_out(TM.f12_coords(TM.f12_mul(m, m))), "cyc_sqr" + " in place" * (i & 1))
            f.add([CYC_SQR, (i + 1) & 1] + tower_limbs(x), tower_out(TM.f12_coords(TM.f12_mul(m, m))), "cyc_sqr" + " in place" * ((i + 1) & 1))
        if i < len(pow_cases):
            x, m = pow_cases[i]
            f.add([CYC_POW_X, 0] + tower_limbs(x), tower_out(TM.f12_coords(TM.cyc_pow_x(m))), "cyc_pow_x_28")
    assert len(f) == 3 * len(e2) + 2 * len(cyc) + 4 and len(cyc) == 14
    return f


@functools.lru_cache(None)
def pairing_stage_points():
    """the G1 pairs (a, b) of the Miller cases: two random, one of KZG shape (e(a, x_h) e(b, h) = 1), every identity placement"""
    import kzg_ref as K
    rnd = random.Random(2807)
    g = lambda k: E.g1_mul(E.G1_GEN, k % Q)      # noqa: E731
    r = rnd.randrange(1, Q)
    return ((g(rnd.randrange(1, Q)), g(rnd.randrange(1, Q))), (g(-r), g(r * K.TAU)), (None, g(rnd.randrange(1, Q))),
            (g(rnd.randrange(1, Q)), g(rnd.randrange(1, Q))), (g(rnd.randrange(1, Q)), None), (None, None))


def _pairing_stages():
    """The Miller value is compared AFTER the final exponentiation: the model's final exponentiation of the product's Miller
    output against the model's final exponentiation of the product of its own two Miller loops (the prepared lines of the
    product are scaled by factors the final exponentiation removes, which the model does not reproduce)."""
    import g2_ref as G2
    import kzg_ref as K
    TM = _tm()
    f = Family("pairing_stages", "II48I28II28II168I", "I168I")
    f.shared = pairing_shared_blob()
    rnd = random.Random(2808)
    xh = G2.g2_mul(G2.G2_GEN, K.TAU)
    zg1, zaff, z12 = [0] * 48, [0] * 28, [0] * 168

    def aff_out(inf, x, y):
        coords = tower_out([x, y] + [0] * 10, 1)

        def check(rec, where):
            assert rec[0] == inf, ("inf", where)
            coords(rec, where)
        return check

    def miller_out(a, b):
        want = TM.final_exponentiation(TM.f12_mul(TM.miller_loop(a, xh), TM.miller_loop(b, G2.G2_GEN)))

        def check(rec, where):
            got = []
            for j in range(12):
                ls = rec[1 + 14 * j:15 + 14 * j]
                assert all(x <= M28 for x in ls) and value28(ls) < 2 * P, ("coordinate not normalised or not below 2p", where, j)
                got.append(res28(value28(ls)))
            assert TM.final_exponentiation(TM.f12_of_coords(got)) == want, ("Miller value after the final exponentiation", where)
        return check

    def aff28(pt, reps):
        return zaff + [1] if pt is None else limbs28(mont28(pt[0]) + P * (reps & 1)) + limbs28(mont28(pt[1]) + P * (reps >> 1)) + [0]

    # XYZZ points with ZZ != 1: (x zz, y zzz, zz, zzz), zz = z^2, zzz = z^3; and the identity (ZZ = 0)
    pt = E.g1_mul(E.G1_GEN, rnd.randrange(1, Q))
    xyzz = []
    for z in (1, 2, P - 1, rnd.randrange(2, P), rnd.randrange(2, P)):
        zz, zzz = z * z % P, z * z * z % P
        xyzz.append((fp_mont(pt[0] * zz % P) + fp_mont(pt[1] * zzz % P) + fp_mont(zz) + fp_mont(zzz), aff_out(0, pt[0], pt[1]), "g1aff28_of_g1 z = %x" % z))
    xyzz.append((fp_mont(1) + fp_mont(1) + [0] * 24, aff_out(1, 0, 0), "g1aff28_of_g1 identity"))
    units = [TM.f12_of_coords(rnd.randrange(P) for _ in range(12)) for _ in range(2)]
    finals = [(tower_raw(units[0], 12, 0), units[0], 0), ([mont28(1)] + [0] * 11, TM.F12_ONE, 1), (tower_raw(units[1], 12, 0xB6D), units[1], 1),
              ([mont28(1) + P] + [P] * 11, TM.F12_ONE, 0)]
    millers = pairing_stage_points()
    for i in range(6):                     # the stages side by side in the wave
        g1, want, label = xyzz[i]
        f.add([STAGE_AFF, 0] + g1 + zaff + [0] + zaff + [0] + z12, want, label)
        a, b = millers[i]
        f.add([STAGE_MILLER, 0] + zg1 + aff28(a, i) + aff28(b, i >> 1) + z12, miller_out(a, b),
              "miller2_28 a %s, b %s" % ("identity" if a is None else "finite", "identity" if b is None else "finite"))
        if i < len(finals):
            x, xm, alias = finals[i]
            f.add([STAGE_FINAL_EXP, alias] + zg1 + zaff + [0] + zaff + [0] + tower_limbs(x),
                  _stage_final(TM.f12_coords(TM.final_exponentiation(xm))), "final_exponentiation_28" + " in place" * alias)
    assert len(f) == 6 + 6 + 4
    return f


def _stage_final(residues):
    coords = tower_out(residues, 1)

    def check(rec, where):
        assert rec[0] == 0, ("inf", where)
        coords(rec, where)
    return check


_BUILDERS = {"fr": _fr, "fp": _fp, "g1": _g1, "g1_full": _g1_full, "fp28": _fp28, "fp28_raw": _fp28_raw, "g1r": _g1r, "glv": _glv, "fr29": _fr29,
             "safegcd": _safegcd, "decompress": _decompress, "recode": _recode, "merlin": _merlin, "p28_red": _p28_red, "f2r": _f2r, "f6r": _f6r,
             "f12r": _f12r, "f12r_frob": _f12r_frob, "f12r_cyc": _f12r_cyc, "pairing_stages": _pairing_stages}
FAMILIES = tuple(_BUILDERS)


@functools.lru_cache(None)
def family(name):
    return _BUILDERS[name]()
