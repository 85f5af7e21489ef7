"""GPU: what follows the bucket sort in plonk_amd/csrc/msm.hip — accumulation, bucket sums, heavy buckets, row / column sums,
fold, bit sums — stage by stage against the big-int model of tests/msm_tail_model.py, and g1r_add_quad (curve28_quad.cuh) on
its own.  The other half of tests/test_gpu_msm_sort.py: given the arrays the sort writes, what must be written next.

The kernels are reached through tests/_build/libdev_msm_tail.so (tests/csrc/dev_msm_tail.hip, built by build()): one
msm_batch_device_v call per door call, phase 1 or phase 2, under the Config switches of that call; the only kernel of the
door library is the test kernel around g1r_add_quad.  All comparisons are exact.  Every point is [k]G with k known, so an
expected sum is one fixed-base multiplication however many buckets fed it.  partial, seg_sum, buckets, chunk and the
output slots of all four commitments are filled with 0xA5; after a call every word of what it may write is compared or
shown untouched, and the regions of the commitments that were not launched are untouched.  (Phase 2 takes no pointer to
partial and seg_sum: those two are filled once per test and shown untouched at its end, not after every launch.)  A failure
names the commitment, the array, the bucket or sum index and the variant.

  A  g1r_add_quad alone: generic pairs, identities, equal and opposite operands under different Z, identical slots, results
     of dbl() and of earlier quad additions as operands, every coordinate at canonical / + p / its largest admissible
     multiple of p; the four lanes of a quad bit-identical, the result the oracle's sum and inside the stated output bounds.
  B  phase 2 on crafted buckets (random, all identity, one bucket, one point everywhere, cancelling +-P at every stride, the
     largest representatives), groups of 1, 2 and 4: every intermediate sum in chunk and every output slot, for every
     row / column kernel (msm_rowcol_quad_kernel<1/2/4>, msm_rowcol_kernel + msm_bits_kernel, msm_final_kernel,
     msm_rowcol_tp_kernel<4/8/16/32> with quad and lane trees).
  C  phase 1 behind the real sort on a test-owned table of multiples of G (equal and opposite points among them), at the
     bucket populations and launch rules of msm_tail_model.PHASE1_LAUNCHES; partial slice by slice, buckets, then phase 2 on
     the same state and every bit sum; a group of three launched by columns.

Not covered: order = 0 over 2^19 buckets with more than 8 slices per bucket (needs m > 2^23); the opt-in 2^17-bucket build;
msm_points.hip.

One difference from what one might expect: msm_bits_kernel (the serial tail) writes S into slot rb + 8 for every kind of rows,
the quad kernel for bit-position rows only; the slot is compared where it is written and shown untouched where it is not.

On an MI355X the file takes about 25 seconds (tests/test_gpu_msm_sort.py: about ten).  Every case but one takes between 0.2
and 2.6 s; the slowest, 5.1 s, is the first case over 2^19 crafted buckets: its host model multiplies G by the 9000 distinct
scalars of the row / column sums of a random array (about 3 s of big-int work, done once and shared by the cases after it)."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import msm_sort_model as S
import msm_tail_model as T
from oracle import bls12_381 as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_msm_tail.so")
P, Q = E.P, E.Q
KB = T.MAX_BATCH
NB_MAX = 1 << 19
SLOT = 256                                   # bytes of a G1RSlot
OUT = 192                                    # bytes of a G1
CHUNK_SLOTS = (2 * (NB_MAX // 128) + 1024) * KB
A5 = np.uint64(0xA5A5A5A5A5A5A5A5)
CFG_FIELDS = ("ksl", "order", "acc_lds", "acc_wg", "bsum_lane", "tail_serial", "rc_lane_tree", "lps", "rcwv")
CFG_DEFAULT = dict(ksl=0, order=-1, acc_lds=0, acc_wg=0, bsum_lane=0, tail_serial=0, rc_lane_tree=0, lps=0, rcwv=0)


class Cfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in CFG_FIELDS]


class Report(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("ksl", "heavy_thresh", "ordered", "wide")] + [("last_rowbits", ctypes.c_int)]


class Work(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("entries", "offsets", "slice_off", "full_off", "part_list", "multi_list", "nheavy",
                                                "heavy_list", "buckets", "tmp_words", "partial", "seg_sum", "chunk")] \
        + [(n, ctypes.c_uint64) for n in ("cap_m", "cap_slices", "cap_segs")]


def cfg(**kw):
    assert set(kw) <= set(CFG_FIELDS)
    return Cfg(**dict(CFG_DEFAULT, **kw))


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(SO), "tests/_build/libdev_msm_tail.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dmt_quad_add.argtypes = [vp, vp, vp, vp, vp, u32]
    so.dmt_phase.argtypes = [vp, ci, ci, u32, vp, u64, ci, ci, ci, vp, vp, ci, vp, vp, vp]
    so.dmt_work.argtypes = [vp, u64, vp, vp]
    so.dmt_fill.argtypes = [vp, vp, ci, u64]
    so.dmt_read.argtypes = [vp, vp, vp, u64]
    so.dmt_write.argtypes = [vp, vp, vp, u64]
    so.dmt_scatter.argtypes = [vp, vp, u64, vp, vp, u64]
    return so


class Rig:
    """one context, its work buffers, the output slots and the device arrays of the current test"""
    STAGE = 64 << 20

    def __init__(self, lib):
        import plonk_amd
        self.ctx, self.lib, self.bufs = plonk_amd.Context(0), lib, []
        self.h = self.ctx.handle
        self.outs = self.ctx.alloc(OUT * T.BIT_SUMS * KB + OUT)          # + one guard slot
        self.pinned = plonk_amd.PinnedBuffer(self.STAGE)
        self.stage = np.frombuffer((ctypes.c_uint8 * self.STAGE).from_address(self.pinned.ptr), dtype=np.uint64)

    def close(self):
        self.free()
        self.outs.free()
        self.pinned.free()
        self.ctx.close()

    def alloc(self, nbytes, keep=False):
        b = self.ctx.alloc(max(nbytes, 16))
        if not keep:
            self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def work(self, m, c=None) -> Work:
        w = Work()
        assert self.lib.dmt_work(self.h, m, ctypes.byref(c) if c is not None else None, ctypes.byref(w)) == 0
        assert w.cap_m >= m
        return w

    def fill(self, ptr, nbytes, byte=0xA5):
        assert self.lib.dmt_fill(self.h, ptr, byte, nbytes) == 0

    def write(self, ptr, a):
        a = np.ascontiguousarray(a)
        assert self.lib.dmt_write(self.h, ptr, a.ctypes.data, a.nbytes) == 0

    def copy(self, dst, src, nbytes):
        assert self.lib.dmt_write(self.h, dst, src, nbytes) == 0

    def read(self, ptr, count, dtype=np.uint32):
        a = np.empty(count, dtype=dtype)
        if a.nbytes:
            assert self.lib.dmt_read(self.h, ptr, a.ctypes.data, a.nbytes) == 0
        return a

    def untouched(self, ptr, nbytes) -> bool:
        """every byte of [ptr, ptr + nbytes) is still 0xA5 (through the pinned staging buffer: the regions are large)"""
        assert nbytes % 8 == 0
        for off in range(0, nbytes, self.STAGE):
            n = min(self.STAGE, nbytes - off)
            assert self.lib.dmt_read(self.h, ptr + off, self.pinned.ptr, n) == 0
            if not (self.stage[:n // 8] == A5).all():
                return False
        return True

    # the regions of one call
    def fill_small(self, w):
        self.fill(w.chunk, SLOT * CHUNK_SLOTS)
        self.fill(self.outs.ptr, self.outs.nbytes)

    def fill_big(self, w):
        self.fill(w.partial, SLOT * w.cap_slices * KB)
        self.fill(w.seg_sum, SLOT * w.cap_segs * KB)

    def fill_buckets(self, w):
        self.fill(w.buckets, SLOT * NB_MAX * KB)

    def out_ptrs(self, n):
        return (ctypes.c_void_p * n)(*[self.outs.ptr + OUT * T.BIT_SUMS * k for k in range(n)])

    def phase(self, phase, bits, rows, table, table_n, ms, c, scalars=None, kb0=0, count=None, bit_sums=True):
        n = len(ms)
        rep = Report()
        sc = (ctypes.c_void_p * n)(*[(b.ptr if b is not None else None) for b in (scalars or [None] * n)])
        rc = self.lib.dmt_phase(self.h, phase, bits, rows, table, table_n, n, kb0, n - kb0 if count is None else count, sc,
                                (ctypes.c_uint64 * n)(*ms), int(bit_sums), self.out_ptrs(n), ctypes.byref(c), ctypes.byref(rep))
        return rc, rep


@pytest.fixture(scope="module")
def rig(lib):
    r = Rig(lib)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def release(request):
    yield
    if "rig" in request.fixturenames:
        request.getfixturevalue("rig").free()


# ---- comparing points ---------------------------------------------------------------------------------------------------
_seen = set()


def expect_slot(words, k, what):
    """the G1RSlot `words` (64 uint32) is [k]G inside the storage contract"""
    key = (words.tobytes(), k)
    if key in _seen:
        return
    try:
        got = T.decode_slot(words)
        raw = T.raw_coords(words)
        if got is not None:
            assert all(v < b * P for v, b in zip(raw, T.BOUNDS)), "a coordinate is outside X < 16p, Y < 8p, ZZ, ZZZ < 2p"
        assert T.same_point(got, T.mul_g(k)), "holds %s, the model says [%#x]G" % ("the identity" if got is None else "another point", k)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    _seen.add(key)


def expect_out(words, k, what):
    key = (words.tobytes(), k, "out")
    if key in _seen:
        return
    try:
        got = T.decode_out(words)
        assert T.same_point(got, T.mul_g(k)), "holds %s, the model says [%#x]G" % ("the identity" if got is None else "another point", k)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    _seen.add(key)


def kept(a) -> bool:
    return bool((np.asarray(a).view(np.uint8) == 0xA5).all())


# =====================================================================================================================
# A. g1r_add_quad alone
# =====================================================================================================================
def quad_cases():
    """[(name, slot a, slot b, op, expected scalar, passthrough)]: passthrough 'a' / 'b' = the result must be that operand, bit for bit"""
    r = random.Random(2024)
    cases = []

    def k():
        return r.randrange(1, Q)

    def z():
        return r.randrange(2, P)

    def rnd_mult():
        return tuple(r.randrange(b) for b in T.BOUNDS)

    def add(name, ka, kb, a, b, op=0, passthrough=None):
        exp = {0: ka + kb, 1: 2 * ka + kb, 2: ka + 2 * kb, 3: 2 * ka + kb, 4: 2 * ka + 2 * kb}[op] % Q
        cases.append((name, a, b, op, exp, passthrough))

    pt = T.affine_g
    for i in range(100):
        ka, kb = k(), k()
        add("generic %d" % i, ka, kb, T.encode_slot(pt(ka), z(), rnd_mult()), T.encode_slot(pt(kb), z(), rnd_mult()))
    ka = k()
    zero = [0] * 64
    for name, ida in (("identity()", T.IDENTITY_SLOT), ("all-zero slot", zero)):
        add("identity (%s) + P" % name, 0, ka, ida, T.encode_slot(pt(ka), z()), passthrough="b")
        add("P + identity (%s)" % name, ka, 0, T.encode_slot(pt(ka), z(), rnd_mult()), ida, passthrough="a")
        add("identity + identity (%s)" % name, 0, 0, ida, T.IDENTITY_SLOT, passthrough="b")
    for i in range(6):
        ka = k()
        add("P + P, different Z %d" % i, ka, ka, T.encode_slot(pt(ka), z(), rnd_mult()), T.encode_slot(pt(ka), z(), rnd_mult()))
        add("P + (-P), different Z %d" % i, ka, Q - ka, T.encode_slot(pt(ka), z(), rnd_mult()), T.encode_slot(pt(Q - ka), z(), rnd_mult()))
        s = T.encode_slot(pt(ka), z(), rnd_mult())
        add("P + P, identical slots %d" % i, ka, ka, s, list(s))
        add("P + P, both affine %d" % i, ka, ka, T.encode_slot(pt(ka)), T.encode_slot(pt(ka)))
        add("P + (-P), Z = 1 against Z %d" % i, ka, Q - ka, T.encode_slot(pt(ka)), T.encode_slot(pt(Q - ka), z()))
    for op in (1, 2, 3, 4):
        for i in range(6):
            ka, kb = k(), k()
            add("fed back, op %d, %d" % (op, i), ka, kb, T.encode_slot(pt(ka), z(), rnd_mult()), T.encode_slot(pt(kb), z(), rnd_mult()), op)
        ka = k()
        # dbl(a) + b with b = 2a: equal operands of which one is a dbl() result; (a + b) + a with b = -2a: opposite operands
        add("fed back, op %d, equal after the first step" % op, ka, {1: 2 * ka, 2: ka * pow(2, -1, Q), 3: Q - ka, 4: ka}[op] % Q,
            T.encode_slot(pt(ka), z()), T.encode_slot(pt({1: 2 * ka, 2: ka * pow(2, -1, Q), 3: Q - ka, 4: ka}[op] % Q), z()), op)
        add("fed back, op %d, opposite after the first step" % op, ka, {1: Q - 2 * ka, 2: (Q - ka) * pow(2, -1, Q), 3: Q - 2 * ka, 4: Q - ka}[op] % Q,
            T.encode_slot(pt(ka), z()), T.encode_slot(pt({1: Q - 2 * ka, 2: (Q - ka) * pow(2, -1, Q), 3: Q - 2 * ka, 4: Q - ka}[op] % Q), z()), op)
    # every coordinate of either operand at canonical, + p and the largest admissible multiple, alone and all together
    ka, kb = k(), k()
    za, zb = z(), z()
    top = tuple(b - 1 for b in T.BOUNDS)
    for side in (0, 1):
        for c in range(4):
            for mult in sorted({0, 1, top[c]}):
                m = [0, 0, 0, 0]
                m[c] = mult
                a = T.encode_slot(pt(ka), za, tuple(m) if side == 0 else (0, 0, 0, 0))
                b = T.encode_slot(pt(kb), zb, tuple(m) if side == 1 else (0, 0, 0, 0))
                add("operand %d, coordinate %d + %d p" % (side, c, mult), ka, kb, a, b)
    for ma, mb in ((top, (0, 0, 0, 0)), ((0, 0, 0, 0), top), (top, top), ((1, 1, 1, 1), (1, 1, 1, 1))):
        add("all coordinates + %r p / + %r p" % (ma, mb), ka, kb, T.encode_slot(pt(ka), za, ma), T.encode_slot(pt(kb), zb, mb))
        add("P + P at + %r p / + %r p" % (ma, mb), ka, ka, T.encode_slot(pt(ka), za, ma), T.encode_slot(pt(ka), zb, mb))
        add("P + (-P) at + %r p / + %r p" % (ma, mb), ka, Q - ka, T.encode_slot(pt(ka), za, ma), T.encode_slot(pt(Q - ka), zb, mb))
        for op in (1, 3):
            add("op %d at + %r p / + %r p" % (op, ma, mb), ka, kb, T.encode_slot(pt(ka), za, ma), T.encode_slot(pt(kb), zb, mb), op)
    r.shuffle(cases)                  # cases that take different branches share a wave
    return cases


def test_quad_add(rig):
    cases = quad_cases()
    n = len(cases)
    assert 150 <= n <= 1000
    a = np.array([c[1] for c in cases], dtype=np.uint32)
    b = np.array([c[2] for c in cases], dtype=np.uint32)
    op = np.array([c[3] for c in cases], dtype=np.uint32)
    da, db, dop, dout = rig.alloc(a.nbytes), rig.alloc(b.nbytes), rig.alloc(op.nbytes), rig.alloc(4 * SLOT * n + SLOT)
    rig.write(da.ptr, a)
    rig.write(db.ptr, b)
    rig.write(dop.ptr, op)
    rig.fill(dout.ptr, 4 * SLOT * n + SLOT)
    assert rig.lib.dmt_quad_add(rig.h, da.ptr, db.ptr, dop.ptr, dout.ptr, n) == 0
    got = rig.read(dout.ptr, 4 * 64 * n + 64).reshape(n * 4 + 1, 64)
    assert kept(got[4 * n]), "the slot past the last result was written"
    for i, (name, sa, sb, o, k, passthrough) in enumerate(cases):
        lanes = got[4 * i:4 * i + 4]
        for q in (1, 2, 3):
            diff = np.nonzero(lanes[q] != lanes[0])[0]
            assert not len(diff), "%s: lane %d differs from lane 0 in word %d (coordinate %d, limb %d): %#x / %#x" \
                % (name, q, diff[0], diff[0] // 16, diff[0] % 16, lanes[q][diff[0]], lanes[0][diff[0]])
        expect_slot(lanes[0], k, name)
        if passthrough:
            assert lanes[0].tolist() == (sa if passthrough == "a" else sb), "%s: the other operand was not returned as it is" % name
        elif T.decode_slot(lanes[0]) is not None:
            raw = T.raw_coords(lanes[0])
            assert all(v < bd * P for v, bd in zip(raw, (14, 4, 2, 2))), \
                "%s: outside X < 14p, Y < 4p, ZZ, ZZZ < 2p: %s" % (name, [v // P for v in raw])


# =====================================================================================================================
# B. the tail on crafted buckets (phase 2)
# =====================================================================================================================
class Crafted:
    """one bucket array: bucket b holds sgn[b] * pool point idx[b] (idx < 0: the identity) in representation rep[b]"""

    def __init__(self, name, bits, idx, sgn, rep, pool_k=None):
        self.name, self.bits, self.nb = name, bits, 1 << bits
        self.idx, self.sgn, self.rep = idx.astype(np.int64), sgn.astype(np.int64), rep.astype(np.int64)
        self.pool_k = T.POOL_K if pool_k is None else pool_k
        self._scalars, self.dev = {}, None

    def words(self):
        """(nb, 64) uint32"""
        table = T.pool_slots()                                     # [sign][member][rep] -> 64 words; member NPOOL = the identities
        member = np.where(self.idx >= 0, self.idx, T.NPOOL)
        return table[(self.sgn < 0).astype(np.int64), member, self.rep]

    def scalars(self, name):
        got = self._scalars.get(name)
        if got is None:
            if name == "final":
                got = T.set_scalars([np.zeros(self.nb, dtype=np.int64)], 1, self.idx, self.sgn, self.pool_k,
                                    weights=np.arange(1, self.nb + 1, dtype=np.int64))
            else:
                ids, n = T.set_ids(self.bits, name)
                got = T.set_scalars(ids, n, self.idx, self.sgn, self.pool_k)
            self._scalars[name] = got
        return got


@functools.lru_cache(maxsize=None)
def crafted_arrays(bits):
    """{name: Crafted} — (i) random x 4, (ii) all identity, (iv) one point everywhere x 2, (v) +-P at every stride, (vi) = (i) at the
    largest representatives; the arrays of (iii) are all identity with one slot written (one_bucket)"""
    nb = 1 << bits
    rnd = np.random.RandomState(1900 + bits)
    out = {}
    for j in range(4 if bits == 15 else 1):            # (2^19: 9000 sums per array, each a multiplication of its own)
        idx = np.where(rnd.randint(0, 2, nb) == 1, rnd.randint(0, T.NPOOL, nb), -1)
        sgn = rnd.choice([-1, 1], nb)
        out["random %d" % j] = Crafted("random %d" % j, bits, idx, sgn, rnd.randint(0, T.NREP - 1, nb))
        out["largest %d" % j] = Crafted("largest %d" % j, bits, idx, sgn, np.full(nb, T.NREP - 1))
    none, one = np.full(nb, -1), np.ones(nb)
    out["all identity"] = Crafted("all identity", bits, none, one, rnd.randint(0, T.NREP, nb))
    out["one point, identical slots"] = Crafted("one point, identical slots", bits, np.full(nb, 5), one, np.full(nb, 1))
    out["one point, varying Z"] = Crafted("one point, varying Z", bits, np.full(nb, 7), one, rnd.randint(0, T.NREP, nb))
    b = np.arange(nb)
    for s in (1, 2, 4, 8, 16, 32, 64):
        # +-P with the sign changing every s buckets along a row and every s rows along a column: the sums cancel inside a lane's
        # serial chain (s below the lane's stride), at the first level of the tree or at its last, whatever the kernel's shape
        sgn = np.where((((b & 127) // s) ^ ((b >> 7) // s)) & 1, -1, 1)
        out["+-P every %d" % s] = Crafted("+-P every %d" % s, bits, np.full(nb, 9), sgn, rnd.randint(0, T.NREP - 1, nb))
    return out


def ONE_BUCKET(nb):
    """(iii): where the only non-identity bucket of an array sits"""
    return 0, 1, 127, 128, nb // 2 - 1, nb // 2, nb - 128, nb - 1


def one_bucket(bits, b):
    nb = 1 << bits
    idx = np.full(nb, -1)
    idx[b] = 11 + (b % 7)
    return Crafted("one bucket, %d" % b, bits, idx, np.ones(nb), np.zeros(nb))


def groups_of(names):
    """every array in a group of 1, of 2 and of 4, a different array per commitment"""
    out = [[n] for n in names]
    for g in (2, 4):
        out += [names[i:i + g] if i + g <= len(names) else names[-g:] for i in range(0, len(names), g)]
    return out


class Tail:
    """phase 2 over device-resident bucket arrays"""

    def __init__(self, rig, bits):
        self.rig, self.bits, self.nb = rig, bits, 1 << bits
        self.arrays = dict(crafted_arrays(bits))
        for b in ONE_BUCKET(self.nb):
            a = one_bucket(bits, b)
            self.arrays[a.name] = a
        self.w = rig.work(300)
        for a in self.arrays.values():
            if a.dev is None:
                a.dev = rig.alloc(SLOT * self.nb, keep=True)
                if a.name.startswith("one bucket"):
                    ident = self.arrays["all identity"]
                    rig.copy(a.dev.ptr, ident.dev.ptr, SLOT * self.nb)
                    b = int(np.nonzero(a.idx >= 0)[0][0])
                    rig.write(a.dev.ptr + SLOT * b, T.pool_slots()[0, a.idx[b], a.rep[b]])
                else:
                    rig.write(a.dev.ptr, a.words())

    def close(self):
        for a in self.arrays.values():
            if a.dev is not None:
                a.dev.free()
                a.dev = None

    def run(self, names, rows, variant, bit_sums=True, **switches):
        rig, w, bits, nb = self.rig, self.w, self.bits, self.nb
        g = len(names)
        what = "%s, group %r, rows %d" % (variant, names, rows)
        rig.fill_small(w)
        rig.fill_buckets(w)
        for kb, n in enumerate(names):
            rig.copy(w.buckets + SLOT * nb * kb, self.arrays[n].dev.ptr, SLOT * nb)
        table = w.buckets                                         # never read by phase 2; any device pointer
        rc, rep = rig.phase(2, bits, rows, table, 300, [300] * g, cfg(**switches), bit_sums=bit_sums)
        assert rc == 0, "%s: phase 2 returned %d" % (what, rc)
        rb = T.rowbits(bits)
        assert rep.last_rowbits == rb, what
        # ---- chunk
        chunk = rig.read(w.chunk, 64 * CHUNK_SLOTS).reshape(CHUNK_SLOTS, 64)
        written = np.zeros(CHUNK_SLOTS, dtype=bool)
        if bits == 15:
            layout = [("rc" if (switches.get("tail_serial") or not bit_sums) else "rcq", 0)]
        else:
            layout = [("rc1", 0), ("rc2", 8192 * KB)]
        for set_name, base in layout:
            nsets = T.set_ids(bits, set_name)[1]
            for kb, n in enumerate(names):
                exp = self.arrays[n].scalars(set_name)
                first = base + nsets * kb
                written[first:first + nsets] = True
                for s in range(nsets):
                    expect_slot(chunk[first + s], exp[s], "%s: commitment %d (%s): %s[%d]" % (what, kb, n, set_name, s))
                    if set_name == "rc2" and 384 <= s < 512:
                        assert T.decode_slot(chunk[first + s]) is None
        assert kept(chunk[~written]), "%s: chunk was written outside the sums of the %d launched commitments" % (what, g)
        # ---- output slots
        outs = rig.read(rig.outs.ptr, 48 * T.BIT_SUMS * KB + 48).reshape(T.BIT_SUMS * KB + 1, 48)
        done = np.zeros(T.BIT_SUMS * KB + 1, dtype=bool)
        for kb, n in enumerate(names):
            a = self.arrays[n]
            first = T.BIT_SUMS * kb
            if not bit_sums:
                expect_out(outs[first], a.scalars("final")[0] if rows != S.ROWS_BITPOS else
                           (2 * a.scalars("final")[0] - a.scalars("out")[rb + 8]) % Q, "%s: commitment %d (%s): the result" % (what, kb, n))
                done[first] = True
                continue
            exp = a.scalars("out")
            # S (slot rb + 8) is written for bit-position rows only — by the quad kernel; msm_bits_kernel of the serial tail writes it always
            for j in range(rb + 9 if (rows == S.ROWS_BITPOS or switches.get("tail_serial")) else rb + 8):
                expect_out(outs[first + j], exp[j], "%s: commitment %d (%s): output slot %d" % (what, kb, n, j))
                done[first + j] = True
            assert T.finish_scalar(exp, rb, False) == a.scalars("final")[0]
        assert kept(outs[~done]), "%s: an output slot that this launch does not own was written (slots %r)" \
            % (what, np.nonzero(~done & ~(outs.view(np.uint8) == 0xA5).all(axis=1))[0].tolist())
        # ---- buckets: phase 2 only reads them
        for kb in range(g, KB):
            assert rig.untouched(w.buckets + SLOT * nb * kb, SLOT * nb), "%s: buckets of commitment %d, not launched, were written" % (what, kb)


@pytest.fixture(scope="module")
def tail15(rig):
    t = Tail(rig, 15)
    yield t
    t.close()


@pytest.fixture(scope="module")
def tail19(rig):
    t = Tail(rig, 19)
    yield t
    t.close()


def run_all(tail, variant, rows_cycle, bit_sums=True, **switches):
    rig = tail.rig
    w = tail.w = rig.work(300)                                # (partial and seg_sum move when a test between reserved for more terms)
    rig.fill_big(w)
    for i, names in enumerate(groups_of(sorted(tail.arrays))):
        tail.run(names, rows_cycle[i % len(rows_cycle)], variant, bit_sums=bit_sums, **switches)
    assert rig.untouched(w.partial, SLOT * w.cap_slices * KB), "%s: phase 2 wrote to partial" % variant
    assert rig.untouched(w.seg_sum, SLOT * w.cap_segs * KB), "%s: phase 2 wrote to seg_sum" % variant


@pytest.mark.parametrize("wv", (1, 2, 4))
def test_tail_2_15_quad(tail15, wv):
    """msm_rowcol_quad_kernel<wv> + msm_bits_quad_kernel for every group size (rcwv = wv wv wv); the S slot for bit-position rows"""
    run_all(tail15, "rowcol_quad<%d>" % wv, (S.ROWS_BITPOS, S.ROWS_WINDOW, S.ROWS_HALFPOS), rcwv=111 * wv)


def test_tail_2_15_serial(tail15):
    """msm_rowcol_kernel + msm_bits_kernel"""
    run_all(tail15, "tail_serial", (S.ROWS_WINDOW, S.ROWS_BITPOS), tail_serial=1)


def test_tail_2_15_final(tail15):
    """msm_rowcol_kernel + msm_final_kernel: one point per commitment, [sum (b + 1) k_b]G (bit-position rows: 2 W - S)"""
    run_all(tail15, "final", (S.ROWS_WINDOW, S.ROWS_BITPOS), bit_sums=False)


@pytest.mark.parametrize("lps,lane_tree", [(4, 0), (8, 0), (16, 0), (32, 0), (8, 1)])
def test_tail_2_19(tail19, lps, lane_tree):
    """msm_rowcol_tp_kernel<lps, quad tree / lane tree> + msm_fold_quad_kernel + msm_bits_quad_kernel (outputs shifted by E = 4)"""
    run_all(tail19, "rowcol_tp<%d, %s>" % (lps, "lane" if lane_tree else "quad"), (S.ROWS_BITPOS, S.ROWS_QUARTERPOS, S.ROWS_HALFPOS),
            lps=lps, rc_lane_tree=lane_tree)


# =====================================================================================================================
# C. accumulation, bucket sums and heavy buckets on a crafted table (phase 1, the real sort in front), then phase 2
# =====================================================================================================================
FR_R = (1 << 256) % Q
BIG_BUCKET_SLICES = 300            # a designated bucket of more slices has 64 of them compared (the first and last among them)


def put_scalars(rig, scalars):
    m = S.length(scalars)
    host = np.zeros((m, 32), dtype=np.uint8)
    for i, s in S.nonzero(scalars):
        host[i] = np.frombuffer((s * FR_R % Q).to_bytes(32, "little"), dtype=np.uint8)
    buf = rig.alloc(32 * m)
    rig.write(buf.ptr, host)
    return buf


def put_table(rig, rows, table_n, tables_and_models):
    """the whole table 0xA5, then the entries the models say are read"""
    tbl = rig.alloc(128 * rows * table_n)
    rig.fill(tbl.ptr, 128 * rows * table_n)
    for table, md in tables_and_models:
        used = np.unique(md.entries & np.uint32(0x7FFFFFFF)).astype(np.uint32)
        words = np.ascontiguousarray(table.entry_words(used))
        assert rig.lib.dmt_scatter(rig.h, tbl.ptr, rows * table_n, used.ctypes.data, words.ctypes.data, len(used)) == 0
    return tbl


def check_phase1(rig, w, kb, md, inp, rule, what, events=None):
    """partial (slice by slice for the designated buckets) and buckets of commitment kb after phase 1"""
    bits, nb, ksl = md.bits, md.nb, md.ksl
    offsets = rig.read(w.offsets + 4 * kb * (nb + 1), nb + 1)
    slice_off = rig.read(w.slice_off + 4 * kb * (nb + 1), nb + 1)
    S.check_scan(md, kb, "offsets", offsets, md.offsets)
    S.check_scan(md, kb, "slice_off", slice_off, md.slice_off)
    entries = rig.read(w.entries + 4 * kb * 16 * w.cap_m, md.total)
    S.check_entries(md, kb, entries)
    nsl = int(md.slice_off[nb])
    partial = rig.read(w.partial + SLOT * kb * w.cap_slices, 64 * nsl).reshape(nsl, 64)
    buckets = rig.read(w.buckets + SLOT * kb * nb, 64 * nb).reshape(nb, 64)
    ej, esg = T.entry_terms(inp.table, entries)
    term = [(T.TABLE_K[j] if sg > 0 else Q - T.TABLE_K[j]) for j, sg in zip(ej.tolist(), esg.tolist())]
    rnd = random.Random(nb + nsl)
    written = np.zeros(nsl, dtype=bool)
    for b in sorted(inp.entries_of):
        lo, hi, so, ns = int(offsets[b]), int(offsets[b + 1]), int(slice_off[b]), int(md.ns[b])
        direct = rule.direct and ns == 1
        if not direct:
            written[so:so + ns] = True
        qs = range(ns) if ns <= BIG_BUCKET_SLICES else sorted({0, ns - 1, 127, 128} | set(rnd.sample(range(ns), 60)))
        for q in qs:
            terms = term[lo + q * ksl:min(lo + (q + 1) * ksl, hi)]
            k, ev = T.chain_events(terms)
            if events is not None and b in inp.chains:
                events |= ev
            if direct:
                assert kept(partial[so]), "%s: commitment %d: partial[%d] of bucket %d, which is one slice written directly, was written" % (what, kb, so, b)
            else:
                expect_slot(partial[so + q], k, "%s: commitment %d: partial[%d], slice %d of bucket %d (%d entries)" % (what, kb, so + q, q, b, hi - lo))
    # every slice of a bucket of one slice is skipped by a direct launch, every other slice is written
    one = np.repeat(md.ns == 1, md.ns) if nsl else np.zeros(0, dtype=bool)
    is_kept = (partial.view(np.uint8) == 0xA5).all(axis=1)
    bad = np.nonzero(is_kept != (one & rule.direct))[0]
    assert not len(bad), "%s: commitment %d: partial[%d] is %s" % (what, kb, bad[0], "untouched" if is_kept[bad[0]] else "written")
    # ---- buckets
    nonempty = np.nonzero(md.counts)[0]
    compact = np.full(nb, -1, dtype=np.int64)
    compact[nonempty] = np.arange(len(nonempty))
    ks = T.sums_by(inp.table, md.entries, [compact[md.bucket_of]], len(nonempty))
    sample = set(inp.entries_of) | set(rnd.sample(nonempty.tolist(), min(512, len(nonempty))))
    for b in sorted(sample):
        expect_slot(buckets[b], ks[compact[b]], "%s: commitment %d: bucket %d (%d entries, %d slices)" % (what, kb, b, md.counts[b], md.ns[b]))
    want = np.zeros(64, dtype=np.uint32) if rule.empty == "zero" else np.array(T.IDENTITY_SLOT, dtype=np.uint32)
    bad = np.nonzero((md.counts == 0) & (buckets != want).any(axis=1))[0]
    assert not len(bad), "%s: commitment %d: the empty bucket %d does not hold %s" % (what, kb, bad[0], rule.empty)
    bad = np.nonzero((md.counts > 0) & (buckets.view(np.uint8) == 0xA5).all(axis=1))[0]
    assert not len(bad), "%s: commitment %d: bucket %d (%d entries) was not written" % (what, kb, bad[0], md.counts[bad[0]])
    return dict(zip(nonempty.tolist(), ks))


def check_bit_sums(rig, kb, md, inp, rows, serial, what):
    rb = T.rowbits(md.bits)
    ids, n = T.set_ids(md.bits, "out")
    exp = T.sums_by(inp.table, md.entries, [row[md.bucket_of] for row in ids], n)
    outs = rig.read(rig.outs.ptr + OUT * T.BIT_SUMS * kb, 48 * T.BIT_SUMS).reshape(T.BIT_SUMS, 48)
    nout = rb + 9 if (rows == S.ROWS_BITPOS or serial) else rb + 8
    for j in range(nout):
        expect_out(outs[j], exp[j], "%s: commitment %d: output slot %d" % (what, kb, j))
    assert kept(outs[nout:]), "%s: commitment %d: an output slot past %d was written" % (what, kb, nout - 1)


@pytest.mark.parametrize("name", [c[0] for c in T.PHASE1_LAUNCHES])
def test_phase1(rig, name):
    bits, rows, mmax, sw, rule, inp = T.phase1_case(name)
    nb, c = 1 << bits, cfg(**sw)
    md = S.sort_model(inp.scalars, rows, mmax, bits, rule.ksl, rule.heavy_thresh)
    w = rig.work(mmax, c)
    tbl = put_table(rig, rows, mmax, [(inp.table, md)])
    sc = put_scalars(rig, inp.scalars)
    rig.fill_small(w)
    rig.fill_big(w)
    rig.fill_buckets(w)
    rc, rep = rig.phase(1, bits, rows, tbl.ptr, mmax, [mmax], c, scalars=[sc])
    assert rc == 0, "%s: phase 1 returned %d" % (name, rc)
    assert (rep.ksl, rep.heavy_thresh, rep.ordered) == (rule.ksl, rule.heavy_thresh, int(rule.ordered)), \
        "%s: the launch chose ksl %d, heavy_thresh %d, ordered %d" % (name, rep.ksl, rep.heavy_thresh, rep.ordered)
    events = set()
    check_phase1(rig, w, 0, md, inp, rule, name, events)
    assert events >= {"pair", "double", "cancel+", "identity"}, "%s: the chain buckets met only %r" % (name, sorted(events))
    nsl, nsegs = int(md.slice_off[nb]), sum(md.heavy.values())
    assert rig.untouched(w.partial + SLOT * nsl, SLOT * (w.cap_slices * KB - nsl)), "%s: partial was written past the %d slices of commitment 0" % (name, nsl)
    assert rig.untouched(w.seg_sum + SLOT * nsegs, SLOT * (w.cap_segs * KB - nsegs)), "%s: seg_sum was written past the %d segments of commitment 0" % (name, nsegs)
    assert rig.untouched(w.buckets + SLOT * nb, SLOT * (NB_MAX * KB - nb)), "%s: buckets were written past commitment 0" % name
    assert rig.untouched(w.chunk, SLOT * CHUNK_SLOTS) and rig.untouched(rig.outs.ptr, OUT * T.BIT_SUMS * KB + OUT), "%s: phase 1 wrote to chunk or to an output slot" % name
    rc, rep = rig.phase(2, bits, rows, tbl.ptr, mmax, [mmax], c)
    assert rc == 0 and rep.last_rowbits == T.rowbits(bits)
    check_bit_sums(rig, 0, md, inp, rows, bool(sw.get("tail_serial")), name + ", phase 2")
    assert kept(rig.read(rig.outs.ptr + OUT * T.BIT_SUMS, 48 * T.BIT_SUMS * (KB - 1) + 48)), "%s: phase 2 wrote to the output slots of another commitment" % name


def test_a_group_of_three_by_columns(rig):
    """phase 1 for column 0, then column 1 alone, then column 2 alone (the only one with heavy buckets), phase 2 once"""
    bits, rows, m, sw = 15, S.ROWS_WINDOW, 300, dict(ksl=4)
    nb, c = 1 << bits, cfg(**sw)
    rule = T.launch_rule(bits, m, ksl=4)
    light = {b: ns for b, ns in T.slice_plan(bits, rule.lanes, rule.heavy_thresh, False).items() if ns <= rule.heavy_thresh and b < 64}
    heavy = {b + 30: ns for b, ns in T.slice_plan(bits, rule.lanes, rule.heavy_thresh, False).items() if ns <= T.HEAVY_SEG + 1 and b < 64}
    inps = [T.phase1_input(bits, rows, m, 4, light, 900, chains=10), T.phase1_input(bits, rows, m, 4, light, 901, chains=0),
            T.phase1_input(bits, rows, m, 4, heavy, 902, chains=0)]
    inps[1].table = inps[2].table = inps[0].table          # one table for the group: the special entries are those of column 0
    mds = [S.sort_model(i.scalars, rows, m, bits, 4, rule.heavy_thresh) for i in inps]
    assert not mds[0].heavy and not mds[1].heavy and sum(mds[2].heavy.values()) >= 4 and max(mds[2].heavy.values()) >= 2
    w = rig.work(m, c)
    tbl = put_table(rig, rows, m, [(i.table, md) for i, md in zip(inps, mds)])
    scs = [put_scalars(rig, i.scalars) for i in inps]
    rig.fill_small(w)
    rig.fill_big(w)
    rig.fill_buckets(w)
    rig.fill(w.nheavy, 4 * 4 * KB)

    def region(kb):
        return [rig.read(w.partial + SLOT * kb * w.cap_slices, 64 * int(mds[kb].slice_off[nb])), rig.read(w.buckets + SLOT * kb * nb, 64 * nb),
                rig.read(w.nheavy, 4 * KB)[[2 * kb, 2 * kb + 1]]]

    done = {}
    for kb in range(3):
        rc, rep = rig.phase(1, bits, rows, tbl.ptr, m, [m] * 3, c, scalars=scs, kb0=kb, count=1)
        what = "column %d alone" % kb
        assert rc == 0, what
        check_phase1(rig, w, kb, mds[kb], inps[kb], rule, what)
        done[kb] = region(kb)
        for other in range(KB):
            if other in done:
                for name, a, b in zip(("partial", "buckets", "nheavy"), region(other), done[other]):
                    assert (a == b).all(), "%s: %s of commitment %d, launched before, changed" % (what, name, other)
            else:
                assert rig.untouched(w.partial + SLOT * other * w.cap_slices, SLOT * w.cap_slices), "%s: partial of commitment %d was written" % (what, other)
                assert rig.untouched(w.seg_sum + SLOT * other * w.cap_segs, SLOT * w.cap_segs), "%s: seg_sum of commitment %d was written" % (what, other)
                assert rig.untouched(w.buckets + SLOT * other * nb, SLOT * nb), "%s: buckets of commitment %d were written" % (what, other)
                assert kept(rig.read(w.nheavy, 4 * KB)[[2 * other, 2 * other + 1, 2 * KB + other]]), "%s: nheavy of commitment %d was written" % (what, other)
        assert rig.untouched(w.chunk, SLOT * CHUNK_SLOTS), what
    rc, rep = rig.phase(2, bits, rows, tbl.ptr, m, [m] * 3, c)
    assert rc == 0
    for kb in range(3):
        check_bit_sums(rig, kb, mds[kb], inps[kb], rows, False, "phase 2 over the group")
    assert kept(rig.read(rig.outs.ptr + OUT * T.BIT_SUMS * 3, 48 * T.BIT_SUMS + 48))
