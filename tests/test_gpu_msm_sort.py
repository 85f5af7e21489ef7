"""GPU: the bucket sort of plonk_amd/csrc/msm_sort.hip (msm_group_sort of both compiled bucket counts) on its own, every
output array against the big-int model of tests/msm_sort_model.py — which states what the accumulation and bucket-sum
kernels read — at the populations where its twelve kernels take another path: a coarse bin of 10240 / 10241 words (register
cache and LDS staging of msm_fine_kernel), of 65536 / 65537 (BIG_LIMIT), an oversized last bin, a last chunk of one word,
buckets of heavy_thresh slices and one entry more, of 128 and 129 slices, every slice length, ordered and not, a group
launched whole and by columns, the tail / split forms of a scalar array, and table indices up to bit 30.

The sort is reached through tests/_build/libdev_msm_sort.so (tests/csrc/dev_msm_sort.hip, built by build(): doors only, the
kernels are libplonk_hip.so's).  Before every call entries, offsets, slice_off, full_off, part_list, multi_list, heavy_list,
nheavy, buckets and the sort's scratch are filled with 0xA5; after it every word of every output of the launched
commitments is compared or shown untouched, and the neighbouring commitment's regions are untouched.  All comparisons are
exact; a failure names the commitment, the array, the first differing bucket and its coarse bin.  The designed inputs are
those tests/test_msm_sort_model_host.py shows to have the populations their names claim.

No upload exceeds 2^19 + 1 scalars, so the tables of 2^31 entries (256 rows x 2^23 points) are indexed with i < 2^19 only: the
row term alone sets bits 24 .. 30 of those entries.  Where m = table_n the top entry is rows * table_n - 1 for the recodings
that reach their last row; a row per bit position never does (no digit starts above bit 254), the model says which row it is.

On an MI355X every case takes under a second (the slowest, 0.7 s: the eleven launches of a recoding over 2^19 buckets and the
group over 2^19 buckets) and the file about ten seconds."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import msm_sort_model as S
from oracle.bls12_381 import Q

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_msm_sort.so")
ERR_ARG = -1
NB_MAX = 1 << 19
KB = S.MAX_BATCH
R = (1 << 256) % Q
SCANS = ("offsets", "slice_off", "full_off", "part_list")


class Work(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("entries", "offsets", "slice_off", "full_off", "part_list", "multi_list", "nheavy",
                                                "heavy_list", "buckets", "tmp_words")] + [("cap_m", ctypes.c_uint64), ("cap_slices", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(SO), "tests/_build/libdev_msm_sort.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dms_group_sort.argtypes = [vp, ci, u32, u64, ci, ci, ci, vp, vp, vp, vp, u32, u32, u32, ci, ci]
    so.dms_work.argtypes = [vp, u64, vp]
    so.dms_fill.argtypes = [vp, vp, ci, u64]
    so.dms_read.argtypes = [vp, vp, vp, u64]
    so.dms_needs_wide.argtypes = [ci, u32, u64]
    return so


_mont = {0: bytes(32)}


def mont(s: int) -> bytes:
    b = _mont.get(s)
    if b is None:
        b = (s % Q * R % Q).to_bytes(32, "little")
        if len(_mont) < (1 << 18):
            _mont[s] = b
    return b


class Rig:
    """one context, its work buffers and the device arrays of the current test"""

    def __init__(self, lib):
        import plonk_amd
        self.ctx, self.lib, self.bufs = plonk_amd.Context(0), lib, []
        self.h = self.ctx.handle

    def close(self):
        self.free()
        self.ctx.close()

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def put(self, scalars):
        """the scalars in Montgomery form on the device (a sparse set: a cleared buffer and its few elements)"""
        m = S.length(scalars)
        b = self.ctx.alloc(32 * max(m, 1))
        self.bufs.append(b)
        if isinstance(scalars, S.Sparse):
            assert self.lib.dms_fill(self.h, b.ptr, 0, 32 * m) == 0
            for i, s in scalars.items.items():
                b.upload(mont(s), 32 * i)
        elif m:
            b.upload(b"".join(mont(s) for s in scalars))
        return b

    def work(self, mmax) -> Work:
        w = Work()
        assert self.lib.dms_work(self.h, mmax, ctypes.byref(w)) == 0
        assert w.cap_m >= mmax
        return w

    def fill(self, w: Work):
        cap = 16 * w.cap_m
        for ptr, nbytes in ((w.entries, 4 * cap * KB), (w.tmp_words, 8 * cap * KB), (w.multi_list, 4 * NB_MAX * KB),
                            (w.heavy_list, 16 * NB_MAX * KB), (w.buckets, 256 * NB_MAX * KB), (w.nheavy, 4 * 4 * KB)) \
                + tuple((getattr(w, n), 4 * (NB_MAX + 1) * KB) for n in SCANS):
            assert self.lib.dms_fill(self.h, ptr, 0xA5, nbytes) == 0

    def read(self, ptr, count, dtype=np.uint32):
        a = np.empty(count, dtype=dtype)
        assert self.lib.dms_read(self.h, ptr, a.ctypes.data, a.nbytes) == 0
        return a

    def sort(self, bits, rows, table_n, bufs, ms, ksl, ht, ordered, kb0=0, count=None, wide=-1, sort13=0, tails=None, splits=None):
        n = len(ms)
        vps, u64s = ctypes.c_void_p * n, ctypes.c_uint64 * n
        tails = tails or [None] * n
        return self.lib.dms_group_sort(self.h, bits, rows, table_n, n, kb0, n - kb0 if count is None else count,
                                       vps(*[b.ptr for b in bufs]), u64s(*ms), vps(*[t.ptr if t else None for t in tails]),
                                       u64s(*(splits or [0] * n)), ksl, ht, int(ordered), wide, sort13)


@pytest.fixture(scope="module")
def small(lib):
    r = Rig(lib)
    yield r
    r.close()


@pytest.fixture(scope="module")
def big(lib):
    """the inputs of more than 2^15 scalars have a context of their own: the work buffers of a context never shrink, and every
    case downloads the whole entry region of its commitments"""
    r = Rig(lib)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def release(request):
    yield
    for name in ("small", "big"):
        if name in request.fixturenames:
            request.getfixturevalue(name).free()


def untouched(a) -> bool:
    return bool((a.view(np.uint8) == 0xA5).all())


def region(rig, w, bits, kb, name):
    nb = 1 << bits
    if name in SCANS:
        return rig.read(getattr(w, name) + 4 * kb * (nb + 1), nb + 1)
    if name == "entries":
        return rig.read(w.entries + 4 * kb * 16 * w.cap_m, 16 * w.cap_m)
    if name == "heavy_list":
        return rig.read(w.heavy_list + 16 * kb * nb, 4 * nb)
    if name == "multi_list":
        return rig.read(w.multi_list + 4 * kb * nb, nb)
    assert name == "buckets"
    return rig.read(w.buckets + 256 * kb * nb, 32 * nb, np.uint64)


def check_commitment(rig, w, md, kb, ordered, what=""):
    """every output of commitment kb against the model md"""
    bits = md.bits
    try:
        S.check_scan(md, kb, "offsets", region(rig, w, bits, kb, "offsets"), md.offsets)
        S.check_entries(md, kb, region(rig, w, bits, kb, "entries"))
        S.check_scan(md, kb, "slice_off", region(rig, w, bits, kb, "slice_off"), md.slice_off)
        nheavy = rig.read(w.nheavy, 4 * KB)
        S.check_heavy(md, kb, nheavy, region(rig, w, bits, kb, "heavy_list"))
        if bits == 15 and not ordered:
            for name in ("full_off", "part_list"):
                assert untouched(region(rig, w, bits, kb, name)), "commitment %d: %s was written by a launch that is not ordered" % (kb, name)
        else:
            S.check_scan(md, kb, "full_off", region(rig, w, bits, kb, "full_off"), md.full_off)
            S.check_part_list(md, kb, region(rig, w, bits, kb, "part_list"))
        if bits > 15:
            S.check_multi(md, kb, nheavy, region(rig, w, bits, kb, "multi_list"))
            S.check_buckets(md, kb, region(rig, w, bits, kb, "buckets"))
        else:
            assert nheavy[2 * KB + kb] == 0, "commitment %d: nheavy[2 KB + kb] is %#x over 2^15 buckets" % (kb, nheavy[2 * KB + kb])
            assert untouched(region(rig, w, bits, kb, "multi_list")), "commitment %d: multi_list was written over 2^15 buckets" % kb
    except AssertionError as e:
        raise AssertionError("%s%s" % (what and what + ": ", e)) from None


def check_untouched(rig, w, bits, kb, what="", buckets=False, whole_group=False):
    """nothing of commitment kb's regions (as this bucket count lays them out) was written; the launch of a WHOLE group clears
    the counters of all four commitments, a column launch only its own"""
    for name in SCANS + ("entries", "heavy_list", "multi_list") + (("buckets",) if buckets else ()):
        assert untouched(region(rig, w, bits, kb, name)), "%s: %s of commitment %d, which was not launched, was written" % (what, name, kb)
    nheavy = rig.read(w.nheavy, 4 * KB)
    assert all(int(nheavy[i]) == (0 if whole_group else S.UNTOUCHED) for i in (2 * kb, 2 * kb + 1, 2 * KB + kb)), \
        "%s: nheavy of commitment %d, which was not launched, was written" % (what, kb)


def run_one(rig, bits, rows, scalars, ksl, ht, ordered, table_n=None, sort13=0, want_wide=None, what=""):
    """one commitment, launched alone, checked whole; its neighbour's regions stay untouched"""
    m = S.length(scalars)
    table_n = m + 3 if table_n is None else table_n
    w = rig.work(m)
    rig.fill(w)
    buf = rig.put(scalars)
    if want_wide is not None:
        assert rig.lib.dms_needs_wide(bits, rows, table_n) == want_wide, what
    rc = rig.sort(bits, rows, table_n, [buf], [m], ksl, ht, ordered, sort13=sort13)
    assert rc == 0, "%s: msm_group_sort returned %d" % (what, rc)
    md = S.sort_model(scalars, rows, table_n, bits, ksl, ht)
    check_commitment(rig, w, md, 0, ordered, what)
    check_untouched(rig, w, bits, 1, what, whole_group=True)
    buf.free()
    rig.bufs.remove(buf)
    return md


# =====================================================================================================================
# recodings and sizes
# =====================================================================================================================
SIZES = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4097)        # around the tiles of the histogram and partition passes (2048, 1024)


@functools.lru_cache(maxsize=None)
def uniform(m, seed=0):
    return S.uniform_with_edges(m, 5000 + m + seed)


@pytest.mark.parametrize("bits,rows,sort13", [(15, 16, 0), (15, 64, 0), (15, 128, 0), (15, 256, 0), (19, 256, 0), (19, 128, 0), (19, 64, 0),
                                              (19, 256, 1), (19, 128, 1)])
def test_every_recoding_at_the_tile_edges(small, bits, rows, sort13):
    """uniform scalars with the edge scalars of test_edge_scalars among them, m around the tile sizes; the lanes ordered for every
    second size; sort13: the two-workgroups-per-CU partition pass of the 2^19-bucket variant"""
    for k, m in enumerate(SIZES):
        run_one(small, bits, rows, uniform(m), 4, 16, ordered=k % 2, sort13=sort13, what="m = %d" % m)
    run_one(small, bits, rows, S.EDGE_SCALARS, 8, 16, ordered=1, sort13=sort13, what="the edge scalars alone")
    run_one(small, bits, rows, [0] * 50, 8, 16, ordered=1, sort13=sort13, what="all zero")


def test_window_rows_over_2_19_buckets_are_refused(small):
    w = small.work(300)
    small.fill(w)
    buf = small.put(uniform(300))
    assert small.sort(19, S.ROWS_WINDOW, 303, [buf], [300], 32, 16, 1) == ERR_ARG
    check_untouched(small, w, 19, 0, "refused")


# =====================================================================================================================
# designed coarse bins
# =====================================================================================================================
@pytest.mark.parametrize("bits", (15, 19))
@pytest.mark.parametrize("name", ("bins_at_the_edges", "oversized_last_bin", "last_chunk_of_one_word"))
def test_designed_bins(big, bits, name):
    """bins of exactly 10240 / 10241 / 65536 / 65537 words with five words in bin 2047; an oversized bin 2047 (its first chunk writes
    offsets[NB]); a bin whose last chunk holds one word — window rows over 2^15 buckets, width-21 NAF digits over 2^19"""
    scalars = getattr(S, name)(bits)
    md = run_one(big, bits, S.designed_rows(bits), scalars, 32, 16, ordered=1, what=name)
    assert md.bin_counts.max() > S.FINE_CACHE_WORDS


# =====================================================================================================================
# hot buckets
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def hot(name):
    r, m = random.Random(41), 20000
    return {"equal": [0x1234567890ABCDEF1234567890ABCDEF % Q] * m,                     # one bucket per digit
            "minus_one": [Q - 1] * m,
            "mix": [r.randrange(Q) if i % 3 else 7 for i in range(m)]}[name]           # heavy + uniform buckets


@pytest.mark.parametrize("bits,rows", [(15, 16), (15, 256), (19, 256), (19, 64)])
@pytest.mark.parametrize("name", ("equal", "minus_one", "mix"))
def test_hot_buckets(small, bits, rows, name):
    md = run_one(small, bits, rows, hot(name), 8, 16, ordered=name != "equal", what=name)
    assert md.heavy and max(md.heavy.values()) >= 6


# =====================================================================================================================
# slices
# =====================================================================================================================
@pytest.mark.parametrize("bits", (15, 19))
@pytest.mark.parametrize("ordered", (0, 1))
@pytest.mark.parametrize("ksl", (4, 8, 16, 32, 64, 128))
def test_slice_layout_at_the_designed_bucket_counts(big, bits, ksl, ordered):
    """buckets of 0, 1, ksl - 1, ksl, ksl + 1, heavy_thresh * ksl (+ 1) and 128 * ksl (+ 1) entries, at both ends of the bucket range"""
    md = run_one(big, bits, S.designed_rows(bits), S.slice_edges(bits, ksl, 16), ksl, 16, ordered)
    assert sorted(md.heavy.values()) == [1, 1, 1, 1, 2, 2]


def test_a_slice_length_of_256_is_refused_where_the_layout_cannot_hold_it(small):
    """the ordered layout over 2^15 buckets and both layouts over 2^19 count remainders below 128; the unordered 2^15 layout
    does not, and sorts"""
    scalars = uniform(300)
    w = small.work(300)
    buf = small.put(scalars)
    for bits, rows, ordered in ((15, 16, 1), (19, 256, 1), (19, 256, 0)):
        assert small.sort(bits, rows, 303, [buf], [300], 256, 16, ordered) == ERR_ARG, (bits, ordered)
    small.fill(w)
    assert small.sort(15, 16, 303, [buf], [300], 256, 16, 0) == 0
    check_commitment(small, w, S.sort_model(scalars, 16, 303, 15, 256, 16), 0, 0)


# =====================================================================================================================
# groups and column launches
# =====================================================================================================================
@pytest.mark.parametrize("bits,rows", [(15, 16), (19, 256)])
def test_a_group_whole_and_by_columns(small, bits, rows):
    """four commitments of 2049, 0, 1 and 300 terms as one launch, then as two column launches (kb0 = 0 and kb0 = 2): the same
    outputs, the columns not launched untouched, and the first columns' outputs still there after the second launch"""
    r = random.Random(300)
    first = list(uniform(2049))
    first[100:300:2] = [13] * 100                                    # a heavy and a multi-slice bucket in the first column too: its
    first[301:331:2] = [15] * 15                                     # counters have to survive the launch of the later columns
    sets = [first, [], [Q - 5], [r.randrange(Q) if i % 2 else (11 if i % 20 == 0 else 9) for i in range(300)]]
    ms = [len(s) for s in sets]
    ksl, ht, ordered, table_n = 4, 16, 1, 2100
    mds = [S.sort_model(s, rows, table_n, bits, ksl, ht) for s in sets]
    assert all(mds[k].heavy and mds[k].multi.size for k in (0, 3)) and mds[0].total > 2049 * 10
    w = small.work(max(ms))
    bufs = [small.put(s) for s in sets]

    def scans(kb):
        return [region(small, w, bits, kb, n) for n in SCANS]

    small.fill(w)
    assert small.sort(bits, rows, table_n, bufs, ms, ksl, ht, ordered) == 0
    for kb in range(4):
        check_commitment(small, w, mds[kb], kb, ordered, "one launch")
    whole = [scans(kb) for kb in range(4)]

    small.fill(w)
    assert small.sort(bits, rows, table_n, bufs, ms, ksl, ht, ordered, kb0=0, count=2) == 0
    for kb in (0, 1):
        check_commitment(small, w, mds[kb], kb, ordered, "columns 0, 1")
    for kb in (2, 3):
        check_untouched(small, w, bits, kb, "columns 0, 1", buckets=True)
    assert small.sort(bits, rows, table_n, bufs, ms, ksl, ht, ordered, kb0=2, count=2) == 0
    for kb in range(4):
        check_commitment(small, w, mds[kb], kb, ordered, "columns 2, 3 after 0, 1")
        for name, a, b in zip(SCANS[:3], scans(kb), whole[kb]):
            assert (a == b).all(), (kb, name)

    # a middle column alone: both neighbours stay as they were
    small.fill(w)
    assert small.sort(bits, rows, table_n, bufs, ms, ksl, ht, ordered, kb0=2, count=1) == 0
    check_commitment(small, w, mds[2], 2, ordered, "column 2")
    for kb in (0, 1, 3):
        check_untouched(small, w, bits, kb, "column 2", buckets=True)


@pytest.mark.parametrize("bits", (15, 19))
def test_oversized_bins_in_column_launches(big, bits):
    """two commitments with chunked bins, launched one column at a time over the counters a whole launch of other inputs left
    behind: a column launch clears the chunk counters of its own columns only, and needs no more than that"""
    rows, ksl, ht = S.designed_rows(bits), 32, 16
    sets = [S.oversized_last_bin(bits), S.last_chunk_of_one_word(bits)]
    ms = [len(s) for s in sets]
    table_n = max(ms)
    mds = [S.sort_model(s, rows, table_n, bits, ksl, ht) for s in sets]
    w = big.work(max(ms))
    bufs = [big.put(s) for s in sets]
    assert big.sort(bits, rows, table_n, bufs[::-1], ms[::-1], ksl, ht, 1) == 0          # the same bins, the other way round
    big.fill(w)
    assert big.sort(bits, rows, table_n, bufs, ms, ksl, ht, 1, kb0=1, count=1) == 0
    check_commitment(big, w, mds[1], 1, 1, "column 1")
    check_untouched(big, w, bits, 0, "column 1")
    assert big.sort(bits, rows, table_n, bufs, ms, ksl, ht, 1, kb0=0, count=1) == 0
    for kb in (0, 1):
        check_commitment(big, w, mds[kb], kb, 1, "column 0 after column 1")
    check_untouched(big, w, bits, 2, "column 0 after column 1")


# =====================================================================================================================
# tail and split
# =====================================================================================================================
@pytest.mark.parametrize("bits,rows", [(15, 16), (19, 256), (19, 128)])
def test_scalars_in_two_arrays(small, bits, rows):
    """scalar i from the main array below `split`, from the tail array above: a split at 0, 1, inside a tile, at m - 1 and at m"""
    m = 2049
    scalars = uniform(m)
    table_n, ksl, ht = m, 4, 16
    md = S.sort_model(scalars, rows, table_n, bits, ksl, ht)
    w = small.work(m)
    for split in (0, 1, 1000, m - 1, m):
        small.fill(w)
        # each array holds its part only, followed by scalars that would change the result if an index went past the part
        main = small.put(scalars[:split] + [3] * 8)
        tail = small.put(scalars[split:] + [5] * 8)
        assert small.sort(bits, rows, table_n, [main], [m], ksl, ht, 1, tails=[tail], splits=[split], sort13=split & 1 if bits == 19 else 0) == 0
        check_commitment(small, w, md, 0, 1, "split = %d" % split)
        small.free()


# =====================================================================================================================
# index width
# =====================================================================================================================
def index_scalars(m, rows, bits):
    """digits in the lowest and in the highest row the recoding reaches, at i = 0, at i = m - 1 and at a few places between; every
    other scalar is zero"""
    top = 1 << 254
    items = {0: top + 1, m - 1: top + 1, 1: Q - 1, m // 2: 1, m // 2 + 1: Q - 2, m - 2: random.Random(m).randrange(Q)}
    return S.Sparse(m, items), max(row for row, _, _ in S.digits(top + 1, rows, bits))


INDEX_CASES = [
    # bits, rows, table_n, m, wide words
    (15, 256, 1 << 19, 1 << 19, 0),            # narrow at the limit: 2^27 table entries
    (15, 256, (1 << 19) + 1, (1 << 19) + 1, 1),
    (15, 16, 1 << 23, 1 << 19, 0),             # 2^27 again, the last row reached: bits 23 .. 26 of the index from the row
    (15, 16, (1 << 23) + 1, 1 << 19, 1),
    (15, 256, 1 << 23, 1 << 19, 1),            # 2^31 table entries: the row term alone sets bits 24 .. 30
    (19, 256, 1 << 15, 1 << 15, 0),            # narrow at the limit: 2^23
    (19, 256, (1 << 15) + 1, (1 << 15) + 1, 1),
    (19, 128, 1 << 16, 1 << 16, 0),            # 2^23 with the last row reached: the top entry is 2^23 - 1
    (19, 128, (1 << 16) + 1, (1 << 16) + 1, 1),
    (19, 64, 1 << 17, 1 << 17, 0),
    (19, 256, 1 << 23, 1 << 19, 1),
]


@pytest.mark.parametrize("bits,rows,table_n,m,wide", INDEX_CASES)
def test_index_width(big, bits, rows, table_n, m, wide):
    scalars, top_row = index_scalars(m, rows, bits)
    md = run_one(big, bits, rows, scalars, 4, 16, 1, table_n=table_n, want_wide=wide)
    top = int((md.entries & 0x7FFFFFFF).max())
    assert top == top_row * table_n + m - 1 and int((md.entries & 0x7FFFFFFF).min()) == 0
    assert top_row == rows - 1 or rows == 256            # a row per bit position: no digit starts above bit 254
    if m == table_n and rows != 256:
        assert top == rows * table_n - 1
    assert (md.entries >> 31).any()


@pytest.mark.parametrize("bits", (15, 19))
def test_a_table_of_more_than_2_31_entries_is_refused(small, bits):
    w = small.work(300)
    small.fill(w)
    buf = small.put(uniform(300))
    assert small.sort(bits, 256, (1 << 23) + 1, [buf], [300], 4, 16, 1) == ERR_ARG
    check_untouched(small, w, bits, 0, "refused")
    assert small.sort(bits, 256, 1 << 23, [buf], [300], 4, 16, 1) == 0
    check_commitment(small, w, S.sort_model(uniform(300), 256, 1 << 23, bits, 4, 16), 0, 1)
