"""Executable statement of what the bucket sort of the MSM (plonk_amd/csrc/msm_sort.hip, msm_group_sort) hands to the
accumulation and bucket-sum kernels of msm.hip, for (scalars, table rows, points per row, bucket bits, slice length, heavy
threshold).  Big integers and numpy, built on the recodings of tests/msm_wide_model.py (each pinned to the product's
msm_recode.cuh by a CPU test of its own).  Not product code.

The contract, per commitment of a group:

  entries     per bucket the MULTISET of sign << 31 | row * table_n + i over the non-zero digits; order inside a bucket free
  offsets     exclusive scan of the bucket counts, [NB] = the total
  slice_off   exclusive scan of ceil(count / ksl), [NB] = the total
  full_off    exclusive scan of count // ksl, [NB] = the total
  part_list   [NB] = number of buckets with count % ksl != 0; those buckets, remainders never increasing along the list,
              every length class a SET (the kernels fill a class with atomics)
  heavy list  the set of (bucket, nseg = ceil(ns / 128)) for ns > heavy_thresh, pad == 0, the ranges [seg_base, seg_base +
              nseg) tile [0, nheavy[2 kb + 1]) exactly, nheavy[2 kb] = the number of heavy buckets
  2^19 buckets only: multi_list = the set of buckets with 2 <= ns <= heavy_thresh, its length in nheavy[2 * 4 + kb]; the
              256-byte slot of `buckets` zero for every empty bucket and untouched for every other

The intermediates (coarse offsets, chunk prefix, coarse-partitioned words) are NOT part of it.  Every check_* below fails
with a message that names the commitment, the array, the first differing bucket and its coarse bin.

Also here: the generators of the designed inputs (single-digit scalars that put an exact number of words into a coarse bin
or a bucket).  tests/test_msm_sort_model_host.py shows through the model alone that each has the population its name
claims; tests/test_gpu_msm_sort.py imports the same generators."""
import random

import numpy as np

from msm_wide_model import bitpos_digits, even_digits, quad_digits, signed_digits
from oracle import bls12_381 as E

Q = E.Q
ROWS_WINDOW, ROWS_QUARTERPOS, ROWS_HALFPOS, ROWS_BITPOS = 16, 64, 128, 256
COARSE = 2048                       # coarse bins of the two-level sort: the top 11 bits of a bucket index
MAX_BATCH = 4                       # commitments per group (MSM_MAX_BATCH)
HEAVY_SEG_SLICES = 128
BIG_LIMIT, BIG_CHUNK = 1 << 16, 1 << 14      # a coarse bin above BIG_LIMIT words is cut into chunks of BIG_CHUNK
FINE_CACHE_WORDS = 512 * 20         # words of a bin msm_fine_kernel keeps in registers (and stages in LDS over 2^19 buckets)
UNTOUCHED = 0xA5A5A5A5              # what the GPU tests fill every output with before a call
VALID = {15: (ROWS_WINDOW, ROWS_QUARTERPOS, ROWS_HALFPOS, ROWS_BITPOS), 19: (ROWS_QUARTERPOS, ROWS_HALFPOS, ROWS_BITPOS)}


def fine_bits(bits: int) -> int:
    return bits - 11


def digit_width(rows: int, bits: int) -> int:
    """msm_sort.hip: 16-bit windows, MSM_NAF_WIDTH = bits + 2, MSM_EVEN_WIDTH = (bits + 1) & ~1, MSM_QUAD_WIDTH = (bits + 1) & ~3"""
    return {ROWS_WINDOW: 16, ROWS_BITPOS: bits + 2, ROWS_HALFPOS: (bits + 1) & ~1, ROWS_QUARTERPOS: (bits + 1) & ~3}[rows]


def row_shift(rows: int, row: int) -> int:
    """table row `row` holds 2^row_shift * P_i"""
    return {ROWS_WINDOW: 16, ROWS_BITPOS: 1, ROWS_HALFPOS: 2, ROWS_QUARTERPOS: 4}[rows] * row


def bucket_weight(rows: int, bucket: int) -> int:
    return 2 * bucket + 1 if rows == ROWS_BITPOS else bucket + 1


_memo = {}


def digits(s: int, rows: int, bits: int):
    """((row, bucket, sign), ...) of the canonical scalar s under the recoding the sort uses for `rows` over 2^bits buckets"""
    assert 0 <= s < Q and rows in VALID[bits], (rows, bits)
    if rows == ROWS_WINDOW and 0 < s <= 32768:                      # the single-digit fast paths the designed inputs live on
        return ((0, s - 1, 0),)
    if rows == ROWS_BITPOS and (s & 1) and s < (1 << (bits + 1)):
        return ((0, s >> 1, 0),)
    key = (s, rows, bits)
    got = _memo.get(key)
    if got is None:
        w = digit_width(rows, bits)
        if rows == ROWS_WINDOW:
            got = tuple((row, abs(d) - 1, int(d < 0)) for row, d in enumerate(signed_digits(s, 16)) if d)
        elif rows == ROWS_BITPOS:
            got = tuple((row, abs(d) >> 1, int(d < 0)) for row, d in bitpos_digits(s, w))
        elif rows == ROWS_HALFPOS:
            got = tuple((row, abs(d) - 1, int(d < 0)) for row, d in even_digits(s, w))
        else:
            got = tuple((row, abs(d) - 1, int(d < 0)) for row, d in quad_digits(s, w))
        assert len(got) <= 16 and all(0 <= row < rows and 0 <= b < (1 << bits) for row, b, _ in got), (hex(s), rows, bits)
        if len(_memo) < (1 << 18):
            _memo[key] = got
    return got


class Sparse:
    """m scalars of which only `items` ({index: scalar}) are not zero"""

    def __init__(self, m: int, items: dict):
        assert all(0 <= i < m for i in items)
        self.m, self.items = m, dict(items)


def length(scalars) -> int:
    return scalars.m if isinstance(scalars, Sparse) else len(scalars)


def nonzero(scalars):
    if isinstance(scalars, Sparse):
        return sorted((i, s % Q) for i, s in scalars.items.items() if s % Q)
    return [(i, s % Q) for i, s in enumerate(scalars) if s and s % Q]


class SortModel:
    pass


def sort_model(scalars, rows: int, table_n: int, bits: int, ksl: int, heavy_thresh: int) -> SortModel:
    nb = 1 << bits
    assert rows * table_n <= (1 << 31) and ksl & (ksl - 1) == 0 and 1 <= ksl <= 256
    bl, el = [], []
    for i, s in nonzero(scalars):
        for row, b, sg in digits(s, rows, bits):
            bl.append(b)
            el.append((sg << 31) | (row * table_n + i))
    md = SortModel()
    md.rows, md.table_n, md.bits, md.nb, md.ksl, md.heavy_thresh = rows, table_n, bits, nb, ksl, heavy_thresh
    bucket = np.array(bl, dtype=np.int64)
    entry = np.array(el, dtype=np.uint32)
    order = np.lexsort((entry, bucket))
    md.entries = entry[order]                      # grouped by bucket, ascending inside a bucket: the canonical form of the multisets
    md.bucket_of = bucket[order]
    md.counts = np.bincount(bucket, minlength=nb).astype(np.int64)
    md.total = int(md.counts.sum())
    md.nfull = md.counts // ksl
    md.rem = md.counts % ksl
    md.ns = md.nfull + (md.rem > 0)

    def scan(v):
        return np.concatenate(([0], np.cumsum(v))).astype(np.uint32)

    md.offsets, md.slice_off, md.full_off = scan(md.counts), scan(md.ns), scan(md.nfull)
    part = np.nonzero(md.rem)[0]
    md.part_list = part[np.lexsort((part, -md.rem[part]))].astype(np.uint32)      # longest first, ties by bucket index
    md.heavy = {int(b): int(-(-md.ns[b] // HEAVY_SEG_SLICES)) for b in np.nonzero(md.ns > heavy_thresh)[0]}
    md.multi = np.nonzero((md.ns >= 2) & (md.ns <= heavy_thresh))[0].astype(np.uint32)
    md.bin_counts = md.counts.reshape(COARSE, -1).sum(axis=1)
    return md


def lanes(md: SortModel):
    """lane -> (bucket, slice of the bucket, first entry inside the bucket, length) as msm_accumulate_ordered reads full_off and
    part_list: the full slices in bucket order (a search in full_off), then the partial slices along part_list"""
    out = []
    nfull_total = int(md.full_off[md.nb])
    owner = np.searchsorted(md.full_off, np.arange(nfull_total), side="right") - 1
    for s, b in enumerate(owner):
        q = s - int(md.full_off[b])
        out.append((int(b), q, q * md.ksl, md.ksl))
    for b in md.part_list:
        out.append((int(b), int(md.nfull[b]), int(md.nfull[b]) * md.ksl, int(md.rem[b])))
    return out


# ---- the checks of one commitment's outputs ------------------------------------------------------------------------------
def fail(md, kb, array, bucket, detail):
    raise AssertionError("commitment %d: %s differs first at bucket %d (coarse bin %d): %s"
                         % (kb, array, bucket, bucket >> fine_bits(md.bits), detail))


def check_scan(md, kb, array, got, want):
    """got: the NB + 1 words of offsets / slice_off / full_off"""
    got = np.asarray(got, dtype=np.uint32)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        fail(md, kb, array, i, "[%d] is %#x, the model says %#x%s" % (i, got[i], want[i], " (the total)" if i == md.nb else ""))


def check_entries(md, kb, region):
    """region: every word of the commitment's part of `entries` (16 * cap_m words); offsets were checked first"""
    region = np.asarray(region, dtype=np.uint32)
    assert md.total <= len(region)
    got = region[:md.total]
    got = got[np.lexsort((got, md.bucket_of))]          # bucket_of never decreases: this sorts INSIDE every bucket only
    bad = np.nonzero(got != md.entries)[0]
    if len(bad):
        p = int(bad[0])
        b = int(md.bucket_of[p])
        lo, hi = int(md.offsets[b]), int(md.offsets[b + 1])
        fail(md, kb, "entries", b, "the bucket's %d entries sorted: %s ..., the model says %s ..."
             % (hi - lo, [hex(x) for x in got[lo:hi][:6]], [hex(x) for x in md.entries[lo:hi][:6]]))
    past = np.nonzero(region[md.total:] != UNTOUCHED)[0]
    assert not len(past), "commitment %d: entries: word %d, past the total of %d, was written (%#x)" \
        % (kb, md.total + past[0], md.total, region[md.total + past[0]])


def check_part_list(md, kb, got):
    got = np.asarray(got, dtype=np.uint32)
    n, want = int(got[md.nb]), md.part_list
    if n != len(want):
        fail(md, kb, "part_list", md.nb, "[NB] is %d, the model counts %d buckets with a remainder" % (n, len(want)))
    lst = got[:n]
    if n and int(lst.max()) >= md.nb:
        p = int(np.nonzero(lst >= md.nb)[0][0])
        fail(md, kb, "part_list", int(want[p]), "position %d holds %#x, no bucket" % (p, lst[p]))
    bad = np.nonzero(md.rem[lst] != md.rem[want])[0]            # the remainders along the list: never increasing, class sizes right
    if len(bad):
        p = int(bad[0])
        fail(md, kb, "part_list", int(lst[p]), "position %d holds a bucket of remainder %d, the model has remainder %d there (bucket %d)"
             % (p, md.rem[lst[p]], md.rem[want[p]], want[p]))
    canon = lst[np.lexsort((lst, -md.rem[lst]))]               # every class as a set
    bad = np.nonzero(canon != want)[0]
    if len(bad):
        p = int(bad[0])
        fail(md, kb, "part_list", int(min(canon[p], want[p])), "the class of remainder %d lists bucket %d, the model %d"
             % (md.rem[want[p]], canon[p], want[p]))
    past = np.nonzero(got[n:md.nb] != UNTOUCHED)[0]
    assert not len(past), "commitment %d: part_list: position %d, past its %d buckets, was written" % (kb, n + past[0], n)


def check_heavy(md, kb, nheavy, region):
    """nheavy: the 4 * MAX_BATCH counters; region: the commitment's NB items of 4 words"""
    items = np.asarray(region, dtype=np.uint32).reshape(-1, 4)
    n, nseg_total = int(nheavy[2 * kb]), int(nheavy[2 * kb + 1])
    want = sorted(md.heavy)
    first = want[0] if want else 0
    if n != len(want):
        fail(md, kb, "nheavy[2 kb]", first, "%d heavy buckets, the model says %d: %r" % (n, len(want), want[:8]))
    got = items[:n]
    got = got[np.argsort(got[:, 0], kind="stable")]
    for (b, base, nseg, pad), wb in zip(got.tolist(), want):
        if b != wb:
            fail(md, kb, "heavy_list", min(b, wb), "lists bucket %d, the model %d" % (b, wb))
        if nseg != md.heavy[wb]:
            fail(md, kb, "heavy_list", wb, "nseg %d for %d slices, the model says %d" % (nseg, md.ns[wb], md.heavy[wb]))
        if pad != 0:
            fail(md, kb, "heavy_list", wb, "pad is %#x" % pad)
    run = 0
    for b, base, nseg, pad in sorted(got.tolist(), key=lambda it: it[1]):
        if base != run:
            fail(md, kb, "heavy_list", b, "seg_base %d where the ranges before it end at %d" % (base, run))
        run += nseg
    if run != nseg_total:
        fail(md, kb, "nheavy[2 kb + 1]", first, "%d segments, the listed ranges end at %d" % (nseg_total, run))
    past = np.nonzero(items[n:] != UNTOUCHED)[0]
    assert not len(past), "commitment %d: heavy_list: item %d, past its %d, was written" % (kb, n + past[0], n)


def check_multi(md, kb, nheavy, region):
    region = np.asarray(region, dtype=np.uint32)
    n = int(nheavy[2 * MAX_BATCH + kb])
    first = int(md.multi[0]) if len(md.multi) else 0
    if n != len(md.multi):
        fail(md, kb, "nheavy[2 KB + kb]", first, "%d listed buckets of 2 .. heavy_thresh slices, the model says %d" % (n, len(md.multi)))
    got = np.sort(region[:n])
    bad = np.nonzero(got != md.multi)[0]
    if len(bad):
        p = int(bad[0])
        fail(md, kb, "multi_list", int(min(got[p], md.multi[p])), "lists bucket %d, the model %d" % (got[p], md.multi[p]))
    past = np.nonzero(region[n:] != UNTOUCHED)[0]
    assert not len(past), "commitment %d: multi_list: position %d, past its %d buckets, was written" % (kb, n + past[0], n)


def check_buckets(md, kb, region):
    """region: the commitment's NB slots of 256 bytes as (NB, 32) uint64"""
    slots = np.asarray(region, dtype=np.uint64).reshape(md.nb, 32)
    zero = (slots == 0).all(axis=1)
    kept = (slots == np.uint64(0xA5A5A5A5A5A5A5A5)).all(axis=1)
    empty = md.counts == 0
    bad = np.nonzero(np.where(empty, ~zero, ~kept))[0]
    if len(bad):
        b = int(bad[0])
        fail(md, kb, "buckets", b, "the slot of %s bucket is %s" % (("an empty", "not zero") if empty[b] else ("a non-empty", "written")))


# ---- designed inputs -----------------------------------------------------------------------------------------------
def designed_rows(bits: int) -> int:
    """the recoding the designed inputs are written for: window rows over 2^15 buckets, width-21 NAF digits over 2^19"""
    return ROWS_WINDOW if bits == 15 else ROWS_BITPOS


def in_bucket(bucket: int, bits: int) -> int:
    """the scalar whose only digit (row 0, positive) falls into `bucket` under designed_rows(bits)"""
    assert 0 <= bucket < (1 << bits)
    return bucket + 1 if bits == 15 else 2 * bucket + 1


def scatter(words, m: int, seed: int):
    """the scalars `words` at random places among m - len(words) zeros, so that every tile of the partition pass holds a share of every bin"""
    assert len(words) <= m
    out = list(words) + [0] * (m - len(words))
    random.Random(seed).shuffle(out)
    return out


def bin_words(bits: int, bin_: int, count: int, rnd):
    """count single-digit scalars in coarse bin bin_, spread over its fine buckets"""
    nf = 1 << fine_bits(bits)
    return [in_bucket(bin_ * nf + rnd.randrange(nf), bits) for _ in range(count)]


EDGE_BINS = {3: FINE_CACHE_WORDS, 700: FINE_CACHE_WORDS + 1, 1024: BIG_LIMIT, 1500: BIG_LIMIT + 1, COARSE - 1: 5}


def bins_at_the_edges(bits: int):
    """coarse bins of exactly 10240, 10241, 65536 and 65537 words, and five words in the last bin"""
    rnd = random.Random(1500 + bits)
    words = [s for b, n in EDGE_BINS.items() for s in bin_words(bits, b, n, rnd)]
    return scatter(words, 160000, 1)


LAST_BIN_WORDS = 70000


def oversized_last_bin(bits: int):
    """bin 2047 above BIG_LIMIT (five chunks): the first chunk's workgroup has to write offsets[NB]"""
    rnd = random.Random(2047 + bits)
    words = bin_words(bits, COARSE - 1, LAST_BIN_WORDS, rnd) + bin_words(bits, 0, 300, rnd) + bin_words(bits, COARSE - 2, 17, rnd)
    return scatter(words, 73000, 2)


ONE_WORD_CHUNK = BIG_LIMIT + 3 * BIG_CHUNK + 1
ONE_WORD_CHUNK_BIN = 1033


def last_chunk_of_one_word(bits: int):
    """one bin of 65536 + 3 * 16384 + 1 words: eight chunks, the last of a single word; its neighbours hold a few"""
    rnd = random.Random(1033 + bits)
    words = bin_words(bits, ONE_WORD_CHUNK_BIN, ONE_WORD_CHUNK, rnd) + bin_words(bits, ONE_WORD_CHUNK_BIN - 1, 40, rnd) \
        + bin_words(bits, ONE_WORD_CHUNK_BIN + 1, 40, rnd)
    return scatter(words, 120000, 3)


def slice_edge_counts(ksl: int, heavy_thresh: int):
    """the bucket populations at which the slice layout changes: around one slice, around the heavy threshold, around one
    heavy segment (ns = 128 / 129)"""
    return [1, ksl - 1, ksl, ksl + 1, heavy_thresh * ksl, heavy_thresh * ksl + 1, HEAVY_SEG_SLICES * ksl, HEAVY_SEG_SLICES * ksl + 1]


def slice_edge_buckets(bits: int, ksl: int, heavy_thresh: int):
    """{bucket: population}: the eight edge counts twice — in the adjacent buckets 0 .. 7 (bucket 8 stays empty between them and
    bucket 9) and in every third bucket down from the last one, so that every remainder class is shared by two buckets"""
    nb, counts = 1 << bits, slice_edge_counts(ksl, heavy_thresh)
    plan = {}
    for j, n in enumerate(counts):
        plan[j] = n
        plan[nb - 1 - 3 * j] = n
    plan[9] = 2
    plan[5000] = ksl + 1
    return {b: n for b, n in plan.items() if n > 0}


def slice_edges(bits: int, ksl: int, heavy_thresh: int):
    plan = slice_edge_buckets(bits, ksl, heavy_thresh)
    words = [in_bucket(b, bits) for b, n in plan.items() for _ in range(n)]
    m = len(words) + 1000
    return scatter(words, m, 4 + ksl)


EDGE_SCALARS = [0, 1, 2, Q - 1, Q - 2, 32767, 32768, 32769, 65535, 65536, 65537,
                (1 << 254) + 12345, (1 << 16) * 32768, (1 << 32) - 1, 0x8000800080008000, 0xFFFFFFFFFFFFFFFF,
                int("8000" * 15, 16), int("7fff" * 15, 16), int("ffff" * 15, 16) % Q]      # those of test_edge_scalars (tests/test_gpu_msm.py)


def uniform_with_edges(m: int, seed: int):
    """m uniform scalars with as many of the edge scalars as fit at random places, the first and the last index among them"""
    rnd = random.Random(seed)
    out = [rnd.randrange(Q) for _ in range(m)]
    places = [0, m - 1] + [rnd.randrange(m) for _ in EDGE_SCALARS]
    for i, s in zip(places, rnd.sample(EDGE_SCALARS, len(EDGE_SCALARS))):
        out[i] = s
    return out
