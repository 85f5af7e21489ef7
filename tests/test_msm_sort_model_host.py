"""CPU: the model of the MSM bucket sort's outputs (tests/msm_sort_model.py) against the oracle and against slice_order; the
designed inputs of tests/test_gpu_msm_sort.py shown, through the model alone, to have the populations their names claim
(a GPU case that missed its edge would otherwise pass without anyone noticing); the checks shown to notice a wrong array;
and the door library tests/_build/libdev_msm_sort.so exists and exports every door.  All comparisons are exact."""
import ctypes
import os
import random
import time

import numpy as np
import pytest

import msm_sort_model as S
from msm_wide_model import slice_order
from oracle import bls12_381 as E

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_msm_sort.so")
DOORS = ["dms_group_sort", "dms_work", "dms_fill", "dms_read", "dms_needs_wide"]
Q = E.Q
COMBOS = [(bits, rows) for bits in (15, 19) for rows in S.VALID[bits]]
KSLS = (4, 8, 16, 32, 64, 128)


@pytest.fixture(scope="module")
def points():
    """24 points with their doublings: tab[i][k] = 2^k P_i (Jacobian)"""
    r = random.Random(2424)
    pts = [E.g1_mul(E.G1_GEN, r.randrange(1, Q)) for _ in range(24)]
    tab = []
    for pt in pts:
        t, lst = E.to_jac(pt), []
        for _ in range(256):
            lst.append(t)
            t = E.jac_double(t)
        tab.append(lst)
    return pts, tab


@pytest.mark.parametrize("bits,rows", COMBOS)
def test_model_entries_sum_to_the_naive_msm(points, bits, rows):
    """every entry decoded (sign, row, point) and weighted by its bucket: the sum is the oracle's MSM, for random and edge scalars"""
    pts, tab = points
    r = random.Random(100 * bits + rows)
    scalars = [r.randrange(Q) for _ in range(12)] + r.sample(S.EDGE_SCALARS, 12)
    table_n = 37                                                   # more points per row than scalars: the row stride is the table's
    md = S.sort_model(scalars, rows, table_n, bits, 4, 16)
    acc = E.JAC_ID
    for e, b in zip(md.entries.tolist(), md.bucket_of.tolist()):
        row, i = divmod(e & 0x7FFFFFFF, table_n)
        assert i < len(scalars) and row < rows
        t = E.jac_mul(tab[i][S.row_shift(rows, row)], S.bucket_weight(rows, b))
        acc = E.jac_add(acc, E.jac_neg(t) if e >> 31 else t)
    assert E.to_affine(acc) == E.msm_naive(pts, scalars)
    assert md.total == sum(len(S.digits(s % Q, rows, bits)) for s in scalars) == int(md.offsets[md.nb])
    # the same through a sparse input
    sp = S.sort_model(S.Sparse(len(scalars), dict(enumerate(scalars))), rows, table_n, bits, 4, 16)
    assert (sp.entries == md.entries).all() and (sp.offsets == md.offsets).all()


@pytest.mark.parametrize("ksl", (4, 32))
def test_slice_offsets_and_the_lane_map_agree_with_slice_order(ksl):
    r = random.Random(ksl)
    scalars = [r.randrange(Q) if i % 3 else r.randrange(1, 4) for i in range(900)]      # uniform buckets and three of many slices
    md = S.sort_model(scalars, S.ROWS_WINDOW, 900, 15, ksl, 16)
    want_lanes, want_slice_off = slice_order(md.counts.tolist(), ksl)
    assert md.slice_off.tolist() == want_slice_off
    assert S.lanes(md) == want_lanes
    assert int(md.full_off[md.nb]) + len(md.part_list) == int(md.slice_off[md.nb])
    assert max(md.ns) > 2 and len(set(md.rem[md.part_list].tolist())) >= 3


@pytest.mark.parametrize("bits", (15, 19))
def test_designed_bins_have_the_populations_their_names_claim(bits):
    rows = S.designed_rows(bits)
    t0 = time.time()
    sc = S.bins_at_the_edges(bits)
    md = S.sort_model(sc, rows, len(sc), bits, 32, 16)
    print("model of %d scalars, %d words: %.2f s" % (len(sc), md.total, time.time() - t0))
    assert md.total == sum(1 for s in sc if s)                     # single-digit scalars: a word each
    assert S.FINE_CACHE_WORDS == 10240 and S.BIG_LIMIT == 65536
    want = np.zeros(S.COARSE, dtype=np.int64)
    want[3], want[700], want[1024], want[1500], want[2047] = 10240, 10241, 65536, 65537, 5
    assert (md.bin_counts == want).all()
    assert len(sc) <= 1 << 19

    sc = S.oversized_last_bin(bits)
    md = S.sort_model(sc, rows, len(sc), bits, 32, 16)
    assert md.bin_counts[2047] == 70000 > S.BIG_LIMIT and md.total == 70317
    assert md.bin_counts[0] == 300 and md.bin_counts[2046] == 17

    sc = S.last_chunk_of_one_word(bits)
    md = S.sort_model(sc, rows, len(sc), bits, 32, 16)
    n = int(md.bin_counts[S.ONE_WORD_CHUNK_BIN])
    assert n == 65536 + 3 * 16384 + 1 and n > S.BIG_LIMIT and n % S.BIG_CHUNK == 1
    assert md.bin_counts[S.ONE_WORD_CHUNK_BIN - 1] == 40 and md.bin_counts[S.ONE_WORD_CHUNK_BIN + 1] == 40


@pytest.mark.parametrize("bits", (15, 19))
@pytest.mark.parametrize("ksl", KSLS)
def test_designed_buckets_sit_on_the_slice_edges(bits, ksl):
    ht = 16
    plan = S.slice_edge_buckets(bits, ksl, ht)
    sc = S.slice_edges(bits, ksl, ht)
    md = S.sort_model(sc, S.designed_rows(bits), len(sc), bits, ksl, ht)
    assert {int(b): int(md.counts[b]) for b in np.nonzero(md.counts)[0]} == plan
    have = set(plan.values())
    assert {1, ksl - 1, ksl, ksl + 1, ht * ksl, ht * ksl + 1, 128 * ksl, 128 * ksl + 1} <= have
    assert md.counts[8] == 0 and md.counts[7] > 0 and md.counts[9] > 0          # an empty bucket between populated ones
    ns = set(md.ns[list(plan)].tolist())
    assert {1, 2, ht, ht + 1, 128, 129} <= ns
    # a bucket of exactly heavy_thresh slices is not heavy, one entry more makes it so; ns = 128 is one segment, 129 two
    by_ns = {int(md.ns[b]): md.heavy.get(b) for b in plan}
    assert by_ns[ht] is None and by_ns[ht + 1] == 1 and by_ns[128] == 1 and by_ns[129] == 2
    assert sorted(md.heavy.values()) == [1, 1, 1, 1, 2, 2]
    assert len(md.multi) >= 4 and md.counts[md.nb - 1] > 0 and md.counts[0] > 0
    assert len(sc) <= 1 << 19


def perfect_outputs(md, cap_words):
    """the arrays a correct sort leaves in memory filled with 0xA5 (entries inside a bucket in DEscending order, the part_list
    classes reversed, the heavy items reversed: every freedom of the contract used)"""
    out = {}
    ent = np.full(cap_words, S.UNTOUCHED, dtype=np.uint32)
    ent[:md.total] = md.entries[np.lexsort((-md.entries.astype(np.int64), md.bucket_of))]
    out["entries"] = ent
    pl = np.full(md.nb + 1, S.UNTOUCHED, dtype=np.uint32)
    lst = md.part_list
    pl[:len(lst)] = lst[np.lexsort((-lst.astype(np.int64), -md.rem[lst]))]
    pl[md.nb] = len(lst)
    out["part_list"] = pl
    nheavy = np.zeros(16, dtype=np.uint32)
    hv = np.full((md.nb, 4), S.UNTOUCHED, dtype=np.uint32)
    run = 0
    for k, b in enumerate(sorted(md.heavy, reverse=True)):
        hv[k] = (b, run, md.heavy[b], 0)
        run += md.heavy[b]
    nheavy[2], nheavy[3], nheavy[9] = len(md.heavy), run, len(md.multi)
    out["nheavy"], out["heavy_list"] = nheavy, hv
    ml = np.full(md.nb, S.UNTOUCHED, dtype=np.uint32)
    ml[:len(md.multi)] = md.multi[::-1]
    out["multi_list"] = ml
    bk = np.full((md.nb, 32), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    bk[md.counts == 0] = 0
    out["buckets"] = bk
    return out


def run_checks(md, o, kb=1):
    S.check_scan(md, kb, "offsets", o.get("offsets", md.offsets), md.offsets)
    S.check_entries(md, kb, o["entries"])
    S.check_part_list(md, kb, o["part_list"])
    S.check_heavy(md, kb, o["nheavy"], o["heavy_list"])
    S.check_multi(md, kb, o["nheavy"], o["multi_list"])
    S.check_buckets(md, kb, o["buckets"])


def test_the_checks_accept_every_freedom_and_name_what_differs():
    r = random.Random(77)
    scalars = [r.randrange(Q) if i % 2 else r.randrange(1, 40) for i in range(900)]
    md = S.sort_model(scalars, S.ROWS_WINDOW, 900, 15, 4, 2)
    assert len(md.heavy) >= 2 and len(md.multi) and len(md.part_list)
    good = perfect_outputs(md, 16 * 900)
    run_checks(md, good)

    def broken(name, edit, words):
        o = {k: v.copy() for k, v in good.items()}
        edit(o)
        with pytest.raises(AssertionError) as info:
            run_checks(md, o)
        msg = str(info.value)
        assert msg.startswith("commitment 1: ") and name in msg and all(w in msg for w in words), msg

    b = int(np.nonzero(md.counts > 1)[0][3])
    lo = int(md.offsets[b])

    def shift_offset(o):
        o["offsets"] = md.offsets.copy()
        o["offsets"][b + 1] += 1
    broken("offsets", shift_offset, ["bucket %d " % (b + 1), "coarse bin %d" % ((b + 1) >> 4)])
    broken("entries", lambda o: o["entries"].__setitem__(lo, o["entries"][lo] ^ (1 << 31)), ["bucket %d " % b, "coarse bin %d" % (b >> 4)])
    broken("entries", lambda o: o["entries"].__setitem__(lo, o["entries"][lo] ^ (1 << 30)), ["bucket %d " % b])
    # an entry moved to the neighbouring bucket: the same words overall, two wrong multisets
    nxt = int(md.offsets[b + 1])

    def swap(o):
        o["entries"][[nxt - 1, nxt]] = o["entries"][[nxt, nxt - 1]]
    if md.counts[b + 1]:
        broken("entries", swap, ["bucket %d " % b])
    broken("entries", lambda o: o["entries"].__setitem__(md.total, 0), ["past the total"])
    n = len(md.part_list)
    broken("part_list", lambda o: o["part_list"].__setitem__(md.nb, n - 1), ["[NB]"])
    broken("part_list", lambda o: o["part_list"].__setitem__(slice(0, n), o["part_list"][:n][::-1].copy()), ["remainder"])
    broken("part_list", lambda o: o["part_list"].__setitem__(0, o["part_list"][1]), ["class of remainder"])
    broken("part_list", lambda o: o["part_list"].__setitem__(n, 0), ["past its"])
    broken("heavy_list", lambda o: o["heavy_list"].__setitem__((0, 3), 1), ["pad"])
    broken("heavy_list", lambda o: o["heavy_list"].__setitem__((0, 2), o["heavy_list"][0, 2] + 1), ["nseg"])
    broken("heavy_list", lambda o: o["heavy_list"].__setitem__((1, 1), o["heavy_list"][1, 1] + 1), ["seg_base"])
    broken("nheavy[2 kb + 1]", lambda o: o["nheavy"].__setitem__(3, o["nheavy"][3] + 1), ["segments"])
    broken("nheavy[2 kb]", lambda o: o["nheavy"].__setitem__(2, o["nheavy"][2] - 1), ["heavy buckets"])
    broken("multi_list", lambda o: o["multi_list"].__setitem__(0, o["multi_list"][1]), ["lists bucket"])
    broken("nheavy[2 KB + kb]", lambda o: o["nheavy"].__setitem__(9, o["nheavy"][9] + 1), ["listed buckets"])
    empty = int(np.nonzero(md.counts == 0)[0][5])
    broken("buckets", lambda o: o["buckets"].__setitem__((empty, 31), 1), ["bucket %d " % empty, "not zero"])
    broken("buckets", lambda o: o["buckets"].__setitem__((b, 0), 0), ["bucket %d " % b, "written"])


def test_door_library_is_built_and_exports_every_door():
    import plonk_amd
    import __graft_entry__
    if not os.path.exists(plonk_amd.LIB_PATH):      # nothing built yet (as test_capi_symbols.py): build the pair
        __graft_entry__.build_hip(verbose=False)
    if not os.path.exists(SO):
        __graft_entry__.build_dev_msm_sort(verbose=False)
    assert os.path.exists(SO), "tests/_build/libdev_msm_sort.so is missing: run build() of __graft_entry__.py first"
    lib = ctypes.CDLL(SO)
    for name in DOORS:
        assert hasattr(lib, name), name
    # every extern "C" door of the source is in the list above
    import re
    src = open(os.path.join(HERE, "csrc", "dev_msm_sort.hip")).read()
    assert sorted(set(re.findall(r"^int (dms_\w+)\(", src, flags=re.M))) == sorted(DOORS)
