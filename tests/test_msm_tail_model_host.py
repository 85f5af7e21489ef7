"""CPU: the big-int model of tests/msm_tail_model.py on its own — what tests/test_gpu_msm_tail.py compares the kernels of
msm.hip with.  The membership sets of the reduction tail reproduce the commitment through a scalar restatement of
finish_bit_sums (both bucket counts, both weightings) and agree with the point-level model of msm_wide_model on a small
instance; the slot codec round-trips; the fixed-base multiplication is the oracle's; the launch rule gives the lane counts and
modes the designed launches are named after; and every designed input has the populations its name claims."""
import random

import numpy as np
import pytest

import msm_sort_model as S
import msm_tail_model as T
import msm_wide_model as W
from oracle import bls12_381 as E

P, Q = E.P, E.Q


def random_buckets(bits, seed, npool=200):
    """about half of the buckets hold +- a member of a pool of random scalars"""
    nb = 1 << bits
    rnd = np.random.RandomState(seed)
    r = random.Random(seed)
    pool = [r.randrange(Q) for _ in range(npool)]
    idx = np.where(rnd.randint(0, 2, nb) == 1, rnd.randint(0, npool, nb), -1)
    idx[[0, 127, 128, nb - 128, nb - 1]] = [0, 1, 2, 3, 4]                      # the corners of the row / column split are never empty
    return idx, rnd.choice([-1, 1], nb), pool


@pytest.mark.parametrize("bits", (15, 19))
def test_bit_sums_finish_to_the_commitment(bits):
    idx, sgn, pool = random_buckets(bits, 7 + bits)
    rb = T.rowbits(bits)
    ids, n = T.set_ids(bits, "out")
    assert n == rb + 9
    u = T.set_scalars(ids, n, idx, sgn, pool)
    k = [0 if i < 0 else int(s) * pool[i] for i, s in zip(idx.tolist(), sgn.tolist())]
    assert T.finish_scalar(u, rb, False) == sum((b + 1) * kb for b, kb in enumerate(k)) % Q
    assert T.finish_scalar(u, rb, True) == sum((2 * b + 1) * kb for b, kb in enumerate(k)) % Q
    assert u[rb + 8] == sum(k) % Q
    weighted = T.set_scalars([np.zeros(1 << bits, dtype=np.int64)], 1, idx, sgn, pool, weights=np.arange(1, (1 << bits) + 1, dtype=np.int64))
    assert weighted[0] == T.finish_scalar(u, rb, False)


@pytest.mark.parametrize("bits,first,second", [(15, "rcq", None), (15, "rc", None), (19, "rc1", "rc2")])
def test_intermediate_sums_add_up_to_the_bit_sums(bits, first, second):
    """every output is the sum of the intermediate sums the kernels take it from (msm_bits_quad_kernel, msm_bits_kernel)"""
    idx, sgn, pool = random_buckets(bits, 70 + bits)
    rb = T.rowbits(bits)
    out = T.set_scalars(*T.set_ids(bits, "out"), idx, sgn, pool)
    a = T.set_scalars(*T.set_ids(bits, first), idx, sgn, pool)
    if bits == 15:
        rows = a[:256]
        col = [(a[256 + l] + a[384 + l]) % Q for l in range(128)] if first == "rcq" else a[256:384]
    else:
        b = T.set_scalars(*T.set_ids(bits, second), idx, sgn, pool)
        rows = a[:4096]
        col = b[256:384]
        assert all(x == 0 for x in b[384:512])
        assert b[:256] == [sum(rows[16 * g:16 * g + 16]) % Q for g in range(256)]                      # G_g
        assert col == [sum(a[4096 + 128 * p + l] for p in range(32)) % Q for l in range(128)]             # C_l from the CP[p][l]
        for sg in range(16):
            for r in range(16):                                                                           # P[sg][r]: 16 of the terms of H_r
                assert b[512 + 16 * sg + r] == sum(rows[16 * (16 * sg + i) + r] for i in range(16)) % Q
    for j in range(rb):
        assert out[j] == sum(r for h, r in enumerate(rows) if (h >> j) & 1) % Q
    for j in range(7):
        assert out[rb + j] == sum(c for l0, c in enumerate(col[:127]) if ((l0 + 1) >> j) & 1) % Q
    assert out[rb + 7] == col[127] and out[rb + 8] == sum(rows) % Q


def test_the_point_level_model_agrees_on_a_small_instance():
    """msm_wide_model.bit_sums / host_finish over 2^15 buckets (c = 16) against the membership sets"""
    r = random.Random(16)
    nb = 1 << 15
    buckets = {b: r.randrange(1, Q) for b in [0, 127, 128, 255, 16383, 16384, nb - 128, nb - 1] + r.sample(range(nb), 32)}
    idx = np.full(nb, -1)
    pool = []
    for b, k in buckets.items():
        idx[b] = len(pool)
        pool.append(k)
    u = T.set_scalars(*T.set_ids(15, "out"), idx, np.ones(nb, dtype=np.int64), pool)
    Tr, Tp, C_top = W.bit_sums({b: T.mul_g(k) for b, k in buckets.items()}, 16)
    for j, pt in enumerate(list(Tr) + list(Tp) + [C_top]):
        assert E.to_affine(pt) == T.affine_g(u[j]), j
    assert W.host_finish(Tr, Tp, C_top) == T.affine_g(T.finish_scalar(u, 8, False))


def test_mul_g_is_the_oracles_multiplication():
    r = random.Random(3)
    for k in [0, 1, 2, 255, 256, Q - 1, Q, (1 << 255) % Q] + [r.randrange(Q) for _ in range(8)]:
        assert T.affine_g(k) == (E.g1_mul(E.G1_GEN, k) if k % Q else None), hex(k)


def test_the_slot_codec_round_trips():
    r = random.Random(4)
    for i in range(20):
        k = r.randrange(1, Q)
        pt = T.affine_g(k)
        mult = tuple(r.randrange(b) for b in T.BOUNDS) if i % 3 else tuple(b - 1 for b in T.BOUNDS)
        words = T.encode_slot(pt, r.randrange(1, P), mult)
        assert len(words) == 64 and all(0 <= w < (1 << 28) for w in words)
        raw = T.raw_coords(words)
        assert all(m * P <= v < (m + 1) * P for v, m in zip(raw, mult))
        got = T.decode_slot(words)
        assert T.to_affine(got) == pt and T.same_point(got, T.mul_g(k)) and not T.same_point(got, T.mul_g(k + 1))
        aff = T.encode_affine(pt, (i & 1, (i >> 1) & 1))
        assert [v % P * T.FP28_RINV % P for v in T.raw_coords(aff)] == list(pt)
    assert T.decode_slot(T.IDENTITY_SLOT) is None and T.decode_slot([0] * 64) is None and T.encode_slot(None) == T.IDENTITY_SLOT
    assert T.same_point(None, E.JAC_ID) and not T.same_point(None, T.mul_g(1))
    with pytest.raises(AssertionError):
        bad = T.encode_slot(T.affine_g(5), 3)
        bad[0] ^= 1
        T.decode_slot(bad)
    # the output form: 4 x 12 words, radix 2^384
    pt = T.affine_g(77)
    z = 12345
    out = []
    for v in (pt[0] * z * z, pt[1] * z ** 3, z * z, z ** 3):
        out += [(v % P * E.FP_R % P >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
    assert T.to_affine(T.decode_out(out)) == pt and T.decode_out([1] + [0] * 47) is None
    slots = T.pool_slots()
    for j in (0, 17, T.NPOOL - 1):
        for rep in range(T.NREP):
            assert T.same_point(T.decode_slot(slots[0, j, rep]), T.mul_g(T.POOL_K[j]))
            assert T.same_point(T.decode_slot(slots[1, j, rep]), T.mul_g(Q - T.POOL_K[j]))
    assert all(T.decode_slot(slots[s, T.NPOOL, rep]) is None for s in (0, 1) for rep in range(T.NREP))


def test_the_launch_rule_at_the_designed_sizes():
    """the smallest mmax with an average of 9, 17 and 33 slices of 4 entries per bucket; what each switch changes"""
    for mmax, avg, bsum in ((73728, 9, 2), (139264, 17, 4), (270336, 33, 8)):
        r = T.launch_rule(15, mmax, ksl=4)
        assert (r.avg, r.bsum, r.lanes, r.dense_quad, r.heavy_thresh) == (avg, bsum, bsum, False, 2 * avg)
        assert T.launch_rule(15, mmax - 1, ksl=4).avg == avg - 1
    r = T.launch_rule(15, 300, ksl=4)
    assert r.dense_quad and r.lanes == 4 and not r.ordered and r.fused == 128 and r.heavy_thresh == 16 and r.empty == "identity"
    assert T.launch_rule(15, 73727, ksl=4).dense_quad
    r = T.launch_rule(15, 300, ksl=4, bsum_lane=True)
    assert not r.dense_quad and r.bsum == 1 and r.lanes == 1
    r = T.launch_rule(15, 300, ksl=4, tail_serial=True)
    assert not r.dense_quad and r.fused == 0
    assert T.launch_rule(15, 300, ksl=4, order=1).direct and not T.launch_rule(15, 300, ksl=4, order=1, acc_lds=True).direct
    assert [T.launch_rule(15, m).ksl for m in (300, 1 << 16, 1 << 17, 1 << 18, 1 << 20)] == [4, 8, 16, 32, 32]
    r = T.launch_rule(19, 6000)
    assert r.ksl == 32 and r.ordered and r.list_mode and r.direct and not r.dense_quad and r.fused == 512 and r.empty == "zero"
    r = T.launch_rule(19, 300, ksl=4, order=0)
    assert r.dense_quad and not r.list_mode and r.empty == "identity"
    assert [T.launch_rule(19, m).ksl for m in (1 << 19, 1 << 20, 1 << 21, 1 << 22)] == [32, 64, 128, 128]


@pytest.mark.parametrize("name", [c[0] for c in T.PHASE1_LAUNCHES])
def test_the_designed_inputs_have_their_populations(name):
    bits, rows, mmax, sw, rule, inp = T.phase1_case(name)
    assert S.length(inp.scalars) == mmax <= (1 << 19) + 1
    md = S.sort_model(inp.scalars, rows, mmax, bits, rule.ksl, rule.heavy_thresh)
    assert {int(b): int(md.counts[b]) for b in np.nonzero(md.counts)[0]} == inp.entries_of
    ns = sorted(set(int(x) for x in md.ns[np.nonzero(md.ns)[0]]))
    G, ht = rule.lanes, rule.heavy_thresh
    want = {1, 2, G, G + 1, 2 * G + 1, ht, ht + 1, T.HEAVY_SEG, T.HEAVY_SEG + 1} | ({G - 1} if G > 1 else set())
    if mmax > 300:
        want.add(2 * T.HEAVY_SEG + 1)
    assert want <= set(ns), (name, sorted(want - set(ns)))
    segs = sum(md.heavy.values())
    assert sorted(set(md.heavy.values()))[:2] == [1, 2]
    big = [c[5] for c in T.PHASE1_LAUNCHES if c[0] == name][0]
    if big:
        assert max(md.heavy.values()) > 64 and segs > T.fused_workers(bits)
    if rule.list_mode:
        assert (md.ns == 1).sum() >= 20 and len(md.multi) >= 10          # buckets of exactly one slice beside listed ones
    # the switches the name promises
    promised = {"dense quad": rule.dense_quad, "BSUM(1) by lanes": rule.bsum == 1 and not rule.dense_quad, "BSUM(2)": rule.bsum == 2,
                "BSUM(4)": rule.bsum == 4, "BSUM(8)": rule.bsum == 8, "order 0": not rule.ordered, "order 1": rule.direct,
                "order 1, BSUM(2)": rule.direct and rule.bsum == 2, "acc_lds": not rule.ordered, "acc_wg 64": rule.ordered,
                "tail_serial": rule.fused == 0 and rule.bsum == 2, "2^19 list mode": rule.list_mode and rule.direct and rule.ksl == 32,
                "2^19 list mode, quarter rows": rule.list_mode, "2^19 list mode, short slices, many segments": rule.list_mode and rule.ksl == 4,
                "2^19 dense quad": rule.dense_quad and bits == 19}
    assert promised[name], name
    # the chains: whatever order the sort leaves the entries of a bucket in, the designed buckets contain equal and opposite points
    terms = {b: [(T.TABLE_K[j] if not s else Q - T.TABLE_K[j]) for j, s in members] for b, members in inp.chains.items()}
    assert any(len(t) == 2 and t[0] == t[1] for t in terms.values()) and any(len(t) == 2 and (t[0] + t[1]) % Q == 0 for t in terms.values())
    assert any(len(t) == 3 and len(set(t)) == 1 for t in terms.values())
    assert all(int(md.counts[b]) == len(t) for b, t in terms.items())
    assert (md.entries >> 31).any()                                      # negative digits among the entries


def test_chain_events():
    a, b = T.TABLE_K[0], T.TABLE_K[1]
    assert T.chain_events([a, a]) == (2 * a % Q, {"pair", "double"})      # the pair is left to the general path, which doubles
    assert T.chain_events([a, Q - a]) == (0, {"pair", "identity"})
    assert T.chain_events([a, a, a]) == (3 * a % Q, {"pair", "double"})
    assert T.chain_events([a, Q - a, b]) == (b, {"pair", "cancel+"})
    assert T.chain_events([a, b, (Q - a - b) % Q]) == (0, {"identity"})
    assert T.chain_events([a, b, (a + b) % Q]) == (2 * (a + b) % Q, {"double"})
    assert T.chain_events([a]) == (a, set())


def test_the_table_holds_equal_and_opposite_points():
    j, rep = T.Table().points(np.arange(4096))
    assert set(j.tolist()) == set(range(T.NT)) and set(rep.tolist()) == {0, 1, 2, 3}
    assert all((T.TABLE_K[i] + T.TABLE_K[(i + T.NT // 2) % T.NT]) % Q == 0 for i in range(T.NT))
    t = T.Table({5: (3, 2)})
    assert [int(x[5]) for x in t.points(np.arange(8))] == [3, 2]
    w = t.entry_words(np.array([5]))[0]
    x, y = (v for v in T.raw_coords(w))
    pt = T.affine_g(T.TABLE_K[3])
    assert x == pt[0] * T.FP28_R % P and y == pt[1] * T.FP28_R % P + P


DOORS = ("dmt_quad_add", "dmt_phase", "dmt_work", "dmt_fill", "dmt_read", "dmt_write", "dmt_scatter")


def test_door_library_is_built_and_exports_every_door():
    import ctypes
    import os
    import re

    import plonk_amd
    import __graft_entry__
    here = os.path.dirname(os.path.abspath(__file__))
    so = os.path.join(here, "_build", "libdev_msm_tail.so")
    if not os.path.exists(plonk_amd.LIB_PATH):      # nothing built yet (as test_capi_symbols.py): build the pair
        __graft_entry__.build_hip(verbose=False)
    if not os.path.exists(so):
        __graft_entry__.build_dev_msm_tail(verbose=False)
    assert os.path.samefile(__graft_entry__.DEV_MSM_TAIL_LIB, so)
    lib = ctypes.CDLL(so)
    for name in DOORS:
        assert hasattr(lib, name), name
    src = open(os.path.join(here, "csrc", "dev_msm_tail.hip")).read()
    assert sorted(set(re.findall(r"^int (dmt_\w+)\(", src, flags=re.M))) == sorted(DOORS)
    # the quad addition has one definition: the header the product and the test kernel both include
    msm = open(os.path.join(here, "..", "plonk_amd", "csrc", "msm.hip")).read()
    assert '#include "curve28_quad.cuh"' in msm and '#include "curve28_quad.cuh"' in src
    assert "G1R g1r_add_quad(" not in msm and "G1R g1r_add_quad(" not in src
