"""GPU: Lagrange-basis tables on a KZG domain handle (plonk_kzg_evals_tables_build / _drop / _last; plonk_amd/csrc/kzg_evals.hip).

The finish kernel is tested on its own through tests/_build/libdev_kzg_evals_tables.so (tests/csrc/dev_kzg_evals_tables.hip,
built by build(): a door only, the kernel is libplonk_hip.so's) against the big-int model tests/kzg_evals_tables_model.py: bit
sums [k_j] G for scalars the model chooses, both row counts, both weightings, every operand family the chain has a branch for,
1, 63 | 64 | 65 and 4096 commitments in a launch, guard bytes around the output.

The calls are tested for byte identity: commit_evals, open_evals and open_multi, host and resident forms, give the same bytes
before the handle has tables, with them, after they were dropped and after a second build; at 2^5 and 2^12 those bytes are the
closed forms of tests/test_gpu_kzg_evals.py, and proofs made with tables pass the pairing checks.  plonk_kzg_evals_tables_last
is compared with the plan computed on the host after every call that used the tables."""
import ctypes
import os
import random

import pytest

from oracle import bls12_381 as E
from tests import kzg_evals_model as EM
from tests import kzg_evals_tables_model as M
from tests import kzg_ref as K
from tests.test_gpu_kzg_evals import Guarded, assert_last, expected, load_key, random_raw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_evals_tables.so")
Q = E.Q
OK, ERR_ARG, ERR_STATE, ERR_DATA = 0, -1, -7, -9
ID48 = K.IDENTITY48
KEY_POINTS = (1 << 12) + 3
LAYOUTS = [(8, False), (8, True), (12, False), (12, True)]
STATES = ("before", "built", "dropped", "rebuilt")


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, KEY_POINTS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key(ctx):
    import plonk_amd
    k = plonk_amd.KzgKey(ctx, K.opening_key())
    yield k
    k.close()


@pytest.fixture(scope="module")
def door():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_evals_tables.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    so.dkt_finish.argtypes = [vp, vp, u32, ci, ci, vp]
    so.dkt_const.argtypes = [ci]
    so.dkt_const.restype = ctypes.c_uint64
    return so


# ---- the finish kernel alone ----------------------------------------------------------------------------------------------------
PATTERNS = 97


def commitments_of(rb, bitpos):
    """PATTERNS distinct commitments: (bit-sum bytes, the model's 48 bytes).  The operand families first, then draws from a
    pool of points: identities, small and full-width multiples of G, a point and its negative"""
    rnd = random.Random(1000 * rb + bitpos)
    pool = [0, 0, 1, 2, Q - 1, Q - 2, 3, 5] + [rnd.randrange(Q) for _ in range(8)]
    cache = {}

    def slot(k):
        if k not in cache:
            cache[k] = M.slot_bytes(E.g1_mul(E.G1_GEN, k) if k else None)
        return cache[k]
    scalars = list(M.special_scalars(rb, bitpos).values())
    while len(scalars) < PATTERNS:
        scalars.append([rnd.choice(pool) for _ in range(rb + 9)])
    filler = bytes([0xEE]) * (M.SLOT_BYTES * (M.BIT_SUMS - rb - 9))
    return [(b"".join(slot(k % Q) for k in ks) + filler, M.finish_bytes_of_scalars(ks, rb, bitpos)) for ks in scalars]


@pytest.mark.parametrize("rb,bitpos", LAYOUTS)
def test_finish_kernel_against_the_model(ctx, door, rb, bitpos):
    assert [door.dkt_const(k) for k in range(5)] == [M.BIT_SUMS, M.SLOT_BYTES, M.FINISH_CHUNK, M.TABLE_GROUP, 64]
    pats = commitments_of(rb, bitpos)
    flags = set()
    for count, first in ((1, 40), (63, 0), (64, 11), (65, 23), (4096, 0)):
        lanes = [pats[(first + i) % PATTERNS] for i in range(count)]
        bits = ctx.alloc(M.BIT_SUMS * M.SLOT_BYTES * count)
        bits.upload(b"".join(b for b, _ in lanes))
        out = Guarded(ctx, 48 * count)
        assert door.dkt_finish(ctx.handle, bits.ptr, count, rb, int(bitpos), out.ptr) == 0
        got = out.read()
        for i, (_, want) in enumerate(lanes):
            assert got[48 * i:48 * i + 48] == want, (count, i)
        flags |= {got[48 * i] & 0xE0 for i in range(count)}
        bits.free()
        out.free()
    assert flags == {0x80, 0xA0, 0xC0}                          # y in either half, and the identity
    assert pats[0][1] == ID48                                    # all slots the identity


def test_finish_door_refuses_a_layout_the_slots_cannot_hold(ctx, door):
    bits, out = ctx.alloc(M.BIT_SUMS * M.SLOT_BYTES), ctx.alloc(48)
    for rb in (7, 13):
        assert door.dkt_finish(ctx.handle, bits.ptr, 1, rb, 0, out.ptr) == ERR_ARG
    assert door.dkt_finish(ctx.handle, bits.ptr, 0, 8, 0, out.ptr) == ERR_ARG
    bits.free()
    out.free()


# ---- the calls: four states of one handle ------------------------------------------------------------------------------------------
def in_four_states(dom, run):
    """run(tabled) in the four states of the handle -> its (identical) result"""
    outs = []
    dom.drop_tables()
    for state in STATES:
        if state in ("built", "rebuilt"):
            info = dom.build_tables()
            assert info["built"] == 1 and info["table_rows"] in (16, 64, 128, 256) and info["msms"] == 0
            assert info["table_bytes"] == info["table_rows"] * dom.n * 128
            assert dom.build_tables()["built"] == 0              # a second call finds them
        elif state == "dropped":
            dom.drop_tables()
            dom.drop_tables()                                    # and again: nothing to drop
            assert dom.tables_last()["table_rows"] == 0
        outs.append(run(state in ("built", "rebuilt")))
    dom.drop_tables()
    for state, o in zip(STATES[1:], outs[1:]):
        assert o == outs[0], state
    return outs[0]


def assert_tables_last(dom, plan):
    last = dom.tables_last()
    assert (last["msms"], last["group_launches"], last["device_finished"]) == (plan["msms"], plan["group_launches"], plan["device_finished"])
    assert last["bucket_bits"] in (15, 17, 18, 19) and last["log_n"] == dom.log_n
    return last


def assert_evals_tables_last(dom, count, commitments, witness, host_form):
    g = EM.plan(dom.log_n, count, commitments, witness, host_form)["group_vectors"]
    return assert_tables_last(dom, M.evals_plan(g, count, commitments, witness))


class Resident:
    def __init__(self, ctx, raws):
        self.bufs = []
        for r in raws:
            b = ctx.alloc(len(r))
            b.upload(r)
            self.bufs.append(b)
        self.ptrs = [b.ptr for b in self.bufs]

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("log_n", [1, 2, 5, 8, 12])
def test_commit_and_open_are_byte_identical_with_and_without_tables(ctx, key, log_n):
    import plonk_amd as P
    n = 1 << log_n
    dom = P.KzgDomain(ctx, log_n)
    rnd = random.Random(120 + log_n)
    raws = [random_raw(rnd, n) for _ in range(9)]
    res = Resident(ctx, raws)
    pts = EM.domain_points(log_n)
    zs = [rnd.randrange(Q), 0, pts[0], pts[n - 1]]
    v = rnd.randrange(Q)

    def run(tabled):
        out = {}
        for count in (1, 4, 5, 8, 9):
            out["commit", count] = dom.commit_evals(raws[:count])
            if tabled:
                assert_evals_tables_last(dom, count, True, False, True)
            out["commit dev", count] = dom.commit_evals_dev(res.ptrs[:count])
            if tabled:
                assert_evals_tables_last(dom, count, True, False, False)
            assert_last(dom, count, EM.NONE, True, False, False)
            out["open", count] = dom.open_evals(raws[:count], zs[0], v)
            if tabled:
                assert_evals_tables_last(dom, count, True, True, True)
            for z in zs:
                out["open dev", count, z] = dom.open_evals_dev(res.ptrs[:count], z, v)
                if tabled:
                    last = assert_evals_tables_last(dom, count, True, True, False)
                    assert last["device_finished"] == 1         # the commitments' launch and the witness's: two at least
                assert_last(dom, count, pts.index(z) if z in pts else EM.NONE, True, True, False)
            out["witness only", count] = dom.open_evals_dev(res.ptrs[:count], zs[0], v, commitments=False)
            if tabled:
                assert assert_evals_tables_last(dom, count, False, True, False)["device_finished"] == 0   # one launch: the host finishes
        return out

    out = in_four_states(dom, run)
    for count in (1, 4, 5, 8, 9):
        assert out["commit", count] == out["commit dev", count] == out["open", count][1] == out["open dev", count, zs[0]][1]
        assert out["open", count] == out["open dev", count, zs[0]]
        assert out["witness only", count][2] == out["open", count][2]
    if log_n in (5, 12):
        vectors = [P.fr_from_bytes_mont(r) for r in raws]
        for count in (1, 5, 9):
            for z in zs:
                assert out["open dev", count, z] == expected(vectors[:count], z, v, log_n), (count, z)
    # proofs made with tables pass the pairing check
    dom.build_tables()
    for z in zs:
        ev, cm, wit = dom.open_evals_dev(res.ptrs[:5], z, v)
        assert key.check_each([z], [ctx.kzg_flatten(cm, ev, v, wit)]) == [OK]
    res.free()
    dom.close()


def test_host_form_across_the_staging_group_boundary(ctx):
    """64 | 65 vectors at 2^5: one staging group, and a second of one vector whose commitment is a launch of its own"""
    import plonk_amd as P
    log_n, n = 5, 32
    dom = P.KzgDomain(ctx, log_n)
    rnd = random.Random(6465)
    raws = [random_raw(rnd, n) for _ in range(65)]
    vectors = [P.fr_from_bytes_mont(r) for r in raws]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    want = expected(vectors, z, v, log_n)
    plain = {c: (dom.commit_evals(raws[:c]), dom.open_evals(raws[:c], z, v)) for c in (64, 65)}
    dom.build_tables()
    for count in (64, 65):
        assert dom.commit_evals(raws[:count]) == plain[count][0] == want[1][:count]
        last = assert_evals_tables_last(dom, count, True, False, True)
        assert last["group_launches"] == 16 + (count - 64) and last["device_finished"] == 1
        assert dom.open_evals(raws[:count], z, v) == plain[count][1]
        assert assert_evals_tables_last(dom, count, True, True, True)["msms"] == count + 1
    assert plain[65][1] == want
    dom.close()


@pytest.mark.parametrize("log_n", [2, 5, 12])
def test_multiproofs_are_byte_identical_with_and_without_tables(ctx, key, log_n):
    import plonk_amd as P
    n = 1 << log_n
    dom = P.KzgDomain(ctx, log_n)
    rnd = random.Random(190 + log_n)
    raws = [random_raw(rnd, n) for _ in range(9)]
    res = Resident(ctx, raws)

    def items_of(m):
        return [(rnd.randrange(m), rnd.randrange(n)) for _ in range(7)] + [(m - 1, n - 1), (0, 0)]
    items = {m: items_of(m) for m in (1, 5, 9)}
    given = {m: dom.commit_evals(raws[:m]) for m in (1, 5, 9)}

    def run(tabled):
        out = {}
        for m in (1, 5, 9):
            before = dom.evals_last()
            out["host", m] = dom.open_multi(raws[:m], items[m], b"tables")
            if tabled:
                last = assert_tables_last(dom, M.multiproof_plan(m))
                assert last["device_finished"] == (1 if m > 4 else 0)
            out["dev", m] = dom.open_multi_dev(res.ptrs[:m], items[m], b"tables")
            ml = dom.multi_last()
            assert (ml["commitments_computed"], ml["msm_launches"]) == (m, m + 2)
            out["given", m] = dom.open_multi_dev(res.ptrs[:m], items[m], b"tables", commitments=given[m])
            if tabled:
                assert_tables_last(dom, M.multiproof_plan(0))
            assert dom.multi_last()["msm_launches"] == 2
            assert dom.evals_last() == before                     # plonk_kzg_evals_last does not see multiproofs
        return out

    out = in_four_states(dom, run)
    for m in (1, 5, 9):
        assert out["host", m] == out["dev", m] == out["given", m]
        values, cm, proof = out["host", m]
        assert cm == given[m]
        assert key.check_multi(log_n, cm, items[m], values, proof, b"tables")
        assert not key.check_multi(log_n, cm, items[m], values, proof, b"other label")
    res.free()
    dom.close()


# ---- forced layouts ---------------------------------------------------------------------------------------------------------------
def forced_case(mode, bucket_bits, log_n, want_bits=None):
    import plonk_amd as P
    n = 1 << log_n
    c = P.Context(0, P.GpuConfig(table_mode=mode, msm_bucket_bits=bucket_bits))
    load_key(c, n + 3)
    dom = P.KzgDomain(c, log_n)
    rnd = random.Random(mode + log_n)
    raws = [random_raw(rnd, n) for _ in range(5)]
    vectors = [P.fr_from_bytes_mont(r) for r in raws]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    items = [(0, 1), (4, n - 1), (2, 0)]
    plain = (dom.commit_evals(raws), dom.open_evals(raws, z, v), dom.open_evals(raws[:1], z), dom.open_multi(raws, items))
    held = c.table_bytes()[0]
    info = dom.build_tables()
    assert info["table_rows"] == mode and c.table_bytes()[0] == held + mode * n * 128
    described = c.describe_msm(n, count=4, bit_sum_tail=True, table_rows=mode, table_points=n)
    got = (dom.commit_evals(raws), dom.open_evals(raws, z, v))
    last = assert_evals_tables_last(dom, 5, True, True, True)
    assert (last["table_rows"], last["bucket_bits"]) == (mode, described["bucket_bits"])
    if want_bits is not None:
        assert last["bucket_bits"] == want_bits
    got += (dom.open_evals(raws[:1], z), dom.open_multi(raws, items))
    assert dom.tables_last()["bucket_bits"] == described["bucket_bits"]
    assert got == plain
    assert got[1] == expected(vectors, z, v, log_n)
    dom.close()
    assert c.table_bytes()[0] == held                            # destroy gives the bytes back as well
    c.close()


@pytest.mark.parametrize("mode", [16, 64, 128, 256])
def test_forced_table_layouts(mode):
    forced_case(mode, 0, 8)


def test_bit_position_rows_over_2_to_19_buckets():
    forced_case(256, 19, 12, want_bits=19)


# ---- accounting, errors -------------------------------------------------------------------------------------------------------------
def test_table_bytes_accounting_and_refusals():
    import plonk_amd as P
    c = P.Context(0)
    load_key(c, 64)
    d = P.KzgDomain(c, 6)
    lib = c.lib
    held = c.table_bytes()[0]
    assert d.tables_last() == {"log_n": 6, "table_rows": 0, "table_bytes": 0, "built": 0, "bucket_bits": 0, "msms": 0,
                               "group_launches": 0, "device_finished": 0}
    info = d.build_tables()
    assert c.table_bytes()[0] == held + info["table_rows"] * 64 * 128 == held + info["table_bytes"]
    assert d.evals_last()["lagrange_bytes"] == 96 * 64          # the build made the points
    d.drop_tables()
    assert c.table_bytes()[0] == held
    d.build_tables()
    d.close()
    assert c.table_bytes()[0] == held
    # NULL
    assert lib.plonk_kzg_evals_tables_build(None) == ERR_ARG and lib.plonk_kzg_evals_tables_drop(None) == ERR_ARG
    d = P.KzgDomain(c, 6)
    assert lib.plonk_kzg_evals_tables_last(d.handle, None) == ERR_ARG
    assert lib.plonk_kzg_evals_tables_last(None, ctypes.byref(P._KzgEvalsTablesInfo())) == ERR_ARG
    d.close()
    c.close()


def test_a_communicator_context_refuses_the_build():
    """refused before anything is allocated: no points, no tables, nothing counted"""
    import plonk_amd as P
    c = P.Context(0)
    load_key(c, 64)
    d = P.KzgDomain(c, 6)
    held = c.table_bytes()[0]
    c.comm_init(P.Context.comm_unique_id(), 0, 1)
    assert c.lib.plonk_kzg_evals_tables_build(d.handle) == ERR_STATE
    assert c.table_bytes()[0] == held and d.tables_last()["table_rows"] == 0
    c.comm_destroy()
    assert d.evals_last()["lagrange_bytes"] == 0
    assert d.build_tables()["built"] == 1
    d.close()
    c.close()


def test_a_reloaded_key_refuses_the_build_and_lets_the_tables_go():
    """build refuses, drop works, the evaluation calls refuse as before"""
    import plonk_amd as P
    c = P.Context(0)
    load_key(c, 64)
    d = P.KzgDomain(c, 6)
    lib = c.lib
    held = c.table_bytes()[0]
    e = [list(range(1, 65))]
    d.build_tables()
    with_tables = c.table_bytes()[0]
    before = d.open_evals(e, 9)
    load_key(c, 64)
    held = c.table_bytes()[0] - (with_tables - held)            # the new key's tables may differ; the handle's bytes are still held
    assert lib.plonk_kzg_evals_tables_build(d.handle) == ERR_STATE
    for call in (lambda: d.open_evals(e, 9), lambda: d.commit_evals(e)):
        with pytest.raises(P.PlonkError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    assert d.tables_last()["table_rows"] != 0
    d.drop_tables()
    assert c.table_bytes()[0] == held and d.tables_last()["table_rows"] == 0
    assert lib.plonk_kzg_evals_tables_build(d.handle) == ERR_STATE
    assert c.table_bytes()[0] == held
    d.close()
    d2 = P.KzgDomain(c, 6)
    d2.build_tables()
    assert d2.open_evals(e, 9) == before
    d2.close()
    c.close()


def test_errors_with_tables_leave_the_outputs_untouched(ctx):
    import plonk_amd as P
    dom, n = P.KzgDomain(ctx, 3), 8
    dom.build_tables()
    lib, mont = ctx.lib, P.fr_to_bytes_mont
    good, noncanon = mont(range(1, 9)), mont([1, 2]) + b"\xff" * 32 + mont([4, 5, 6, 7, 8])
    ev = ctypes.create_string_buffer(b"\xA5" * 160, 160)
    cm = ctypes.create_string_buffer(b"\xA5" * 240, 240)
    wit = ctypes.create_string_buffer(b"\xA5" * 48, 48)
    point, v = mont([5]), mont([6])
    keep = [ctypes.create_string_buffer(b, len(b)) for b in (good, good, good, good, noncanon)]
    arr = (ctypes.c_void_p * 5)(*[ctypes.cast(k, ctypes.c_void_p).value for k in keep])
    assert lib.plonk_kzg_open_evals(dom.handle, arr, 5, point, v, ev, cm, wit) == ERR_DATA
    assert lib.plonk_kzg_commit_evals(dom.handle, arr, 5, cm) == ERR_DATA
    assert lib.plonk_kzg_open_evals(dom.handle, arr, 5, point, None, ev, cm, wit) == ERR_ARG
    assert lib.plonk_kzg_open_evals(dom.handle, arr, 5, b"\xff" * 32, v, ev, cm, wit) == ERR_DATA
    bufs = Resident(ctx, [good, good, good, good, noncanon])
    darr = (ctypes.c_void_p * 5)(*bufs.ptrs)
    assert lib.plonk_kzg_open_evals_dev(dom.handle, darr, 5, point, v, ev, cm, wit) == ERR_DATA
    assert lib.plonk_kzg_commit_evals_dev(dom.handle, darr, 5, cm) == ERR_DATA
    assert ev.raw == b"\xA5" * 160 and cm.raw == b"\xA5" * 240 and wit.raw == b"\xA5" * 48
    # and the same buffers take a good call of one vector fewer
    assert lib.plonk_kzg_open_evals_dev(dom.handle, darr, 4, point, v, ev, cm, wit) == OK
    want = expected([list(range(1, 9))] * 4, 5, 6, 3)
    assert ev.raw[:128] == mont(want[0]) and cm.raw[:192] == b"".join(want[1]) and wit.raw == want[2]
    assert ev.raw[128:] == b"\xA5" * 32 and cm.raw[192:] == b"\xA5" * 48
    bufs.free()
    dom.close()


def test_zero_vectors_give_identities(ctx):
    import plonk_amd as P
    log_n, n = 5, 32
    dom = P.KzgDomain(ctx, log_n)
    dom.build_tables()
    rnd = random.Random(50)
    zero, e = [0] * n, [rnd.randrange(Q) for _ in range(n)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    assert dom.commit_evals([zero]) == [ID48]                                        # one launch, finished on the host
    assert dom.commit_evals([zero] * 5) == [ID48] * 5                                # all slots the identity, on the device
    got = dom.commit_evals([zero, e, zero, zero, e, zero])
    assert got == [ID48, got[1], ID48, ID48, got[1], ID48] and got[1] == expected([e], z, 1, log_n)[1][0]
    assert dom.open_evals([zero] * 5, z, v) == ([0] * 5, [ID48] * 5, ID48)
    assert dom.open_evals([zero], z) == ([0], [ID48], ID48)
    assert dom.open_evals([zero, e], z, v) == expected([zero, e], z, v, log_n)
    dom.close()


# ---- the context is left as it was found ----------------------------------------------------------------------------------------
def test_context_left_as_found_with_tables_held():
    """plonk_ctx_last_msm, plonk_ctx_last_msm_points and a prover's proof bytes on the same context are what they were, with the
    handle's tables built, used and still held meanwhile; the only trace is the handle's share of plonk_ctx_table_bytes"""
    import plonk_amd as P
    from tests import circuits as C
    c = P.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=78)()
    case = C.compile_fast(comp, b"kzg-evals-tables")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = P.Prover.compile(c, b"kzg-evals-tables", cols["selectors"], cols["wires"], cols["witnesses"])
    rnd = random.Random(77)
    proof = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    assert len(proof) == 1008
    c.msm([rnd.randrange(Q) for _ in range(100)])
    msm_report = c.last_msm()
    c.msm_points([E.g1_mul(E.G1_GEN, 3), E.g1_mul(E.G1_GEN, 5)], [2, 9])
    points_report = c.last_msm_points()
    dom = P.KzgDomain(c, 6)
    tables, rows = c.table_bytes(), c.table_rows()
    info = dom.build_tables()
    e = [[rnd.randrange(Q) for _ in range(64)] for _ in range(6)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    for zz in (z, EM.domain_points(6)[9]):
        assert dom.open_evals(e, zz, v) == expected(e, zz, v, 6)
    assert dom.commit_evals(e[:1]) == expected(e[:1], z, v, 6)[1]
    dom.open_multi(e, [(0, 3), (5, 63)])
    assert dom.tables_last()["group_launches"] == 4
    assert c.last_msm() == msm_report
    assert c.last_msm_points() == points_report
    assert prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3)) == proof
    assert c.table_bytes() == (tables[0] + info["table_bytes"], tables[1]) and c.table_rows() == rows
    dom.close()
    assert c.table_bytes() == tables
    prover.close()
    c.close()
