"""GPU: KZG10 cell recovery (plonk_kzg_recover_cells / _dev / plonk_kzg_recover_last; plonk_amd/csrc/kzg_recover.hip) on the
suite's synthetic known-tau key.  Round trips go through plonk_kzg_open_cells: cells are dropped, recovered, and the
coefficients must be the polynomial's, the cells, proofs and commitments byte for byte those of open_cells.  The four kernels
are also run on their own through tests/_build/libdev_kzg_recover.so (tests/csrc/dev_kzg_recover.hip, built by build(): doors
only, the kernels are libplonk_hip.so's) against the big-int model tests/kzg_recover_model.py, with guard slots.  Every
comparison is exact."""
import ctypes
import os
import random

import pytest

from oracle import bls12_381 as E
from tests import kzg_recover_model as M
from tests import kzg_ref as K
from tests.test_gpu_kzg_cells import cell_key, load_key

pytestmark = pytest.mark.gpu
Q = E.Q
OK, ERR_ARG, ERR_DEGREE, ERR_STATE, ERR_DATA, ERR_VERIFY = 0, -1, -3, -7, -9, -12
ID48 = K.IDENTITY48
KEY_POINTS = 1 << 13
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_recover.so")
GUARD = b"\xA5"


@pytest.fixture(scope="module")
def doors():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_recover.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    so.dkr_vanish.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    so.dkr_scatter.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp]
    so.dkr_divide.argtypes = [vp, vp, vp, u32, u32, u32]
    so.dkr_tail.argtypes = [vp, vp, u32, u64, u32, vp]
    return so


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, KEY_POINTS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def domains(ctx):
    import plonk_amd
    made = {}

    def get(log_n):
        if log_n not in made:
            made[log_n] = plonk_amd.KzgDomain(ctx, log_n)
        return made[log_n]
    yield get
    for d in made.values():
        d.close()


def mont(values):
    import plonk_amd
    return plonk_amd.fr_to_bytes_mont(values)


def unmont(raw):
    import plonk_amd
    return plonk_amd.fr_from_bytes_mont(raw)


def rand_raw(rnd, m):
    """m random canonical field elements as Montgomery bytes"""
    raw = bytearray(rnd.randbytes(32 * m))
    for i in range(31, 32 * m, 32):
        raw[i] &= 0x3F
    return bytes(raw)


def pick(cells_raw, ids, l, n, j=0):
    """the packed input of polynomial j: the cells `ids` of open_cells' cell-major bytes"""
    return b"".join(cells_raw[32 * (j * n + k * l):32 * (j * n + (k + 1) * l)] for k in ids)


def assert_last(dom, log_cell, count, available, max_len, cap=M.WS_CAP_DEFAULT, want_values=True, inconsistent=0):
    last, p = dom.recover_last(), M.plan(dom.log_n, log_cell, count, available, cap, want_values)
    assert (last["log_n"], last["log_cell"], last["count"], last["available"], last["max_len"]) == (dom.log_n, log_cell, count, available, max_len)
    assert (last["missing"], last["chunks"], last["chunk_polys"], last["transforms"], last["vanish_muls"], last["workspace_bytes"]) == \
        (p["missing"], p["chunks"], p["chunk_polys"], p["transforms"], p["vanish_muls"], p["ws_bytes"])
    assert last["inconsistent"] == inconsistent
    return last


def patterns(r, need, rnd):
    """the available cells per missing pattern, at least `need` of them: none missing, all but `need`, a contiguous block, every
    odd cell, every even cell, a random set in shuffled order"""
    block = set(range(r // 4, r // 4 + max(r // 2, 1)))
    out = {"none": list(range(r)),
           "all but the needed": sorted(rnd.sample(range(r), need)),
           "block": [k for k in range(r) if k not in block],
           "odd": list(range(0, r, 2)),
           "even": list(range(1, r, 2))}
    ids = rnd.sample(range(r), rnd.randint(need, r))
    out["random shuffled"] = ids
    return {name: ids for name, ids in out.items() if len(ids) >= need}


# ---- round trips at small sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_cell", [(a, b) for a in (2, 3, 4, 6) for b in range(1, a)])
def test_round_trip_every_pattern_and_length(domains, log_n, log_cell):
    dom, n, l, r = domains(log_n), 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(100 * log_n + log_cell)
    polys = {d: [rnd.randrange(1, Q) for _ in range(d)] for d in sorted({1, l - 1, l, l + 1, n // 2, n} - {0})}
    polys[0] = [0]                                             # the zero polynomial, presented with max_len = 1
    seen = set()
    for d, f in polys.items():
        d = max(d, 1)
        ref = dom.open_cells([f], log_cell)
        for name, ids in patterns(r, -(-d // l), rnd).items():
            a = len(ids)
            got = dom.recover_cells(ids, [[ref[0][0][k] for k in ids]], log_cell, d, coeffs=True)
            assert got[3] == [f + [0] * (n - len(f))], (d, name)
            assert got[:3] == ref, (d, name)
            assert_last(dom, log_cell, 1, a, d)
            seen.add(name)
            if name in ("none", "block", "odd") and (a, "exact") not in seen:      # d = a l exactly: a polynomial that fills the given cells
                seen.add((a, "exact"))
                g = [rnd.randrange(1, Q) for _ in range(a * l)]
                ref2 = dom.open_cells([g], log_cell)
                got = dom.recover_cells(ids, [[ref2[0][0][k] for k in ids]], log_cell, a * l, coeffs=True)
                assert got[3] == [g + [0] * (n - a * l)] and got[:3] == ref2, (a, name)
    assert {"none", "all but the needed", "block", "random shuffled"} <= seen and (r, "exact") in seen
    assert r == 2 or {"odd", "even"} <= seen
    zero = dom.recover_cells([0], [[[0] * l]], log_cell, 1, coeffs=True)
    assert zero[1] == [[ID48] * r] and zero[2] == [ID48] and zero[3] == [[0] * n]


# ---- larger round trips: the multi-pass transforms, the verifier, the cap on r ------------------------------------------------
@pytest.mark.parametrize("log_n", [11, 12])
def test_half_of_the_cells_of_64_missing_three_polynomials(ctx, domains, log_n):
    import plonk_amd
    dom, n, log_cell, l = domains(log_n), 1 << log_n, 6, 64
    r = n // l
    rnd = random.Random(log_n)
    raws = [rand_raw(rnd, n // 2), rand_raw(rnd, n // 2 - 3), rand_raw(rnd, 70)]
    cells, proofs, cm = dom.open_cells_bytes(raws, log_cell)
    ids = rnd.sample(range(r), r // 2)
    got = dom.recover_cells_bytes(ids, [pick(cells, ids, l, n, j) for j in range(3)], log_cell, n // 2, coeffs=True)
    assert got[0] == cells and got[1] == proofs and got[2] == cm
    assert got[3] == b"".join(raw + bytes(32 * n - len(raw)) for raw in raws)
    assert_last(dom, log_cell, 3, r // 2, n // 2)
    # the recovered proofs of the cells that were missing pass the cell verifier
    key = plonk_amd.KzgKey(ctx, cell_key(l))
    ver = plonk_amd.KzgCellVerifier(key, log_n, log_cell)
    lost = [k for k in range(r) if k not in ids]
    items = [(j, k, got[0][32 * (j * n + k * l):32 * (j * n + (k + 1) * l)], got[1][48 * (j * r + k):48 * (j * r + k + 1)])
             for j in range(3) for k in rnd.sample(lost, 4)]
    assert ver.verify([got[2][48 * j:48 * j + 48] for j in range(3)], items)
    ver.close()
    key.close()


def test_2048_cells_of_two_is_the_cap(domains):
    dom, n, log_cell, l, r = domains(12), 1 << 12, 1, 2, 2048
    rnd = random.Random(2048)
    raw = rand_raw(rnd, n // 2)
    cells, proofs, cm = dom.open_cells_bytes([raw], log_cell)
    ids = rnd.sample(range(r), r // 2)
    got = dom.recover_cells_bytes(ids, [pick(cells, ids, l, n)], log_cell, n // 2, coeffs=True)
    assert got == (cells, proofs, cm, raw + bytes(32 * n - len(raw)))
    last = assert_last(dom, log_cell, 1, r // 2, n // 2)
    assert last["vanish_muls"] == 2 * 2048 * 1024
    # log_n = 13 with cells of two: r = 4096
    import plonk_amd
    d13 = domains(13)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        d13.recover_cells_bytes([0, 1], [bytes(32 * 4)], 1, 4)
    assert ei.value.code == ERR_ARG
    assert d13.recover_cells_bytes([0, 1], [mont([1, 2, 3, 4, 5, 6, 7, 8])], 2, 8, proofs=False, commitments=False)[0] is not None


# ---- no redundancy, inconsistency -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_cell", [(4, 2), (6, 1), (6, 3), (6, 5)])
def test_no_redundancy_every_input_is_consistent(domains, log_n, log_cell):
    dom, n, l, r = domains(log_n), 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(log_n + log_cell)
    for a in sorted({1, r // 2, r - 1, r}):
        ids = rnd.sample(range(r), a)
        vals = [[[rnd.randrange(Q) for _ in range(l)] for _ in range(a)] for _ in range(2)]
        cells, proofs, cm, coeffs = dom.recover_cells(ids, vals, log_cell, a * l, coeffs=True)
        for j in range(2):
            assert [cells[j][k] for k in ids] == vals[j], (a, j)      # re-evaluating the result returns the given values
            assert coeffs[j][a * l:] == [0] * (n - a * l)
            assert (cells[j], proofs[j], cm[j]) == tuple(x[0] for x in dom.open_cells([coeffs[j]], log_cell))
        if a <= 4 and a * l <= 16:
            assert coeffs[0] == M.recover(ids, [x for c in vals[0] for x in c], log_n, log_cell, a * l)[0]


class Outputs:
    """the four outputs and the status with guard bytes around them, host memory"""

    def __init__(self, n, r, count):
        self.sizes = [32 * n * count, 32 * n * count, 48 * r * count, 48 * count, 4 * count]
        self.bufs = [ctypes.create_string_buffer(GUARD * (s + 64), s + 64) for s in self.sizes]

    def ptr(self, i):
        return ctypes.c_void_p(ctypes.addressof(self.bufs[i]) + 32)

    def untouched(self, which=(0, 1, 2, 3)):
        return all(self.bufs[i].raw == GUARD * (self.sizes[i] + 64) for i in which)

    def guards_intact(self):
        return all(b.raw[:32] == GUARD * 32 and b.raw[-32:] == GUARD * 32 for b in self.bufs)

    def status(self, count):
        return list((ctypes.c_int32 * count).from_buffer_copy(self.bufs[4].raw[32:32 + 4 * count]))


def raw_call(lib, handle, log_cell, ids, bufs, max_len, out, count=None, available=None, nulls=(), values_null=False, ids_null=False):
    keep = [ctypes.create_string_buffer(b, len(b)) if b is not None else None for b in bufs]
    parr = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.cast(k, ctypes.c_void_p).value if k is not None else None for k in keep])
    iarr = (ctypes.c_uint32 * max(len(ids), 1))(*ids)
    ptrs = [None if i in nulls else out.ptr(i) for i in range(5)]
    return lib.plonk_kzg_recover_cells(handle, log_cell, None if ids_null else iarr, len(ids) if available is None else available,
                                       None if values_null else parr, len(bufs) if count is None else count, max_len, *ptrs)


def test_one_changed_value_rejects_the_call_and_names_the_polynomial(ctx, domains):
    import plonk_amd
    dom, n, log_cell, l, r = domains(6), 64, 3, 8, 8
    rnd = random.Random(4)
    d, ids = 20, [6, 1, 4, 3]                                  # a l = 32 > d
    polys = [[rnd.randrange(1, Q) for _ in range(d)] for _ in range(4)]
    cells, proofs, cm = dom.open_cells_bytes([mont(f) for f in polys], log_cell)
    vals = [pick(cells, ids, l, n, j) for j in range(4)]
    good = dom.recover_cells_bytes(ids, vals, log_cell, d, coeffs=True)
    assert good[:3] == (cells, proofs, cm)
    bad = list(vals)
    at = 32 * 13
    bad[2] = vals[2][:at] + mont([(unmont(vals[2][at:at + 32])[0] + 1) % Q]) + vals[2][at + 32:]
    out = Outputs(n, r, 4)
    assert raw_call(ctx.lib, dom.handle, log_cell, ids, bad, d, out) == ERR_VERIFY
    assert out.status(4) == [OK, OK, ERR_VERIFY, OK] and out.untouched() and out.guards_intact()
    assert_last(dom, log_cell, 4, 4, d, inconsistent=1)
    with pytest.raises(plonk_amd.ProofVerificationError) as ei:
        dom.recover_cells_bytes(ids, bad, log_cell, d)
    assert ei.value.status == [OK, OK, ERR_VERIFY, OK] and ei.value.code == ERR_VERIFY
    # the resident form: device outputs keep their pattern too
    ins = [ctx.alloc(len(v)) for v in bad]
    for b, v in zip(ins, bad):
        b.upload(v)
    outs = [ctx.alloc(s) for s in (32 * n * 4, 32 * n * 4, 48 * r * 4, 48 * 4)]
    for b in outs:
        b.upload(GUARD * b.nbytes)
    with pytest.raises(plonk_amd.ProofVerificationError) as ei:
        dom.recover_cells_dev(ids, [b.ptr for b in ins], log_cell, d, *[b.ptr for b in outs])
    assert ei.value.status == [OK, OK, ERR_VERIFY, OK]
    assert all(b.download() == GUARD * b.nbytes for b in outs)
    # success fills the status with PLONK_OK and the outputs inside their guards
    assert raw_call(ctx.lib, dom.handle, log_cell, ids, vals, d, out) == OK
    assert out.status(4) == [OK] * 4 and out.guards_intact()
    assert tuple(out.bufs[i].raw[32:-32] for i in (1, 2, 3, 0)) == good
    # a polynomial of d + 1 coefficients presented with max_len = d; accepted with max_len = d + 1
    f1 = [rnd.randrange(1, Q) for _ in range(d + 1)]
    c1 = dom.open_cells_bytes([mont(f1)], log_cell)
    with pytest.raises(plonk_amd.ProofVerificationError) as ei:
        dom.recover_cells_bytes(ids, [pick(c1[0], ids, l, n)], log_cell, d)
    assert ei.value.status == [ERR_VERIFY]
    assert dom.recover_cells_bytes(ids, [pick(c1[0], ids, l, n)], log_cell, d + 1)[:3] == c1
    for b in ins + outs:
        b.free()


# ---- the kernels on their own -------------------------------------------------------------------------------------------------
def guarded(ctx, payload_bytes):
    b = ctx.alloc(payload_bytes + 64)
    b.upload(GUARD * b.nbytes)
    return b


def payload(buf):
    raw = buf.download()
    assert raw[:32] == GUARD * 32 and raw[-32:] == GUARD * 32
    return raw[32:-32]


@pytest.mark.parametrize("log_n,log_cell", [(2, 1), (7, 1), (12, 1), (12, 6)])
def test_vanish_kernel(ctx, doors, log_n, log_cell):
    """r = 2, 64, 2048 (and 64 with cells of 64): |M| = 0, 1, r - 1 against the model, and against the closed form
    Z_r(Y) = (Y^r - 1) / (Y - phi^k) of a single given cell k"""
    l, r = 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(r)
    phi, shift = (M.root(log_n - log_cell) if r > 1 else 1), pow(M.GEN, l, Q)
    pw = ctx.alloc(32 * r)
    k0 = rnd.randrange(r)
    for miss in ([], [rnd.randrange(r)], [k for k in range(r) if k != k0]):
        mbuf = ctx.alloc(4 * max(len(miss), 1))
        mbuf.upload(bytes((ctypes.c_uint32 * max(len(miss), 1))(*miss)))
        zd, zc = guarded(ctx, 32 * r), guarded(ctx, 32 * r)
        assert doors.dkr_vanish(ctx.handle, pw.ptr, mbuf.ptr, len(miss), log_n, log_cell, zd.ptr + 32, zc.ptr + 32) == 0
        got = unmont(payload(zd)), unmont(payload(zc))
        if len(miss) <= 1 or r <= 64:
            assert got == tuple(M.vanish(log_n, log_cell, miss))
        if len(miss) == r - 1:
            given = (set(range(r)) - set(miss)).pop()          # (at r = 2 the single missing cell of the second round too)
            x0 = pow(phi, given, Q)
            assert got[0] == [r * pow(x0, -1, Q) % Q if k == given else 0 for k in range(r)]
            ys = [shift * pow(phi, k, Q) % Q for k in range(r)]
            assert got[1] == [(pow(y, r, Q) - 1) * pow(y - x0, -1, Q) % Q for y in ys]
        assert all(got[1]) and [k for k in range(r) if got[0][k] == 0] == sorted(miss)
        for b in (mbuf, zd, zc):
            b.free()
    assert doors.dkr_vanish(ctx.handle, pw.ptr, None, 1, log_n, log_cell, pw.ptr, pw.ptr) == ERR_ARG
    pw.free()
    assert doors.dkr_vanish(ctx.handle, None, None, 0, 13, 1, None, None) == ERR_ARG


@pytest.mark.parametrize("log_n,log_cell", [(6, 1), (6, 5), (9, 3)])
def test_scatter_kernel(ctx, doors, log_n, log_cell):
    """the first and the last cell missing, l = 2 and l = n / 2, two polynomials, more than one workgroup (n = 512)"""
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(log_n * 10 + log_cell)
    for ids in ([k for k in range(1, r)][::-1], list(range(r - 1)), [r - 1] if r == 2 else rnd.sample(range(1, r - 1), (r - 2) // 2 + 1)):
        slot = M.slot_table(r, ids)
        zdom = [rnd.randrange(1, Q) for _ in range(r)]
        vals = [[rnd.randrange(Q) for _ in range(len(ids) * l)] for _ in range(2)]
        ins = [ctx.alloc(32 * len(v)) for v in vals]
        for b, v in zip(ins, vals):
            b.upload(mont(v))
        vecs, sl, zd = ctx.alloc(16), ctx.alloc(4 * r), ctx.alloc(32 * r)
        vecs.upload(bytes((ctypes.c_uint64 * 2)(*[b.ptr for b in ins])))
        sl.upload(bytes((ctypes.c_int32 * r)(*slot)))
        zd.upload(mont(zdom))
        out = guarded(ctx, 32 * n * 2)
        assert doors.dkr_scatter(ctx.handle, vecs.ptr, sl.ptr, zd.ptr, log_n, log_cell, 2, out.ptr + 32) == 0
        assert unmont(payload(out)) == M.scatter(vals[0], slot, zdom, log_n, log_cell) + M.scatter(vals[1], slot, zdom, log_n, log_cell)
        for b in ins + [vecs, sl, zd, out]:
            b.free()
    assert doors.dkr_scatter(ctx.handle, None, None, None, log_n, log_n, 1, None) == ERR_ARG
    assert doors.dkr_scatter(ctx.handle, None, None, None, log_n, log_cell, 0, None) == ERR_ARG


def test_divide_kernel(ctx, doors):
    log_n, log_cell, n, r = 9, 4, 512, 32
    rnd = random.Random(9)
    v = [[rnd.randrange(Q) for _ in range(n)] for _ in range(2)]
    zinv = [rnd.randrange(Q) for _ in range(r)]
    buf, z = guarded(ctx, 32 * n * 2), ctx.alloc(32 * r)
    buf.upload(mont(v[0] + v[1]), offset=32)
    z.upload(mont(zinv))
    assert doors.dkr_divide(ctx.handle, buf.ptr + 32, z.ptr, log_n, log_cell, 2) == 0
    assert unmont(payload(buf)) == M.divide(v[0], zinv, log_n, log_cell) + M.divide(v[1], zinv, log_n, log_cell)
    assert doors.dkr_divide(ctx.handle, buf.ptr + 32, z.ptr, log_n, 0, 2) == ERR_ARG
    buf.free()
    z.free()


@pytest.mark.parametrize("log_n", [3, 9, 19])
def test_tail_kernel(ctx, doors, log_n):
    """the empty range, the only non-zero coefficient at max_len - 1, at max_len and at n - 1; 2^19: more blocks than the grid has"""
    n, batch = 1 << log_n, 4
    max_len = n // 2 + 3
    rows = [{}, {max_len - 1: 5}, {max_len: 1 << 200}, {n - 1: 1}]
    buf = ctx.alloc(32 * n * batch)
    buf.upload(bytes(32 * n * batch))
    for b, row in enumerate(rows):
        for i, x in row.items():
            buf.upload(mont([x]), offset=32 * (b * n + i))
    flags = guarded(ctx, 4 * batch)
    assert doors.dkr_tail(ctx.handle, buf.ptr, log_n, max_len, batch, flags.ptr + 32) == 0
    got = list((ctypes.c_int32 * batch).from_buffer_copy(payload(flags)))
    assert got == [0, 0, 1, 1] == [M.tail([row.get(i, 0) for i in range(n)], max_len) for row in rows]
    assert doors.dkr_tail(ctx.handle, buf.ptr, log_n, n, batch, flags.ptr + 32) == 0          # max_len = n: nothing to look at
    assert list((ctypes.c_int32 * batch).from_buffer_copy(payload(flags))) == [0] * batch
    assert doors.dkr_tail(ctx.handle, buf.ptr, log_n, 1, batch, flags.ptr + 32) == 0
    assert list((ctypes.c_int32 * batch).from_buffer_copy(payload(flags))) == [0, 1, 1, 1]
    assert doors.dkr_tail(ctx.handle, buf.ptr, log_n, n + 1, batch, flags.ptr + 32) == ERR_ARG
    buf.free()
    flags.free()


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_every_documented_error_in_the_documented_order_with_nothing_written(ctx, domains):
    import plonk_amd
    dom, n, log_cell, l, r = domains(4), 16, 2, 4, 4
    lib = ctx.lib
    good = mont(list(range(1, 9)))                             # two cells
    noncanon = good[:32 * 5] + b"\xff" * 32 + good[32 * 6:]
    junk = rand_raw(random.Random(1), 8)                       # fits no polynomial of 5 coefficients
    out = Outputs(n, r, 2)

    def call(bufs=(good, good), ids=(2, 0), max_len=8, **kw):
        return raw_call(lib, kw.pop("h", dom.handle), kw.pop("lc", log_cell), list(ids), list(bufs), max_len, out, **kw)

    assert call(h=None) == ERR_ARG
    for lc in (0, 4, 5, 64, 0xffffffff):
        assert call(lc=lc) == ERR_ARG and call(lc=lc, bufs=[], count=0) == ERR_ARG
    assert call(count=65537) == ERR_ARG
    assert call(ids=[], available=0) == ERR_ARG and call(ids=[0, 1, 2, 3, 0], bufs=[good * 3]) == ERR_ARG
    assert call(ids=[2, 4]) == ERR_ARG and call(ids=[2, 2]) == ERR_ARG and call(ids=[0xffffffff, 1]) == ERR_ARG
    assert call(ids_null=True) == ERR_ARG and call(values_null=True) == ERR_ARG and call(bufs=[good, None]) == ERR_ARG
    assert call(max_len=0) == ERR_ARG and call(max_len=17) == ERR_ARG
    assert call(nulls=(0, 1, 2, 3)) == ERR_ARG and call(nulls=(0, 1, 2, 3), bufs=[], count=0) == ERR_ARG
    # ARG before DEGREE, DEGREE before DATA, DATA before VERIFY
    assert call(max_len=9, ids=[2, 2]) == ERR_ARG
    assert call(max_len=9) == ERR_DEGREE and call(max_len=9, bufs=[good, noncanon]) == ERR_DEGREE
    assert call(bufs=[good, noncanon]) == ERR_DATA and call(bufs=[junk, noncanon], max_len=5) == ERR_DATA
    assert out.untouched((0, 1, 2, 3, 4))
    assert call(bufs=[good, junk], max_len=5) == ERR_VERIFY and out.status(2)[1] == ERR_VERIFY and out.untouched()
    # count == 0 is PLONK_OK before the degree check and writes nothing; NULL arrays are legal there
    out = Outputs(n, r, 2)
    assert call(bufs=[], count=0, max_len=9) == OK and call(bufs=[], count=0, ids_null=True, values_null=True, available=2) == OK
    assert out.untouched((0, 1, 2, 3, 4))
    # the resident form scans the values on the device
    b0, b1 = ctx.alloc(len(good)), ctx.alloc(len(good))
    b0.upload(good)
    b1.upload(noncanon)
    cells = ctx.alloc(32 * n * 2)
    cells.upload(GUARD * cells.nbytes)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        dom.recover_cells_dev([2, 0], [b0.ptr, b1.ptr], log_cell, 8, cells=cells.ptr)
    assert ei.value.code == ERR_DATA and cells.download() == GUARD * cells.nbytes
    with pytest.raises(plonk_amd.PolynomialDegreeTooLarge):
        dom.recover_cells_dev([2, 0], [b0.ptr, b1.ptr], log_cell, 9, cells=cells.ptr)
    assert dom.recover_cells_dev([2, 0], [b0.ptr, b0.ptr], log_cell, 8, cells=cells.ptr) == [OK, OK]
    info = plonk_amd._KzgRecoverInfo()
    assert lib.plonk_kzg_recover_last(dom.handle, None) == ERR_ARG and lib.plonk_kzg_recover_last(None, ctypes.byref(info)) == ERR_ARG
    # a handle of log_n = 1 has no cell size at all
    for lc in (0, 1, 2):
        assert call(h=domains(1).handle, lc=lc) == ERR_ARG
    for b in (b0, b1, cells):
        b.free()


def test_state_errors_come_before_the_degree_check():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, 16)
    d = plonk_amd.KzgDomain(c, 3)
    vals = [mont([1, 2, 3, 4])]
    before = d.recover_cells_bytes([1, 3], vals, 1, 4, coeffs=True)
    assert d.recover_last()["count"] == 1
    c.comm_init(plonk_amd.Context.comm_unique_id(), 0, 1)
    for max_len in (4, 5):                                      # 5 > a l would be PLONK_ERR_DEGREE
        with pytest.raises(plonk_amd.PlonkError) as ei:
            d.recover_cells_bytes([1, 3], vals, 1, max_len)
        assert ei.value.code == ERR_STATE
    with pytest.raises(plonk_amd.PlonkError) as ei:
        d.recover_cells_bytes([1, 1], vals, 1, 4)
    assert ei.value.code == ERR_ARG                             # the arguments come first
    c.comm_destroy()
    assert d.recover_cells_bytes([1, 3], vals, 1, 4, coeffs=True) == before
    load_key(c, 16)                                             # the same key again: still another generation
    for call in (lambda: d.recover_cells_bytes([1, 3], vals, 1, 4), lambda: d.recover_cells_bytes([1, 3], vals, 1, 5),
                 lambda: d.recover_cells_bytes([1, 3], [], 1, 4), d.recover_last):
        with pytest.raises(plonk_amd.PlonkError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    d.close()
    d2 = plonk_amd.KzgDomain(c, 3)
    assert d2.recover_last() == dict.fromkeys(d2.recover_last(), 0) | {"log_n": 3}      # before the first call
    assert d2.recover_cells_bytes([1, 3], vals, 1, 4, coeffs=True) == before
    d2.close()
    c.close()


# ---- chunking, the resident form, two cell sizes, the neighbours ---------------------------------------------------------------
def test_forced_chunking_gives_the_same_bytes(domains):
    import plonk_amd
    dom, n, log_cell, l, r = domains(6), 64, 3, 8, 8
    rnd = random.Random(66)
    ids, d = [7, 2, 5, 0, 3], 33
    raws = [mont([rnd.randrange(Q) for _ in range(m)]) for m in (33, 10, 1, 32, 33)]
    cells, proofs, cm = dom.open_cells_bytes(raws, log_cell)
    vals = [pick(cells, ids, l, n, j) for j in range(5)]
    whole = dom.recover_cells_bytes(ids, vals, log_cell, d, coeffs=True)
    assert whole[:3] == (cells, proofs, cm)
    assert assert_last(dom, log_cell, 5, 5, d)["chunks"] == 1
    per = 3 * n * 32
    bad = list(vals)
    bad[4] = vals[4][:-32] + mont([7])
    try:
        for cap, chunks, polys in ((3 * per, 2, 3), (2 * per, 3, 2), (1, 5, 1)):
            dom._set_workspace_cap(cap)
            assert dom.recover_cells_bytes(ids, vals, log_cell, d, coeffs=True) == whole, cap
            last = assert_last(dom, log_cell, 5, 5, d, cap)
            assert (last["chunks"], last["chunk_polys"], last["transforms"]) == (chunks, polys, 5 * 7)
            assert dom.recover_cells_bytes(ids, vals, log_cell, d, proofs=False, commitments=False) == (cells, None, None, None)
            assert dom.recover_cells_bytes(ids, vals, log_cell, d, proofs=False, cells=False) == (None, None, cm, None)
            assert_last(dom, log_cell, 5, 5, d, cap, want_values=False)
            with pytest.raises(plonk_amd.ProofVerificationError) as ei:      # the verdict of the last chunk stops the whole call
                dom.recover_cells_bytes(ids, bad, log_cell, d)
            assert ei.value.status == [OK, OK, OK, OK, ERR_VERIFY]
    finally:
        dom._set_workspace_cap(0)
    assert dom.recover_cells_bytes(ids, vals, log_cell, d, coeffs=True) == whole


def test_resident_form_gives_the_bytes_of_the_host_form(ctx, domains):
    dom, n, log_cell, l, r = domains(6), 64, 2, 4, 16
    rnd = random.Random(67)
    ids = rnd.sample(range(r), 9)
    d = 30
    raws = [mont([rnd.randrange(Q) for _ in range(m)]) for m in (30, 1, 17)]
    cells, proofs, cm = dom.open_cells_bytes(raws, log_cell)
    vals = [pick(cells, ids, l, n, j) for j in range(3)]
    whole = dom.recover_cells_bytes(ids, vals, log_cell, d, coeffs=True)
    ins = [ctx.alloc(len(v)) for v in vals]
    for b, v in zip(ins, vals):
        b.upload(v)
    outs = [ctx.alloc(s) for s in (32 * n * 3, 32 * n * 3, 48 * r * 3, 48 * 3)]
    assert dom.recover_cells_dev(ids, [b.ptr for b in ins], log_cell, d, *[b.ptr for b in outs]) == [OK] * 3
    assert (outs[1].download(), outs[2].download(), outs[3].download(), outs[0].download()) == whole
    assert_last(dom, log_cell, 3, 9, d)
    # every subset of the outputs: what is not asked for is not written
    for keep in ((0,), (1,), (2,), (3,), (1, 3), (0, 2)):
        for b in outs:
            b.upload(GUARD * b.nbytes)
        args = [outs[i].ptr if i in keep else None for i in range(4)]
        assert dom.recover_cells_dev(ids, [b.ptr for b in ins], log_cell, d, *args) == [OK] * 3
        got = [b.download() for b in outs]
        for i, want in enumerate((whole[3], whole[0], whole[1], whole[2])):
            assert got[i] == (want if i in keep else GUARD * outs[i].nbytes), (keep, i)
        assert_last(dom, log_cell, 3, 9, d, want_values=(1 in keep or 2 in keep))
    for b in ins + outs:
        b.free()


def test_two_cell_sizes_alternate_and_the_other_entry_points_keep_their_state(ctx):
    import plonk_amd
    dom, n = plonk_amd.KzgDomain(ctx, 6), 64
    rnd = random.Random(77)
    polys = [[rnd.randrange(Q) for _ in range(32)], [rnd.randrange(Q) for _ in range(9)]]
    z = rnd.randrange(Q)
    opened = dom.open(polys)
    evals = dom.open_evals([opened[0][0]], z)
    a_ref, b_ref = dom.open_cells(polys, 2), dom.open_cells(polys, 4)
    info, evals_info, cells_info = dom.last(), dom.evals_last(), dom.cells_last()
    tables = ctx.table_bytes()
    ids2, ids4 = rnd.sample(range(16), 8), [3, 0]
    v2 = [[a_ref[0][j][k] for k in ids2] for j in range(2)]
    v4 = [[b_ref[0][j][k] for k in ids4] for j in range(2)]
    for _ in range(2):                                          # without proofs: the handle's other state does not move
        got = dom.recover_cells(ids2, v2, 2, 32, proofs=False, coeffs=True)
        assert (got[0], got[2], got[3]) == (a_ref[0], a_ref[2], [f + [0] * (n - len(f)) for f in polys])
        got = dom.recover_cells(ids4, v4, 4, 32, proofs=False)
        assert (got[0], got[2]) == (b_ref[0], b_ref[2])
        assert (dom.last(), dom.evals_last(), dom.cells_last()) == (info, evals_info, cells_info)
    assert dom.open_cells(polys, 2) == a_ref and dom.open_cells(polys, 4) == b_ref
    # with proofs the call runs open_cells' body: its info reports that, the tables are reused
    assert dom.recover_cells(ids2, v2, 2, 32)[:3] == a_ref and dom.recover_last()["built_table"] == 0
    assert dom.cells_last()["log_cell"] == 2 and dom.cells_last()["table_bytes"] == cells_info["table_bytes"]
    assert dom.recover_cells(ids4, v4, 4, 32)[:3] == b_ref
    assert (dom.last(), dom.evals_last()) == (info, evals_info) and ctx.table_bytes() == tables
    assert dom.open(polys) == opened and dom.last() == info and dom.open_evals([opened[0][0]], z) == evals
    dom.close()
    # a fresh handle: the recovery is the first to need the A^(u) of its cell size
    dom = plonk_amd.KzgDomain(ctx, 6)
    assert dom.recover_cells(ids2, v2, 2, 32, proofs=False)[0] == a_ref[0] and dom.recover_last()["built_table"] == 0
    assert dom.cells_last()["table_bytes"] == 0
    assert dom.recover_cells(ids2, v2, 2, 32)[:3] == a_ref and dom.recover_last()["built_table"] == 1
    assert dom.recover_cells(ids2, v2, 2, 32)[:3] == a_ref and dom.recover_last()["built_table"] == 0
    dom.close()


def test_context_left_as_found(ctx, domains):
    rnd = random.Random(78)
    f = [rnd.randrange(Q) for _ in range(300)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    sc = [rnd.randrange(Q) for _ in range(64)]
    opening, msm = ctx.kzg_open([f, f[:7]], z, v), ctx.msm(sc)
    tables, rows = ctx.table_bytes(), ctx.table_rows()
    dom = domains(6)
    ref = dom.open_cells([f[:40]], 3)
    assert dom.recover_cells([1, 2, 4, 6, 7], [[ref[0][0][k] for k in (1, 2, 4, 6, 7)]], 3, 40)[:3] == ref
    assert ctx.kzg_open([f, f[:7]], z, v) == opening and ctx.msm(sc) == msm
    assert (ctx.table_bytes(), ctx.table_rows()) == (tables, rows)
