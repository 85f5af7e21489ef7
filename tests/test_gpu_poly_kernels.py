"""GPU: the O(n) kernels of plonk_amd/csrc/poly.hip ONE BY ONE against the big-int models of tests/poly_ref.py (pinned to
oracle.plonk by tests/test_poly_ref_host.py), at the sizes where their code takes another path — the four batch-inversion
geometries and their ragged tails, zeros in the inversion, the 2 / 8 elements per lane of the prefix product, more than 256
block totals, the 4 / 16 coefficients per lane of poly_eval and the Horner loop of its final kernel, the three geometries of
the power kernel behind the Ruffini division, the range forms a sharded proof uses — which whole proofs only reach at
power-of-two sizes, on non-zero data, or in the minutes-long cases.

The launchers are reached through tests/_build/libdev_poly.so (tests/csrc/dev_poly.hip, built by build(): doors only, the
kernels are libplonk_hip.so's).  Every test draws from a fixed seed, puts 0 (where the operation allows it), 1, 2, q - 1 and
(q + 1) / 2 among random operands, compares EVERY output element, and gives each buffer one guard element past its end
that must come back unchanged.  Nothing here has a tolerance: all comparisons are exact integers mod q."""
import ctypes
import functools
import os
import random

import pytest

import poly_ref as M
from oracle import plonk as O
from oracle.bls12_381 import Q
from oracle.fft import EvaluationDomain

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_poly.so")
ERR_ARG = -1
GUARD = bytes(range(0xA0, 0xC0))            # 32 bytes no kernel writes (and no canonical field element: the top limb is above q's)
FILL = b"\x5A" * 32                         # what output buffers hold before a call
CLEAR_TOP = bytes(b & 0x3F for b in range(256))
HALF = (Q + 1) // 2


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(SO), "tests/_build/libdev_poly.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dp_batch_inverse.argtypes = [vp, vp, u64, ci, ci]
    so.dp_scan_prefix_product.argtypes = [vp, vp, u64, vp]
    so.dp_scan_prefix_product_local.argtypes = [vp, vp, u64, vp]
    so.dp_scan_prefix_product_apply.argtypes = [vp, vp, u64, vp, vp]
    so.dp_scan_prefix_blocks.argtypes = [u64]
    so.dp_scan_prefix_blocks.restype = u32
    so.dp_scan_suffix_sum.argtypes = [vp, vp, u64, vp]
    so.dp_poly_eval.argtypes = [vp, vp, vp, vp, ci, u64, vp, u32, vp]
    so.dp_poly_lincomb.argtypes = [vp, vp, vp, vp, ci, u64, vp, vp]
    so.dp_poly_ruffini.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp]
    so.dp_poly_ruffini_local.argtypes = [vp, vp, u64, u64, vp, vp, vp]
    so.dp_poly_ruffini_finish.argtypes = [vp, vp, vp, u64, u64, vp, vp, u64]
    so.dp_poly_mul_arrays.argtypes = [vp, vp, vp, u64, vp]
    so.dp_poly_trimmed_len.argtypes = [vp, vp, u64, vp]
    so.dp_poly_split_t.argtypes = [vp, vp, u64, u64, vp, vp, u64]
    so.dp_poly_fold.argtypes = [vp, vp, vp, u64, u32, vp]
    so.dp_grand_product.argtypes = [vp, u32, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp]
    return so


class Dev:
    """device buffers of one test: n elements + the guard, freed when the test ends"""

    def __init__(self, ctx, lib):
        self.ctx, self.lib, self.h, self.bufs = ctx, lib, ctx.handle, []

    def put(self, data: bytes):
        b = self.ctx.alloc(len(data) + 32)
        b.upload(data + GUARD)
        b.n = len(data) // 32
        self.bufs.append(b)
        return b

    def out(self, n: int):
        return self.put(FILL * n)

    def get(self, b, n=None) -> bytes:
        """the buffer's elements; the guard must be as it was"""
        raw = b.download()
        assert raw[32 * b.n:] == GUARD, "the element past the end of a buffer was written"
        return raw[:32 * (b.n if n is None else n)]

    def ints(self, b, n=None):
        return M.raw_ints(self.get(b, n))

    def flag(self, value=0):
        b = self.ctx.alloc(8)
        b.upload(value.to_bytes(4, "little") + b"\xEE\xEE\xEE\xEE")
        self.bufs.append(b)
        return b

    def flag_value(self, b) -> int:
        raw = b.download()
        assert raw[4:] == b"\xEE\xEE\xEE\xEE"
        return int.from_bytes(raw[:4], "little")

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


@pytest.fixture
def dev(ctx, lib):
    d = Dev(ctx, lib)
    yield d
    d.free()


def fr(x: int) -> bytes:
    """one field element as a host argument (data form)"""
    return (x % Q * M.R % Q).to_bytes(32, "little")


def draw_both(rnd, n, form=M.R, zeros=True, specials=True):
    """n raw integers and their bytes: random ones below 2^254 with the edge operands 1, 2, q - 1, (q + 1) / 2 (and 0) of
    `form` among them, every edge operand at the first and the last index of some draw as the seeds go"""
    raw = bytearray(rnd.randbytes(32 * n))
    raw[31::32] = raw[31::32].translate(CLEAR_TOP)
    v = M.raw_ints(bytes(raw))
    if specials and n:
        for s in M.SPECIALS + ((0,) if zeros else ()):
            i = rnd.choice((0, n - 1, rnd.randrange(n), rnd.randrange(n)))
            v[i] = s * form % Q
            raw[32 * i:32 * i + 32] = v[i].to_bytes(32, "little")
    return v, bytes(raw)


def draw(rnd, n, form=M.R, zeros=True, specials=True):
    return draw_both(rnd, n, form, zeros, specials)[0]


@functools.lru_cache(maxsize=2)
def shared_draw(seed, n, zeros=True):
    """one array per (seed, size) for the tests that only differ in a scalar: (raw integers, their bytes)"""
    return draw_both(random.Random(seed), n, zeros=zeros)


def mismatches(got, want):
    assert len(got) == len(want)
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]


# =====================================================================================================================
# batch inversion
# =====================================================================================================================
def zero_patterns(rnd, n, lanes, per_lane):
    """(name, indices to zero): the shapes the nz mask of batch_inverse_kernel has to get right"""
    w = lanes * per_lane
    g = max(0, (n - 1) // w - 1) if n > w else 0          # a full workgroup when there is one, not always the first
    t0 = rnd.randrange(lanes)
    return [("none", []),
            ("first", [0]),
            ("last", [n - 1]),
            ("one lane", [i for i in (g * w + t0 + k * lanes for k in range(per_lane)) if i < n]),
            ("one workgroup", [i for i in range(g * w, (g + 1) * w) if i < n]),
            ("all", list(range(n))),
            ("a tenth", [i for i in range(n) if rnd.random() < 0.1])]


def run_batch_inverse(dev, rnd, n, twiddle, bi_cfg):
    lanes, per_lane = M.BI_GEOMETRY[bi_cfg if bi_cfg >= 0 else M.bi_auto(n)]
    form = M.T if twiddle else M.R
    base = draw(rnd, n, form, zeros=False)
    k = M.BI_CONST[twiddle]
    for name, idx in zero_patterns(rnd, n, lanes, per_lane):
        v = list(base)
        for i in idx:
            v[i] = 0
        buf = dev.put(M.raw_bytes(v))
        assert dev.lib.dp_batch_inverse(dev.h, buf.ptr, n, int(twiddle), bi_cfg) == 0
        got = dev.ints(buf)
        # by multiplication: got * x = the form's constant, canonical; a zero stays zero
        bad = [i for i, (r, o) in enumerate(zip(v, got)) if (o != 0 if r == 0 else (o >= Q or r * o % Q != k))][:8]
        assert not bad, "bi_cfg %d, n = %d, zeros: %s: wrong at %r" % (bi_cfg, n, name, bad)
        buf.free()
    # and the edge operands by value
    v = [s * form % Q for s in (1, 2, Q - 1, HALF)]
    buf = dev.put(M.raw_bytes(v))
    assert dev.lib.dp_batch_inverse(dev.h, buf.ptr, 4, int(twiddle), bi_cfg) == 0
    assert dev.ints(buf) == [s * form % Q for s in (1, HALF, Q - 1, 2)]


@pytest.mark.parametrize("twiddle", [False, True], ids=["data", "twiddle"])
@pytest.mark.parametrize("bi_cfg", [0, 1, 2, 3])
def test_batch_inverse_every_geometry_with_ragged_tails_and_zeros(dev, bi_cfg, twiddle):
    lanes, per_lane = M.BI_GEOMETRY[bi_cfg]
    w = lanes * per_lane
    assert w == (4096, 256, 1024, 1024)[bi_cfg]
    rnd = random.Random(100 + 2 * bi_cfg + twiddle)
    for n in (1, 2, 63, 64, 65, w - 1, w, w + 1, 3 * w + 5):
        run_batch_inverse(dev, rnd, n, twiddle, bi_cfg)


@pytest.mark.parametrize("twiddle", [False, True], ids=["data", "twiddle"])
@pytest.mark.parametrize("n", [1, 65, 1 << 17, (1 << 17) + 1])
def test_batch_inverse_automatic_geometry_and_its_switch(dev, n, twiddle):
    run_batch_inverse(dev, random.Random(200 + n % 7 + twiddle), n, twiddle, -1)


# =====================================================================================================================
# prefix product (the grand product's scan) and its range form
# =====================================================================================================================
# one block, the 512-element block edge, 256 totals with one per lane of the totals kernel, the switch to 8 per lane, 257
# totals (two per lane, ragged last block) and 258, the first size at which the LAST of more than 256 totals is read
PREFIX_SIZES = [1, 2, 511, 512, 513, 1 << 17, (1 << 17) + 1, (1 << 19) + 1, (1 << 19) + 2049]


def run_prefix(dev, v, raw=None):
    n = len(v)
    data = dev.put(M.raw_bytes(v) if raw is None else raw)
    totals = dev.out(M.scan_prefix_blocks(n))
    assert dev.lib.dp_scan_prefix_blocks(n) == M.scan_prefix_blocks(n)
    assert dev.lib.dp_scan_prefix_product(dev.h, data.ptr, n, totals.ptr) == 0
    dev.get(totals)
    return dev.ints(data)


@pytest.mark.parametrize("n", PREFIX_SIZES)
def test_prefix_product(dev, n):
    v, raw = draw_both(random.Random(300 + n % 11), n, M.T, zeros=False)
    assert not mismatches(run_prefix(dev, v, raw), M.prefix_product_raw(v))


@pytest.mark.parametrize("n,at", [(1537, 700), ((1 << 17) + 1, 70000), ((1 << 19) + 1, (1 << 19) - 3000)])
def test_prefix_product_is_zero_from_a_zero_on(dev, n, at):
    v = draw(random.Random(310 + n % 11), n, M.T, zeros=False)
    v[at] = 0
    got = run_prefix(dev, v)
    assert not mismatches(got, M.prefix_product_raw(v))
    assert got[at - 1] != 0 and got[at:] == [0] * (n - at)


@pytest.mark.parametrize("cuts", [(5, 70000), (3, (1 << 17) + 4)], ids=["2-per-lane", "8-per-lane"])
def test_prefix_product_by_ranges_equals_the_whole(dev, cuts):
    """three unequal ranges of 2^17 + 5 elements as three ranks of a sharded proof run them: _local on each, the range
    products carried forward on the host (prover.hip), _apply"""
    n = (1 << 17) + 5
    v = draw(random.Random(320 + cuts[0]), n, M.T, zeros=False)
    whole = M.prefix_product_raw(v)
    data = dev.put(M.raw_bytes(v))
    ranges = list(zip((0,) + cuts, cuts + (n,)))
    tot_bufs, want_local = [], []
    for lo, hi in ranges:
        nb = M.scan_prefix_blocks(hi - lo)
        assert dev.lib.dp_scan_prefix_blocks(hi - lo) == nb
        t = dev.out(nb)
        assert dev.lib.dp_scan_prefix_product_local(dev.h, data.ptr + 32 * lo, hi - lo, t.ptr) == 0
        local, totals = M.prefix_local_raw(v[lo:hi])
        assert not mismatches(dev.ints(t), totals)
        tot_bufs.append((t, totals))
        want_local += local
    assert not mismatches(dev.ints(data), want_local)
    carry, before = M.T, 1
    for (lo, hi), (t, totals) in zip(ranges, tot_bufs):
        # the reported range product: (everything before) * (this range) = the whole scan at the range's last element
        assert before * totals[-1] % Q * M.TINV % Q * M.R % Q == whole[hi - 1]
        before = before * totals[-1] % Q * M.TINV % Q
        assert dev.lib.dp_scan_prefix_product_apply(dev.h, data.ptr + 32 * lo, hi - lo, t.ptr, carry.to_bytes(32, "little")) == 0
        carry = M.carry_next_raw(carry, totals[-1])
    assert not mismatches(dev.ints(data), whole)


# =====================================================================================================================
# suffix sum
# =====================================================================================================================
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, (1 << 19) + 2049])
def test_suffix_sum(dev, n):
    v, raw = draw_both(random.Random(400 + n % 13), n)
    data = dev.put(raw)
    totals = dev.out((n + 2047) // 2048)
    assert dev.lib.dp_scan_suffix_sum(dev.h, data.ptr, n, totals.ptr) == 0
    dev.get(totals)
    assert not mismatches(dev.ints(data), M.suffix_sum(v))        # linear: the model on data-form raws


# =====================================================================================================================
# poly_eval
# =====================================================================================================================
def call_eval(dev, base, items, max_len, max_blocks=None, out=None, slots=None):
    """items: (offset into base, length, point); returns (code, out buffer, partial buffer)"""
    count = len(items)
    slots = count if slots is None else slots
    nb = M.eval_blocks(max_len) if max_blocks is None else max_blocks
    polys = (ctypes.c_void_p * max(count, 1))(*[base.ptr + 32 * off for off, _, _ in items])
    lens = (ctypes.c_uint64 * max(count, 1))(*[ln for _, ln, _ in items])
    xs = b"".join(fr(x) for _, _, x in items)
    partial = dev.out(max(1, min(slots, 16) * nb))
    out = dev.out(max(1, min(slots, 16))) if out is None else out
    rc = dev.lib.dp_poly_eval(dev.h, polys, lens, xs, count, max_len, partial.ptr, nb, out.ptr)
    return rc, out, partial


def eval_items(rnd, max_len, count, points):
    """item 0 is the longest; lengths 0, 1 and others beside it, each a view of the one buffer, at either point"""
    lens = [max_len, 0, 1, max_len - 1, max_len // 2, 2, max_len, 3] + [rnd.randrange(max_len + 1) for _ in range(8)]
    items = []
    for k in range(count):
        ln = min(lens[k], max_len)
        items.append((rnd.randrange(max_len - ln + 1), ln, points[k % len(points)] if k else points[0]))
    if count >= 2:
        items[1] = (items[1][0], items[1][1], points[-1])      # both points in one call whenever there are two
    return items


def check_eval(dev, rnd, max_len, count, points):
    v, raw = draw_both(rnd, max_len)
    base = dev.put(raw)
    items = eval_items(rnd, max_len, count, points)
    rc, out, partial = call_eval(dev, base, items, max_len)
    assert rc == 0
    dev.get(partial)
    dev.get(base)
    want = [M.poly_eval(v[off:off + ln], x) for off, ln, x in items]      # linear: data-form raws in, data-form raw out
    assert dev.ints(out) == want


POINT_SETS = {"0,r": lambda r: (0, r), "1,q-1": lambda r: (1, Q - 1), "r,r'": lambda r: (r, r * r % Q + 5), "q-1,0": lambda r: (Q - 1, 0)}


@pytest.mark.parametrize("points", list(POINT_SETS))
@pytest.mark.parametrize("count", [1, 2, 15, 16])
def test_poly_eval_counts_and_points(dev, count, points):
    rnd = random.Random(500 + count)
    check_eval(dev, rnd, 1025, count, POINT_SETS[points](rnd.randrange(2, Q)))


@pytest.mark.parametrize("max_len", [1, 1023, 1024, 1025, 1 << 17, (1 << 17) + 1, 5 * 4096 + 1])
def test_poly_eval_sizes(dev, max_len):
    rnd = random.Random(510 + max_len % 17)
    r = rnd.randrange(2, Q)
    check_eval(dev, rnd, max_len, 16 if max_len < 100000 else 5, (r, Q - 1) if max_len % 2 else (r, rnd.randrange(2, Q)))


@pytest.mark.parametrize("max_len", [(1 << 20) + 1, 2 * (1 << 20) + 4097], ids=["final-loop-once", "final-loop-twice"])
def test_poly_eval_more_than_256_workgroups(dev, max_len):
    """the Horner loop of eval_final_kernel over the partials t, t + 256, ...: three items that are views of ONE buffer —
    the whole, a suffix of it at the same point (its value falls out of the same Horner pass) and a short view at a second
    point whose upper workgroups are all empty"""
    assert M.eval_blocks(max_len) == (257 if max_len < (1 << 21) else 514)       # lanes 0, 1: two steps of the loop
    rnd = random.Random(520)
    v, raw = draw_both(rnd, max_len)
    base = dev.put(raw)
    x1, k = rnd.randrange(2, Q), 4099
    short = (max_len - 70001, 70001, Q - 1)
    rc, out, partial = call_eval(dev, base, [(0, max_len, x1), (k, max_len - k, x1), short], max_len)
    assert rc == 0
    dev.get(partial)
    ev = M.suffix_evals(v, x1, [0, k])
    assert dev.ints(out) == [ev[0], ev[k], M.poly_eval(v[short[0]:], short[2])]


def test_poly_eval_refusals_launch_nothing(dev):
    rnd = random.Random(530)
    n = 1025
    base = dev.put(M.raw_bytes(draw(rnd, n)))
    x = [rnd.randrange(2, Q) for _ in range(3)]
    out = dev.out(16)
    cases = {"three points": dict(items=[(0, n, x[0]), (0, n, x[1]), (0, n, x[2])], max_len=n),
             "17 items": dict(items=[(0, n, x[0])] * 17, max_len=n),
             "max_len 0": dict(items=[(0, 0, x[0])], max_len=0, max_blocks=1),
             "max_blocks too small": dict(items=[(0, n, x[0])], max_len=n, max_blocks=M.eval_blocks(n) - 1)}
    for name, kw in cases.items():
        rc, _, partial = call_eval(dev, base, out=out, slots=16, **{"max_blocks": 2, **kw})
        assert rc == ERR_ARG, name
        assert dev.get(out) == FILL * 16 and dev.get(partial) == FILL * partial.n, name
    # and the same call with what it lacked goes through
    rc, _, _ = call_eval(dev, base, [(0, n, x[0])], n, out=out, slots=16)
    assert rc == 0 and dev.get(out)[32:] == FILL * 15


# =====================================================================================================================
# poly_lincomb
# =====================================================================================================================
@pytest.mark.parametrize("count", [0, 1, 24])
@pytest.mark.parametrize("length", [1, 255, 256, 257])
def test_poly_lincomb(dev, length, count):
    rnd = random.Random(600 + length + count)
    v = draw(rnd, 3 * length + 8)
    base = dev.put(M.raw_bytes(v))
    lens = [length, 0, length - 1, length + 3, 1, length // 2] + [rnd.randrange(length + 4) for _ in range(18)]
    scal = [rnd.randrange(1, Q), 0, 1, Q - 1, HALF, 2] + [rnd.randrange(Q) for _ in range(18)]
    if count == 1:
        lens, scal = [max(1, length - 1)], [scal[0]]
    terms = [(rnd.randrange(2 * length), lens[k], scal[k]) for k in range(count)]
    const = rnd.randrange(1, Q)
    polys = (ctypes.c_void_p * 24)(*[base.ptr + 32 * off for off, _, _ in terms])
    lens_c = (ctypes.c_uint64 * 24)(*[ln for _, ln, _ in terms])
    out = dev.out(length)
    rc = dev.lib.dp_poly_lincomb(dev.h, polys, lens_c, b"".join(fr(s) for _, _, s in terms) or fr(0), count, length, fr(const), out.ptr)
    assert rc == 0
    want = M.lincomb([(v[off:off + ln], s) for off, ln, s in terms], length, const * M.R % Q)
    assert dev.ints(out) == want
    dev.get(base)


# =====================================================================================================================
# Ruffini: division by X - z
# =====================================================================================================================
def z_of(kind):
    return {"1": 1, "q-1": Q - 1, "random": random.Random(700).randrange(2, Q - 1)}[kind]


@pytest.mark.parametrize("kind", ["1", "q-1", "random"])      # (the upper list varies fastest: one draw per size)
@pytest.mark.parametrize("n", [1, 2, 1 << 17, (1 << 17) + 1, 1 << 19, (1 << 19) + 1])
def test_ruffini(dev, n, kind):
    z = z_of(kind)
    v, raw = shared_draw(710, n)
    src, dst, scratch = dev.put(raw), dev.out(n), dev.out(n)
    totals = dev.out((n + 2047) // 2048)
    assert dev.lib.dp_poly_ruffini(dev.h, src.ptr, dst.ptr, n, fr(z), fr(M.inv(z)), scratch.ptr, totals.ptr) == 0
    got = dev.ints(dst)
    assert got[n - 1] == 0                                        # the remainder slot
    assert not mismatches(got, M.ruffini(v, z))
    assert dev.get(src) == raw
    dev.get(scratch)
    dev.get(totals)


@pytest.mark.parametrize("kind", ["q-1", "random"])
def test_ruffini_by_ranges_equals_the_whole(dev, kind):
    """three ranges, two of them with lo > 0 and one longer than 2^17 (another geometry of the power kernel); the test is
    the host of prover.hip: it reads every range's scratch[0] and hands each range the sum of those above it"""
    z = z_of(kind)
    n = (1 << 18) + 777
    v, raw = shared_draw(720, n)
    bounds = [0, 1000, (1 << 17) + 2000, n]
    src, dst = dev.put(raw), dev.out(n)
    parts = []
    for lo, hi in zip(bounds, bounds[1:]):
        scratch, totals = dev.out(hi - lo + 1), dev.out((hi - lo + 2047) // 2048)
        assert dev.lib.dp_poly_ruffini_local(dev.h, src.ptr + 32 * lo, lo, hi - lo, fr(z), scratch.ptr, totals.ptr) == 0
        s = dev.ints(scratch)
        assert not mismatches(s, M.ruffini_local(v[lo:hi], lo, z))
        dev.get(totals)
        parts.append((lo, hi, scratch, s[0]))
    assert sum(p[3] for p in parts) % Q == M.poly_eval(v, z)      # the numerator at z, as prove() uses it
    for k, (lo, hi, scratch, _) in enumerate(parts):
        carry = sum(p[3] for p in parts[k + 1:]) % Q
        rc = dev.lib.dp_poly_ruffini_finish(dev.h, scratch.ptr, dst.ptr, lo, hi - lo, fr(M.inv(z)), carry.to_bytes(32, "little"), n - 1)
        assert rc == 0
    got = dev.ints(dst)
    assert got[n - 1] == 0
    assert not mismatches(got, M.ruffini(v, z))


# =====================================================================================================================
# small kernels
# =====================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 257])
def test_mul_arrays_flags_a_zero_of_b_only(dev, n):
    rnd = random.Random(800 + n)
    for zero_in in ("neither", "a", "b"):
        a, b = draw(rnd, n, M.T, zeros=False), draw(rnd, n, M.T, zeros=False)
        if zero_in != "neither":
            (a if zero_in == "a" else b)[rnd.randrange(n)] = 0
        da, db, flag = dev.put(M.raw_bytes(a)), dev.put(M.raw_bytes(b)), dev.flag()
        assert dev.lib.dp_poly_mul_arrays(dev.h, da.ptr, db.ptr, n, flag.ptr) == 0
        assert dev.ints(da) == [x * y % Q * M.TINV % Q for x, y in zip(a, b)]      # twiddle form is closed under the product
        assert dev.flag_value(flag) == (1 if zero_in == "b" else 0) == M.mul_arrays(a, b)[1]
        assert dev.ints(db) == b


@pytest.mark.parametrize("n", [255, 256, 257, 70000])
def test_trimmed_len(dev, n):
    rnd = random.Random(810 + n % 5)
    for last in sorted({0, n - 1, n // 2, min(n - 1, 300)}):      # index 0, the end, another block
        v = draw(rnd, last + 1) + [0] * (n - 1 - last)
        v[last] = v[last] or 1
        if last:
            v[last - 1] = 0
        word = dev.ctx.alloc(16)
        dev.bufs.append(word)
        word.upload(bytes(8) + GUARD[:8])
        assert dev.lib.dp_poly_trimmed_len(dev.h, dev.put(M.raw_bytes(v)).ptr, n, word.ptr) == 0
        raw = word.download()
        assert int.from_bytes(raw[:8], "little") == last + 1 == M.trimmed_len(v) and raw[8:] == GUARD[:8]
    word = dev.ctx.alloc(16)
    dev.bufs.append(word)
    word.upload(bytes(8) + GUARD[:8])
    assert dev.lib.dp_poly_trimmed_len(dev.h, dev.put(bytes(32 * n)).ptr, n, word.ptr) == 0
    assert word.download() == bytes(8) + GUARD[:8]                # all zero: the word stays 0


@pytest.mark.parametrize("n", [4, 1024])
def test_split_t(dev, n):
    rnd = random.Random(820 + n)
    np_ = n + 8
    t = draw(rnd, 3 * n + 7)
    b = [rnd.randrange(1, Q) for _ in range(3)]
    dt, out = dev.put(M.raw_bytes(t)), dev.out(3 * np_)
    assert dev.lib.dp_poly_split_t(dev.h, dt.ptr, n, np_, out.ptr, b"".join(fr(x) for x in b), 7) == 0
    want_out, want_t = M.split_t(t, n, np_, [x * M.R % Q for x in b])
    assert dev.ints(out) == want_out
    assert dev.ints(dt) == want_t


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("n", [4, 1024])
def test_fold(dev, n, extra):
    rnd = random.Random(830 + n + extra)
    src = draw(rnd, n + extra)
    c = rnd.randrange(1, Q)
    ds, dst = dev.put(M.raw_bytes(src)), dev.out(n)
    assert dev.lib.dp_poly_fold(dev.h, ds.ptr, dst.ptr, n, extra, fr(c)) == 0
    assert dev.ints(dst) == M.fold(src, n, extra, c)
    assert dev.ints(ds) == src


# =====================================================================================================================
# the grand-product chain of prove(): terms -> inversion -> product -> scan
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def perm_case(log_n):
    """random wires, sigma = a random permutation of the positions K_j w^i, and the oracle's z for them"""
    rnd = random.Random(900 + log_n)
    n = 1 << log_n
    dom = EvaluationDomain(n)
    roots = dom.elements()
    wires = [[rnd.choice(M.SPECIALS + (0,)) if rnd.random() < 0.1 else rnd.randrange(Q) for _ in range(n)] for _ in range(4)]
    pos = [k * r % Q for k in (1, 7, 13, 17) for r in roots]
    rnd.shuffle(pos)
    sigma = [pos[k * n:(k + 1) * n] for k in range(4)]
    beta, gamma = rnd.randrange(1, Q), rnd.randrange(1, Q)
    z = O.permutation_vec(dom, wires, beta, gamma, sigma)
    return roots, wires, sigma, beta, gamma, z


def upload_perm(dev, wires, sigma):
    w = [dev.put(M.raw_bytes(M.to_data(col))) for col in wires]
    s = [dev.put(M.raw_bytes(M.to_data(col))) for col in sigma]
    return (ctypes.c_void_p * 4)(*[b.ptr for b in w]), (ctypes.c_void_p * 4)(*[b.ptr for b in s])


@pytest.mark.parametrize("log_n", [1, 2, 5, 13, 14])
def test_grand_product_chain_is_the_oracles_permutation_vec(dev, log_n):
    roots, wires, sigma, beta, gamma, z = perm_case(log_n)
    n = 1 << log_n
    wp, sp = upload_perm(dev, wires, sigma)
    num, den, totals, flag = dev.out(n), dev.out(n), dev.out(M.scan_prefix_blocks(n)), dev.flag()
    rc = dev.lib.dp_grand_product(dev.h, log_n, wp, sp, fr(beta), fr(gamma), 0, 0, num.ptr, den.ptr, totals.ptr, flag.ptr)
    assert rc == 0
    assert not mismatches(dev.ints(num), M.to_data(z))
    assert dev.flag_value(flag) == 0
    dev.get(den)
    dev.get(totals)


@pytest.mark.parametrize("log_n", [1, 2, 5, 13, 14])
def test_grand_product_over_two_ranges_equals_the_whole(dev, log_n):
    roots, wires, sigma, beta, gamma, z = perm_case(log_n)
    n = 1 << log_n
    cut = 1 if n == 2 else n // 2 + n // 8 + 1
    wp, sp = upload_perm(dev, wires, sigma)
    num, den, flag = dev.out(n), dev.out(n), dev.flag()
    carry, tots = M.T, []
    for lo, hi in ((0, cut), (cut, n)):
        t = dev.out(M.scan_prefix_blocks(hi - lo))
        rc = dev.lib.dp_grand_product(dev.h, log_n, wp, sp, fr(beta), fr(gamma), lo, hi - lo, num.ptr, den.ptr, t.ptr, flag.ptr)
        assert rc == 0
        tots.append((lo, hi, t, dev.ints(t)[-1]))
    assert dev.flag_value(flag) == 0
    for lo, hi, t, total in tots:
        assert carry * total % Q * M.TINV % Q * M.TINV % Q == z[hi - 1]        # carry * range product = z at the range's end
        assert dev.lib.dp_scan_prefix_product_apply(dev.h, num.ptr + 32 * lo, hi - lo, t.ptr, carry.to_bytes(32, "little")) == 0
        carry = M.carry_next_raw(carry, total)
    assert not mismatches(dev.ints(num), M.to_data(z))
    dev.get(den)


@pytest.mark.parametrize("log_n", [2, 5, 13])
def test_grand_product_flags_a_zero_denominator(dev, log_n):
    roots, wires, sigma, beta, gamma, _ = perm_case(log_n)
    n = 1 << log_n
    row = n // 2 - 1
    wires = [list(col) for col in wires]
    wires[2][row] = (-beta * sigma[2][row] - gamma) % Q            # one factor of den[row + 1] is zero
    want, want_flag = M.grand_product(roots, wires, sigma, beta, gamma)
    assert want_flag == 1 and want[row] != 0 and want[row + 1:] == [0] * (n - row - 1)
    wp, sp = upload_perm(dev, wires, sigma)
    num, den, totals, flag = dev.out(n), dev.out(n), dev.out(M.scan_prefix_blocks(n)), dev.flag()
    rc = dev.lib.dp_grand_product(dev.h, log_n, wp, sp, fr(beta), fr(gamma), 0, 0, num.ptr, den.ptr, totals.ptr, flag.ptr)
    assert rc == 0
    assert dev.flag_value(flag) == 1
    assert not mismatches(dev.ints(num), M.to_data(want))           # the skipped zero stays zero; everything else is finite
    inv_den = dev.ints(den)
    assert inv_den[row + 1] == 0 and all(x < Q for x in inv_den)
    assert sum(1 for x in inv_den if x == 0) == 1
