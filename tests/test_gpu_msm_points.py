"""GPU: plonk_msm_points / plonk_msm_points_dev — the variable-base MSM over caller-supplied points (msm_points.hip) — against
the oracle (oracle/bls12_381.py: msm_naive, g1_mul) or a closed form, never against Context.msm, the per-term kernel or the
code under test.  Both layouts (raw x || y and compressed), both entry points, both paths (buckets and the per-term kernel
below min_bucket_terms), forced digit widths and slice lengths, the adversarial point sets of tests/msm_points_cases.py, the
plan a call reports against the plan the shared header computes on the host, and the error paths."""
import ctypes
import functools
import random
from collections import Counter

import pytest

import plonk_amd
from oracle import bls12_381 as E
from tests import msm_points_cases as C

pytestmark = pytest.mark.gpu
Q, LAMBDA = C.Q, C.LAMBDA
PER_TERM = 1 << 30   # min_bucket_terms that sends every call to the per-term kernel


@pytest.fixture(scope="module")
def ctx():
    c = plonk_amd.Context(0)
    yield c
    c.close()


def call_dev(ctx, points, scalars, compressed=False, **opts):
    """msm_points_dev on uploaded copies; returns the affine sum"""
    m = len(scalars)
    pb = b"".join(plonk_amd.g1_compress(p) for p in points) if compressed else C.raw96(points)
    dp, ds, do = ctx.alloc(max(len(pb), 16)), ctx.alloc(max(32 * m, 16)), ctx.alloc(112)
    try:
        if m:
            dp.upload(pb)
            ds.upload(plonk_amd.fr_to_bytes_mont(scalars))
        ctx.msm_points_dev(dp.ptr, ds.ptr, m, do.ptr, compressed=compressed, **opts)
        return plonk_amd.g1_from_raw97(do.download(97))
    finally:
        dp.free(), ds.free(), do.free()


@functools.lru_cache(maxsize=None)
def random_terms():
    """200 seeded terms and the running sums of s_i P_i: expected[m] = the sum of the first m"""
    rnd = random.Random(0x7465726d)
    pts = C.pool()[:200]
    scalars = [rnd.randrange(Q) for _ in pts]
    acc, sums = None, [None]
    for p, s in zip(pts, scalars):
        acc = E.g1_add(acc, E.g1_mul(p, s))
        sums.append(acc)
    return pts, scalars, sums


@pytest.mark.parametrize("m", [0, 1, 2, 3, 63, 64, 65, 200])
def test_trivial_sizes_both_layouts_entries_and_paths(ctx, m):
    pts, scalars, sums = random_terms()
    pts, scalars, want = pts[:m], scalars[:m], sums[m]
    for min_terms, path in ((1, 1), (PER_TERM, 0)):
        for compressed in (False, True):
            assert ctx.msm_points(pts, scalars, compressed=compressed, min_bucket_terms=min_terms) == want
            info = ctx.last_msm_points()
            assert (info["path"], info["terms"]) == (path if m else info["path"], m)
            assert call_dev(ctx, pts, scalars, compressed=compressed, min_bucket_terms=min_terms) == want
    # bytes in, as the binding's other form takes them
    assert ctx.msm_points(C.raw96(pts), scalars) == want


@functools.lru_cache(maxsize=None)
def edge_case():
    s = C.edge_scalars([2, 4, 5, 13, 16])
    pts = C.pool()[:len(s)]
    return pts, s, E.msm_naive(pts, s)


@pytest.mark.parametrize("window_bits", [2, 4, 5, 13, 16, 0])
def test_edge_scalars_at_forced_widths(ctx, window_bits):
    pts, s, want = edge_case()
    assert ctx.msm_points(pts, s, window_bits=window_bits, min_bucket_terms=1) == want
    info = ctx.last_msm_points()
    assert info["path"] == 1
    assert info["window_bits"] == (window_bits or C.host_plan(len(s))["window_bits"])
    assert info["nonzero_digits"] == C.host_count_digits(pts, s, info["window_bits"])
    assert call_dev(ctx, pts, s, window_bits=window_bits, slice_entries=3, min_bucket_terms=1) == want


CASES = C.point_cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_point_cases(ctx, name):
    _, pts, scalars, opts, want = next(c for c in CASES if c[0] == name)
    assert ctx.msm_points(pts, scalars, min_bucket_terms=1, **opts) == want
    assert ctx.last_msm_points()["path"] == 1
    # few buckets and slices of two: cut buckets, equal and opposite points inside one slice and across slices
    assert ctx.msm_points(pts, scalars, window_bits=3, slice_entries=2, min_bucket_terms=1) == want
    assert ctx.msm_points(pts, scalars, compressed=True, window_bits=2, slice_entries=1, min_bucket_terms=1) == want
    assert call_dev(ctx, pts, scalars, compressed=True, check=True, min_bucket_terms=1, **opts) == want
    assert ctx.last_msm_points()["path"] == 1
    # and as a caller gets it: the path by the default threshold (the per-term kernel at these sizes)
    assert ctx.msm_points(pts, scalars) == want
    assert ctx.last_msm_points()["path"] == C.host_plan(len(pts))["path"]
    if want is None:   # the infinity byte
        assert ctx.msm_points_bytes(C.raw96(pts), plonk_amd.fr_to_bytes_mont(scalars), len(pts)) == bytes(96) + b"\x01"


@pytest.mark.parametrize("m", [4, 5, 13, 64, 257])
def test_slices_of_one_bucket_per_window(ctx, m):
    """all scalars equal: every term lands in the same bucket of a window, so that bucket is cut into ceil(m / 4) slices
    and summed by the lane (up to 8 slices) or by the tree"""
    s = 0x2d1f3a7c9b2e4f60718293a4b5c6d7e8   # below LAMBDA: half 2 is zero, so no two entries of a term share a bucket
    pts = C.pool()[:m]
    assert ctx.msm_points(pts, [s] * m, slice_entries=4, min_bucket_terms=1) == C.equal_sum(pts, s)
    info = ctx.last_msm_points()
    plan = C.host_plan(m, slice_entries=4, min_bucket_terms=1)
    assert plan["path"] == 1
    c = plan["window_bits"]
    _, _, d1, d2 = C.host_recode(s, c)
    per_bucket = Counter((w, abs(d)) for digits in (d1, d2) for w, d in enumerate(digits) if d)
    assert s < LAMBDA and not any(d2) and max(per_bucket.values()) == 1   # a non-zero window's bucket holds exactly m entries
    assert {k: info[k] for k in plan} == plan
    assert info["nonzero_digits"] == m * len(per_bucket)
    assert info["slices"] == len(per_bucket) * -(-m // 4)
    assert info["longest_bucket"] == m
    # the same through a forced width, where both halves meet in one bucket of window 0 (2 m entries)
    assert ctx.msm_points(pts, [LAMBDA + 1] * m, window_bits=8, slice_entries=4, min_bucket_terms=1) == C.equal_sum(pts, LAMBDA + 1)
    info = ctx.last_msm_points()
    assert (info["window_bits"], info["longest_bucket"], info["slices"]) == (8, 2 * m, -(-2 * m // 4))


@pytest.mark.parametrize("opts", [{}, {"window_bits": 6}, {"window_bits": 16, "slice_entries": 7}, {"min_bucket_terms": 100},
                                  {"min_bucket_terms": 1, "window_bits": 3},
                                  {"min_bucket_terms": 101}, {"min_bucket_terms": PER_TERM, "window_bits": 9}])
def test_plan_report_equals_the_shared_header(ctx, opts):
    pts, scalars, sums = random_terms()
    m = 100
    pts, scalars = list(pts[:m]), list(scalars[:m])
    pts[7], scalars[9] = None, 0   # neither gives an entry
    want = E.g1_add(sums[m], E.g1_add(C.neg(E.g1_mul(C.pool()[7], scalars[7])), C.neg(E.g1_mul(C.pool()[9], random_terms()[1][9]))))
    assert ctx.msm_points(pts, scalars, **opts) == want
    info, plan = ctx.last_msm_points(), C.host_plan(m, **opts)
    assert {k: info[k] for k in plan} == plan
    assert plan["path"] == (0 if opts.get("min_bucket_terms", 64) > m else 1)   # 64: the measured default
    if plan["path"]:
        assert info["nonzero_digits"] == C.host_count_digits(pts, scalars, plan["window_bits"])
        assert info["slices"] >= info["nonzero_digits"] // plan["slice_entries"] and info["longest_bucket"] >= 1
    else:
        assert (info["nonzero_digits"], info["slices"], info["longest_bucket"]) == (0, 0, 0)


@pytest.mark.parametrize("window_bits", [0, 8])
def test_closed_form_over_a_generated_key(ctx, window_bits):
    """m = 2^14 + 3 points [g tau^i] G made on the device, seeded f_i: sum_i f_i [g tau^i] G = [g f(tau)] G — chunks, scans and
    trees all have several levels at this size"""
    m = (1 << 14) + 3
    rnd = random.Random(0x636c6f736564)
    tau, g = rnd.randrange(1, Q), rnd.randrange(1, Q)
    f = [rnd.randrange(Q) for _ in range(m)]
    acc = 0
    for v in reversed(f):
        acc = (acc * tau + v) % Q
    want = E.g1_mul(E.G1_GEN, g * acc % Q)
    dp, ds, do = ctx.alloc(96 * m), ctx.alloc(32 * m), ctx.alloc(112)
    try:
        ctx.srs_generate_dev(tau, g, m, dp.ptr)
        ds.upload(plonk_amd.fr_to_bytes_mont(f))
        ctx.msm_points_dev(dp.ptr, ds.ptr, m, do.ptr, window_bits=window_bits)
        assert plonk_amd.g1_from_raw97(do.download(97)) == want
        info, plan = ctx.last_msm_points(), C.host_plan(m, window_bits=window_bits)
        assert {k: info[k] for k in plan} == plan and info["path"] == 1
        assert info["nonzero_digits"] > 2 * m * (info["windows"] - 2) * 0.9
    finally:
        dp.free(), ds.free(), do.free()


def off_subgroup_point():
    """on the curve, outside the prime-order subgroup (the cofactor is ~2^126: a curve point found from its x is outside)"""
    x = 5
    while True:
        rhs = (x * x * x + 4) % E.P
        y = pow(rhs, (E.P + 1) // 4, E.P)
        if y * y % E.P == rhs and E.g1_add(E.g1_mul((x, y), Q - 1), (x, y)) is not None:   # [q] P (g1_mul reduces its scalar mod q)
            return x, y
        x += 1


def raw_call(ctx, fn, points, scalars, m, out, **fields):
    opts = plonk_amd._MsmPointsOpts(**fields)
    if "struct_size" in fields:
        opts.struct_size = fields["struct_size"]
    return fn(ctx.handle, points, scalars, m, ctypes.byref(opts), out)


def test_checks_and_errors(ctx):
    pts, scalars, sums = random_terms()
    pts, scalars = list(pts[:20]), list(scalars[:20])
    assert ctx.msm_points(pts, scalars, check=True, min_bucket_terms=1) == sums[20]
    assert ctx.msm_points(pts, scalars, check=True) == sums[20]
    assert ctx.msm_points(pts, scalars, check=True, min_bucket_terms=PER_TERM) == sums[20]
    x, y = pts[4]
    sc = plonk_amd.fr_to_bytes_mont(scalars)
    filler = bytes(range(97))
    for bad in (off_subgroup_point(), (x, (y + 1) % E.P)):
        bad_pts = pts[:11] + [bad] + pts[12:]
        for min_terms in (1, PER_TERM):
            out = ctypes.create_string_buffer(filler, 97)
            rc = raw_call(ctx, ctx.lib.plonk_msm_points, C.raw96(bad_pts), sc, 20, out, flags=plonk_amd.POINTS_CHECK, min_bucket_terms=min_terms)
            assert rc == -10 and out.raw == filler
            with pytest.raises(plonk_amd.PointMalformed):
                ctx.msm_points(bad_pts, scalars, check=True, min_bucket_terms=min_terms)
        dp, ds, do = ctx.alloc(96 * 20), ctx.alloc(32 * 20), ctx.alloc(112)
        dp.upload(C.raw96(bad_pts)), ds.upload(sc), do.upload(filler)
        with pytest.raises(plonk_amd.PointMalformed):
            ctx.msm_points_dev(dp.ptr, ds.ptr, 20, do.ptr, check=True, min_bucket_terms=1)
        assert do.download(97) == filler
        dp.free(), ds.free(), do.free()
    # a compressed point that does not decode is an error with or without the check
    comp = b"".join(plonk_amd.g1_compress(p) for p in pts)
    no_flag = comp[:48 * 3] + bytes(48) + comp[48 * 4:]
    x_no_root = 5
    while pow((x_no_root ** 3 + 4) % E.P, (E.P - 1) // 2, E.P) == 1:
        x_no_root += 1
    not_on_curve = comp[:48 * 3] + bytes([0x80]) + x_no_root.to_bytes(48, "big")[1:] + comp[48 * 4:]
    for bad_comp in (no_flag, not_on_curve):
        for min_terms in (1, PER_TERM):
            out = ctypes.create_string_buffer(filler, 97)
            assert raw_call(ctx, ctx.lib.plonk_msm_points, bad_comp, sc, 20, out, flags=plonk_amd.POINTS_COMPRESSED, min_bucket_terms=min_terms) == -10
            assert out.raw == filler
    assert ctx.msm_points(comp, scalars, compressed=True, min_bucket_terms=1) == sums[20]
    # arguments
    out = ctypes.create_string_buffer(filler, 97)
    lib = ctx.lib
    assert raw_call(ctx, lib.plonk_msm_points, C.raw96(pts), sc, (1 << 24) + 1, out) == -1
    assert raw_call(ctx, lib.plonk_msm_points, C.raw96(pts), sc, 20, out, struct_size=16) == -1
    assert raw_call(ctx, lib.plonk_msm_points, C.raw96(pts), sc, 20, out, window_bits=1) == -1
    assert raw_call(ctx, lib.plonk_msm_points, C.raw96(pts), sc, 20, out, window_bits=17) == -1
    assert raw_call(ctx, lib.plonk_msm_points, C.raw96(pts), sc, 20, out, flags=4) == -1
    assert raw_call(ctx, lib.plonk_msm_points, None, sc, 20, out) == -1
    assert raw_call(ctx, lib.plonk_msm_points_dev, None, None, (1 << 24) + 1, None) == -1
    assert out.raw == filler
    assert lib.plonk_msm_points(ctx.handle, C.raw96(pts), sc, 20, None, out) == 0     # NULL opts = automatic
    assert plonk_amd.g1_from_raw97(out.raw) == sums[20]
    assert ctx.last_msm_points()["terms"] == 20    # the failed calls left the report of the last good one


def wires_of(composer, size):
    W = composer.witnesses
    cols = [[0] * size for _ in range(4)]
    for i, g in enumerate(composer.constraints):
        cols[0][i], cols[1][i], cols[2][i], cols[3][i] = W[g.a], W[g.b], W[g.c], W[g.d]
    return cols


def test_determinism_and_isolation(kat_setup):
    """the same call twice gives the same bytes; a commit-key MSM and a proof on the same context are byte-identical before
    and after msm_points calls (the call has its own workspace and touches neither the key nor the MSM scratch)"""
    from oracle.rng import StdRng
    _, oprover, circuit = kat_setup
    ctx = plonk_amd.Context(0)
    fresh = plonk_amd.Context(0)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        fresh.last_msm_points()
    assert ei.value.code == -7
    fresh.close()
    ctx.srs_load(oprover.ck)
    prover = plonk_amd.Prover(ctx, oprover.constraints, oprover.label, oprover.pk.polys, None)
    rng = StdRng.seed_from_u64(0x9235E701)
    blinders = [rng.random_scalar() for _ in range(14)]
    comp = circuit()
    rnd = random.Random(11)
    key_scalars = plonk_amd.fr_to_bytes_mont([rnd.randrange(Q) for _ in range(len(oprover.ck))])
    msm_before = ctx.msm_bytes(key_scalars, len(oprover.ck))
    proof_before = prover.prove(wires_of(comp, oprover.size), {}, blinders)
    pts, scalars, sums = random_terms()
    raw, sc = C.raw96(pts), plonk_amd.fr_to_bytes_mont(scalars)
    for opts in ({}, {"min_bucket_terms": PER_TERM}, {"window_bits": 5, "slice_entries": 2, "min_bucket_terms": 1}):
        a = ctx.msm_points_bytes(raw, sc, 200, **opts)
        b = ctx.msm_points_bytes(raw, sc, 200, **opts)
        assert a == b and plonk_amd.g1_from_raw97(a) == sums[200]
    assert ctx.msm_bytes(key_scalars, len(oprover.ck)) == msm_before
    assert prover.prove(wires_of(comp, oprover.size), {}, blinders) == proof_before
    prover.close()
    ctx.close()
