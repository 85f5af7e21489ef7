"""GPU: quarter-density commit-key tables (PLONK_TABLE_QUARTERPOS: 64 rows, T[r][i] = 2^(4 r) P_i, 8 KiB per point) —
plonk_gpu_config.table_mode / PLONK_MSM_TABLE=quarter force the layout at any key size, every entry point over a key computes
the same bytes as with the other layouts, and the library reports what it ran (rows 64, digits of 16 bits over 2^15 buckets
or 20 bits over 2^19).  The recoding itself is checked on the CPU in tests/test_msm_quad_host.py."""
import json
import os
import random
import subprocess
import sys

import pytest

from oracle import bls12_381 as E

pytestmark = pytest.mark.gpu
Q = E.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KLO = "nbl::msm_accumulate_ordered_kernel"
SELECT = "basic or edge or skew or small_scalars or doubling"
PROVER_SELECT = "deterministic_v3 or random_arithmetic or host_time_slots or (proof_bytes_equal_c_oracle and not 16 and not 2p20)"
EDGE_VARIANTS = [
    ({"PLONK_MSM_TABLE": "quarter"}, {"table_rows": 64, "digit_width": 16, "bucket_bits": 15}),
    ({"PLONK_MSM_TABLE": "quarter", "PLONK_MSM_BUCKETS": "19"},
     {"table_rows": 64, "digit_width": 20, "bucket_bits": 19, "accumulate_kernel": KLO}),
    # the 13-slot partition is not built for quarter rows: with the switch set they still take msm_partition_kernel and the plan
    # does not claim PLONK_PLAN_SORT13 (flags: 2 = a lane per bucket sum, as for every ordered 2^19-bucket group)
    ({"PLONK_MSM_TABLE": "quarter", "PLONK_MSM_BUCKETS": "19", "PLONK_MSM_SORT13": "1"},
     {"table_rows": 64, "digit_width": 20, "bucket_bits": 19, "flags": 2, "accumulate_kernel": KLO}),
]
PROVER_VARIANT = {"PLONK_MSM_TABLE": "quarter", "PLONK_MSM_BUCKETS": "19"}


def run_variant(env_extra, select=SELECT, marker="gpu", target="tests/test_gpu_msm.py"):
    """tests/test_gpu_msm_variants.py's child: the selected tests of `target` in a process of their own under the switches"""
    env = dict(os.environ, **env_extra)
    return subprocess.run([sys.executable, "-m", "pytest", *target.split(), "-x", "-q", "-m", marker, "-k", select],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def _key(env):
    return ",".join(f"{k}={x}" for k, x in sorted(env.items()))


@pytest.fixture(scope="module")
def children():
    """the four children side by side, started when the first test asks for one; each test owns one child"""
    import concurrent.futures as cf
    pool = cf.ThreadPoolExecutor(max_workers=4)
    futs = {"prover": pool.submit(run_variant, PROVER_VARIANT, PROVER_SELECT, "gpu and not slow",
                                  "tests/test_gpu_prover.py tests/test_gpu_prove_sizes.py")}
    for variant, plan in EDGE_VARIANTS:
        futs["edge:" + _key(variant)] = pool.submit(run_variant, dict(variant, PLONK_TEST_EXPECT_PLAN=json.dumps(plan)))
    yield futs
    pool.shutdown(wait=False, cancel_futures=True)


@pytest.fixture(scope="module")
def srs300():
    r = random.Random(11)
    tau, g = r.randrange(1, Q), r.randrange(1, Q)
    base = E.g1_mul(E.G1_GEN, g)
    pts, p = [], 1
    for _ in range(300):
        pts.append(E.g1_mul(base, p))
        p = p * tau % Q
    return pts


# recoding boundaries of the 4-bit groups: digit widths 16 and 20, nibbles equal to the carry, the shared top digits
EDGE = [0, 1, 15, 16, 17, Q - 1, Q - 2,
        1 << 15, (1 << 15) - 1, (1 << 15) + 1, 1 << 16,
        1 << 19, (1 << 19) - 1, (1 << 19) + 1, 1 << 20, (1 << 20) - 1, (1 << 20) + 1,
        int("80000" * 12, 16), int("7ffff" * 12, 16), int("fffff" * 12, 16) % Q, int("8" * 63, 16) % Q, int("f" * 63, 16) % Q,
        (1 << 254) + 12345]


@pytest.mark.parametrize("bucket_bits", [0, 19], ids=["buckets-default", "buckets-2p19"])
def test_quarter_rows_on_a_300_point_key(srs300, bucket_bits):
    import plonk_amd
    n = len(srs300)
    ctx = plonk_amd.Context(0, plonk_amd.GpuConfig(table_mode=plonk_amd.TABLE_QUARTERPOS, msm_bucket_bits=bucket_bits))
    try:
        ctx.srs_load(srs300)
        assert plonk_amd.TABLE_QUARTERPOS == 64
        assert ctx.table_rows() == 64
        assert ctx.table_bytes()[0] == 64 * 128 * n
        assert ctx.get_config().table_mode == 64
        want_plan = {"table_rows": 64, "digit_width": 20 if bucket_bits else 16, "bucket_bits": 19 if bucket_bits else 15}
        if bucket_bits:
            want_plan["accumulate_kernel"] = KLO
        r = random.Random(1)
        for m in (1, 2, 3, 31, 32, 33, 64, 300):
            sc = [r.randrange(Q) for _ in range(m)]
            assert ctx.msm(sc) == E.msm_pippenger(srs300, sc), m
            plan = ctx.last_msm()
            assert plan == dict(ctx.describe_msm(m), terms=m)
            assert {k: plan[k] for k in want_plan} == want_plan, plan
        assert ctx.msm(EDGE) == E.msm_naive(srs300, EDGE)
        for s in EDGE:
            assert ctx.msm([s]) == (E.g1_mul(srs300[0], s) if s % Q else None), hex(s)
        assert ctx.msm([1] * 300) == E.msm_naive(srs300, [1] * 300)       # one hot bucket
        assert ctx.msm([5, Q - 5]) == E.msm_naive(srs300, [5, Q - 5])     # a cancelling pair
        assert ctx.msm([0] * 50) is None
        d = ctx.describe_msm(300, table_rows=64, table_points=300)
        assert {k: d[k] for k in want_plan} == want_plan and d["wide_words"] == 0
        # plonk_msm_batch: six unequal sets (two groups), an empty set and an all-zero set, against the single calls
        sets = [[r.randrange(Q) for _ in range(m)] for m in (300, 1, 0, 17, 299, 64)]
        sets[3] = [0] * len(sets[3])
        raw = [plonk_amd.fr_to_bytes_mont(s) for s in sets]
        got = ctx.msm_batch_bytes(raw)
        for k, s in enumerate(sets):
            assert got[k] == ctx.msm_bytes(raw[k], len(s)), k
            assert plonk_amd.g1_from_raw97(got[k]) == E.msm_pippenger(srs300[:len(s)], s), k
    finally:
        ctx.close()


def test_an_unknown_row_count_is_refused():
    import plonk_amd
    with pytest.raises(plonk_amd.PlonkError) as ei:
        plonk_amd.Context(0, plonk_amd.GpuConfig(table_mode=65))
    assert ei.value.code == -1                                             # PLONK_ERR_ARG


@pytest.mark.parametrize("variant,plan", EDGE_VARIANTS, ids=[_key(v) for v, _ in EDGE_VARIANTS])
def test_quarter_rows_match_the_oracle_on_the_edge_cases(children, variant, plan):
    """the edge-case MSM tests of tests/test_gpu_msm.py under PLONK_MSM_TABLE=quarter; the child's
    test_basic_plan_is_the_variant_that_was_asked_for compares the plan, so an ignored override fails there"""
    r = children["edge:" + _key(variant)].result()
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_prover_parity_holds_with_quarter_rows(children):
    """whole proofs (reference KAT digest, random circuits, widget circuits vs the C oracle) with every key in quarter rows"""
    r = children["prover"].result()
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_kat_proof_bytes_are_the_same_on_quarter_rows(kat_setup):
    """the reference KAT circuit proved on a quarter-rows context and on a default one: identical proof bytes, and the
    provers say which rows their Lagrange-basis keys took"""
    import plonk_amd
    from oracle.rng import StdRng
    _, oprover, circuit = kat_setup
    rng = StdRng.seed_from_u64(0x9235E701)
    blinders = [rng.random_scalar() for _ in range(14)]
    comp = circuit()
    W = comp.witnesses
    cols = [[0] * oprover.size for _ in range(4)]
    for i, g in enumerate(comp.constraints):
        cols[0][i], cols[1][i], cols[2][i], cols[3][i] = W[g.a], W[g.b], W[g.c], W[g.d]
    proofs = []
    for cfg, rows in ((plonk_amd.GpuConfig(table_mode=plonk_amd.TABLE_QUARTERPOS), 64), (plonk_amd.GpuConfig(), 16)):
        ctx = plonk_amd.Context(0, cfg)
        try:
            ctx.srs_load(oprover.ck)
            assert ctx.table_rows() == rows
            p = plonk_amd.Prover(ctx, oprover.constraints, oprover.label, oprover.pk.polys, None)
            assert p.describe()["lagrange_table_rows"] == rows
            proofs.append(p.prove(cols, {}, blinders))
            p.close()
        finally:
            ctx.close()
    assert len(proofs[0]) == 1008 and proofs[0] == proofs[1]


def test_wide_sort_words_with_quarter_rows():
    """the smallest key whose 64 rows need the 64-bit sort words over 2^15 buckets (rows * points > 2^27): 2^21 + 64 points,
    17 GB of tables; 1 024 random scalars against the closed form [g sum s_i tau^i] G, over 2^15 and over 2^19 buckets"""
    import plonk_amd
    from conftest import configure
    r = random.Random(2164)
    n = (1 << 21) + 64
    tau, g = r.randrange(1, Q), r.randrange(1, Q)
    ctx = plonk_amd.Context(0, plonk_amd.GpuConfig(table_mode=plonk_amd.TABLE_QUARTERPOS))
    try:
        buf = ctx.alloc(96 * n)
        ctx.srs_generate_dev(tau, g, n, buf.ptr)
        ctx.srs_load_dev(buf.ptr, n)
        buf.free()
        assert ctx.table_rows() == 64 and ctx.table_bytes()[0] == 64 * 128 * n
        sc = [r.randrange(Q) for _ in range(1024)]
        acc, p = 0, 1
        for s in sc:
            acc = (acc + s * p) % Q
            p = p * tau % Q
        want = E.g1_mul(E.G1_GEN, g * acc % Q)
        for bits, width in ((15, 16), (19, 20)):
            configure(ctx, msm_bucket_bits=bits)
            assert ctx.msm(sc) == want, bits
            plan = ctx.last_msm()
            assert (plan["table_rows"], plan["bucket_bits"], plan["digit_width"], plan["wide_words"]) == (64, bits, width, 1), plan
    finally:
        ctx.close()
