"""GPU: witness diagnosis (plonk_prover_diagnose / _dev / _witnesses) against the plain-Python yardstick of
tests/diagnose_ref.py — exact reports through the three entry points and the three ways of building a prover, the
wrap-around of the last row, public inputs, truncation, agreement with prove() on both quotient domains, no disturbance
of the proofs that follow, 2^20 gates, the error surface."""
import ctypes
import random

import pytest

from tests import circuits as C
from tests import diagnose_cases as DC
from tests import diagnose_ref as DR

pytestmark = pytest.mark.gpu
Q = DC.Q


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    yield c
    c.close()


def load_srs(ctx, n):
    srs = C.synthetic_srs(n + 7)
    ctx.srs_load_bytes(srs, len(srs) // 96)


def col_bytes(cols):
    return [C.fr_bytes(c) for c in cols]


class Resident:
    """the four columns in HBM, contiguous a|b|c|d, as the _dev entry points take them"""

    def __init__(self, ctx, n):
        self.n, self.buf = n, ctx.alloc(4 * 32 * n)

    def put(self, raw_cols):
        for k in range(4):
            self.buf.upload(raw_cols[k], 32 * self.n * k)
        return self.buf.ptr

    def free(self):
        self.buf.free()


def check(d, want, n, cap=None):
    """a Diagnosis against the yardstick's full report"""
    assert d.ok == (not want)
    assert d.rows == (want if cap is None else want[:cap])
    assert d.info == DR.info(want, n)


def three_provers(ctx, comp, label):
    """created from coefficient forms, compiled from gate columns, loaded from a serialised prover (on a context of its
    own: loading replaces the commit key)"""
    import plonk_amd
    case = C.compile_fast(comp, label)
    load_srs(ctx, case["size"])
    cols = C.circuit_columns(comp)
    created = plonk_amd.Prover(ctx, case["constraints"], label, case["polys"])
    compiled = plonk_amd.Prover.compile(ctx, label, cols["selectors"], cols["wires"], cols["witnesses"])
    ctx2 = plonk_amd.Context(0)
    loaded = plonk_amd.Prover.from_bytes(ctx2, compiled.to_bytes())
    return case, cols, created, compiled, loaded, ctx2


def test_exact_reports_through_every_entry_point_and_every_kind_of_prover(ctx):
    for name, comp in DC.small_circuits():
        n = DC.size_of(comp)
        case, cc, created, compiled, loaded, ctx2 = three_provers(ctx, comp, b"diagnose-" + name.encode())
        pi = dict(comp.public_inputs)
        sigma = comp.sigma_mappings(n)
        res = {id(ctx): Resident(ctx, n), id(ctx2): Resident(ctx2, n)}
        cases = [(None, list(comp.witnesses))] + list(DC.witness_mutations(comp))
        nonempty = 0
        for w, vals in cases:
            cols = DR.columns(comp, n, vals)
            want = DR.report(comp, n, cols, sigma=sigma)
            assert (w is not None) or want == []
            nonempty += bool(want)
            raw = col_bytes(cols)
            check(compiled.diagnose_witnesses(vals, pi, cap=n), want, n)
            for gp in (created, compiled, loaded):
                check(gp.diagnose(raw, pi, cap=n), want, n)
                check(gp.diagnose_dev(res[id(gp.ctx)].put(raw), pi, cap=n), want, n)
        assert nonempty >= len(cases) - 12
        # single-cell forgeries of the raw columns: copy constraints (the witness form cannot express them)
        rnd = random.Random(1717)
        seen = 0
        for col, row in DC.cell_forgeries(comp, n, rnd, 32):
            cols = DR.columns(comp, n)
            cols[col][row] = (cols[col][row] + 1) % Q
            want = DR.report(comp, n, cols, sigma=sigma)
            raw = col_bytes(cols)
            for gp in (created, compiled, loaded):
                check(gp.diagnose(raw, pi, cap=n), want, n)
                check(gp.diagnose_dev(res[id(gp.ctx)].put(raw), pi, cap=n), want, n)
            for _, _, cp in want:
                seen |= cp
        assert seen == 0b1111
        for r in res.values():
            r.free()
        for gp in (created, compiled, loaded):
            gp.close()
        ctx2.close()


def test_the_last_row_reads_row_zero_when_there_is_no_padding(ctx):
    import plonk_amd
    comp, cols, want = DC.wraparound_case()
    assert want == [(0, 0, 0b1100), (63, 1 << 4, 0)]
    load_srs(ctx, 64)
    cc = C.circuit_columns(comp)
    gp = plonk_amd.Prover.compile(ctx, b"wrap", cc["selectors"], cc["wires"], cc["witnesses"])
    assert gp.size == 64
    check(gp.diagnose_witnesses(cc["values"], {}, cap=64), [], 64)
    check(gp.diagnose(col_bytes(cols), {}, cap=64), want, 64)
    gp.close()


def test_a_wrong_public_input_flags_the_arithmetic_identity_on_its_row(ctx):
    import plonk_amd
    comp = C.big_widget_circuit(256, 3)()
    cc = C.circuit_columns(comp)
    load_srs(ctx, 256)
    gp = plonk_amd.Prover.compile(ctx, b"pi", cc["selectors"], cc["wires"], cc["witnesses"])
    pi = dict(comp.public_inputs)
    assert len(pi) >= 2
    check(gp.diagnose_witnesses(cc["values"], pi, cap=256), [], 256)
    for row in sorted(pi):
        bad = dict(pi)
        bad[row] = (bad[row] + 1) % Q
        want = DR.report(comp, 256, DR.columns(comp, 256), pi=bad)
        assert want == [(row, 1, 0)]
        check(gp.diagnose_witnesses(cc["values"], bad, cap=256), want, 256)
    missing = dict(pi)
    row = sorted(missing)[0]
    del missing[row]                                     # an input the caller forgot: PI = 0 on that row
    check(gp.diagnose_witnesses(cc["values"], missing, cap=256), [(row, 1, 0)], 256)
    gp.close()


def test_truncation_keeps_the_lowest_rows_and_counts_everything(ctx):
    import plonk_amd
    comp = C.big_widget_circuit(1 << 10, seed=31)()
    n = DC.size_of(comp)
    cc = C.circuit_columns(comp)
    load_srs(ctx, n)
    gp = plonk_amd.Prover.compile(ctx, b"cap", cc["selectors"], cc["wires"], cc["witnesses"])
    vals = [(v + 1) % Q for v in comp.witnesses]         # every witness off by one: most rows fail something
    cols = DR.columns(comp, n, vals)
    want = DR.report(comp, n, cols)
    assert len(want) > 300
    pi = dict(comp.public_inputs)
    for cap in (0, 1, 5, 64, 257, len(want), n):
        check(gp.diagnose_witnesses(vals, pi, cap=cap), want, n, cap=cap)
    # cap = 0 with out = NULL straight through the C-ABI
    info = plonk_amd._UnsatInfo()
    raw = C.fr_bytes(vals)
    idx, val, cnt = gp._pi(pi)
    assert ctx.lib.plonk_prover_diagnose_witnesses(gp.handle, raw, len(vals), idx, val, cnt, None, 0, ctypes.byref(info)) == -6
    assert info.rows_failing == len(want) and info.first_row == want[0][0]
    assert ctx.lib.plonk_prover_diagnose_witnesses(gp.handle, raw, len(vals), idx, val, cnt, None, 0, None) == -6
    gp.close()


@pytest.mark.parametrize("domain", [4, 8])
def test_diagnose_and_prove_agree_on_which_witnesses_are_unsatisfied(ctx, domain):
    import plonk_amd
    from conftest import configure
    configure(ctx, quotient_domain=domain)
    try:
        comp = C.big_widget_circuit(1 << 12, seed=412)()
        n = DC.size_of(comp)
        cc = C.circuit_columns(comp)
        load_srs(ctx, n)
        gp = plonk_amd.Prover.compile(ctx, b"agree", cc["selectors"], cc["wires"], cc["witnesses"])
        assert gp.describe()["quotient_domain"] == domain
        pi = dict(comp.public_inputs)
        sigma = comp.sigma_mappings(n)
        bl = C.fr_vals(C.blinders(77))
        rnd = random.Random(4120 + domain)
        unused = [w for w, uses in comp.witness_map.items() if not uses][:3]
        cases = [("honest", DR.columns(comp, n))]
        for w in unused + [rnd.randrange(len(comp.witnesses)) for _ in range(24)]:
            vals = list(comp.witnesses)
            vals[w] = (vals[w] + 1) % Q
            cases.append((("witness", w), DR.columns(comp, n, vals)))
        for col, row in DC.cell_forgeries(comp, n, rnd, 12):
            cols = DR.columns(comp, n)
            cols[col][row] = (cols[col][row] + 1) % Q
            cases.append((("cell", col, row), cols))
        verdicts = []
        for what, cols in cases:
            want = DR.report(comp, n, cols, sigma=sigma)
            raw = col_bytes(cols)
            d = gp.diagnose(raw, pi, cap=n)
            check(d, want, n)
            try:
                gp.prove(raw, pi, bl)
                proved = True
            except plonk_amd.CircuitUnsatisfied:
                proved = False
            assert proved == d.ok == (not want), what
            verdicts.append(proved)
        assert verdicts[0] and verdicts.count(False) >= 24
        gp.close()
    finally:
        configure(ctx, quotient_domain=4)


def test_a_diagnose_call_does_not_disturb_the_proofs_that_follow(ctx):
    import plonk_amd
    comp = C.big_widget_circuit(1 << 11, seed=88)()
    n = DC.size_of(comp)
    case = C.compile_fast(comp, b"calm")
    cc = C.circuit_columns(comp)
    load_srs(ctx, n)
    bl = C.blinders(5)
    for gp in (plonk_amd.Prover.compile(ctx, b"calm", cc["selectors"], cc["wires"], cc["witnesses"]),
               plonk_amd.Prover(ctx, case["constraints"], b"calm", case["polys"])):
        res = Resident(ctx, n)
        ptr = res.put(case["wires"])
        before = gp.prove_dev(ptr, case["pi"], bl)
        assert gp.diagnose_dev(ptr, case["pi"]).ok                       # first call: builds the caches
        assert gp.prove_dev(ptr, case["pi"], bl) == before
        bad = DR.columns(comp, n)
        bad[2][n // 3] = (bad[2][n // 3] + 1) % Q
        assert not gp.diagnose(col_bytes(bad), case["pi"]).ok            # through the prover's own wire buffer
        assert gp.prove_dev(ptr, case["pi"], bl) == before
        assert gp.prove_host_bytes(case["wires"], case["pi"], bl) == before
        assert gp.diagnose_dev(ptr, case["pi"]).ok
        res.free()
        gp.close()


def test_scale_2p20_gates(ctx):
    """big_widget_circuit(2^20): honest -> PLONK_OK; three forged cells (row 0, a middle row, the last live row) -> the rows
    the yardstick reports when it is evaluated on the forged rows and on every row whose rotation or sigma touches them."""
    import bench
    import plonk_amd
    log_n = 20
    n = 1 << log_n
    comp = C.big_widget_circuit(n, seed=2020)()
    assert len(comp.constraints) == n
    cc = C.circuit_columns(comp)
    pts = ctx.alloc(96 * (n + 7))
    ctx.srs_generate_dev(bench.TAU, bench.G_SCALAR, n + 7, pts.ptr)      # bench.py's commit key, generated on the device
    ctx.srs_load_dev(pts.ptr, n + 7)
    pts.free()
    gp = plonk_amd.Prover.compile(ctx, b"scale", cc["selectors"], cc["wires"], cc["witnesses"])
    pi = dict(comp.public_inputs)
    d = gp.diagnose_witnesses(cc["values"], pi)
    check(d, [], n)
    cols = DR.columns(comp, n)
    res = Resident(ctx, n)
    ptr = res.put(col_bytes(cols))
    check(gp.diagnose_dev(ptr, pi), [], n)
    cells = [(0, 0), (1, n // 2 + 3), (3, n - 1)]
    inverse = {}
    for uses in comp.witness_map.values():
        for k, cell in enumerate(uses):
            if cell in cells:
                inverse[cell] = uses[k - 1]                               # the cell sigma maps ONTO this one
    for col, row in cells:
        cols[col][row] = (cols[col][row] + 1) % Q
        res.buf.upload(C.fr_bytes([cols[col][row]]), 32 * (n * col + row))
    touched = DR.touched_rows(n, lambda c_, r_: inverse.get((c_, r_), (c_, r_)), cells)
    want = DR.report(comp, n, cols, pi=pi, rows=touched, sigma=comp.sigma_mappings(n))
    assert {r for r, _, _ in want} >= {0, n // 2 + 3, n - 1}
    d = gp.diagnose_dev(ptr, pi)
    assert not d.ok and d.rows == want
    assert d.info == DR.info(want, n)
    res.free()
    gp.close()


def test_error_surface(ctx):
    import plonk_amd
    comp = C.big_widget_circuit(200, seed=5)()
    case = C.compile_fast(comp, b"errors")
    n = case["size"]
    load_srs(ctx, n)
    cc = C.circuit_columns(comp)
    plain = plonk_amd.Prover(ctx, case["constraints"], b"errors", case["polys"])
    with pytest.raises(plonk_amd.PlonkError) as e:            # the witness form needs plonk_compile's wire -> witness table
        plain.diagnose_witnesses(cc["values"], case["pi"])
    assert e.value.code == -7
    info = plonk_amd._UnsatInfo()
    lib = ctx.lib
    assert lib.plonk_prover_diagnose(plain.handle, None, None, None, 0, None, 0, ctypes.byref(info)) == -1       # NULL wires
    assert lib.plonk_prover_diagnose_dev(plain.handle, None, None, None, 0, None, 0, ctypes.byref(info)) == -1
    three = (ctypes.c_void_p * 4)(1, 1, 1, None)                                                                 # one NULL column
    assert lib.plonk_prover_diagnose(plain.handle, three, None, None, 0, None, 0, ctypes.byref(info)) == -1
    res = Resident(ctx, n)
    ptr = res.put(case["wires"])
    assert lib.plonk_prover_diagnose_dev(plain.handle, ptr, None, None, 0, None, 5, None) == -1                  # cap without out
    assert lib.plonk_prover_diagnose_dev(plain.handle, ptr, None, None, 2, None, 0, None) == -1                  # inputs without arrays
    compiled = plonk_amd.Prover.compile(ctx, b"errors", cc["selectors"], cc["wires"], cc["witnesses"])
    with pytest.raises(plonk_amd.PlonkError) as e:            # wrong number of witness values
        compiled.diagnose_witnesses(cc["values"][:-32], case["pi"])
    assert e.value.code == -1
    with pytest.raises(plonk_amd.PlonkError) as e:            # a public input beyond the domain
        compiled.diagnose_witnesses(cc["values"], {n: 1})
    assert e.value.code == -1
    assert compiled.diagnose_witnesses(cc["values"], case["pi"]).ok
    assert plain.diagnose_dev(ptr, case["pi"]).ok
    res.free()
    plain.close()
    compiled.close()


def test_a_sharded_prover_refuses_to_diagnose():
    """The multi-rank harness of tests/test_gpu_multirank.py starts bench.py under torch.distributed.run: its child
    processes run bench.py's own main and cannot host another call without editing a file that stays as it is.  The guard
    is covered here instead: rank 0 of a world of 2 over the host-callback transport, in this process, its peer played by
    the callback (it answers with the rank's own contribution, which is all that prover creation compares)."""
    import plonk_amd
    ctx = plonk_amd.Context(0)
    try:
        comp = C.big_widget_circuit(256, 3)()
        case = C.compile_fast(comp, b"sharded")
        n = case["size"]
        total = n + 7
        lo, hi = plonk_amd.shard_range(total, 0, 2)
        srs = C.synthetic_srs(total)
        ctx.srs_load_bytes(srs[96 * lo:96 * hi], hi - lo)
        gp = plonk_amd.Prover(ctx, case["constraints"], b"sharded", case["polys"], vk_commitments=bytes(15 * 48), rank=0, world=2,
                              srs_total=total, allgather=lambda send: send * 2)
        assert gp.describe()["shard_world"] == 2
        with pytest.raises(plonk_amd.PlonkError) as e:
            gp.diagnose(case["wires"], case["pi"])
        assert e.value.code == -7 and "sharded" in str(e.value)
        res = Resident(ctx, n)
        with pytest.raises(plonk_amd.PlonkError) as e:
            gp.diagnose_dev(res.put(case["wires"]), case["pi"])
        assert e.value.code == -7
        res.free()
        gp.close()
    finally:
        ctx.close()
