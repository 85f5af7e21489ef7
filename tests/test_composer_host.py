"""CPU: the gadget composer's recorder and one-thread host executor (plonk_amd/csrc/composer_core.hpp + composer_host.hpp,
compiled with g++ through tests/csrc/host_composer.cpp) against the reference's own layout digests
(tests/golden/composer_layouts.json), the diagnosis yardstick tests/diagnose_ref.py and plain Python."""
import pytest

import plonk_amd
from tests import composer_cases as CC
from tests import diagnose_ref as DR

Q = CC.Q


def filled(case):
    table, pi, err = case.c.fill(case.inputs)
    assert err is None
    return plonk_amd.fr_from_bytes_mont(table), pi


@pytest.fixture(scope="module")
def circuit_a():
    case = CC.circuit_a(CC.HostComposer())
    return case, filled(case)


@pytest.mark.parametrize("entry", CC.GOLDEN["layouts"], ids=lambda e: e["name"])
def test_layouts_give_the_reference_digests(entry):
    c = CC.HostComposer()
    ins = []
    for what in entry["append"]:
        ins += [c.append_witness()] if what == "witness" else list(c.append_point())
    if entry.get("second_input") == "ZERO":
        ins.append(c.ZERO)
    consts = list(CC.GEN) if entry["gadget"] == "MUL_GENERATOR" else []
    nout = {"RANGE": 0, "TORSION_FREE": 0, "LOGIC_XOR": 1, "LOGIC_AND": 1}.get(entry["gadget"], 2)
    c.gadget(entry["gadget"], ins, width=entry["width"], consts=consts, nout=nout)
    info = c.info()
    assert info["constraints"] == entry["gates"]
    if entry["witnesses"] is not None:
        assert info["witnesses"] == entry["witnesses"]
    assert CC.layout_digest(c.layout()) == entry["digest"], entry["ref"]


def test_every_gadget_row_is_satisfied_by_the_host_executor(circuit_a):
    case, (table, pi) = circuit_a
    layout = case.c.layout()
    assert (1 << 13) < len(layout["wires"][0]) <= (1 << 14)
    comp = CC.as_oracle(layout, table, pi)
    n = CC.domain_size(len(comp.constraints))
    assert DR.report(comp, n, DR.columns(comp, n)) == []
    # the selectors of every widget family occur, and there are public rows with non-zero values
    sel = {name: plonk_amd.fr_from_bytes_mont(raw) for name, raw in layout["selectors"].items()}
    for name in ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add"):
        assert any(sel[name]), name
    assert len(pi) == len(layout["pi_rows"]) >= 6 and sum(1 for v in pi if v) >= 5


def test_outputs_mean_what_plain_python_says(circuit_a):
    case, (table, _) = circuit_a
    assert len(case.expect) > 300
    for w, v, what in case.expect:
        assert table[w] == v, what


def test_bench_circuit_rows_are_satisfied_and_mean_the_right_thing():
    case = CC.circuit_d(CC.HostComposer())
    table, pi = filled(case)
    layout = case.c.layout()
    assert (1 << 12) < len(layout["wires"][0]) <= (1 << 13)
    comp = CC.as_oracle(layout, table, pi)
    n = CC.domain_size(len(comp.constraints))
    assert DR.report(comp, n, DR.columns(comp, n)) == []
    for w, v, what in case.expect:
        assert table[w] == v, what


@pytest.mark.parametrize("build", [CC.rejected_range, CC.rejected_boolean], ids=["300 under range_bits<8>", "2 under boolean"])
def test_rejected_values_fail_at_the_gadgets_closing_row(build):
    case, first, closing = build(CC.HostComposer())
    table, pi = filled(case)
    comp = CC.as_oracle(case.c.layout(), table, pi)
    n = CC.domain_size(len(comp.constraints))
    rep = DR.report(comp, n, DR.columns(comp, n))
    assert [(row, fam, cp) for row, fam, cp in rep if row == closing] == [(closing, 1, 0)]
    assert all(row >= first for row, _, _ in rep)


def test_malformed_jubjub_scalar_is_reported_by_record():
    c = CC.HostComposer()
    k = CC.Case(c)
    good, bad = k.inp(5), k.inp(CC.ORDER)
    c.component_mul_generator(good, CC.GEN)
    before = c.info()["records"]
    c.component_mul_generator(bad, CC.GEN)
    _, _, err = c.fill(k.inputs)
    assert err == before


def test_constant_points_are_validated_like_the_reference():
    c = CC.HostComposer()
    s = c.append_witness()
    order8 = None
    for y in range(2, 200):          # a point with a torsion component: on the curve, not killed by the subgroup order
        from tests.widget_circuits import EDWARDS_D, fr_sqrt
        x = fr_sqrt((y * y - 1) * pow(EDWARDS_D * y * y + 1, -1, Q))
        if x and CC.jj_mul((x, y), CC.ORDER) != CC.IDENTITY:
            order8 = (x, y)
            break
    assert order8 is not None
    for bad in ((1, 1), order8):
        with pytest.raises(plonk_amd.PointMalformed):
            c.append_constant_point(bad)
        with pytest.raises(plonk_amd.PointMalformed):
            c.component_mul_generator(s, bad)
    with pytest.raises(plonk_amd.PointMalformed):
        c.component_mul_generator(s, CC.IDENTITY)          # torsion-free but not of prime order
    c.append_constant_point(CC.IDENTITY)
    with pytest.raises(plonk_amd.PlonkError):
        c.component_boolean(10 ** 6)                         # not an allocated witness
    with pytest.raises(plonk_amd.PlonkError):
        c.component_truncate(s, 255)


def check_schedule(c):
    records, off = c.program()
    level_of = {}
    for r in records:
        for w in range(r["out0"], r["out0"] + r["nout"]):
            level_of[w] = r["level"]
    for r in records:
        ins = [r["in0"], r["in1"], r["in2"], r["in3"]]
        for w in ins:
            assert level_of.get(w, 0) < r["level"] or r["kind"] == 0, r
    for l in range(len(off) - 1):
        seg = records[off[l]:off[l + 1]]
        assert all(r["level"] == l for r in seg)
        kinds = [r["kind"] for r in seg]
        assert kinds == sorted(kinds)
    assert off[-1] == len(records) and sorted(r["id"] for r in records) == list(range(len(records)))
    return records, off


def test_schedule_orders_records_by_level_then_kind(circuit_a):
    case, _ = circuit_a
    records, off = check_schedule(case.c)
    info = case.c.info()
    assert info["records"] == len(records) and info["levels"] == len(off) - 1
    assert info["widest_level"] == max(off[i + 1] - off[i] for i in range(len(off) - 1))
    assert info["levels"] >= 6          # the pipeline: mul_generator, add_point, select_point, decomposition, logic


def test_a_dependent_chain_is_one_record_per_level():
    case = CC.circuit_b(CC.HostComposer())
    records, off = check_schedule(case.c)
    widths = [off[i + 1] - off[i] for i in range(len(off) - 1)]
    assert sum(1 for w in widths if w == 1) >= 3000
    table, _ = filled(case)
    for w, v, what in case.expect:
        assert table[w] == v, what
