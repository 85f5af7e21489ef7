"""GPU: circuits from gadgets (plonk_composer_*, plonk_compile_composer) and witness generation on the device
(plonk_prover_fill_inputs / _prove_inputs / _diagnose_inputs, plonk_amd/csrc/composer.hip) against the one-thread host
executor of the same gadget statements (tests/composer_cases.py: the CPU harness, itself held to the reference's layout
digests, the diagnosis yardstick and plain Python by tests/test_composer_host.py).

Circuits: A every gadget kind with a pipeline of whole-gadget lanes feeding later levels (2^14 gates); B a 3000-deep chain
of dependent gates (2^12: one walk of the narrow-level kernel, far more levels than a workgroup has lanes); C 5000
independent range checks and 5000 selections (2^16: wide levels over many workgroups, a record count that is no multiple of
64 or 256); D two rounds of the reference's bench circuit (2^13)."""
import pytest

from tests import circuits as C
from tests import composer_cases as CC
from tests import diagnose_ref as DR
from tests.kzg_ref import opening_key

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSAT, ERR_STATE, ERR_DATA = -1, -6, -7, -9


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    yield c
    c.close()


class Built:
    """one circuit recorded twice — through the library and through the CPU harness — and compiled; the host executor's
    table and public inputs are computed once"""

    def __init__(self, ctx, build, label):
        import plonk_amd
        self.host = build(CC.HostComposer())
        self.dev = build(plonk_amd.Composer())
        self.host_case = self.host[0] if isinstance(self.host, tuple) else self.host
        self.dev_case = self.dev[0] if isinstance(self.dev, tuple) else self.dev
        assert self.dev_case.inputs == self.host_case.inputs
        info = self.dev_case.c.info()
        assert info == self.host_case.c.info()
        self.info = info
        n = CC.domain_size(info["constraints"])
        srs = C.synthetic_srs(n + 7)
        ctx.srs_load_bytes(srs, len(srs) // 96)
        self.prover = plonk_amd.Prover.compile_composer(ctx, label, self.dev_case.c)
        self.n, self.label = n, label
        self.table, self.pi, err = self.host_case.c.fill(self.host_case.inputs)
        assert err is None
        self.inputs = self.host_case.inputs

    def pi_map(self, layout):
        return dict(zip(layout["pi_rows"], self.pi))


def check_fill(b):
    table, pi = b.prover.fill_inputs(b.inputs)
    assert pi == b.pi
    assert table == b.table
    assert b.prover.diagnose_inputs(b.inputs).ok


def check_proof(ctx, b, seed):
    import plonk_amd
    layout = b.dev_case.c.layout()
    assert layout == b.host_case.c.layout()
    bl = C.blinders(seed)
    proof, pi = b.prover.prove_inputs(b.inputs, bl)
    assert pi == b.pi and len(pi) == len(layout["pi_rows"])
    assert proof == b.prover.prove_witnesses(b.table, b.pi_map(layout), bl)
    v = plonk_amd.Verifier(ctx, b.prover.verifier_to_bytes(opening_key(), layout["pi_rows"]))
    assert v.verify(proof, pi)
    if any(pi):
        assert not v.verify(proof, [(x + 1) % CC.Q for x in pi])
    v.close()
    return proof, bl


def test_every_gadget_kind_fills_proves_and_verifies(ctx):
    b = Built(ctx, CC.circuit_a, b"composer-a")
    assert (1 << 13) < b.info["constraints"] <= (1 << 14) and b.info["levels"] >= 6
    check_fill(b)
    proof, bl = check_proof(ctx, b, 31)
    # a proof from the witness values before and after a fill is the same proof: the fill leaves the prover as it found it
    layout = b.dev_case.c.layout()
    before = b.prover.prove_witnesses(b.table, b.pi_map(layout), bl)
    b.prover.fill_inputs(b.inputs, want_witnesses=False)
    assert b.prover.prove_witnesses(b.table, b.pi_map(layout), bl) == before == proof
    b.prover.close()


def test_a_deep_chain_is_walked_by_one_workgroup(ctx):
    b = Built(ctx, CC.circuit_b, b"composer-b")
    assert b.info["levels"] > 3000 and b.info["widest_level"] <= 256 and b.info["constraints"] <= (1 << 12)
    check_fill(b)
    b.prover.close()


def test_wide_levels_span_many_workgroups(ctx):
    b = Built(ctx, CC.circuit_c, b"composer-c")
    assert (1 << 15) < b.info["constraints"] <= (1 << 16)
    assert b.info["widest_level"] > 256 and b.info["widest_level"] % 64 != 0
    check_fill(b)
    b.prover.close()


def test_bench_circuit_fills_proves_and_verifies(ctx):
    b = Built(ctx, CC.circuit_d, b"composer-d")
    assert (1 << 12) < b.info["constraints"] <= (1 << 13)
    check_fill(b)
    check_proof(ctx, b, 32)
    b.prover.close()


@pytest.mark.parametrize("build", [CC.rejected_range, CC.rejected_boolean], ids=["300 under range_bits<8>", "2 under boolean"])
def test_rejected_inputs_are_diagnosed_like_the_yardstick_and_not_proved(ctx, build):
    import plonk_amd
    b = Built(ctx, build, b"composer-rejected")
    table, pi = b.prover.fill_inputs(b.inputs)
    assert table == b.table and pi == b.pi
    comp = CC.as_oracle(b.host_case.c.layout(), plonk_amd.fr_from_bytes_mont(b.table), b.pi)
    want = DR.report(comp, b.n, DR.columns(comp, b.n))
    assert want and want[-1][0] == b.host[2]
    d = b.prover.diagnose_inputs(b.inputs, cap=b.n)
    assert not d.ok and d.rows == want
    with pytest.raises(plonk_amd.CircuitUnsatisfied):
        b.prover.prove_inputs(b.inputs, C.blinders(3))
    b.prover.close()


def test_a_malformed_jubjub_scalar_is_an_error_that_names_the_gadget(ctx):
    import plonk_amd

    def build(c):
        k = CC.Case(c)
        c.component_mul_generator(k.inp(5), CC.GEN)
        c.component_mul_generator(k.inp(9), CC.GEN)
        return k
    b = Built(ctx, build, b"composer-scalar")
    bl = C.blinders(7)
    good, _ = b.prover.prove_inputs(b.inputs, bl)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        b.prover.prove_inputs([5, CC.ORDER], bl)
    assert ei.value.code == ERR_DATA and "component_mul_generator" in str(ei.value)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        b.prover.fill_inputs([CC.ORDER, CC.Q - 1])
    assert ei.value.code == ERR_DATA and "component_mul_generator" in str(ei.value)
    assert b.prover.prove_inputs(b.inputs, bl)[0] == good
    b.prover.close()


def test_state_and_argument_errors(ctx):
    import plonk_amd
    b = Built(ctx, CC.rejected_boolean, b"composer-errors")
    with pytest.raises(plonk_amd.PlonkError) as ei:
        b.prover.fill_inputs(b.inputs + [1])
    assert ei.value.code == ERR_ARG
    with pytest.raises(plonk_amd.PlonkError) as ei:
        b.prover.prove_inputs([], C.blinders(1))
    assert ei.value.code == ERR_ARG
    # a prover without a witness program answers PLONK_ERR_STATE before any device work: the one plonk_prover_create builds
    # from coefficient forms (it has neither a witness table nor a wire -> witness map), and the one plonk_compile builds
    layout = b.dev_case.c.layout()
    comp = CC.as_oracle(layout, plonk_amd.fr_from_bytes_mont(b.table), b.pi)
    case = C.compile_fast(comp, b"composer-created")
    created = plonk_amd.Prover(ctx, case["constraints"], b"composer-created", case["polys"])
    plain = plonk_amd.Prover.compile(ctx, b"composer-plain", layout["selectors"], layout["wires"], layout["witnesses"])
    for other in (created, plain):
        other.composer_counts = b.prover.composer_counts
        for call in (lambda: other.fill_inputs(b.inputs), lambda: other.prove_inputs(b.inputs, C.blinders(1)),
                     lambda: other.diagnose_inputs(b.inputs)):
            with pytest.raises(plonk_amd.PlonkError) as ei:
                call()
            assert ei.value.code == ERR_STATE
    created.close()
    # the composer may be destroyed once the prover is compiled
    b.dev_case.c.close()
    assert b.prover.fill_inputs(b.inputs)[0] == b.table
    plain.close()
    b.prover.close()
