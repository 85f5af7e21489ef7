"""The degenerate corpus shared by tests/test_degenerate_host.py and tests/test_gpu_degenerate.py: circuits and witnesses at
the edges a random proof never reaches — domains of 2 and 4 rows, identically zero wire and quotient polynomials, zero
blinders, every wire value q - 1 on one permutation cycle through all wire slots, no copy constraint at all, a public input
(0 and q - 1 among them) on every row, no selector, the circuit of an empty Composer — each with the proof the C restatement
of the reference prover (oracle/c/oracle_prove.c) gives for it.

A case is raw columns, not a Composer: the constraint count, the per-gate selector values, the sigma mapping as the
(column, row) successor lists of oracle.plonk.Composer.sigma_mappings, four wire columns over the domain, sparse public
inputs, the expected outcome.  The key polynomials are interpolated with the C restatement of EvaluationDomain::ifft, as
tests/circuits.py compile_fast does.  Every proving case runs with 14 blinders drawn from a fixed seed and with 14 zeros."""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass

from oracle import bls12_381 as E
from oracle import cbind
from oracle import plonk as O
from tests import circuits as C

Q = E.Q
LABEL = b"degenerate"
TAU, G_SCALAR = 0x5EED0000 * 0x9E3779B97F4A7C15 % Q, 0xA5A5A5A5DEADBEEF      # tests/circuits.py synthetic_srs's defaults
SMALL_DOMAINS = (2, 4, 8, 16, 64)          # 2, 4: the n < 8 fallback to the 8n quotient domain; 8: first size on 4n; 16: below a
LARGE_DOMAIN = 4096                        # wavefront; 64: exactly one.  4096: scan and batch inversion over several workgroups
RAW_FAMILIES = ("zero-witness", "all-minus-one-one-cycle", "pi-every-row", "no-selectors", "unsat")
LARGE_FAMILIES = ("zero-witness", "all-minus-one-one-cycle", "unsat")
_blinder_rng = random.Random(0xB11D)
BLINDERS = {"random": [_blinder_rng.randrange(1, Q) for _ in range(14)], "zero": [0] * 14}
# commitments (of the proof's 11) that must be the identity under ZERO blinders, per family: the table of the issue that
# introduced the corpus (figures of the C oracle), restricted to where it applies; random blinders must leave none
IDENTITY_FLOOR = {"zero-witness": 9, "no-selectors": 4, "all-minus-one-one-cycle": 3, "empty-composer": 1, "pi-every-row": 3}


@dataclass
class Case:
    family: str
    n: int
    constraints: int
    selectors: dict                    # name -> [constraints] ints, the selectors that are not identically zero
    sigma: list                        # [4][n] (column, row): where the permutation sends the slot
    wires: list                        # [4][n] ints, zero past the last gate
    pi: dict                           # row -> value, zero values included
    expect: str                        # "proof" | "unsat"
    changed_row: int | None = None     # unsat: the one row whose arithmetic identity fails
    honest: "Case | None" = None       # unsat: the satisfied case of the same circuit
    composer: object = None            # empty-composer: the oracle Composer it came from

    @property
    def name(self) -> str:
        return f"{self.family}-n{self.n}-c{self.constraints}"

    @property
    def pi_idx(self):
        return sorted(self.pi)

    def identity_floor(self) -> int:
        """how many of the 11 proof commitments must at least be the identity with zero blinders"""
        if self.family == "all-minus-one-one-cycle" and self.constraints != self.n:
            return 0                   # padded rows: the wire polynomials are no longer constant, the quotient not low-degree
        return IDENTITY_FLOOR[self.family]


def identity_sigma(n):
    return [[(col, i) for i in range(n)] for col in range(4)]


def one_cycle_sigma(n, constraints):
    """one cycle through all 4 * constraints used slots in row-major order (a, b, c, d of row 0, then row 1, ...): what
    Composer.sigma_mappings gives when one witness sits on every wire of every gate; padded rows map to themselves"""
    sig = identity_sigma(n)
    slots = [(col, i) for i in range(constraints) for col in range(4)]
    for k, (col, i) in enumerate(slots):
        sig[col][i] = slots[(k + 1) % len(slots)]
    return sig


def pad(col, n):
    return list(col) + [0] * (n - len(col))


def raw_case(family: str, n: int, constraints: int) -> Case:
    c = constraints
    r = random.Random(f"{family}/{n}/{c}")
    zero = [[0] * n for _ in range(4)]
    if family in ("zero-witness", "unsat"):
        # q_m a b - c = 0, all wires zero
        r = random.Random(f"zero-witness/{n}/{c}")
        sel = {"q_m": [r.randrange(1, Q) for _ in range(c)], "q_o": [Q - 1] * c, "q_arith": [1] * c}
        case = Case("zero-witness", n, c, sel, identity_sigma(n), zero, {}, "proof")
        if family == "unsat":
            wires = [list(w) for w in zero]
            wires[2][c - 1] = 1
            case = Case("unsat", n, c, sel, identity_sigma(n), wires, {}, "unsat", changed_row=c - 1, honest=case)
        return case
    if family == "all-minus-one-one-cycle":
        # a + 1 = 0 with q - 1 on every wire of the used rows
        sel = {"q_l": [1] * c, "q_c": [1] * c, "q_arith": [1] * c}
        return Case(family, n, c, sel, one_cycle_sigma(n, c), [pad([Q - 1] * c, n) for _ in range(4)], {}, "proof")
    if family == "pi-every-row":
        # -a + PI = 0 (Composer::append_public): q - 1 on row 0, 0 on the last used row, random between
        vals = [Q - 1] + [r.randrange(1, Q) for _ in range(c - 2)] + [0]
        sel = {"q_l": [Q - 1] * c, "q_arith": [1] * c}
        return Case(family, n, c, sel, identity_sigma(n), [pad(vals, n), [0] * n, [0] * n, [0] * n],
                    dict(enumerate(vals)), "proof")
    if family == "no-selectors":
        return Case(family, n, c, {}, identity_sigma(n), [pad([r.randrange(Q) for _ in range(c)], n) for _ in range(4)], {}, "proof")
    raise ValueError(family)


def empty_composer_case() -> Case:
    """oracle.plonk.Composer() as constructed: two constant asserts and two dummy gates, n = 4"""
    comp = O.Composer()
    c = len(comp.constraints)
    assert c == 4
    sel = {}
    for name in O.SELECTORS:
        col = [getattr(g, name) % Q for g in comp.constraints]
        if any(col):
            sel[name] = col
    return Case("empty-composer", 4, c, sel, comp.sigma_mappings(4), C.wires_of(comp, 4), dict(comp.public_inputs), "proof",
                composer=comp)


def sizes():
    out = []
    for n in SMALL_DOMAINS:
        for c in (n, n // 2 + 1):
            if c >= 2 and (n, c) not in out:
                out.append((n, c))
    return out


@functools.lru_cache(maxsize=None)
def corpus() -> tuple:
    out = [raw_case(f, n, c) for f in RAW_FAMILIES for n, c in sizes()]
    out.append(empty_composer_case())
    out += [raw_case(f, LARGE_DOMAIN, c) for f in LARGE_FAMILIES for c in (LARGE_DOMAIN, LARGE_DOMAIN // 2 + 1)]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name: str) -> Case:
    return next(c for c in corpus() if c.name == name)


def small_names():
    return [c.name for c in corpus() if c.n < LARGE_DOMAIN]


def large_names():
    return [c.name for c in corpus() if c.n == LARGE_DOMAIN]


# ---- the byte forms both provers take ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def srs(n: int) -> bytes:
    return cbind.srs_generate(C.fr_bytes([TAU]), C.fr_bytes([G_SCALAR]), n + 7)


def sigma_values(case: Case):
    log_n = case.n.bit_length() - 1
    omega = pow(E.ROOT_OF_UNITY, 1 << (32 - log_n), Q)
    roots, cur = [], 1
    for _ in range(case.n):
        roots.append(cur)
        cur = cur * omega % Q
    ks = [1, E.K1, E.K2, E.K3]
    return [[ks[col] * roots[row] % Q for col, row in mapping] for mapping in case.sigma]


def polys(case: Case) -> dict:
    """the 15 key polynomials in coefficient form over the size-n domain (Montgomery bytes; identically zero ones empty)"""
    n, log_n = case.n, case.n.bit_length() - 1
    out = {name: b"" for name in O.SELECTORS}
    for name, col in case.selectors.items():
        out[name] = cbind.ntt_bytes(C.fr_bytes(pad(col, n)), log_n, True, False, n)
    for k, lag in enumerate(sigma_values(case)):
        out[C.SIGMA[k]] = cbind.ntt_bytes(C.fr_bytes(lag), log_n, True, False, n)
    return out


def wire_bytes(case: Case):
    return [C.fr_bytes(w) for w in case.wires]


def gates(case: Case):
    """the rows as oracle Gates (selector values only): what tests/diagnose_ref.py reads"""
    return [O.Gate(**{name: col[i] for name, col in case.selectors.items()}) for i in range(case.constraints)]


def witness_form(case: Case):
    """(wire indices [4][constraints], witness values): one witness per permutation cycle, numbered in the order their first
    slot appears gate by gate — the layout from which Compiler::preprocess arrives at the same sigma (sigma_from_indices)"""
    number, values = {}, []
    idx = [[0] * case.constraints for _ in range(4)]
    for i in range(case.constraints):
        for col in range(4):
            if (col, i) in number:
                continue
            w = len(values)
            values.append(case.wires[col][i])
            slot = (col, i)
            while slot not in number:
                number[slot] = w
                slot = case.sigma[slot[0]][slot[1]]
    for (col, i), w in number.items():
        assert i < case.constraints, "a cycle runs through a padded row"
        idx[col][i] = w
    return idx, values


def unsat_witness_form(case: Case):
    """the witness table of an unsat case over the wire indices of its honest circuit"""
    idx, values = witness_form(case.honest)
    values = list(values)
    for col in range(4):
        for i in range(case.constraints):
            values[idx[col][i]] = case.wires[col][i]
    return idx, values


def sigma_from_indices(idx, n):
    """Composer.sigma_mappings restated on wire indices (permutation.rs:106-139)"""
    uses = {}
    for i in range(len(idx[0])):
        for col in range(4):
            uses.setdefault(idx[col][i], []).append((col, i))
    sig = identity_sigma(n)
    for slots in uses.values():
        for k, (col, i) in enumerate(slots):
            sig[col][i] = slots[(k + 1) % len(slots)]
    return sig


def identity_commitments(proof: bytes) -> int:
    """how many of the proof's 11 commitments are the compressed identity (0xC0 then zeros)"""
    ident = bytes([0xC0]) + bytes(47)
    return sum(proof[48 * k:48 * k + 48] == ident for k in range(11))


@functools.lru_cache(maxsize=None)
def oracle(name: str) -> dict:
    """What the C restatement of the reference prover makes of a case, computed once per session: the 15 VerifierKey
    commitments and, per blinder set, the 1008 proof bytes — or "unsat" where it returns CircuitUnsatisfied."""
    case = by_name(name)
    cp = cbind.CProver(case.constraints, LABEL, polys(case), srs(case.n))
    try:
        out = {"vk": cp.vk(), "proofs": {}}
        idx = case.pi_idx
        pi_val = C.fr_bytes([case.pi[i] for i in idx])
        for kind, bl in BLINDERS.items():
            try:
                out["proofs"][kind] = cp.prove(wire_bytes(case), idx, pi_val, C.fr_bytes(bl))
            except cbind.CircuitUnsatisfied:
                out["proofs"][kind] = "unsat"
        return out
    finally:
        cp.close()
