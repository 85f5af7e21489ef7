"""Inputs shared by tests/test_diagnose_host.py and tests/test_gpu_diagnose.py: the circuits, the single-witness mutations
and the single-cell forgeries of the witness-diagnosis tests, each paired with the yardstick's report
(tests/diagnose_ref.py)."""
from __future__ import annotations

import random

from oracle import bls12_381 as E
from tests import circuits as C
from tests import diagnose_ref as DR
from tests import widget_circuits as WC

Q = E.Q


def small_circuits():
    """(name, composer): every widget family on 2^8 rows with padding, and exactly 256 gates (no padding: the last row's
    rotation reads a live row)"""
    big = C.big_widget_circuit(256, 3)()
    assert len(big.constraints) == 256
    return [("semantic", WC.semantic_widget_circuit(1)()), ("big256", big)]


def size_of(comp):
    return C.next_pow2(len(comp.constraints))


def witness_mutations(comp):
    """every single-witness mutation: witness w takes value + 1"""
    for w in range(len(comp.witnesses)):
        vals = list(comp.witnesses)
        vals[w] = (vals[w] + 1) % Q
        yield w, vals


def cell_forgeries(comp, n, rnd, count):
    """single cells of the raw columns overwritten with value + 1: [(col, row)]"""
    live = len(comp.constraints)
    return [(rnd.randrange(4), rnd.randrange(live)) for _ in range(count)]


def sigma_values(comp, n):
    """the sigma evaluations K_col * omega^row of the circuit over its domain, [4][n] ints"""
    log_n = n.bit_length() - 1
    omega = pow(E.ROOT_OF_UNITY, 1 << (32 - log_n), Q)
    roots, cur = [], 1
    for _ in range(n):
        roots.append(cur)
        cur = cur * omega % Q
    ks = [1, E.K1, E.K2, E.K3]
    return [[ks[col] * roots[row] % Q for col, row in mapping] for mapping in comp.sigma_mappings(n)]


def selector_columns(comp, n):
    """{selector id: [n] ints} for the selectors that are not identically zero (ids in plonk_prover_desc.polys order)"""
    from oracle import plonk as O
    out = {}
    for k, name in enumerate(O.SELECTORS):
        col = [getattr(g, name) % Q for g in comp.constraints]
        if any(col):
            out[k] = col + [0] * (n - len(col))
    return out


def wraparound_case():
    comp = DR.wraparound_example(random.Random(64))
    cols = DR.columns(comp, 64)
    assert DR.report(comp, 64, cols) == []
    cols[3][0] = 5
    want = [(0, 0, 0b1100), (63, 1 << 4, 0)]
    assert DR.report(comp, 64, cols) == want
    return comp, cols, want
