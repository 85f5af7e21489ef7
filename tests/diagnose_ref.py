"""Plain-Python statement of the witness-diagnosis report (include/plonk_hip.h, "witness diagnosis"): the yardstick of
tests/test_diagnose_host.py and tests/test_gpu_diagnose.py.  Big ints, one row at a time, written from the semantics the
header states and from oracle/plonk.py's delta / delta_xor_and; nothing here calls the code under test.

Rows run over the whole domain of size n; row i's rotated values are those of row (i + 1) % n.  For every row the 17
identity values are computed in the reference debugger's order and each is tested for zero on its own; bit k of the copy
mask is set when the cell (k, i) differs from the cell Composer.sigma_mappings sends it to."""
from __future__ import annotations

from oracle import plonk as O
from oracle.bls12_381 import EDWARDS_D, Q

FAMILIES = 17
NONE = (1 << 64) - 1


def columns(composer, n, witnesses=None):
    """the four wire columns over the domain (zero past the last gate) from the composer's — or the given — witness values"""
    W = composer.witnesses if witnesses is None else witnesses
    cols = [[0] * n for _ in range(4)]
    for i, g in enumerate(composer.constraints):
        cols[0][i], cols[1][i], cols[2][i], cols[3][i] = W[g.a] % Q, W[g.b] % Q, W[g.c] % Q, W[g.d] % Q
    return cols


def identity_values(g, a, b, c, d, a_w, b_w, d_w, pi):
    """the 17 values of one row; g: the row's Gate (selector values), or None past the last gate"""
    if g is None:
        g = O.Gate()
    arithmetic = ((g.q_m * a * b + g.q_l * a + g.q_r * b + g.q_o * c + g.q_f * d + g.q_c) * g.q_arith + pi) % Q
    rng = [O.delta(c - 4 * d), O.delta(b - 4 * c), O.delta(a - 4 * b), O.delta(d_w - 4 * a)]
    la, lb, lo = (a_w - 4 * a) % Q, (b_w - 4 * b) % Q, (d_w - 4 * d) % Q
    logic = [O.delta(la), O.delta(lb), O.delta(lo), (c - la * lb) % Q, O.delta_xor_and(la, lb, c, lo, g.q_c)]
    bit = (d_w - d - d) % Q
    y_alpha = (bit * bit * (g.q_r - 1) + 1) % Q
    x_alpha = g.q_l * bit % Q
    cab = c * a * b * EDWARDS_D % Q
    fixed = [bit * (bit - 1) * (bit + 1) % Q, (bit * g.q_c - c) % Q,
             (a_w + a_w * cab - (a * y_alpha + b * x_alpha)) % Q,
             (b_w - b_w * cab - (b * y_alpha + a * x_alpha)) % Q]
    x1y2, y1x2 = d_w, b * c % Q
    dxy = EDWARDS_D * x1y2 * y1x2 % Q
    var = [(a * d - x1y2) % Q, (x1y2 + y1x2 - (a_w + a_w * dxy)) % Q, (b * d + a * c - (b_w - b_w * dxy)) % Q]
    return ([arithmetic] + [v * g.q_range % Q for v in rng] + [v * g.q_logic % Q for v in logic]
            + [v * g.q_fixed_group_add % Q for v in fixed] + [v * g.q_variable_group_add % Q for v in var])


def row_masks(composer, n, cols, pi, sigma, i):
    gates = composer.constraints
    g = gates[i] if i < len(gates) else None
    j = (i + 1) % n
    vals = identity_values(g, cols[0][i], cols[1][i], cols[2][i], cols[3][i], cols[0][j], cols[1][j], cols[3][j], pi.get(i, 0) % Q)
    assert len(vals) == FAMILIES
    fam = sum(1 << f for f, v in enumerate(vals) if v % Q)
    copy = 0
    for k in range(4):
        tc, tr = sigma[k][i]
        if cols[k][i] % Q != cols[tc][tr] % Q:
            copy |= 1 << k
    return fam, copy


def report(composer, n, cols, pi=None, rows=None, sigma=None):
    """[(row, families, copy_wires)] of the failing rows, ascending; rows: restrict the evaluation to these rows"""
    pi = composer.public_inputs if pi is None else pi
    sigma = composer.sigma_mappings(n) if sigma is None else sigma
    out = []
    for i in (range(n) if rows is None else sorted(set(rows))):
        fam, copy = row_masks(composer, n, cols, pi, sigma, i)
        if fam or copy:
            out.append((i, fam, copy))
    return out


def info(rep, n):
    """the plonk_unsat_info fields of a full report (everything but the timing)"""
    family_rows = [sum(1 for _, fam, _ in rep if (fam >> f) & 1) for f in range(FAMILIES)] + [sum(1 for _, _, cp in rep if cp)]
    first_row, first_family = NONE, 0
    if rep:
        first_row, fam, _ = rep[0]
        first_family = next((f for f in range(FAMILIES) if (fam >> f) & 1), FAMILIES)
    return dict(rows_checked=n, rows_failing=len(rep), family_rows=family_rows, first_row=first_row, first_family=first_family)


def touched_rows(n, sigma_inverse_of, cells):
    """rows whose masks a forgery of the raw cells [(col, row)] can change: the row itself, the row before it (its rotation
    reads the forged row) and the rows of the cells sigma maps ONTO the forged cell; sigma_inverse_of(col, row) -> (col, row)"""
    rows = set()
    for col, row in cells:
        rows |= {row, (row - 1) % n, sigma_inverse_of(col, row)[1]}
    return rows


def wraparound_example(rnd):
    """A fresh composer (4 gates of its own), four random witnesses, gate_mul rows with q_f = 1 (wire d live) up to 63
    gates, then a bare q_range gate as gate 64: n = 64 with no padding, so the last row's rotation reads row 0."""
    c = O.Composer()
    ws = [c.append_witness(rnd.randrange(Q)) for _ in range(4)]
    while len(c.constraints) < 63:
        ws.append(c.gate_mul(rnd.choice(ws), rnd.choice(ws), rnd.choice(ws), q_f=1))
    c.append_custom_gate(O.Gate(q_range=1))
    assert len(c.constraints) == 64
    return c
