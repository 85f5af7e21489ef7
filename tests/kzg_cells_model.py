"""Big-int model of the KZG10 cell proofs (plonk_amd/csrc/kzg_cells.hip, kzg_cells_core.hpp), IN THE EXPONENT like
tests/kzg_domain_model.py: a point [x] g is the integer x mod q, the commit key under the suite's known tau is s_i = tau^i.
The steps with the kernels' index arithmetic — the A^(u) tables, the gathered scalar vectors, the multiply-accumulate cut
into S slices with its reduction order, the inverse transform, the extraction and the size-r forward transform — the plan of
a call and the counts plonk_kzg_cells_last reports, and the closed forms the steps are pinned to."""
from tests import kzg_domain_model as D

Q = D.Q
FILL_LANES = 65536
MAX_COUNT, MAX_CHUNK, SLOT_BYTES, WS_CAP_DEFAULT = D.MAX_COUNT, D.MAX_CHUNK, D.SLOT_BYTES, D.WS_CAP_DEFAULT
OK, ERR_ARG = D.OK, D.ERR_ARG
root, rev = D.root, D.rev


def check_cell(log_n: int, log_cell: int) -> int:
    return OK if 1 <= log_cell <= log_n - 1 else ERR_ARG


def a_src(log_cell: int, r: int, u: int, v: int):
    """a^(u)_v = s[a_src] (None: the identity), v < 2r"""
    return u + (v << log_cell) if v <= r - 2 else None


def g_src(log_cell: int, r: int, u: int, t: int):
    """g^(u)_t = f[g_src] (None: 0), t < 2r"""
    v = D.g_src(r, t)
    return None if v is None else u + (v << log_cell)


def cell_dst(log_n: int, log_cell: int, i: int) -> int:
    """cells[cell_dst] = evaluations[i]: i = k + r j -> k l + j"""
    r = 1 << (log_n - log_cell)
    return ((i & (r - 1)) << log_cell) + (i >> (log_n - log_cell))


def slice_terms(log_cell: int, slices: int) -> int:
    return (1 << log_cell) // slices


def slice_first(log_cell: int, slices: int, s: int) -> int:
    return s * slice_terms(log_cell, slices)


def partial_slot(r: int, s: int, p: int) -> int:
    return s * 2 * r + p


def cell_points(log_n: int, log_cell: int):
    """(x, shift): x[k] = w^(l k), shift[k] = w^k, k < r"""
    w, r = root(log_n), 1 << (log_n - log_cell)
    return [pow(w, k << log_cell, Q) for k in range(r)], [pow(w, k, Q) for k in range(r)]


def evaluate(f, x):
    acc = 0
    for c in reversed(f):
        acc = (acc * x + c) % Q
    return acc


# ---- closed forms --------------------------------------------------------------------------------------------------------
def remainder_coeffs(f, log_n: int, log_cell: int, k: int):
    """c_j = sum_t f_(j + t l) x_k^t, j < l: f mod (X^l - x_k)"""
    n, l = 1 << log_n, 1 << log_cell
    f = [c % Q for c in f] + [0] * (n - len(f))
    x = pow(root(log_n), k << log_cell, Q)
    out = []
    for j in range(l):
        acc = 0
        for t in reversed(range(n // l)):
            acc = (acc * x + f[j + t * l]) % Q
        out.append(acc)
    return out


def remainder_from_cell(values, log_n: int, log_cell: int, k: int):
    """the same c_j from the cell's l values: w^(-k j) * (size-l inverse NTT of the values)_j"""
    l = 1 << log_cell
    wl_inv = pow(root(log_cell), -1, Q) if log_cell else 1
    l_inv, w_inv = pow(l, -1, Q), pow(root(log_n), -1, Q)
    out = []
    for j in range(l):
        acc = sum(values[i] * pow(wl_inv, i * j, Q) for i in range(l)) % Q
        out.append(acc * l_inv % Q * pow(w_inv, k * j, Q) % Q)
    return out


def cells_horner(f, log_n: int, log_cell: int):
    """cell-major values by Horner evaluation: cells[k l + j] = f(w^(k + r j))"""
    w, l, r = root(log_n), 1 << log_cell, 1 << (log_n - log_cell)
    return [evaluate(f, pow(w, k + r * j, Q)) for k in range(r) for j in range(l)]


def proof_closed_form(f, log_n: int, log_cell: int, k: int, tau: int) -> int:
    """(f(tau) - r_k(tau)) / (tau^l - x_k), to the base g"""
    l = 1 << log_cell
    x = pow(root(log_n), k << log_cell, Q)
    den = (pow(tau, l, Q) - x) % Q
    assert den, "tau^l equals x_k"
    return (evaluate(f, tau) - evaluate(remainder_coeffs(f, log_n, log_cell, k), tau)) * pow(den, -1, Q) % Q


def h_naive(f, log_n: int, log_cell: int, key):
    """H_m = sum_(j <= n-1-(m+1)l) f_(j+(m+1)l) s_j for m <= r-2, H_(r-1) = 0"""
    n, l = 1 << log_n, 1 << log_cell
    r = n // l
    f = [c % Q for c in f] + [0] * (n - len(f))
    return [sum(f[j + (m + 1) * l] * key[j] for j in range(n - (m + 1) * l)) % Q if m <= r - 2 else 0 for m in range(r)]


def proofs_naive(f, log_n: int, log_cell: int, key):
    """sum_m x_k^m H_m = DFT_r(H)"""
    return D.dft(h_naive(f, log_n, log_cell, key), root(log_n - log_cell))


# ---- the steps as the device runs them -----------------------------------------------------------------------------------
def tables(log_n: int, log_cell: int, key):
    """table[u * 2r + p] = DFT_2r(a^(u))_rev(p): the transform reads the handle's twiddle table of tw_log = log_n + 1"""
    l, r = 1 << log_cell, 1 << (log_n - log_cell)
    LR = log_n - log_cell + 1
    tw = D.twiddle_table(log_n + 1)
    out = []
    for u in range(l):
        a = [key[a_src(log_cell, r, u, v)] if a_src(log_cell, r, u, v) is not None else 0 for v in range(2 * r)]
        out += D.forward(a, LR, tw, log_n + 1)
    return out


def gathered(f, log_n: int, log_cell: int):
    """g[u * 2r + t], 2n values"""
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    f = [c % Q for c in f] + [0] * (n - len(f))
    return [f[g_src(log_cell, r, u, t)] if g_src(log_cell, r, u, t) is not None else 0 for u in range(l) for t in range(2 * r)]


def mulacc(table, G, log_n: int, log_cell: int, slices: int, scale: int, counts=None):
    """the workspace of one polynomial after the accumulate: slices * 2r partials, partial (s, p) at partial_slot"""
    r = 1 << (log_n - log_cell)
    size, LR = 2 * r, log_n - log_cell + 1
    terms = slice_terms(log_cell, slices)
    ws = [0] * (slices * size)
    for s in range(slices):
        first = slice_first(log_cell, slices, s)
        for p in range(size):
            i = rev(p, LR)
            acc = 0
            for k in range(terms):
                u = first + k
                acc = (acc + G[u * size + i] * scale % Q * table[u * size + p]) % Q
            ws[partial_slot(r, s, p)] = acc
    if counts is not None:
        counts[1] += 2 << log_n
    return ws


def reduce(ws, r: int, slices: int):
    """ws[p] += ws[s * 2r + p], s = 1 .. slices - 1 in that order"""
    ws = list(ws)
    for p in range(2 * r):
        acc = ws[p]
        for s in range(1, slices):
            acc = (acc + ws[partial_slot(r, s, p)]) % Q
        ws[p] = acc
    return ws


def steps(f, log_n: int, log_cell: int, key, slices: int = 1, counts=None, table=None):
    """(cell-major values, proof scalars) as the device computes them; counts: [stage launches, scalar multiplications];
    table: tables(log_n, log_cell, key) when the caller keeps it"""
    n, r = 1 << log_n, 1 << (log_n - log_cell)
    log_r = log_n - log_cell
    size, LR = 2 * r, log_r + 1
    f = [c % Q for c in f] + [0] * (n - len(f))
    assert len(f) == n
    tw = D.twiddle_table(log_n + 1)
    if table is None:
        table = tables(log_n, log_cell, key)                               # per (handle, cell size): not counted
    g = gathered(f, log_n, log_cell)
    G = []
    for u in range(1 << log_cell):
        G += D.dft(g[u * size:(u + 1) * size], root(LR))                   # the scalar NTT: natural order
    ws = reduce(mulacc(table, G, log_n, log_cell, slices, pow(size, -1, Q), counts), r, slices)
    c = D.inverse(ws[:size], LR, tw, log_n + 1, counts)
    upper = [c[D.h_src(r, k)] if D.h_src(r, k) is not None else 0 for k in range(r)]
    up = D.forward(upper, log_r, tw, log_n + 1, counts)
    proofs = [up[rev(k, log_r)] for k in range(r)]
    ev = D.dft(f, root(log_n))
    cells = [0] * n
    for i in range(n):
        cells[cell_dst(log_n, log_cell, i)] = ev[i]
    return cells, proofs


def choose_slices(log_n: int, log_cell: int, count: int) -> int:
    l, r = 1 << log_cell, 1 << (log_n - log_cell)
    polys = max(min(count, MAX_CHUNK), 1)
    S = 1
    while S < l and 2 * r * S * polys < FILL_LANES:
        S <<= 1
    return S


def plan(log_n: int, log_cell: int, count: int, cap_bytes: int = WS_CAP_DEFAULT, forced_slices: int = 0) -> dict:
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    log_r = log_n - log_cell
    S = choose_slices(log_n, log_cell, count)
    if forced_slices and forced_slices <= l and forced_slices & (forced_slices - 1) == 0:
        S = forced_slices
    per_poly = S * 2 * r * SLOT_BYTES
    chunk = min(max(cap_bytes // per_poly, 1), MAX_CHUNK, count)
    chunks = -(-count // chunk) if count else 0
    return {"slices": S, "chunk_polys": chunk, "chunks": chunks, "ws_bytes": chunk * per_poly, "table_bytes": 2 * n * SLOT_BYTES,
            "stage_launches": chunks * (2 * log_r + 1),
            "scalar_muls": count * (2 * n + D.transform_muls(log_r + 1) + D.transform_muls(log_r))}
