"""Big-int model of the KZG10 cell recovery (plonk_amd/csrc/kzg_recover.hip, kzg_recover_core.hpp): the five steps with the
kernels' index arithmetic — the slot table, the 2r points of the vanish kernel, the scatter with its un-transpose and zero
fill, the period i mod r of the division, the range [max_len, n) of the tail — the argument checks in their order, the plan
of a call and the counts plonk_kzg_recover_last reports.  Values are integers mod q; a transform is a plain DFT over the
generator plonk_ntt uses (tests/kzg_domain_model.root), the coset is that of 7."""
from tests import kzg_cells_model as C
from tests import kzg_domain_model as D

Q = D.Q
GEN = 7
MAX_LOG_R = 11
POLY_ARRAYS = 3
MISSING = -1
VANISH_SLICES = 64
MAX_COUNT, MAX_CHUNK, WS_CAP_DEFAULT = D.MAX_COUNT, D.MAX_CHUNK, D.WS_CAP_DEFAULT
OK, ERR_ARG, ERR_DEGREE, ERR_STATE, ERR_DATA, ERR_VERIFY = 0, -1, -3, -7, -9, -12
root = D.root


# ---- index arithmetic ------------------------------------------------------------------------------------------------------
def slot_table(r: int, cell_ids):
    """slot[k] = the position of cell k among the given ones, MISSING otherwise"""
    slot = [MISSING] * r
    for i, k in enumerate(cell_ids):
        slot[k] = i
    return slot


def missing_list(slot):
    return [k for k, s in enumerate(slot) if s == MISSING]


def scatter_src(log_n: int, log_cell: int, i: int, slot):
    """the packed value position i = k + r j of the natural-order array reads (None: zero)"""
    log_r = log_n - log_cell
    s = slot[i & ((1 << log_r) - 1)]
    return None if s < 0 else (s << log_cell) + (i >> log_r)


def period(log_n: int, log_cell: int, i: int) -> int:
    return i & ((1 << (log_n - log_cell)) - 1)


def point_exp(log_r: int, p: int) -> int:
    return p & ((1 << log_r) - 1)


def point_on_coset(log_r: int, p: int) -> bool:
    return (p >> log_r) != 0


def tail_first(max_len: int) -> int:
    return max_len


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def vanish(log_n: int, log_cell: int, miss):
    """(Zdom, Zcoset): Z_r at phi^k and at 7^l phi^k, k < r: per point VANISH_SLICES partial products over every 64th entry
    of the missing list, multiplied pairwise as the kernel's LDS tree does"""
    log_r = log_n - log_cell
    r, phi, shift = 1 << log_r, root(log_r) if log_r else 1, pow(GEN, 1 << log_cell, Q)
    pw = [pow(phi, i, Q) for i in range(r)]
    out = ([0] * r, [0] * r)
    for p in range(2 * r):
        e, coset = point_exp(log_r, p), point_on_coset(log_r, p)
        pt = pw[e] * shift % Q if coset else pw[e]
        part = [1] * VANISH_SLICES
        for s in range(VANISH_SLICES):
            for m in miss[s::VANISH_SLICES]:
                part[s] = part[s] * (pt - pw[m]) % Q
        h = VANISH_SLICES // 2
        while h:
            for t in range(h):
                part[t] = part[t] * part[t + h] % Q
            h >>= 1
        out[1 if coset else 0][e] = part[0]
    return out


def scatter(values, slot, zdom, log_n: int, log_cell: int):
    """values: the a l packed values of one polynomial -> E Z in natural order"""
    out = []
    for i in range(1 << log_n):
        src = scatter_src(log_n, log_cell, i, slot)
        out.append(0 if src is None else values[src] * zdom[period(log_n, log_cell, i)] % Q)
    return out


def divide(v, zinv, log_n: int, log_cell: int):
    return [x * zinv[period(log_n, log_cell, i)] % Q for i, x in enumerate(v)]


def tail(coeffs, max_len: int) -> int:
    return 1 if any(coeffs[tail_first(max_len):]) else 0


# ---- transforms (definitions) ----------------------------------------------------------------------------------------------
def dft(v, w):
    """out[i] = sum_j v[j] w^(i j), w a primitive len(v)-th root of unity: the definition, over a table of its powers"""
    n = len(v)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % Q
    return [sum(x * pw[i * j % n] for j, x in enumerate(v)) % Q for i in range(n)]


def ntt(v, log_n: int):
    return dft(v, root(log_n))


def intt(v, log_n: int):
    n_inv = pow(len(v), -1, Q)
    return [x * n_inv % Q for x in dft(v, pow(root(log_n), -1, Q))]


def coset_ntt(v, log_n: int):
    return ntt([x * pow(GEN, i, Q) % Q for i, x in enumerate(v)], log_n)


def coset_intt(v, log_n: int):
    g_inv = pow(GEN, -1, Q)
    return [x * pow(g_inv, i, Q) % Q for i, x in enumerate(intt(v, log_n))]


# ---- the five steps --------------------------------------------------------------------------------------------------------
def recover(cell_ids, values, log_n: int, log_cell: int, max_len: int):
    """-> (the n coefficients, the tail flag: 1 = inconsistent) of one polynomial from its packed values"""
    r = 1 << (log_n - log_cell)
    slot = slot_table(r, cell_ids)
    zdom, zcoset = vanish(log_n, log_cell, missing_list(slot))
    assert all(zcoset), "Z vanishes on the coset of 7"
    zinv = [pow(z, -1, Q) for z in zcoset]
    p = intt(scatter(values, slot, zdom, log_n, log_cell), log_n)
    g = coset_intt(divide(coset_ntt(p, log_n), zinv, log_n, log_cell), log_n)
    return g, tail(g, max_len)


def cells_of(coeffs, log_n: int, log_cell: int):
    """cell-major values: the forward transform through kzc_transpose's map"""
    ev = ntt(list(coeffs) + [0] * ((1 << log_n) - len(coeffs)), log_n)
    out = [0] * (1 << log_n)
    for i, x in enumerate(ev):
        out[C.cell_dst(log_n, log_cell, i)] = x
    return out


def packed(cells, cell_ids, log_cell: int):
    """the caller's input: the cells cell_ids of a cell-major array, in that order"""
    l = 1 << log_cell
    return [x for k in cell_ids for x in cells[k * l:(k + 1) * l]]


# ---- checks and plan -------------------------------------------------------------------------------------------------------
def check_args(has_domain: bool, log_n: int, log_cell: int, count: int, cell_ids, available: int, has_values: bool, values_all_set: bool,
               max_len: int, any_output: bool) -> int:
    """plonk_kzg_recover_cells' PLONK_ERR_ARG conditions; cell_ids None = a NULL pointer"""
    if not has_domain or C.check_cell(log_n, log_cell) != OK:
        return ERR_ARG
    log_r = log_n - log_cell
    if log_r > MAX_LOG_R or count > MAX_COUNT:
        return ERR_ARG
    r = 1 << log_r
    if available == 0 or available > r:
        return ERR_ARG
    if cell_ids is not None:
        ids = list(cell_ids[:available])
        if any(k >= r for k in ids) or len(set(ids)) != len(ids):
            return ERR_ARG
    if count and (cell_ids is None or not has_values or not values_all_set):
        return ERR_ARG
    if max_len == 0 or max_len > (1 << log_n) or not any_output:
        return ERR_ARG
    return OK


def check_degree(log_cell: int, available: int, max_len: int) -> int:
    return ERR_DEGREE if max_len > (available << log_cell) else OK


def check_call(has_domain, log_n, log_cell, count, cell_ids, available, has_values, values_all_set, max_len, any_output, state_ok=True,
               canonical=True) -> int:
    """the documented order: ARG, STATE, count == 0, DEGREE, DATA (VERIFY comes from the data)"""
    rc = check_args(has_domain, log_n, log_cell, count, cell_ids, available, has_values, values_all_set, max_len, any_output)
    if rc != OK:
        return rc
    if not state_ok:
        return ERR_STATE
    if count == 0:
        return OK
    rc = check_degree(log_cell, available, max_len)
    if rc != OK:
        return rc
    return OK if canonical else ERR_DATA


def plan(log_n: int, log_cell: int, count: int, available: int, cap_bytes: int = WS_CAP_DEFAULT, want_values: bool = True) -> dict:
    n, r = 1 << log_n, 1 << (log_n - log_cell)
    per_poly = POLY_ARRAYS * n * 32
    chunk = min(max(cap_bytes // per_poly, 1), MAX_CHUNK, count)
    chunks = -(-count // chunk) if count else 0
    passes = 2 if chunks > 1 else 1
    return {"missing": r - available, "chunk_polys": chunk, "chunks": chunks, "ws_bytes": chunk * per_poly, "passes": passes,
            "transforms": count * (3 * passes + (1 if want_values else 0)), "vanish_muls": 2 * r * (r - available)}
