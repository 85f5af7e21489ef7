"""Big-int model of the KZG10 cell verifier (plonk_amd/csrc/kzg_cell_verify.hip, kzg_cell_verify_core.hpp), IN THE EXPONENT
like tests/kzg_cells_model.py: a point [x] g is the integer x mod q, the commit key under the suite's known tau is
s_j = tau^j, a commitment is f(tau), a proof its closed form.  The steps with the kernels' index arithmetic — the twist (the
bit-reversed load, the inverse decimation in time, the power of w^(-k) from shared squarings), the column sums by passes of 64
rows, the weights with the counting sort — both equations, the challenge over oracle/merlin.py, the argument checks, the
layouts and the plan plonk_kzg_cell_verifier_last reports."""
from oracle.merlin import Transcript
from tests import kzg_cells_model as C
from tests import kzg_domain_model as D

Q = D.Q
OK, ERR_ARG = D.OK, D.ERR_ARG
root, rev = D.root, D.rev
MAX_LOG_N, NTT_MAX_LOG = 20, 11
MAX_ITEMS, MAX_VALUES, MAX_COMMITMENTS = 1 << 20, 1 << 25, 65536
LANES, PACK_MAX_LOG, COLSUM_ROWS = 256, 6, 64
MIN_BUCKET_TERMS = 64          # plonk_msm_points' own rule (msm_points_core.hpp)


# ---- what the host decides ---------------------------------------------------------------------------------------------------
def check_shape(log_n: int, log_cell: int) -> int:
    return OK if 2 <= log_n <= MAX_LOG_N and 1 <= log_cell <= min(log_n - 1, NTT_MAX_LOG) else ERR_ARG


def check_items(log_n: int, log_cell: int, M: int, cidx, kidx) -> int:
    K, r = len(cidx), 1 << (log_n - log_cell)
    if K > MAX_ITEMS or (K << log_cell) > MAX_VALUES or M > MAX_COMMITMENTS:
        return ERR_ARG
    return ERR_ARG if any(c >= M for c in cidx) or any(k >= r for k in kidx) else OK


def items_per_group(log_cell: int) -> int:
    return LANES >> log_cell if log_cell <= PACK_MAX_LOG else 1


def lanes_per_item(log_cell: int) -> int:
    return 1 << log_cell if log_cell <= PACK_MAX_LOG else LANES


def twist_groups(log_cell: int, K: int) -> int:
    return -(-K // items_per_group(log_cell))


def twist_lds_bytes(log_cell: int) -> int:
    return items_per_group(log_cell) * (32 << log_cell)


def colsum_slices(rows: int) -> int:
    return -(-rows // COLSUM_ROWS)


def colsum_passes(rows: int) -> int:
    p = 1
    while rows > COLSUM_ROWS:
        rows = colsum_slices(rows)
        p += 1
    return p


def layout(log_cell: int, M: int, K: int) -> dict:
    l = 1 << log_cell
    return {"pt_commitment": l, "pt_proof": l + M, "points": l + M + K, "term_w": K, "term_x": K + M, "term_r": 2 * K + M,
            "terms": 2 * K + M + l}


def counting_sort(cidx, M: int):
    """(perm, off): the items ordered by commitment index, stable; off[c] .. off[c + 1] the items of commitment c"""
    off = [0] * (M + 1)
    for c in cidx:
        off[c + 1] += 1
    for c in range(M):
        off[c + 1] += off[c]
    cur, perm = list(off), [0] * len(cidx)
    for i, c in enumerate(cidx):
        perm[cur[c]] = i
        cur[c] += 1
    return perm, off


def plan(log_cell: int, M: int, K: int, each: bool, min_left: int = 0, min_right: int = 0) -> dict:
    l = 1 << log_cell
    left, right = (0, 0) if each else (K, M + K + l)
    return {"transforms": K, "twist_groups": twist_groups(log_cell, K), "colsum_passes": 0 if each else colsum_passes(K),
            "msm_terms_left": left, "msm_terms_right": right,
            "msm_path_left": 0 if each else int(left >= (min_left or MIN_BUCKET_TERMS)),
            "msm_path_right": 0 if each else int(right >= (min_right or MIN_BUCKET_TERMS)),
            "scalar_muls": K * (l + 1) if each else 0, "msm_terms_info": 2 * K + M + l}


def challenge(label: bytes, log_n: int, log_cell: int, opening_key240: bytes, commitments48, items) -> int:
    """items: (commitment index, cell index, values, proof48)"""
    t = Transcript(label)
    t.append_message(b"dom-sep", b"kzg10-cell-batch-check-v1")
    t.append_u64(b"log-n", log_n)
    t.append_u64(b"log-cell", log_cell)
    t.append_u64(b"commitments", len(commitments48))
    t.append_u64(b"items", len(items))
    t.append_message(b"opening-key", bytes(opening_key240))
    for c in commitments48:
        t.append_message(b"commitment", bytes(c))
    for ci, k, values, proof in items:
        t.append_u64(b"commitment-index", ci)
        t.append_u64(b"cell-index", k)
        t.append_message(b"cell", b"".join((v % Q).to_bytes(32, "little") for v in values))
        t.append_message(b"cell-proof", bytes(proof))
    return t.challenge_scalar(b"cell-batch-challenge")


# ---- the device steps --------------------------------------------------------------------------------------------------------
def handle_tables(log_n: int, log_cell: int):
    """(x_k, w^(-k)) for k < r and the l / 2 inverse twiddles"""
    r, l = 1 << (log_n - log_cell), 1 << log_cell
    w_inv, wl_inv = pow(root(log_n), -1, Q), pow(root(log_cell), -1, Q)
    x = [pow(root(log_n - log_cell), k, Q) for k in range(r)]
    return x, [pow(w_inv, k, Q) for k in range(r)], [pow(wl_inv, e, Q) for e in range(l // 2)]


def twist(values, log_n: int, log_cell: int, k: int, weight: int = 1):
    """row i of kzv_twist_kernel: l^-1 * weight * (w^(-k))^j * (inverse DIT of the values)_j"""
    l = 1 << log_cell
    _, winv, itw = handle_tables(log_n, log_cell)
    sq, b = [], winv[k]
    for _ in range(log_cell):                     # the squarings the item's lanes share
        sq.append(b)
        b = b * b % Q
    sh = [0] * l
    for j in range(l):
        sh[rev(j, log_cell)] = values[j] % Q
    for s in range(log_cell):
        half = 1 << s
        for e in range(l // 2):
            j = e & (half - 1)
            lo = ((e - j) << 1) + j
            hi = lo + half
            bb = sh[hi] * itw[j << (log_cell - 1 - s)] % Q
            a = sh[lo]
            sh[lo], sh[hi] = (a + bb) % Q, (a - bb) % Q
    scale = pow(l, -1, Q) * weight % Q
    out = []
    for j in range(l):
        p = scale
        for s in range(log_cell):
            if (j >> s) & 1:
                p = p * sq[s] % Q
        out.append(sh[j] * p % Q)
    return out


def colsum(rows, l: int):
    """R_j by the passes of kzv_colsum_kernel: slices of 64 rows until one row is left"""
    rows = [list(r) for r in rows]
    while len(rows) > COLSUM_ROWS:
        rows = [[sum(r[j] for r in rows[s * COLSUM_ROWS:(s + 1) * COLSUM_ROWS]) % Q for j in range(l)]
                for s in range(colsum_slices(len(rows)))]
    return [sum(r[j] for r in rows) % Q for j in range(l)]


def weights(rho: int, cidx, kidx, M: int, log_n: int, log_cell: int):
    """(rho^i, W_c, rho^i x_(k_i)): W_c over the segments of the counting sort"""
    x, _, _ = handle_tables(log_n, log_cell)
    pw = [pow(rho, i, Q) for i in range(len(cidx))]
    perm, off = counting_sort(cidx, M)
    W = [sum(pw[perm[t]] for t in range(off[c], off[c + 1])) % Q for c in range(M)]
    return pw, W, [pw[i] * x[k] % Q for i, k in enumerate(kidx)]


def folded_terms(commitments, items, rho: int, log_n: int, log_cell: int):
    """the scalars of the 2K + M + l terms in the order of `layout`, and the point each names (an index into the table
    [s | C | pi]); items: (commitment index, cell index, values, proof) with values as integers"""
    l, M, K = 1 << log_cell, len(commitments), len(items)
    cidx, kidx = [it[0] for it in items], [it[1] for it in items]
    pw, W, px = weights(rho, cidx, kidx, M, log_n, log_cell)
    R = colsum([twist(it[2], log_n, log_cell, it[1], pw[i]) for i, it in enumerate(items)], l)
    sc = pw + W + px + [(-x) % Q for x in R]
    ids = [l + M + i for i in range(K)] + [l + c for c in range(M)] + [l + M + i for i in range(K)] + list(range(l))
    return sc, ids


def folded_accepts(commitments, items, rho: int, log_n: int, log_cell: int, tau: int) -> bool:
    """commitments and proofs as exponents: e(L, [tau^l] h) == e(Rhs, h)"""
    l, K = 1 << log_cell, len(items)
    table = [pow(tau, j, Q) for j in range(l)] + [c % Q for c in commitments] + [it[3] % Q for it in items]
    sc, ids = folded_terms(commitments, items, rho, log_n, log_cell)
    left = sum(s * table[p] for s, p in zip(sc[:K], ids[:K])) % Q
    right = sum(s * table[p] for s, p in zip(sc[K:], ids[K:])) % Q
    return left * pow(tau, l, Q) % Q == right


def each_pair(commitment: int, k: int, values, proof: int, log_n: int, log_cell: int, tau: int):
    """(A, B) of one item in the exponent: A = pi, B = C + x_k pi - sum_j c_j s_j"""
    x, _, _ = handle_tables(log_n, log_cell)
    c = twist(values, log_n, log_cell, k)
    return proof % Q, (commitment + x[k] * proof - sum(cj * pow(tau, j, Q) for j, cj in enumerate(c))) % Q


def each_accepts(commitment: int, k: int, values, proof: int, log_n: int, log_cell: int, tau: int) -> bool:
    a, b = each_pair(commitment, k, values, proof, log_n, log_cell, tau)
    return a * pow(tau, 1 << log_cell, Q) % Q == b


def naive_accepts(commitment: int, k: int, values, proof: int, log_n: int, log_cell: int, tau: int) -> bool:
    """the equation straight from the definitions: pi (tau^l - x_k) == C - r_k(tau), r_k by remainder_from_cell"""
    l = 1 << log_cell
    xk = pow(root(log_n), k << log_cell, Q)
    rk = C.evaluate(C.remainder_from_cell(values, log_n, log_cell, k), tau)
    return proof * (pow(tau, l, Q) - xk) % Q == (commitment - rk) % Q
