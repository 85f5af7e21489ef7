"""Big-int model of the KZG10 multiproofs (plonk_amd/csrc/kzg_multiproof.hip, kzg_multiproof_core.hpp): the two challenges over
oracle/merlin.py, g in evaluation form grouped by point index the way the kernels build it, the weights s_j and y, h, the
quotient at t, the proof and the verification equation in the exponent, the two counting sorts, the plan and the argument checks.

Notation: n = 2^log_n, w the size-n generator, vectors[j][i] = p_j(w^i), items = [(j_k, m_k)], y_k = vectors[j_k][m_k]."""
from oracle.merlin import Transcript
from tests import kzg_evals_model as EV

Q = EV.Q
OK, ERR_ARG, ERR_STATE, ERR_DATA, ERR_POINT, ERR_VERIFY = 0, -1, -7, -9, -10, -12
MAX_LOG_N = 20
MAX_ITEMS = 1 << 20
MAX_VECTORS = 65536
MAX_HOST_VALUES = 1 << 28
AGG_BLOCK = EV.FOLD_BLOCK          # values per workgroup of kmp_aggregate_kernel (kze_fold_kernel's shape)
GROUP_CHUNK = 64                   # point groups per launch of kmp_aggregate_kernel
domain_points = EV.domain_points


# ---- the checks -----------------------------------------------------------------------------------------------------------------
def check_items(log_n, nvectors, vector_index, point_index, host_form, check) -> int:
    count = len(vector_index)
    if check and not 1 <= log_n <= MAX_LOG_N:
        return ERR_ARG
    if count == 0 or count > MAX_ITEMS or nvectors == 0 or nvectors > MAX_VECTORS:
        return ERR_ARG
    n = 1 << log_n
    if any(j >= nvectors for j in vector_index) or any(m >= n for m in point_index):
        return ERR_ARG
    if host_form and nvectors * n > MAX_HOST_VALUES:
        return ERR_ARG
    return OK


def check_override(r_raw: int, t_raw: int, log_n: int) -> int:
    """r_raw, t_raw: the integers the override's limbs spell after leaving Montgomery form is undone, that is the plain
    residues when canonical; a value >= Q stands for a non-canonical encoding"""
    if r_raw >= Q or t_raw >= Q:
        return ERR_DATA
    return ERR_DATA if EV.in_domain(t_raw, log_n) else OK


# ---- the sorts -------------------------------------------------------------------------------------------------------------------
def counting_sort(keys, buckets):
    """(perm, off): the items by key, stable; off[b] .. off[b + 1] the items of key b"""
    perm = sorted(range(len(keys)), key=lambda k: keys[k])
    off = [0] * (buckets + 1)
    for x in keys:
        off[x + 1] += 1
    for b in range(buckets):
        off[b + 1] += off[b]
    return perm, off


def sort_points(point_index, n):
    """(perm, group_m, group_off): the point groups in ascending order of m"""
    perm, off = counting_sort(point_index, n)
    group_m = [m for m in range(n) if off[m + 1] != off[m]]
    return perm, group_m, [off[m] for m in group_m] + [len(point_index)]


def plan(log_n, M, K, groups, compute_commitments, host_form) -> dict:
    n = 1 << log_n
    blocks = (n + AGG_BLOCK - 1) // AGG_BLOCK
    waves = blocks * (EV.FOLD_T // 64)
    computed = M if compute_commitments else 0
    return {"point_groups": groups, "agg_launches": (groups + GROUP_CHUNK - 1) // GROUP_CHUNK, "agg_blocks": blocks, "waves": waves,
            "partial_values": min(groups, GROUP_CHUNK) * waves, "products": (K + 2 * groups) * n,
            "fold_launches": (M + EV.GROUP - 1) // EV.GROUP, "commitments_computed": computed, "msm_launches": computed + 2,
            "msm_terms": n, "stage_values": M * n if host_form else 0}


# ---- the challenges --------------------------------------------------------------------------------------------------------------
def transcript_r(label: bytes, log_n: int, commitments48, items, values):
    """(the transcript, ready for D; r)"""
    t = Transcript(label)
    t.append_message(b"dom-sep", b"kzg10-multiproof-v1")
    t.append_u64(b"log-n", log_n)
    t.append_u64(b"commitments", len(commitments48))
    t.append_u64(b"items", len(items))
    for c in commitments48:
        t.append_message(b"commitment", bytes(c))
    for (j, m), y in zip(items, values):
        t.append_u64(b"vector-index", j)
        t.append_u64(b"point-index", m)
        t.append_message(b"value", (y % Q).to_bytes(32, "little"))
    return t, t.challenge_scalar(b"multiproof-r")


def transcript_t(t: Transcript, d48: bytes) -> int:
    t.append_message(b"multiproof-d", bytes(d48))
    return t.challenge_scalar(b"multiproof-t")


# ---- the prover's arithmetic -----------------------------------------------------------------------------------------------------
def invd(log_n: int):
    """1 / (w^s - 1), s < n; 0 at s = 0"""
    return EV.batch_inverse([(x - 1) % Q for x in domain_points(log_n)])


def values_of(vectors, items):
    return [vectors[j][m] for j, m in items]


def group_constants(vectors, items, r, log_n):
    """per point group: (m, Y_m, w^(-m)) — what kmp_groups_kernel leaves for the aggregation"""
    pts = domain_points(log_n)
    n = 1 << log_n
    perm, group_m, group_off = sort_points([m for _, m in items], n)
    rp = powers(r, len(items))
    out = []
    for g, m in enumerate(group_m):
        ks = perm[group_off[g]:group_off[g + 1]]
        out.append((m, sum(rp[k] * vectors[items[k][0]][m] for k in ks) % Q, pts[(n - m) % n]))
    return out


def powers(r, count):
    out, x = [], 1
    for _ in range(count):
        out.append(x)
        x = x * r % Q
    return out


def aggregate(vectors, items, r, log_n):
    """g[i], i < n, built group by group with the derivative entry"""
    n = 1 << log_n
    pts = domain_points(log_n)
    inv = invd(log_n)
    perm, group_m, group_off = sort_points([m for _, m in items], n)
    rp = powers(r, len(items))
    g = [0] * n
    for gi, m in enumerate(group_m):
        ks = perm[group_off[gi]:group_off[gi + 1]]
        A = [sum(rp[k] * vectors[items[k][0]][i] for k in ks) % Q for i in range(n)]
        Y = A[m]
        winv = pts[(n - m) % n]
        q = [(A[i] - Y) * winv % Q * inv[(i - m) % n] % Q for i in range(n)]
        q[m] = -winv * sum(q[i] * pts[i] for i in range(n) if i != m) % Q
        for i in range(n):
            g[i] = (g[i] + q[i]) % Q
    return g


def weights(items, values, r, t, log_n, M):
    """(wt[k] = 1 / (t - w^(m_k)), s_j, y)"""
    pts = domain_points(log_n)
    wt = EV.batch_inverse([(t - pts[m]) % Q for _, m in items])
    rp = powers(r, len(items))
    s = [0] * M
    y = 0
    for k, (j, _) in enumerate(items):
        s[j] = (s[j] + rp[k] * wt[k]) % Q
        y = (y + rp[k] * wt[k] % Q * values[k]) % Q
    return wt, s, y


def fold(vectors, s):
    n = len(vectors[0])
    return [sum(sj * e[i] for sj, e in zip(s, vectors)) % Q for i in range(n)]


def quotient_at(hg, y, t, log_n):
    """((h - g)[i] - y) / (w^i - t)"""
    inv, m = EV.inverses(t, log_n)
    assert m == EV.NONE
    return [(x - y) * d % Q for x, d in zip(hg, inv)]


def prove_scalars(vectors, items, r, t, log_n):
    """everything the prover computes once r and t are fixed: dict with values, g, s, y, h, q"""
    M = len(vectors)
    values = values_of(vectors, items)
    g = aggregate(vectors, items, r, log_n)
    _, s, y = weights(items, values, r, t, log_n, M)
    h = fold(vectors, s)
    q = quotient_at([(a - b) % Q for a, b in zip(h, g)], y, t, log_n)
    return {"values": values, "g": g, "s": s, "y": y, "h": h, "q": q}


# ---- in the exponent, for a known tau --------------------------------------------------------------------------------------------
def at_tau(e, log_n, tau):
    return sum(a * b for a, b in zip(e, EV.lagrange_at(tau, log_n))) % Q


def check_exponent(commit_exp, items, values, d_exp, pi_exp, r, t, log_n, tau) -> bool:
    """the verification equation with every point replaced by its discrete logarithm to the base g:
    pi tau == sum_j s_j C_j - D - y + t pi"""
    _, s, y = weights(items, values, r, t, log_n, len(commit_exp))
    rhs = (sum(sj * c for sj, c in zip(s, commit_exp)) - d_exp - y + t * pi_exp) % Q
    return pi_exp * tau % Q == rhs


def prove_exponent(vectors, items, r, t, log_n, tau):
    """(values, commitment exponents, D exponent, pi exponent)"""
    p = prove_scalars(vectors, items, r, t, log_n)
    return p["values"], [at_tau(e, log_n, tau) for e in vectors], at_tau(p["g"], log_n, tau), at_tau(p["q"], log_n, tau)
