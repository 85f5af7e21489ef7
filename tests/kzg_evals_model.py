"""Big-int model of the scalar stage of KZG10 in evaluation form (plonk_amd/csrc/kzg_evals.hip, kzg_evals_core.hpp): the
shared inverses, the lane m, every y_j, F, Y and the quotient values q, with the formulas the kernels use.  Pinned to the
oracle's ifft + Ruffini division by tests/test_kzg_evals_model_host.py; the GPU tests compare the kernels with it."""
import functools

from oracle import bls12_381 as E
from tests import kzg_domain_model as D

Q = E.Q
NONE = (1 << 64) - 1
MAX_COUNT = 65536
GROUP = 64                      # vectors per launch of the fold kernel
FOLD_T, FOLD_E = 256, 4         # lanes per workgroup, values per lane
FOLD_BLOCK = FOLD_T * FOLD_E    # values per workgroup of the fold kernel
Q_T = 256                       # values per workgroup of the quotient kernel
STAGE_MIN = 1 << 16
POINT_BYTES = 96
ERR_ARG = -1

root = D.root


@functools.lru_cache(maxsize=None)
def _points(log_n: int):
    return tuple(D.domain_points(log_n))


def domain_points(log_n: int):
    """w^i, i < n (computed once per size)"""
    return list(_points(log_n))


def batch_inverse(xs):
    """1 / x for every x, zeros left alone (one modular inversion)"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        if x:
            acc = acc * x % Q
    inv = pow(acc, -1, Q)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        if xs[i]:
            out[i] = inv * pre[i] % Q
            inv = inv * xs[i] % Q
    return out


def in_domain(z: int, log_n: int) -> bool:
    return pow(z, 1 << log_n, Q) == 1


def eval_scale(z: int, log_n: int) -> int:
    """the factor of sum_i e[i] (1 + z d_i): (1 - z^n) / n outside the domain, 1 inside"""
    n = 1 << log_n
    t = pow(z, n, Q)
    return 1 if t == 1 else (1 - t) * pow(n, -1, Q) % Q


def inverses(z: int, log_n: int):
    """(d, m): d[i] = 1 / (w^i - z), 0 at the lane m with w^m == z (NONE when there is none)"""
    pts = domain_points(log_n)
    den = [(x - z) % Q for x in pts]
    m = den.index(0) if 0 in den else NONE
    return batch_inverse(den), m


def scalar_stage(vectors, z: int, v: int, log_n: int) -> dict:
    """everything the kernels compute for one call: inv, m, y (per vector), F, Y, q"""
    n = 1 << log_n
    assert all(len(e) == n for e in vectors)
    pts = domain_points(log_n)
    inv, m = inverses(z, log_n)
    if m == NONE:
        weights = [(1 + z * d) % Q for d in inv]          # w^i / (w^i - z)
    else:
        weights = [1 if i == m else 0 for i in range(n)]
    scale = eval_scale(z, log_n)
    y = [scale * sum(e[i] * weights[i] for i in range(n)) % Q for e in vectors]
    F, Y, vp = [0] * n, 0, 1
    for e, yj in zip(vectors, y):
        for i in range(n):
            F[i] = (F[i] + vp * e[i]) % Q
        Y = (Y + vp * yj) % Q
        vp = vp * v % Q
    q = [(F[i] - Y) * inv[i] % Q for i in range(n)]
    if m != NONE:
        s = sum(q[i] * pts[i] for i in range(n) if i != m) % Q
        q[m] = (-pow(pts[m], -1, Q) * s) % Q
    return {"inv": inv, "m": m, "y": y, "F": F, "Y": Y, "q": q}


def lagrange_at(tau: int, log_n: int):
    """L_i(tau), i < n: the discrete logs (to the base g) of the Lagrange points"""
    n = 1 << log_n
    pts = domain_points(log_n)
    if tau in pts:
        return [1 if x == tau else 0 for x in pts]
    zh = (pow(tau, n, Q) - 1) * pow(n, -1, Q) % Q
    return [zh * x % Q * d % Q for x, d in zip(pts, batch_inverse([(tau - x) % Q for x in pts]))]


def plan(log_n: int, count: int, commitments: bool, witness: bool, host_form: bool) -> dict:
    n = 1 << log_n
    stage = max(n, STAGE_MIN) if host_form else 0
    g = GROUP
    if host_form:
        g = min(g, stage // n)
    g = min(g, count)
    launches = ((count if commitments else 0) + (1 if witness else 0)) if count else 0
    return {"group_vectors": g, "groups": (count + g - 1) // g if count else 0, "stage_values": stage,
            "msm_launches": launches, "msm_terms": n, "lagrange_bytes": POINT_BYTES * n if launches else 0}


def check_commit(has_domain, has_evals, has_out, count) -> int:
    if not has_domain or count > MAX_COUNT or (count and not (has_evals and has_out)):
        return ERR_ARG
    return 0


def check_open(has_domain, has_evals, has_point, has_v, has_evaluations, count) -> int:
    if not has_domain or not has_point or count > MAX_COUNT:
        return ERR_ARG
    if count and not (has_evals and has_evaluations):
        return ERR_ARG
    if count > 1 and not has_v:
        return ERR_ARG
    return 0
