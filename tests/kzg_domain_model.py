"""Big-int model of the whole-domain KZG10 openings (plonk_amd/csrc/kzg_domain.hip, kzg_domain_core.hpp), IN THE EXPONENT: a
point [x] g is the integer x mod q, the commit key under the suite's known tau is s_i = tau^i, a group transform is a
transform of integers.  The six steps, stage by stage with the index arithmetic of the kernels (decimation in frequency
forward, decimation in time back, one table of split twiddles read with a stride and, for the inverse, as minus the entry at
T - e), the plan of a call and the counts plonk_kzg_domain_last reports."""
from oracle import bls12_381 as E

Q = E.Q
MIN_LOG, MAX_LOG = 1, 20
MAX_COUNT = 65536
SLOT_BYTES = 256
WS_CAP_DEFAULT = 2 << 30
MAX_CHUNK = 4096
OK, ERR_ARG, ERR_DEGREE, ERR_NO_SRS, ERR_STATE, ERR_DATA = 0, -1, -3, -4, -7, -9


def root(log_size: int) -> int:
    """the generator of the size-2^log_size domain: fr_root_of_unity() = 7^((q-1)/2^32) squared 32 - log_size times"""
    return pow(7, (Q - 1) >> log_size, Q)


def domain_points(log_n: int):
    w, x, out = root(log_n), 1, []
    for _ in range(1 << log_n):
        out.append(x)
        x = x * w % Q
    return out


def rev(i: int, bits: int) -> int:
    r = 0
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def g_src(n: int, t: int):
    """g_t = f[g_src] (None: 0), t < 2n"""
    return n - 1 - t if t <= n - 2 else None


def h_src(n: int, k: int):
    """h_k = c[h_src] (None: the identity), k < n"""
    return n - 2 - k if k <= n - 2 else None


def twiddle(size_log: int, half: int, j: int, tw_log: int, inverse: bool):
    """(table index or None for the factor 1, negate) of lane j of the stage with span `half`"""
    e = (j * ((1 << size_log) // (2 * half))) << (tw_log - size_log)
    if e == 0:
        return None, False
    if not inverse:
        return e, False
    return (1 << (tw_log - 1)) - e, True


def twiddle_table(tw_log: int):
    w, x, out = root(tw_log), 1, []
    for _ in range(1 << (tw_log - 1)):
        out.append(x)
        x = x * w % Q
    return out


def stage_muls(size_log: int, half: int) -> int:
    return (1 << size_log) // 2 - (1 << size_log) // (2 * half)


def transform_muls(size_log: int) -> int:
    return sum(stage_muls(size_log, 1 << s) for s in range(size_log))


def forward(v, size_log: int, tw, tw_log: int, counts=None):
    """decimation in frequency, in place on a copy: natural order in, bit-reversed out"""
    v = list(v)
    size = 1 << size_log
    for s in range(size_log):
        half = size >> (s + 1)
        for t in range(size // 2):
            j = t & (half - 1)
            lo = ((t - j) << 1) + j
            hi = lo + half
            a, b = v[lo], v[hi]
            v[lo] = (a + b) % Q
            d = (a - b) % Q
            e, _ = twiddle(size_log, half, j, tw_log, False)
            if e is not None:
                d = d * tw[e] % Q
                if counts is not None:
                    counts[1] += 1
            v[hi] = d
        if counts is not None:
            counts[0] += 1
    return v


def inverse(v, size_log: int, tw, tw_log: int, counts=None):
    """decimation in time, bit-reversed in, natural order out, WITHOUT the 1 / size"""
    v = list(v)
    size = 1 << size_log
    for s in range(size_log):
        half = 1 << s
        for t in range(size // 2):
            j = t & (half - 1)
            lo = ((t - j) << 1) + j
            hi = lo + half
            b = v[hi]
            e, neg = twiddle(size_log, half, j, tw_log, True)
            if e is not None:
                assert neg
                b = (-b) % Q * tw[e] % Q
                if counts is not None:
                    counts[1] += 1
            a = v[lo]
            v[lo] = (a + b) % Q
            v[hi] = (a - b) % Q
        if counts is not None:
            counts[0] += 1
    return v


def dft(v, w):
    """the definition: out[i] = sum_k v[k] w^(ik)"""
    n = len(v)
    return [sum(v[k] * pow(w, i * k, Q) for k in range(n)) % Q for i in range(n)]


def toeplitz_naive(f, n: int, key):
    """h_k = sum_{l=0}^{n-2-k} f_(k+1+l) s_l, h_(n-1) = 0"""
    f = list(f) + [0] * (n - len(f))
    return [sum(f[k + 1 + l] * key[l] for l in range(n - 1 - k)) % Q for k in range(n)]


def witnesses_naive(f, log_n: int, key):
    n = 1 << log_n
    return dft(toeplitz_naive(f, n, key), root(log_n))


def six_steps(f, log_n: int, key, counts=None):
    """(evaluations, witness scalars) as the device computes them; key: s_0 .. s_(n-1) as integers; counts: [stage
    launches, scalar multiplications] added to as plonk_kzg_domain_last counts them"""
    n = 1 << log_n
    N, LN = 2 * n, log_n + 1
    f = [c % Q for c in f] + [0] * (n - len(f))
    assert len(f) == n
    tw = twiddle_table(LN)
    a = [key[l] if l <= n - 2 else 0 for l in range(N)]
    A = forward(a, LN, tw, LN)                                       # bit-reversed; per handle: not counted
    g = [f[g_src(n, t)] if g_src(n, t) is not None else 0 for t in range(N)]
    G = dft(g, root(LN))                                             # the scalar NTT: natural order
    n_inv = pow(N, -1, Q)
    P = [G[rev(p, LN)] * n_inv % Q * A[p] % Q for p in range(N)]
    if counts is not None:
        counts[1] += N
    c = inverse(P, LN, tw, LN, counts)
    slots = c[:n] + [c[h_src(n, k)] if h_src(n, k) is not None else 0 for k in range(n)]
    up = forward(slots[n:], log_n, tw, LN, counts)
    pi = [up[rev(i, log_n)] for i in range(n)]
    return dft(f, root(log_n)), pi


def plan(log_n: int, count: int, cap_bytes: int = WS_CAP_DEFAULT) -> dict:
    n = 1 << log_n
    per_poly = 2 * n * SLOT_BYTES
    chunk = min(max(cap_bytes // per_poly, 1), MAX_CHUNK, count)
    chunks = -(-count // chunk) if count else 0
    return {"chunk_polys": chunk, "chunks": chunks, "ws_bytes": chunk * per_poly,
            "stage_launches": chunks * (2 * log_n + 1),
            "scalar_muls": count * (2 * n + transform_muls(log_n + 1) + transform_muls(log_n))}


def check_create(log_n: int, has_comm: bool, has_srs: bool, srs_n: int) -> int:
    if not MIN_LOG <= log_n <= MAX_LOG:
        return ERR_ARG
    if has_comm:
        return ERR_STATE
    if not has_srs:
        return ERR_NO_SRS
    return ERR_DEGREE if srs_n < (1 << log_n) else OK
