"""Big-int model of the many-vector commitments on a KZG domain handle (plonk_amd/csrc/kzg_many_core.hpp, kzg_many.hip): the
signed-digit recoding of a whole scalar, the window count W(c), the size and the indexing of the window tables, the entry
(i, w, d) as a scalar multiple of L_i(tau), the automatic width and the plan of a call.  Nothing here is derived from the
code under test: W(c) comes from the carry chain written as one addition, the digits from the remainder definition."""
from oracle import bls12_381 as E
from tests import kzg_evals_model as EM
from tests import kzg_ref as K

Q = E.Q
C_MIN, C_MAX = 2, 8
LOG_N_MAX = 12
MAX_COUNT = 1 << 24
MAX_TERMS = 1 << 28
MAX_SEGMENT = 1 << 16           # terms of one segment of the sparse form
ENTRY_BYTES = 128
SLOT_BYTES = 256
LANES = 64
RESIDENT_WAVES = 2048            # 256 CUs x 4 SIMDs x 2 waves
CHUNK_MAX = 1 << 20
TERM_BYTES = 36
WS_CAP_DEFAULT = 2 << 30
ERR_ARG = -1


def recode(s: int, c: int, windows: int):
    """(digits, carry out): d_w = the remainder of what is left modulo 2^c taken in (-2^(c-1), 2^(c-1)]"""
    half, digits = 1 << (c - 1), []
    for _ in range(windows):
        d = s % (1 << c)
        if d > half:
            d -= 1 << c
        digits.append(d)
        s = (s - d) >> c
    return digits, s


def windows(c: int) -> int:
    """the smallest W with ((q - 1) + H) >> c (W - 1) <= 2^(c-1), H = the digit 2^(c-1) - 1 in every window below the top: a
    window carries exactly when adding 2^(c-1) - 1 to it (and the carry below) overflows c bits, so the recoding's carries are
    the carries of s + H, and the top digit grows with s"""
    half = 1 << (c - 1)
    W = 1
    while True:
        H = sum((half - 1) << (c * w) for w in range(W - 1))
        if ((Q - 1 + H) >> (c * (W - 1))) <= half:
            return W
        W += 1


def table_entries(log_n: int, c: int) -> int:
    return (windows(c) << log_n) << (c - 1)


def table_bytes(log_n: int, c: int) -> int:
    return table_entries(log_n, c) * ENTRY_BYTES


def entry_index(c: int, i: int, w: int, d: int) -> int:
    assert 1 <= d <= 1 << (c - 1)
    return ((i * windows(c) + w) << (c - 1)) + d - 1


def entry_scalar(log_n: int, c: int, i: int, w: int, d: int, tau=K.TAU) -> int:
    """the discrete log (to the base g) of table entry (i, w, d): d 2^(c w) L_i(tau)"""
    return d * pow(2, c * w, Q) * EM.lagrange_at(tau, log_n)[i] % Q


def auto_width(log_n: int, left: int) -> int:
    for c in range(C_MAX, C_MIN - 1, -1):
        if table_bytes(log_n, c) <= left:
            return c
    return 0


def slices(log_n: int, count: int, force: int = 0) -> int:
    """doubled while the call has fewer waves than the device holds, down to one value per lane; forced: down to one value"""
    n = 1 << log_n
    s = 1
    if force:
        while s * 2 <= n and s * 2 <= force:
            s *= 2
        return s
    while count * s < RESIDENT_WAVES and s * 2 <= n // LANES:
        s *= 2
    return s


def plan(log_n: int, c: int, count: int, ws_cap: int = WS_CAP_DEFAULT, host_form: bool = False, force_slices: int = 0) -> dict:
    W = windows(c)
    s = slices(log_n, count, force_slices)
    per_vector = SLOT_BYTES * s + 48 + ((64 << log_n) if host_form else 0)
    per = min(max(ws_cap // per_vector, 1), CHUNK_MAX, count)
    return {"log_n": log_n, "window_bits": c, "windows": W, "slices": s, "count": count, "terms": count << log_n,
            "chunk_vectors": per, "chunks": -(-count // per) if count else 0, "additions": (count << log_n) * W}


def sparse_plan(log_n: int, c: int, offsets, ws_cap: int = WS_CAP_DEFAULT) -> dict:
    count = len(offsets) - 1
    W = windows(c)
    chunks, largest, first = 0, 0, 0
    while first < count:
        used, k = 0, first
        while k < count and k - first < CHUNK_MAX:
            add = SLOT_BYTES + 48 + TERM_BYTES * (offsets[k + 1] - offsets[k])
            if k > first and used + add > ws_cap:
                break
            used += add
            k += 1
        largest = max(largest, k - first)
        chunks += 1
        first = k
    terms = offsets[count] if count else 0
    return {"log_n": log_n, "window_bits": c, "windows": W, "slices": 1, "count": count, "terms": terms,
            "chunk_vectors": largest, "chunks": chunks, "additions": terms * W}


def commitment(vector, log_n: int, tau=K.TAU) -> bytes:
    """[sum_i e_i L_i(tau)] G in closed form"""
    L = EM.lagrange_at(tau, log_n)
    return K.scalar_commit(sum(a * b for a, b in zip(vector, L)) % Q)


def updated(base_scalar: int, update, log_n: int, tau=K.TAU) -> bytes:
    """base + sum delta L_index, the base given by its discrete log to the base g"""
    L = EM.lagrange_at(tau, log_n)
    return K.scalar_commit((base_scalar + sum(x * L[i] for i, x in update)) % Q)
