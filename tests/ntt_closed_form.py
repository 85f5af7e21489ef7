"""Closed-form spectra for checking a transform of any size at O(1) per output (test code, host, pure Python).

Let N = 2^L, w the domain generator (oracle.fft.EvaluationDomain.group_gen), g = GENERATOR and e_p the unit vector at p.

  y = ifft(e_p):                 y[j] = N^-1 w^(-p j)              dense; all entries distinct for odd p
  fft(y) = e_p                   one Montgomery 1, every other byte zero
  fft(y[:m])[k]                = N^-1 (s^m - 1) / (s - 1),  s = w^(k - p);   m / N at k = p
  coset_fft(y[:m])[k]          = N^-1 (r^m - 1) / (r - 1),  r = g w^(k - p); r != 1 because g is outside the subgroup
  coset_ifft(coset_fft(y[:m])) = y[:m] followed by zeros

Values are canonical ints; the library's arrays hold them as 32 little-endian bytes of v * 2^256 mod q, and the checker
compares BYTES: a q where a 0 belongs (or any other non-canonical residue) is a mismatch.

The size lists of tests/test_gpu_ntt_plans.py live here as well, so that tests/test_ntt_closed_form_host.py can check
on the host that they cover every (role, radix) pair ntt_plan() produces."""
import random

from oracle.bls12_381 import GENERATOR, Q, ROOT_OF_UNITY

from tests import ntt_model

_R = (1 << 256) % Q

# ---- the sizes tests/test_gpu_ntt_plans.py runs (log2) ----
PLAN_SIZES = (14, 15, 17, 18, 21, 22)        # full arrays against the C oracle
PLAN_SIZES_THREE_MODES = (21, 22)            # ... of which these run three transforms instead of four (oracle time)
SINGLE_KERNEL_SIZES = (2, 4, 5, 7, 8, 9)     # full arrays against the Python oracle
IN_LEN_SIZES = (9, 12, 17, 19)
VALUE_SIZES = (10, 12, 17, 19)
LARGE_SIZES = (24, 25, 26, 27)               # closed form, through plonk_ntt_dev
DEV_CONTRACT_SIZES = (10, 11, 17, 19)
GPU_PLAN_TEST_SIZES = tuple(sorted(set(PLAN_SIZES + SINGLE_KERNEL_SIZES + IN_LEN_SIZES + VALUE_SIZES + LARGE_SIZES
                                       + DEV_CONTRACT_SIZES)))


def roles(L):
    """{(role, radix)} of the passes a 2^L transform runs: A the transposing first pass, B the in-place middle pass of a
    three-pass plan, C the last pass.  Empty for the single-kernel sizes."""
    p = ntt_model.plan(L)
    if len(p) == 1:
        return set()
    out = {("A", p[0]), ("C", p[-1])}
    if len(p) == 3:
        out.add(("B", p[1]))
    return out


def mont_bytes(v):
    return (v % Q * _R % Q).to_bytes(32, "little")


def from_mont_bytes(buf):
    r_inv = pow(_R, -1, Q)
    return [int.from_bytes(buf[i:i + 32], "little") * r_inv % Q for i in range(0, len(buf), 32)]


def omega(L):
    return pow(ROOT_OF_UNITY, 1 << (32 - L), Q)


def default_p(L):
    """an odd position below min(N, 2^16), away from the ends where N allows"""
    return 1 if L <= 1 else (0x9E37 % (1 << min(L, 16))) | 1


def single_frequency(L, p, j):
    """ifft(e_p)[j]"""
    N = 1 << L
    return pow(N, -1, Q) * pow(omega(L), (-p * j) % N, Q) % Q


def _geometric(L, m, base):
    """N^-1 (base^m - 1) / (base - 1); m / N for base == 1"""
    n_inv = pow(1 << L, -1, Q)
    if base == 1:
        return m % Q * n_inv % Q
    return n_inv * (pow(base, m, Q) - 1) % Q * pow(base - 1, -1, Q) % Q


def fft_truncated(L, p, m, k):
    """fft(ifft(e_p)[:m])[k]"""
    return _geometric(L, m, pow(omega(L), (k - p) % (1 << L), Q))


def coset_fft_truncated(L, p, m, k):
    """coset_fft(ifft(e_p)[:m])[k]"""
    return _geometric(L, m, GENERATOR * pow(omega(L), (k - p) % (1 << L), Q) % Q)


def unit_vector(p, k):
    return 1 if k == p else 0


def truncated_frequency(L, p, m, j):
    """(ifft(e_p)[:m] + zeros)[j]"""
    return single_frequency(L, p, j) if j < m else 0


def tile_corners(L):
    """First and last element of the first and of the last tile of every pass of the 2^L plan, for both compiled tile
    sizes (ntt.hip: 1024 and 2048 elements; a radix of 2^9 always takes 2048).  Passes A and C view the array as
    [R rows][N / R columns] with row stride N / R and a tile is all R rows of C consecutive columns; pass B works on
    the slabs of the transposed intermediate (ntt_model.ntt_model: addr)."""
    N = 1 << L
    p = ntt_model.plan(L)
    out = set()
    if len(p) == 1:
        return out
    for role, r in [("A", p[0]), ("C", p[-1])] + ([("B", p[1])] if len(p) == 3 else []):
        for tile_log in ((11,) if r == 9 else (10, 11)):
            C = 1 << (tile_log - r)
            R = 1 << r
            cols = N >> r
            if role == "B":
                R1 = 1 << p[0]

                def addr(row, cg):
                    return (cg >> p[0]) * (R1 * R) + row * R1 + (cg & (R1 - 1))
            else:
                def addr(row, cg):
                    return row * cols + cg
            for cg0 in (0, cols - C):
                out.update((addr(0, cg0), addr(0, cg0 + C - 1), addr(R - 1, cg0), addr(R - 1, cg0 + C - 1)))
    assert all(0 <= i < N for i in out)
    return out


def sample_indices(L, seed, p=None, randoms=4096):
    """The index list of a sampled check, fixed by (L, seed): the ends, the middle, p and its neighbours, every power
    of two and every power of two minus one, the tile corners of every pass, and `randoms` random indices (all of
    0..N-1 where N is not larger than that)."""
    N = 1 << L
    p = default_p(L) if p is None else p
    if N <= randoms:
        return list(range(N))
    s = {0, 1, 2, N // 2, N - 1, p, (p - 1) % N, (p + 1) % N}
    for b in range(L + 1):
        s.add((1 << b) % N)
        s.add((1 << b) - 1)
    s |= tile_corners(L)
    r = random.Random((L << 32) ^ seed)
    s.update(r.sample(range(N), randoms))
    return sorted(s)


def check(read, indices, expected):
    """read(k) -> the 32 bytes of element k; expected(k) -> canonical int.  Returns the list of (k, got, want) that
    differ (bytes), empty when the sample agrees."""
    bad = []
    for k in indices:
        got, want = bytes(read(k)), mont_bytes(expected(k))
        if got != want:
            bad.append((k, got, want))
    return bad


def reader(buf):
    """read callable over a bytes-like array of 32-byte elements; indices outside it read as empty (a mismatch)"""
    mv = memoryview(buf)
    return lambda k: mv[32 * k:32 * k + 32]
