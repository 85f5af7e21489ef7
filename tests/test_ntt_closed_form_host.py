"""Host check of tests/ntt_closed_form.py (the O(1)-per-output reference of tests/test_gpu_ntt_plans.py): it agrees
with both oracles, it reports every corruption a transform bug would cause, and the size lists of the GPU tests cover
every (role, radix) pair ntt_plan() produces."""
import pytest

import tests.ntt_closed_form as CF
from oracle.bls12_381 import Q
from oracle.fft import EvaluationDomain
from tests import ntt_model

SEED = 20


def _mont(vals):
    return b"".join(CF.mont_bytes(v) for v in vals)


def _lengths(N):
    return sorted({1, min(17, N), N // 8 + 3 if N >= 16 else N, N})


def _check_identities(L, fft, ifft, coset_fft, coset_ifft):
    """the five identities of the module docstring; each transform maps (bytes, in_len) -> N * 32 bytes"""
    N, p = 1 << L, CF.default_p(L)
    idx = CF.sample_indices(L, SEED, p)
    e_p = bytes(32 * p) + CF.mont_bytes(1) + bytes(32 * (N - p - 1))
    y = ifft(e_p, N)
    assert CF.check(CF.reader(y), idx, lambda j: CF.single_frequency(L, p, j)) == []
    assert fft(y, N) == e_p
    for m in _lengths(N):
        assert CF.check(CF.reader(fft(y[:32 * m], m)), idx, lambda k: CF.fft_truncated(L, p, m, k)) == [], m
        cf = coset_fft(y[:32 * m], m)
        assert CF.check(CF.reader(cf), idx, lambda k: CF.coset_fft_truncated(L, p, m, k)) == [], m
        assert coset_ifft(cf, N) == y[:32 * m] + bytes(32 * (N - m)), m


@pytest.mark.parametrize("L", range(1, 11))
def test_closed_forms_match_the_python_oracle(L):
    d = EvaluationDomain(1 << L)

    def wrap(f):
        return lambda b, m: _mont(f(CF.from_mont_bytes(b[:32 * m])))
    _check_identities(L, wrap(d.fft), wrap(d.ifft), wrap(d.coset_fft), wrap(d.coset_ifft))


@pytest.mark.parametrize("L", [11, 14, 17])
def test_closed_forms_match_the_c_oracle(L):
    from oracle import cbind

    def mode(inverse, coset):
        return lambda b, m: cbind.ntt_bytes(b, L, inverse, coset, m)
    _check_identities(L, mode(False, False), mode(True, False), mode(False, True), mode(True, True))


# ---- the checker must report what a wrong transform would produce ----
L_BAD, M_BAD = 13, (1 << 13) // 8 + 3


@pytest.fixture(scope="module")
def truncated_spectrum():
    """fft(y[:m]) at 2^13 (plan (7, 6): larger than the 4096 random samples, so the list is a true sample) by the C
    oracle, with the index list and the expectation it satisfies"""
    from oracle import cbind
    N, p = 1 << L_BAD, CF.default_p(L_BAD)
    e_p = bytes(32 * p) + CF.mont_bytes(1) + bytes(32 * (N - p - 1))
    y = cbind.ntt_bytes(e_p, L_BAD, True, False, N)
    out = cbind.ntt_bytes(y[:32 * M_BAD], L_BAD, False, False, M_BAD)
    idx = CF.sample_indices(L_BAD, SEED, p, randoms=1024)
    assert len(idx) < N

    def want(k):
        return CF.fft_truncated(L_BAD, p, M_BAD, k)
    assert CF.check(CF.reader(out), idx, want) == []
    return y, out, idx, want, p


def _element(out, k):
    return int.from_bytes(out[32 * k:32 * k + 32], "little")


def _with_element(out, k, raw):
    return out[:32 * k] + (raw % (1 << 256)).to_bytes(32, "little") + out[32 * k + 32:]


def test_checker_reports_one_element_off_by_one(truncated_spectrum):
    _, out, idx, want, _ = truncated_spectrum
    for k in (idx[0], idx[len(idx) // 2], idx[-1]):
        for delta in (1, -1):
            bad = CF.check(CF.reader(_with_element(out, k, _element(out, k) + delta)), idx, want)
            assert [b[0] for b in bad] == [k]


def test_checker_reports_two_swapped_elements_of_one_tile(truncated_spectrum):
    """the first and the last element of the first and of the last tile of the last pass are in every index list"""
    _, out, idx, want, _ = truncated_spectrum
    N = 1 << L_BAD
    r = ntt_model.plan(L_BAD)[-1]
    for tile_log in (10, 11):
        C, cols = 1 << (tile_log - r), N >> r
        for cg0 in (0, cols - C):
            a, b = cg0, ((1 << r) - 1) * cols + cg0 + C - 1
            assert a in idx and b in idx
            swapped = _with_element(_with_element(out, a, _element(out, b)), b, _element(out, a))
            assert sorted(x[0] for x in CF.check(CF.reader(swapped), idx, want)) == [a, b]


def test_checker_reports_a_rotated_output(truncated_spectrum):
    _, out, idx, want, _ = truncated_spectrum
    for rot in (out[32:] + out[:32], out[-32:] + out[:-32]):
        assert len(CF.check(CF.reader(rot), idx, want)) == len(idx)


def test_checker_reports_a_length_off_by_one(truncated_spectrum):
    from oracle import cbind
    y, _, idx, want, _ = truncated_spectrum
    for m in (M_BAD - 1, M_BAD + 1):
        out = cbind.ntt_bytes(y[:32 * m], L_BAD, False, False, m)
        assert len(CF.check(CF.reader(out), idx, want)) == len(idx)       # every output depends on every coefficient


def test_checker_reports_a_missing_scale(truncated_spectrum):
    y, out, idx, want, p = truncated_spectrum
    N = 1 << L_BAD
    unscaled = _mont(v * N % Q for v in CF.from_mont_bytes(y))      # the inverse transform without n^-1
    assert len(CF.check(CF.reader(unscaled), idx, lambda j: CF.single_frequency(L_BAD, p, j))) == len(idx)
    unscaled = _mont(v * N % Q for v in CF.from_mont_bytes(out))
    assert len(CF.check(CF.reader(unscaled), idx, want)) == len(idx)


def test_checker_reports_q_where_zero_belongs(truncated_spectrum):
    """fft(y) must be e_p as BYTES: q (the non-canonical zero a lazy reduction may leave) is reported"""
    from oracle import cbind
    y, _, idx, _, p = truncated_spectrum
    N = 1 << L_BAD
    e_p = cbind.ntt_bytes(y, L_BAD, False, False, N)
    assert CF.check(CF.reader(e_p), idx, lambda k: CF.unit_vector(p, k)) == []
    k = next(i for i in idx if i != p)
    bad = CF.check(CF.reader(_with_element(e_p, k, Q)), idx, lambda k: CF.unit_vector(p, k))
    assert [b[0] for b in bad] == [k]
    bad = CF.check(CF.reader(_with_element(e_p, p, _element(e_p, p) + Q)), idx, lambda k: CF.unit_vector(p, k))
    assert [b[0] for b in bad] == [p]


def test_checker_reports_a_short_array(truncated_spectrum):
    _, out, idx, want, _ = truncated_spectrum
    assert CF.check(CF.reader(out[:-32]), idx, want)[-1][0] == (1 << L_BAD) - 1


# ---- the index list ----
@pytest.mark.parametrize("L", [11, 13, 17, 19, 24, 27])
def test_index_list_holds_what_it_promises(L):
    N, p = 1 << L, CF.default_p(L)
    idx = CF.sample_indices(L, SEED, p)
    assert idx == CF.sample_indices(L, SEED, p) and idx == sorted(set(idx)) and 0 <= idx[0] and idx[-1] < N
    s = set(idx)
    assert p % 2 == 1 and p < min(N, 1 << 16)
    assert {0, 1, 2, N // 2, N - 1, p, p - 1, p + 1} <= s
    assert all((1 << b) in s for b in range(L)) and all((1 << b) - 1 in s for b in range(L + 1))
    assert CF.tile_corners(L) <= s
    assert len(idx) == N or len(idx) >= 4096
    if N > 1 << 13:
        assert idx != CF.sample_indices(L, SEED + 1, p)
    # the corners of the last pass, written out: [R rows][N / R columns], a tile is R rows of C columns
    r = ntt_model.plan(L)[-1]
    C, cols = 1 << (11 - r), N >> r
    assert {0, C - 1, ((1 << r) - 1) * cols, ((1 << r) - 1) * cols + C - 1, cols - C, cols - 1, N - C, N - 1} <= s


# ---- completeness of the GPU size lists ----
def test_gpu_size_lists_cover_every_pass_role_and_radix():
    """A change to ntt_plan() (mirrored by ntt_model.plan, which test_ntt_model pins to the kernel's limits) breaks
    this test until the size lists of tests/test_gpu_ntt_plans.py follow."""
    produced = set().union(*(CF.roles(L) for L in range(11, 28)))
    covered = set().union(*(CF.roles(L) for L in CF.GPU_PLAN_TEST_SIZES))
    assert produced - covered == set(), sorted(produced - covered)
    assert {("A", 9), ("B", 9), ("C", 9)} <= covered
    # full-array comparisons alone (everything but the closed-form sizes) reach radix 2^9 as first and as last pass
    full = set().union(*(CF.roles(L) for L in CF.PLAN_SIZES + CF.IN_LEN_SIZES + CF.VALUE_SIZES + CF.DEV_CONTRACT_SIZES))
    assert {("A", 9), ("C", 9)} <= full
    # every plan of 11..27 that the older tests/test_gpu_ntt.py does not transform directly is in a list here
    older = {11, 12, 13, 16, 19, 20, 23}
    assert set(range(11, 28)) - older <= set(CF.GPU_PLAN_TEST_SIZES)
    assert set(CF.PLAN_SIZES_THREE_MODES) <= set(CF.PLAN_SIZES)
    assert all(L <= 10 for L in CF.SINGLE_KERNEL_SIZES) and all(11 <= L <= 27 for L in CF.PLAN_SIZES + CF.LARGE_SIZES)
    assert any(L > 25 for L in CF.LARGE_SIZES)          # ntt.hip NTT_DIRECT_MAX_LOG: the two-level path by default


def test_roles_of_known_plans():
    assert CF.roles(17) == {("A", 9), ("C", 8)}
    assert CF.roles(18) == {("A", 9), ("C", 9)}
    assert CF.roles(26) == {("A", 9), ("B", 9), ("C", 8)}
    assert CF.roles(11) == {("A", 6), ("C", 5)}
    assert CF.roles(10) == set()
