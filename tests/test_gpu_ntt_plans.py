"""GPU parity of every pass plan of plonk_ntt / plonk_ntt_dev (ntt.hip: ntt_plan), 2^2 .. 2^27, of the in_len edges of
the first pass, of inputs at the ends of the lazy Fr29 range, and of the device-resident entry point's contract.

Bytes in, bytes out.  Up to 2^22 whole arrays are compared with the C restatement of best_fft (oracle/c, pinned to the
big-int oracle by tests/test_oracle_c.py); 2^24 .. 2^27 are checked against the closed forms of tests/ntt_closed_form.py
(which tests/test_ntt_closed_form_host.py checks against both oracles, and whose size lists it checks for covering
every (role, radix) pair the plans produce).

Three contexts run the plan and in_len tests: the default (4 elements per lane, whole inter-pass twiddle tables), one
created with GpuConfig(ntt_elements_log2=3), and one created while PLONK_NTT_DIRECT=0 is set: capi.hip config_resolve
reads the environment when a context is created (and at plonk_ctx_set_config), per context and not per process, so a
fresh Context under monkeypatch.setenv takes the two-level twiddle path and no child process is needed."""
import ctypes
import functools
import time

import numpy as np
import pytest

import tests.ntt_closed_form as CF
from oracle.bls12_381 import Q
from tests import ntt_model

pytestmark = pytest.mark.gpu

SEED = 20
MODES = {"fft": (False, False), "ifft": (True, False), "coset_fft": (False, True), "coset_ifft": (True, True)}
GUARD = 4096 * 32                     # bytes of 0xA5 on both sides of every plonk_ntt_dev operand
CHUNK = 256 << 20                     # largest single download of a whole-array check


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["default", "elements8", "two_level"])
def vctx(request):
    """the three kernel variants of the module docstring, each on a context of its own"""
    import plonk_amd
    if request.param == "elements8":
        c = plonk_amd.Context(0, plonk_amd.GpuConfig(ntt_elements_log2=3))
        assert c.get_config().ntt_elements_log2 == 3
    elif request.param == "two_level":
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PLONK_NTT_DIRECT", "0")
            c = plonk_amd.Context(0)
    else:
        c = plonk_amd.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    """got == want, reporting element indices instead of a diff of megabytes"""
    if got == want:
        return
    assert len(got) == len(want), (what, len(got), len(want))
    a = np.frombuffer(got, dtype=np.uint64).reshape(-1, 4)
    b = np.frombuffer(want, dtype=np.uint64).reshape(-1, 4)
    bad = np.flatnonzero((a != b).any(axis=1))
    pytest.fail(f"{what}: {len(bad)} of {len(a)} elements differ, the first at {bad[:8].tolist()}")


@functools.lru_cache(maxsize=None)
def _random_input(L):
    """N + 5 dense random elements: Montgomery limbs below 2^254 < q"""
    raw = np.random.default_rng(700 + L).integers(0, 256, size=((1 << L) + 5, 32), dtype=np.uint8)
    raw[:, 31] &= 0x3F
    return raw.tobytes()


@functools.lru_cache(maxsize=None)
def _oracle_of_random(L, mode, in_len):
    """computed once, shared by the three variants"""
    from oracle import cbind
    inverse, coset = MODES[mode]
    return cbind.ntt_bytes(_random_input(L)[:32 * min(in_len, 1 << L)], L, inverse, coset, in_len)


def _gpu_of_random(c, L, mode, in_len):
    inverse, coset = MODES[mode]
    return c.ntt_bytes(_random_input(L)[:32 * min(in_len, (1 << L) + 5)], L, inverse, coset, in_len)


# ---- a. every plan the older tests do not transform directly, whole arrays ----
PLAN_CASES = [(L, m) for L in CF.PLAN_SIZES for m in MODES if not (L in CF.PLAN_SIZES_THREE_MODES and m == "ifft")]


@pytest.mark.parametrize("L,mode", PLAN_CASES)
def test_plan_matches_the_c_oracle(vctx, L, mode):
    N = 1 << L
    in_len = N // 8 + 3 if mode == "coset_fft" else N
    _same(_gpu_of_random(vctx, L, mode, in_len), _oracle_of_random(L, mode, in_len), (L, ntt_model.plan(L), mode))


@pytest.mark.parametrize("L", CF.SINGLE_KERNEL_SIZES)
def test_single_kernel_matches_the_python_oracle(vctx, L):
    from oracle.fft import EvaluationDomain
    N = 1 << L
    d = EvaluationDomain(N)
    raw = _random_input(L)[:32 * N]
    a = CF.from_mont_bytes(raw)
    il = N // 8 + 3

    def mont(vals):
        return b"".join(CF.mont_bytes(v) for v in vals)
    assert vctx.ntt_bytes(raw, L, False, False, N) == mont(d.fft(a))
    assert vctx.ntt_bytes(raw, L, True, False, N) == mont(d.ifft(a))
    assert vctx.ntt_bytes(raw[:32 * il], L, False, True, il) == mont(d.coset_fft(a[:il]))
    assert vctx.ntt_bytes(raw, L, True, True, N) == mont(d.coset_ifft(a))


# ---- b. in_len edges of the first pass ----
def _in_lens(L):
    N = 1 << L
    lens = [1, 2, N // 8 + 3, N // 4 + 3, N // 2, N - 1, N, N + 5]
    if L > 10:                                  # R: one whole row of the first pass's [R1 rows][N / R1 columns] view
        R = N >> ntt_model.plan(L)[0]
        lens += [R - 1, R, R + 1]
    return sorted(set(lens))


@pytest.mark.parametrize("mode", ["fft", "coset_fft"])
@pytest.mark.parametrize("L", CF.IN_LEN_SIZES)
def test_in_len_edges_forward(vctx, L, mode):
    """The host entry point uploads in_len elements only: whatever the staging buffer held before lies behind them, so
    a load that is not masked changes the result."""
    for in_len in _in_lens(L):
        _same(_gpu_of_random(vctx, L, mode, in_len), _oracle_of_random(L, mode, in_len), (L, mode, in_len))


@pytest.mark.parametrize("mode", ["ifft", "coset_ifft"])
@pytest.mark.parametrize("L", CF.IN_LEN_SIZES)
def test_in_len_edge_inverse(vctx, L, mode):
    from oracle import cbind
    N = 1 << L
    in_len = N // 2 + 1
    inverse, coset = MODES[mode]
    want = _oracle_of_random(L, mode, in_len)
    padded = _random_input(L)[:32 * in_len] + bytes(32 * (N - in_len))
    assert want == cbind.ntt_bytes(padded, L, inverse, coset, N)        # the C oracle pads like the kernel masks
    _same(_gpu_of_random(vctx, L, mode, in_len), want, (L, mode, in_len))


# ---- c. values at the ends of the lazy range, and spectra that must be exact zeros ----
def _patterns(L):
    N = 1 << L
    m1, one, zero = CF.mont_bytes(Q - 1), CF.mont_bytes(1), bytes(32)
    top = (Q - 1).to_bytes(32, "little")        # the largest canonical limbs (the field element -2^-256)
    return {
        "all_minus_one": m1 * N,
        "all_one": one * N,
        "alternating_minus_one_zero": (m1 + zero) * (N // 2),
        "alternating_minus_one_one": (m1 + one) * (N // 2),
        "half_minus_one_half_zero": m1 * (N // 2) + zero * (N // 2),
        "all_largest_limbs": top * N,
        "alternating_largest_limbs_zero": (top + zero) * (N // 2),
    }


PATTERN_NAMES = sorted(_patterns(1))


@pytest.mark.parametrize("name", PATTERN_NAMES)
@pytest.mark.parametrize("L", CF.VALUE_SIZES)
def test_value_edges(ctx, L, name):
    from oracle import cbind
    N = 1 << L
    a = _patterns(L)[name]
    for mode, (inverse, coset) in MODES.items():
        _same(ctx.ntt_bytes(a, L, inverse, coset, N), cbind.ntt_bytes(a, L, inverse, coset, N), (L, name, mode))


@pytest.mark.parametrize("L", CF.VALUE_SIZES)
def test_single_frequency(ctx, L):
    """y = ifft(e_p) is dense and its spectrum is one Montgomery 1 with every other BYTE zero"""
    from oracle import cbind
    N, p = 1 << L, CF.default_p(L)
    e_p = bytes(32 * p) + CF.mont_bytes(1) + bytes(32 * (N - p - 1))
    y = cbind.ntt_bytes(e_p, L, True, False, N)
    assert CF.check(CF.reader(y), CF.sample_indices(L, SEED, p), lambda j: CF.single_frequency(L, p, j)) == []
    _same(ctx.ntt_bytes(e_p[:32 * (p + 1)], L, True, False, p + 1), y, (L, "ifft(e_p)"))
    _same(ctx.ntt_bytes(y, L, False, False, N), e_p, (L, "fft(y)"))
    for mode, (inverse, coset) in MODES.items():
        _same(ctx.ntt_bytes(y, L, inverse, coset, N), cbind.ntt_bytes(y, L, inverse, coset, N), (L, "y", mode))


# ---- d. the large plans by closed form, through plonk_ntt_dev ----
def _assert_zero_except(c, pinned, buf, lo, hi, special, what):
    """every byte of the elements [lo, hi) of buf is zero, except the elements of special: {index: 32 bytes};
    downloaded in chunks of 256 MiB through pinned memory"""
    words = np.ctypeslib.as_array((ctypes.c_uint64 * (CHUNK // 8)).from_address(pinned.ptr))
    for a in range(lo, hi, CHUNK // 32):
        b = min(a + CHUNK // 32, hi)
        c.d2h_into(pinned.ptr, buf.ptr + 32 * a, 32 * (b - a))
        v = words[:4 * (b - a)]
        for k, raw in special.items():
            if a <= k < b:
                assert v[4 * (k - a):4 * (k - a) + 4].tobytes() == raw, (what, k)
                v[4 * (k - a):4 * (k - a) + 4] = 0
        if v.any():
            bad = np.flatnonzero(v.reshape(-1, 4).any(axis=1))
            pytest.fail(f"{what}: {len(bad)} non-zero elements in [{a}, {b}), the first at {(bad[:8] + a).tolist()}")


@pytest.mark.parametrize("L", CF.LARGE_SIZES)
def test_large_plan_by_closed_form(ctx, L):
    """2^24 (8,8,8), 2^25 (9,8,8), 2^26 (9,9,8) and 2^27 (9,9,9); the last two take the two-level twiddles by default
    (ntt.hip NTT_DIRECT_MAX_LOG).  One element at p in a source that holds p + 1 elements -> y = ifft -> fft(y) == e_p over
    the whole array; coset_fft(y[:m]) for m = N and N/8 + 3 at the index list; coset_ifft of the latter is y[:m] bit for
    bit (first 4096 elements and the index list) and zero over the whole tail.  Both whole-array checks download every
    byte at every size: measured on an MI355X a case takes 1.0 s at 2^24 and 1.6 s at 2^27 (the 4 GiB download and
    scan 0.4 s of it), so no size needs sampled windows."""
    import plonk_amd
    N, p = 1 << L, CF.default_p(L)
    assert p % 2 == 1 and p < 1 << 16
    idx = CF.sample_indices(L, SEED, p)
    one = CF.mont_bytes(1)
    held = []
    t = [time.perf_counter()]

    def lap(what):
        ctx.sync()
        t.append(time.perf_counter())
        print(f"2^{L} {what}: {t[-1] - t[-2]:.2f} s")

    def sampled(buf, expected, what):
        bad = CF.check(lambda k: buf.download(32, 32 * k), idx, expected)
        assert not bad, (what, len(bad), bad[:3])
    try:
        for n in (32 * (p + 1), 32 * N, 32 * N, 32 * N):
            held.append(ctx.alloc(n))
        src, y, out, tmp = held
        pinned = plonk_amd.PinnedBuffer(CHUNK)
        held.append(pinned)
        src.upload(bytes(32 * p) + one)
        ctx.ntt_dev(src.ptr, y.ptr, tmp.ptr, L, inverse=True, in_len=p + 1)
        lap("ifft (tables built)")
        sampled(y, lambda j: CF.single_frequency(L, p, j), "y")
        lap("index list of y")
        ctx.ntt_dev(y.ptr, out.ptr, tmp.ptr, L)
        lap("fft (tables built)")
        _assert_zero_except(ctx, pinned, out, 0, N, {p: one}, "fft(y)")
        sampled(out, lambda k: CF.unit_vector(p, k), "fft(y)")
        lap("fft(y) == e_p over the array")
        m = N // 8 + 3
        for in_len in (N, m):
            ctx.ntt_dev(y.ptr, out.ptr, tmp.ptr, L, coset=True, in_len=in_len)
            sampled(out, lambda k: CF.coset_fft_truncated(L, p, in_len, k), ("coset_fft", in_len))
            lap(f"coset_fft of {in_len} and its index list")
        ctx.ntt_dev(out.ptr, out.ptr, tmp.ptr, L, inverse=True, coset=True)
        assert out.download(32 * 4096) == y.download(32 * 4096)
        sampled(out, lambda j: CF.truncated_frequency(L, p, m, j), "coset_ifft")
        lap("coset_ifft in place, head and index list")
        _assert_zero_except(ctx, pinned, out, m, N, {}, "tail of coset_ifft")
        lap("tail of coset_ifft is zero")
    finally:
        for b in held:
            b.free()
    print(f"2^{L} total: {time.perf_counter() - t[0]:.2f} s")


# ---- e. plonk_ntt_dev: operands inside larger buffers ----
@pytest.mark.parametrize("mode", ["coset_fft", "coset_ifft"])
@pytest.mark.parametrize("L", CF.DEV_CONTRACT_SIZES)
def test_dev_entry_point_contract(ctx, L, mode):
    """src, dst and tmp are sub-ranges of larger buffers with 4096 elements of 0xA5 on both sides; behind the in_len
    valid elements of src lie N - in_len elements of 0xFF (mapped memory: a read past in_len changes the result, it
    never leaves the allocation).  The result equals the host entry point's, nothing outside dst[0..N) and tmp[0..N)
    is written, src survives when src != dst, src == dst gives the same result, and so does a src allocation of
    exactly in_len elements."""
    N = 1 << L
    inverse, coset = MODES[mode]
    in_len = N if inverse else N // 8 + 3
    data = _random_input(L)[:32 * in_len]
    want = ctx.ntt_bytes(data, L, inverse, coset, in_len)
    _same(want, _oracle_of_random(L, mode, in_len), (L, mode, "host entry point"))
    guard = b"\xa5" * GUARD
    src_image = guard + data + b"\xff" * (32 * (N - in_len)) + guard
    blank = guard + b"\x5a" * (32 * N) + guard
    held = []

    def guarded(buf, what):
        img = buf.download()
        assert img[:GUARD] == guard and img[-GUARD:] == guard, (what, "guard band written")
        return img[GUARD:-GUARD]
    try:
        for n in (len(src_image), len(blank), len(blank), len(data)):
            held.append(ctx.alloc(n))
        src, dst, tmp, exact = held
        src.upload(src_image)
        dst.upload(blank)
        tmp.upload(blank)
        exact.upload(data)
        ctx.ntt_dev(src.ptr + GUARD, dst.ptr + GUARD, tmp.ptr + GUARD, L, inverse, coset, in_len)
        assert src.download() == src_image, "src was written"
        _same(guarded(dst, "dst"), want, (L, mode, "src != dst"))
        guarded(tmp, "tmp")
        # in place
        dst.upload(src_image)
        ctx.ntt_dev(dst.ptr + GUARD, dst.ptr + GUARD, tmp.ptr + GUARD, L, inverse, coset, in_len)
        _same(guarded(dst, "dst in place"), want, (L, mode, "src == dst"))
        guarded(tmp, "tmp in place")
        # a source that ends with its last valid element
        dst.upload(blank)
        ctx.ntt_dev(exact.ptr, dst.ptr + GUARD, tmp.ptr + GUARD, L, inverse, coset, in_len)
        assert exact.download() == data
        _same(guarded(dst, "dst from a short src"), want, (L, mode, "short src"))
    finally:
        for b in held:
            b.free()
