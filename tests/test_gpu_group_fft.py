"""GPU: the batched group transform of plonk_amd/csrc/kzg_domain.hip on its own, with the pointwise, extraction and finishing
kernels around it, reached through tests/_build/libdev_kzg_domain.so (tests/csrc/dev_kzg_domain.hip, built by build(): doors
only, the kernels are libplonk_hip.so's).

Inputs are points with KNOWN discrete logs [a_i] G, so output i of a transform is [DFT(a)_i] G: one oracle multiplication per
output, compared as 48 compressed bytes (the finishing kernel writes them; it is checked by itself against the oracle's
encoding first).  The inputs are made by the pointwise kernel from one base point (checked by itself as well).  Sizes 2, 4, 8,
64, 128 (exactly one workgroup of butterflies) and 512; forward (natural in, bit-reversed out), inverse (bit-reversed in,
natural out, no 1 / size) and the round trip; one polynomial and three with different data, at a stride larger than the size.
Guard slots before, between and after the polynomials are filled with 0xA5 and must come back untouched.  All comparisons
are exact."""
import ctypes
import functools
import os
import random

import pytest

import kzg_domain_model as M
from oracle import bls12_381 as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_domain.so")
Q = E.Q
SLOT = 256
GUARD = 2          # slots before and after the batch
PAD = 1            # slots between two polynomials (stride = size + PAD)
ID48 = bytes([0xC0]) + bytes(47)


@functools.lru_cache(maxsize=None)
def gmul48(s: int) -> bytes:
    s %= Q
    return E.g1_compress(E.g1_mul(E.G1_GEN, s)) if s else ID48


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_domain.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    so.dkd_twiddles.argtypes = [vp, u32, ctypes.POINTER(vp)]
    so.dkd_free.argtypes = [vp, vp]
    so.dkd_transform.argtypes = [vp, vp, u64, u32, u32, ci, vp, u32, vp]
    so.dkd_pointwise.argtypes = [vp, vp, vp, u64, vp, u64, u32, u32, vp]
    so.dkd_extract.argtypes = [vp, vp, u64, u32, u32]
    so.dkd_finish.argtypes = [vp, vp, u64, u64, u32, u32, ci, vp]
    so.dkd_load_raw.argtypes = [vp, vp, u64, vp]
    return so


class Rig:
    def __init__(self, lib):
        import plonk_amd
        self.P = plonk_amd
        self.ctx, self.lib = plonk_amd.Context(0), lib
        self.h = self.ctx.handle
        self.tw = {}
        self.base = {}

    def close(self):
        for t in self.tw.values():
            self.lib.dkd_free(self.h, t)
        for b in self.base.values():
            b.free()
        self.ctx.close()

    def twiddles(self, tw_log):
        if tw_log not in self.tw:
            p = ctypes.c_void_p()
            assert self.lib.dkd_twiddles(self.h, tw_log, ctypes.byref(p)) == 0
            self.tw[tw_log] = p
        return self.tw[tw_log]

    def load(self, points, slots_ptr):
        """affine points (None = identity) -> slots"""
        raw = b"".join(self.P.g1_to_raw96(p) if p is not None else bytes(96) for p in points)
        b = self.ctx.alloc(len(raw))
        b.upload(raw)
        assert self.lib.dkd_load_raw(self.h, b.ptr, len(points), slots_ptr) == 0
        b.free()

    def base_slots(self, size):
        """`size` slots that all hold the generator"""
        if size not in self.base:
            b = self.ctx.alloc(SLOT * size)
            self.load([E.G1_GEN] * size, b.ptr)
            self.base[size] = b
        return self.base[size]

    def points(self, logs, size_log):
        """slots [GUARD | poly 0 | PAD | poly 1 | PAD ...| GUARD] with slot p of polynomial b = [logs[b][p]] G, 0xA5 elsewhere"""
        size, batch = 1 << size_log, len(logs)
        stride = size + PAD
        buf = self.ctx.alloc(SLOT * (2 * GUARD + batch * stride))
        buf.upload(b"\xA5" * buf.nbytes)
        g = self.ctx.alloc(32 * size * batch)
        g.upload(b"".join(self.P.fr_to_bytes_mont([row[M.rev(i, size_log)] for i in range(size)]) for row in logs))
        rc = self.lib.dkd_pointwise(self.h, self.base_slots(size).ptr, g.ptr, size, buf.ptr + SLOT * GUARD, stride, size_log, batch,
                                    self.P.fr_to_bytes_mont([1]))
        assert rc == 0
        g.free()
        return buf, stride

    def read48(self, buf, stride, offset, log_n, batch, bitrev):
        n = 1 << log_n
        out = self.ctx.alloc(48 * (n * batch + 2))
        out.upload(b"\xA5" * out.nbytes)
        assert self.lib.dkd_finish(self.h, buf.ptr + SLOT * GUARD, stride, offset, log_n, batch, int(bitrev), out.ptr + 48) == 0
        raw = out.download()
        out.free()
        assert raw[:48] == b"\xA5" * 48 and raw[-48:] == b"\xA5" * 48, "the finishing kernel wrote outside its output"
        return [[raw[48 * (1 + b * n + i):48 * (2 + b * n + i)] for i in range(n)] for b in range(batch)]

    def guards_untouched(self, buf, stride, size, batch):
        raw = buf.download()
        assert raw[:SLOT * GUARD] == b"\xA5" * (SLOT * GUARD), "guard slots before the batch"
        assert raw[-SLOT * GUARD:] == b"\xA5" * (SLOT * GUARD), "guard slots after the batch"
        for b in range(batch):
            lo = SLOT * (GUARD + b * stride + size)
            assert raw[lo:lo + SLOT * PAD] == b"\xA5" * (SLOT * PAD), f"pad slot after polynomial {b}"

    def transform(self, buf, stride, size_log, batch, inverse, tw_log=None):
        tw_log = tw_log or size_log
        counts = (ctypes.c_uint64 * 2)()
        rc = self.lib.dkd_transform(self.h, buf.ptr + SLOT * GUARD, stride, size_log, batch, int(inverse), self.twiddles(tw_log), tw_log, counts)
        assert rc == 0
        return list(counts)


@pytest.fixture(scope="module")
def rig(lib):
    r = Rig(lib)
    yield r
    r.close()


def dft(a, size_log, inverse=False):
    w = M.root(size_log)
    return M.dft(a, pow(w, -1, Q) if inverse else w)


def run_case(rig, logs, size_log, mode, tw_log=None):
    """logs[b][i]: the discrete logs of polynomial b in NATURAL order"""
    size, batch = 1 << size_log, len(logs)
    if mode == "inverse":
        placed = [[row[M.rev(p, size_log)] for p in range(size)] for row in logs]      # bit-reversed in
    else:
        placed = logs
    buf, stride = rig.points(placed, size_log)
    counts = rig.transform(buf, stride, size_log, batch, mode == "inverse", tw_log)
    want_counts = [size_log, M.transform_muls(size_log) * batch]
    if mode == "roundtrip":
        back = rig.transform(buf, stride, size_log, batch, True, tw_log)
        counts = [counts[0] + back[0], counts[1] + back[1]]
        want_counts = [2 * size_log, 2 * M.transform_muls(size_log) * batch]
        want = [[x * size % Q for x in row] for row in logs]
    else:
        want = [dft(row, size_log, mode == "inverse") for row in logs]
    got = rig.read48(buf, stride, 0, size_log, batch, bitrev=(mode == "forward"))
    rig.guards_untouched(buf, stride, size, batch)
    buf.free()
    assert counts == want_counts
    for b in range(batch):
        for i in range(size):
            assert got[b][i] == gmul48(want[b][i]), (mode, size, b, i)


# ---- the kernels around the transform, each by itself ------------------------------------------------------------------
def test_finishing_kernel_encodes_like_the_oracle(rig):
    """both signs of y, the identity, with and without the bit reversal, at an offset"""
    rnd = random.Random(1)
    pts = [E.g1_mul(E.G1_GEN, rnd.randrange(1, Q)) for _ in range(6)]
    pts += [(pts[0][0], (-pts[0][1]) % E.P), None]
    assert len({E.g1_compress(p)[0] & 0x20 for p in pts[:7]}) == 2, "both signs of y occur"
    buf = rig.ctx.alloc(SLOT * (2 * GUARD + 3 + 8))
    buf.upload(b"\xA5" * buf.nbytes)
    rig.load(pts, buf.ptr + SLOT * (GUARD + 3))
    want = [E.g1_compress(p) if p is not None else ID48 for p in pts]
    assert rig.read48(buf, 0, 3, 3, 1, False)[0] == want
    assert rig.read48(buf, 0, 3, 3, 1, True)[0] == [want[M.rev(i, 3)] for i in range(8)]
    buf.free()


def test_pointwise_kernel_multiplies_by_the_scaled_scalar_in_bit_reversed_order(rig):
    rnd = random.Random(2)
    size_log, size, batch = 3, 8, 2
    k = [rnd.randrange(1, Q) for _ in range(size - 1)] + [None]                  # A: seven finite points and the identity
    A = rig.ctx.alloc(SLOT * size)
    rig.load([E.g1_mul(E.G1_GEN, x) if x is not None else None for x in k], A.ptr)
    G = [[0, 1, Q - 1] + [rnd.randrange(Q) for _ in range(size - 3)], [rnd.randrange(Q) for _ in range(size)]]
    scale = rnd.randrange(1, Q)
    g = rig.ctx.alloc(32 * size * batch)
    g.upload(b"".join(rig.P.fr_to_bytes_mont(row) for row in G))
    stride = size + PAD
    buf = rig.ctx.alloc(SLOT * (2 * GUARD + batch * stride))
    buf.upload(b"\xA5" * buf.nbytes)
    assert rig.lib.dkd_pointwise(rig.h, A.ptr, g.ptr, size, buf.ptr + SLOT * GUARD, stride, size_log, batch, rig.P.fr_to_bytes_mont([scale])) == 0
    got = rig.read48(buf, stride, 0, size_log, batch, False)
    rig.guards_untouched(buf, stride, size, batch)
    for b in range(batch):
        for p in range(size):
            s = G[b][M.rev(p, size_log)] * scale % Q
            assert got[b][p] == (gmul48(s * k[p]) if k[p] is not None else ID48), (b, p)
    assert got[0][M.rev(0, size_log)] == ID48                                    # the zero scalar
    for x in (A, g, buf):
        x.free()


def test_extraction_kernel_reverses_the_lower_half_into_the_upper(rig):
    log_n, n, batch = 3, 8, 2
    rnd = random.Random(3)
    logs = [[rnd.randrange(1, Q) for _ in range(2 * n)] for _ in range(batch)]
    buf, stride = rig.points(logs, log_n + 1)
    assert rig.lib.dkd_extract(rig.h, buf.ptr + SLOT * GUARD, stride, log_n, batch) == 0
    lower = rig.read48(buf, stride, 0, log_n, batch, False)
    upper = rig.read48(buf, stride, n, log_n, batch, False)
    rig.guards_untouched(buf, stride, 2 * n, batch)
    buf.free()
    for b in range(batch):
        assert lower[b] == [gmul48(logs[b][i]) for i in range(n)]
        assert upper[b] == [gmul48(logs[b][n - 2 - k]) for k in range(n - 1)] + [ID48]


# ---- the transform --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["forward", "inverse", "roundtrip"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("size_log", [1, 2, 3, 6, 7])
def test_transform_random_data(rig, size_log, batch, mode):
    rnd = random.Random(100 * size_log + batch)
    logs = [[rnd.randrange(Q) for _ in range(1 << size_log)] for _ in range(batch)]
    run_case(rig, logs, size_log, mode)


@pytest.mark.parametrize("mode", ["forward", "inverse", "roundtrip"])
def test_transform_512(rig, mode):
    rnd = random.Random(512)
    run_case(rig, [[rnd.randrange(Q) for _ in range(512)]], 9, mode)


def test_transform_512_batch_3_forward(rig):
    """three polynomials with different data whose expected outputs cost one oracle multiplication per index: a, 2a and 3a"""
    rnd = random.Random(513)
    a = [rnd.randrange(Q) for _ in range(512)]
    logs = [a, [2 * x % Q for x in a], [3 * x % Q for x in a]]
    buf, stride = rig.points(logs, 9)
    assert rig.transform(buf, stride, 9, 3, False) == [9, 3 * M.transform_muls(9)]
    got = rig.read48(buf, stride, 0, 9, 3, True)
    rig.guards_untouched(buf, stride, 512, 3)
    buf.free()
    want = dft(a, 9)
    for i in range(512):
        p = E.g1_mul(E.G1_GEN, want[i]) if want[i] else None
        p2 = E.g1_add(p, p)
        assert [got[0][i], got[1][i], got[2][i]] == [E.g1_compress(p), E.g1_compress(p2), E.g1_compress(E.g1_add(p2, p))], i


@pytest.mark.parametrize("tw_log", [4, 8])
def test_transform_reads_a_larger_twiddle_table_with_a_stride(rig, tw_log):
    rnd = random.Random(tw_log)
    logs = [[rnd.randrange(Q) for _ in range(8)] for _ in range(2)]
    for mode in ("forward", "inverse"):
        run_case(rig, logs, 3, mode, tw_log)


DEGENERATE = ["identities", "one finite", "all equal", "opposite halves", "equal halves"]


@pytest.mark.parametrize("shape", DEGENERATE)
@pytest.mark.parametrize("size_log", [3, 6])
def test_transform_degenerate_inputs(rig, size_log, shape):
    """the additions meet the identity, P + P and P - P: all identities; one finite point among identities; all points equal
    (every first-stage butterfly adds a point to itself and subtracts it from itself); a_i and a_(i + n/2) opposite / equal"""
    size = 1 << size_log
    rnd = random.Random(size)
    x = rnd.randrange(1, Q)
    half = [rnd.randrange(1, Q) for _ in range(size // 2)]
    logs = {"identities": [0] * size, "one finite": [0] * 5 + [x] + [0] * (size - 6), "all equal": [x] * size,
            "opposite halves": half + [(-v) % Q for v in half], "equal halves": half + half}[shape]
    for mode in ("forward", "inverse", "roundtrip"):
        run_case(rig, [logs], size_log, mode)
