"""GPU: KZG10 cell proofs (plonk_kzg_open_cells / _dev / plonk_kzg_cell_points / plonk_kzg_cells_last;
plonk_amd/csrc/kzg_cells.hip) on the suite's synthetic known-tau key, so proof k of f is
[g (f(tau) - r_k(tau)) / (tau^l - x_k)] G and exists as bytes at every size; cell values are Horner values.  Every comparison is
exact.  The multiply-accumulate and its reduction are also run on their own through tests/_build/libdev_kzg_cells.so
(tests/csrc/dev_kzg_cells.hip, built by build(): doors only, the kernels are libplonk_hip.so's) against the big-int model
tests/kzg_cells_model.py, with guard slots around the partials, and cells go through a REAL pairing with an opening key
whose third element is [tau^l] h."""
import ctypes
import os
import random

import pytest

from oracle import bls12_381 as E
from tests import g2_ref as G2
from tests import kzg_cells_model as M
from tests import kzg_domain_model as D
from tests import kzg_ref as K
from tests.test_gpu_group_fft import GUARD, PAD, SLOT, Rig, gmul48
from tests.test_gpu_group_fft import lib as fft_lib  # noqa: F401  (the doors of dev_kzg_domain.hip: a fixture)

pytestmark = pytest.mark.gpu
Q = E.Q
OK, ERR_ARG, ERR_DEGREE, ERR_STATE, ERR_DATA, ERR_VERIFY = 0, -1, -3, -7, -9, -12
ID48 = K.IDENTITY48
KEY_POINTS = 1 << 12
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_kzg_cells.so")


def load_key(ctx, n, tau=K.TAU):
    buf = ctx.alloc(96 * n)
    ctx.srs_generate_dev(tau, K.G_SCALAR, n, buf.ptr)
    ctx.srs_load_dev(buf.ptr, n)
    ctx.sync()
    buf.free()


@pytest.fixture(scope="module")
def doors():
    assert os.path.exists(SO), "tests/_build/libdev_kzg_cells.so is missing: run build() of __graft_entry__.py first"
    so = ctypes.CDLL(SO)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    so.dkc_table_build.argtypes = [vp, u32, u32, vp, u32, vp]
    so.dkc_gather.argtypes = [vp, vp, u32, u32, u32, vp]
    so.dkc_transpose.argtypes = [vp, vp, u32, u32, u32, vp]
    so.dkc_ntt.argtypes = [vp, vp, u32, u64, u32, vp]
    so.dkc_mulacc.argtypes = [vp, vp, vp, u64, vp, u64, u32, u32, u64, u32, vp]
    so.dkc_reduce.argtypes = [vp, vp, u64, u32, u64, u32]
    so.dkc_set_slices.argtypes = [vp, u64]
    return so


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, KEY_POINTS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def domains(ctx):
    import plonk_amd
    made = {}

    def get(log_n):
        if log_n not in made:
            made[log_n] = plonk_amd.KzgDomain(ctx, log_n)
        return made[log_n]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def big():
    """a context with 2^16 key points for the handles of log_n 14 and 16"""
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, 1 << 16)
    yield c
    c.close()


def proof48(f, log_n, log_cell, k, tau=K.TAU):
    return K.scalar_commit(M.proof_closed_form(f, log_n, log_cell, k, tau))


def check_all(dom, polys, log_cell, tau=K.TAU, proofs_at=None, cells_at=None):
    """every (or the listed) proof and cell of every polynomial against the closed form, the commitments too"""
    cells, proofs, cm = dom.open_cells(polys, log_cell)
    l, r = 1 << log_cell, dom.n >> log_cell
    w = M.root(dom.log_n)
    for j, f in enumerate(polys):
        assert cm[j] == K.commit(f, tau), j
        for k in (range(r) if proofs_at is None else proofs_at):
            assert proofs[j][k] == proof48(f, dom.log_n, log_cell, k, tau), (j, k)
        for k in (range(r) if cells_at is None else cells_at):
            assert cells[j][k] == [K.evaluate(f, pow(w, k + r * i, Q)) for i in range(l)], (j, k)
    return cells, proofs, cm


def assert_last(dom, log_cell, count, cap=M.WS_CAP_DEFAULT, forced=0):
    last, p = dom.cells_last(), M.plan(dom.log_n, log_cell, count, cap, forced)
    assert (last["log_n"], last["log_cell"], last["count"]) == (dom.log_n, log_cell, count)
    assert (last["slices"], last["chunks"], last["chunk_polys"], last["workspace_bytes"], last["stage_launches"], last["scalar_muls"]) == \
        (p["slices"], p["chunks"], p["chunk_polys"], p["ws_bytes"], p["stage_launches"], p["scalar_muls"])
    assert last["table_bytes"] >= p["table_bytes"] and last["table_bytes"] % p["table_bytes"] == 0
    return last


def shaped(log_n, log_cell):
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    x, _ = M.cell_points(log_n, log_cell)
    out = [[0] * (u + l * t) + [1] for u in (0, l - 1) for t in (0, r - 1)]           # one coefficient at u + l t
    out += [[(-x[k]) % Q] + [0] * (l - 1) + [1] for k in sorted({0, 1, r - 1})]       # X^l - x_k
    return out


# ---- small sizes: everything against the closed form ------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_cell", [(a, b) for a in (2, 3, 4, 6) for b in range(1, a)])
def test_small_sizes_every_proof_cell_and_commitment(domains, log_n, log_cell):
    dom, n, l, r = domains(log_n), 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(100 * log_n + log_cell)
    lengths = sorted({0, 1, l - 1, l, l + 1, n - 1, n})
    polys = [[rnd.randrange(1, Q) for _ in range(m)] for m in lengths]
    cells, proofs, cm = check_all(dom, polys, log_cell)
    assert_last(dom, log_cell, len(polys))
    for j, m in enumerate(lengths):
        if m <= l:
            assert proofs[j] == [ID48] * r                     # f shorter than l + 1: f is its own remainder on every cell
    assert cm[0] == ID48 and cells[0] == [[0] * l] * r
    assert dom.cell_points(log_cell) == M.cell_points(log_n, log_cell)
    assert dom.open_cells(polys, log_cell, commitments=False) == (cells, proofs, None)
    # shaped polynomials: single coefficients in the corners of the l x r matrix, and f = X^l - x_k
    sh = shaped(log_n, log_cell)
    cells, proofs, cm = check_all(dom, sh, log_cell)
    for i, k in enumerate(sorted({0, 1, r - 1})):
        assert proofs[4 + i][k] == K.scalar_commit(1) and cells[4 + i][k] == [0] * l


@pytest.mark.parametrize("log_n", [3, 4])
def test_degenerate_key(log_n):
    """tau = (2n-th root of unity)^3: the key's points repeat with period 2n and tau^n = -1, so identities, equal and opposite
    points enter every stage; (tau^l)^r = -1 while x_k^r = 1, so no tau^l - x_k vanishes and the closed form holds"""
    import plonk_amd
    n = 1 << log_n
    tau = pow(M.root(log_n + 1), 3, Q)
    assert pow(tau, n, Q) == Q - 1
    c = plonk_amd.Context(0)
    load_key(c, n, tau)
    dom = plonk_amd.KzgDomain(c, log_n)
    rnd = random.Random(log_n)
    polys = [[rnd.randrange(Q) for _ in range(n)], [1] * n, [0] * (n - 1) + [1], [3, 1]]
    for log_cell in range(1, log_n):
        x, _ = M.cell_points(log_n, log_cell)
        assert all((pow(tau, 1 << log_cell, Q) - xk) % Q for xk in x)
        check_all(dom, polys, log_cell, tau)
    dom.close()
    c.close()


# ---- the kernels on their own -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(fft_lib):  # noqa: F811
    r = Rig(fft_lib)
    yield r
    r.close()


@pytest.mark.parametrize("log_n,log_cell,slices", [(6, 3, 1), (6, 3, 2), (6, 3, 4), (6, 3, 8), (3, 2, 2), (6, 1, 2), (7, 1, 1)])
def test_mulacc_and_reduce_kernels_against_the_model(rig, doors, log_n, log_cell, slices):
    """2r = 16 positions with S = 1, 2, l / 2 and l; 2r = 4 (less than a wave), 64 (exactly one) and 128 (two); two polynomials;
    scalars G = 0 and table entries O among the operands; guard and pad slots around the partials"""
    P = rig.P
    n, l, r = 1 << log_n, 1 << log_cell, 1 << (log_n - log_cell)
    size, batch = 2 * r, 2
    rnd = random.Random(1000 * log_n + 10 * log_cell + slices)
    table = [rnd.randrange(1, Q) for _ in range(2 * n)]
    G = [[rnd.randrange(1, Q) for _ in range(2 * n)] for _ in range(batch)]
    for _ in range(max(n // 4, 2)):                            # zeros and identities, some of them meeting
        table[rnd.randrange(2 * n)] = 0
        G[rnd.randrange(batch)][rnd.randrange(2 * n)] = 0
    G[1][0:size] = [0] * size                                  # a whole term of polynomial 1 multiplies nothing
    scale = pow(size, -1, Q)
    tbuf, _ = rig.points([table], log_n + 1)                   # 2n contiguous slots with known logs behind GUARD slots
    gbuf = rig.ctx.alloc(32 * 2 * n * batch)
    gbuf.upload(b"".join(P.fr_to_bytes_mont(row) for row in G))
    stride = slices * size + PAD
    ws = rig.ctx.alloc(SLOT * (2 * GUARD + batch * stride))
    ws.upload(b"\xA5" * ws.nbytes)
    rc = doors.dkc_mulacc(rig.h, tbuf.ptr + SLOT * GUARD, gbuf.ptr, 2 * n, ws.ptr + SLOT * GUARD, stride, log_n, log_cell, slices, batch,
                          P.fr_to_bytes_mont([scale]))
    assert rc == 0
    want = [M.mulacc(table, G[b], log_n, log_cell, slices, scale) for b in range(batch)]
    slot_log = (slices * size).bit_length() - 1
    got = rig.read48(ws, stride, 0, slot_log, batch, False)
    for b in range(batch):
        assert got[b] == [gmul48(x) for x in want[b]], b
    rig.guards_untouched(ws, stride, slices * size, batch)
    assert doors.dkc_reduce(rig.h, ws.ptr + SLOT * GUARD, stride, log_n - log_cell, slices, batch) == 0
    after = rig.read48(ws, stride, 0, slot_log, batch, False)
    for b in range(batch):
        red = M.reduce(want[b], r, slices)
        assert after[b][:size] == [gmul48(x) for x in red[:size]], b
        assert after[b][size:] == got[b][size:], b             # the other partials stay
    rig.guards_untouched(ws, stride, slices * size, batch)
    # arguments the launcher refuses
    assert doors.dkc_mulacc(rig.h, tbuf.ptr, gbuf.ptr, 2 * n, ws.ptr, stride, log_n, log_cell, 3, batch, P.fr_to_bytes_mont([1])) == ERR_ARG
    assert doors.dkc_mulacc(rig.h, tbuf.ptr, gbuf.ptr, 2 * n, ws.ptr, slices * size - 1, log_n, log_cell, slices, batch,
                            P.fr_to_bytes_mont([1])) == ERR_ARG
    for b in (tbuf, gbuf, ws):
        b.free()


@pytest.mark.parametrize("log_cell", [1, 4])
def test_tables_against_the_group_dft(ctx, doors, fft_lib, log_cell):  # noqa: F811
    """A^(u) at log_n 5 from the context's key: slot u * 2r + p = [g DFT_2r(a^(u))_rev(p)] G"""
    log_n = 5
    n, l, r = 32, 1 << log_cell, 32 >> log_cell
    size, LR = 2 * r, log_n - log_cell + 1
    tw = ctypes.c_void_p()
    assert fft_lib.dkd_twiddles(ctx.handle, log_n + 1, ctypes.byref(tw)) == 0
    table = ctx.alloc(SLOT * (2 * n + 2))
    table.upload(b"\xA5" * table.nbytes)
    assert doors.dkc_table_build(ctx.handle, log_n, log_cell, tw, log_n + 1, table.ptr + SLOT) == 0
    out = ctx.alloc(48 * 2 * n)
    assert fft_lib.dkd_finish(ctx.handle, table.ptr + SLOT, 2 * n, 0, log_n + 1, 1, 0, out.ptr) == 0
    raw = out.download()
    key = [pow(K.TAU, i, Q) for i in range(n)]
    w = M.root(LR)
    for u in range(l):
        a = [key[u + l * v] if v <= r - 2 else 0 for v in range(size)]
        want = D.dft(a, w)
        for p in range(size):
            at = u * size + p
            assert raw[48 * at:48 * at + 48] == K.scalar_commit(want[M.rev(p, LR)]), (u, p)
    guard = table.download()
    assert guard[:SLOT] == b"\xA5" * SLOT and guard[-SLOT:] == b"\xA5" * SLOT
    assert doors.dkc_table_build(ctx.handle, log_n, 5, tw, log_n + 1, table.ptr + SLOT) == ERR_ARG
    fft_lib.dkd_free(ctx.handle, tw)
    table.free()
    out.free()


def test_gather_and_transpose_kernels(ctx, doors):
    import plonk_amd
    log_n, log_cell, batch = 6, 2, 2
    n, l, r = 64, 4, 16
    rnd = random.Random(5)
    f = [[rnd.randrange(Q) for _ in range(n)] for _ in range(batch)]
    src = ctx.alloc(32 * n * batch)
    src.upload(b"".join(plonk_amd.fr_to_bytes_mont(row) for row in f))
    g = ctx.alloc(32 * (2 * n * batch + 2))
    g.upload(b"\xA5" * g.nbytes)
    assert doors.dkc_gather(ctx.handle, src.ptr, log_n, log_cell, batch, g.ptr + 32) == 0
    raw = g.download()
    assert raw[:32] == b"\xA5" * 32 and raw[-32:] == b"\xA5" * 32
    assert plonk_amd.fr_from_bytes_mont(raw[32:-32]) == M.gathered(f[0], log_n, log_cell) + M.gathered(f[1], log_n, log_cell)
    t = ctx.alloc(32 * (n * batch + 2))
    t.upload(b"\xA5" * t.nbytes)
    assert doors.dkc_transpose(ctx.handle, src.ptr, log_n, log_cell, batch, t.ptr + 32) == 0
    raw = t.download()
    assert raw[:32] == b"\xA5" * 32 and raw[-32:] == b"\xA5" * 32
    got = plonk_amd.fr_from_bytes_mont(raw[32:-32])
    for b in range(batch):
        for i in range(n):
            assert got[b * n + M.cell_dst(log_n, log_cell, i)] == f[b][i]
    for b in (src, g, t):
        b.free()


@pytest.mark.parametrize("log_size", [1, 2, 6, 9, 11])
def test_batched_scalar_ntt_kernel(ctx, doors, log_size):
    """kzc_ntt_kernel: 3 x 2 vectors in one launch against the NTT of the C oracle (the definition at the smallest sizes);
    fewer elements than lanes, exactly 256 butterflies (2^9) and the largest size it takes"""
    import plonk_amd
    from oracle import cbind
    size, vectors, batch = 1 << log_size, 3, 2
    rnd = random.Random(log_size)
    raws = []
    for _ in range(vectors * batch):
        raw = bytearray(rnd.randbytes(32 * size))
        for i in range(31, 32 * size, 32):
            raw[i] &= 0x3F
        raws.append(bytes(raw))
    raws[1] = bytes(32 * size)                                  # a zero vector
    w = M.root(log_size)
    tw = ctx.alloc(32 * max(size // 2, 1))
    tw.upload(plonk_amd.fr_to_bytes_mont([pow(w, e, Q) for e in range(size // 2)]))
    g = ctx.alloc(32 * (size * vectors * batch + 2))
    g.upload(b"\xA5" * 32 + b"".join(raws) + b"\xA5" * 32)
    assert doors.dkc_ntt(ctx.handle, g.ptr + 32, log_size, vectors, batch, tw.ptr) == 0
    out = g.download()
    assert out[:32] == b"\xA5" * 32 and out[-32:] == b"\xA5" * 32
    for k, raw in enumerate(raws):
        got = out[32 + 32 * size * k:32 + 32 * size * (k + 1)]
        if log_size <= 6:
            assert plonk_amd.fr_from_bytes_mont(got) == D.dft(plonk_amd.fr_from_bytes_mont(raw), w), k
        else:
            assert got == cbind.ntt_bytes(raw, log_size, False, False, size), k
    assert doors.dkc_ntt(ctx.handle, g.ptr + 32, 12, vectors, batch, tw.ptr) == ERR_ARG
    assert doors.dkc_ntt(ctx.handle, g.ptr + 32, 0, vectors, batch, tw.ptr) == ERR_ARG
    tw.free()
    g.free()


# ---- n = 2^12 against plonk_kzg_open_domain ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run4096(domains):
    import plonk_amd
    dom, n = domains(12), 1 << 12
    rnd = random.Random(12)
    raws = []
    for m in (n, n - 5):
        raw = bytearray(rnd.randbytes(32 * m))
        for i in range(31, 32 * m, 32):
            raw[i] &= 0x3F
        raws.append(bytes(raw))
    polys = [plonk_amd.fr_from_bytes_mont(r) for r in raws]
    before = dom.last()
    out = dom.open_cells_bytes(raws, 6)
    return {"raws": raws, "polys": polys, "out": out, "last": dom.cells_last(), "domain_last_before": before, "domain_last_after": dom.last()}


def test_4096_points_cells_of_64(domains, run4096):
    import plonk_amd
    dom, n, l, r = domains(12), 1 << 12, 64, 64
    cells, proofs, cm = run4096["out"]
    p = M.plan(12, 6, 2)
    last = run4096["last"]
    assert (last["slices"], last["chunks"], last["chunk_polys"], last["workspace_bytes"], last["stage_launches"], last["scalar_muls"], last["count"]) == \
        (p["slices"], p["chunks"], p["chunk_polys"], p["ws_bytes"], p["stage_launches"], p["scalar_muls"], 2)
    assert run4096["domain_last_before"] == run4096["domain_last_after"]
    for j, f in enumerate(run4096["polys"]):
        for k in range(r):
            assert proofs[48 * (j * r + k):48 * (j * r + k + 1)] == proof48(f, 12, 6, k), (j, k)
    ev, _, cm2 = dom.open_bytes(run4096["raws"])
    assert cm == cm2
    for j in range(2):
        for k in range(r):
            want = b"".join(ev[32 * (j * n + k + r * i):32 * (j * n + k + r * i + 1)] for i in range(l))
            assert cells[32 * (j * n + k * l):32 * (j * n + (k + 1) * l)] == want, (j, k)


# ---- the looped table build, the longest transforms ------------------------------------------------------------------------
def test_16384_points_two_cells_of_8192_and_8192_cells_of_two(big):
    """log_cell 13: r = 2 and l = 8192 > the 4096 polynomials a batched transform takes, so the table build loops;
    log_cell 1: r = 8192"""
    import plonk_amd
    log_n, n = 14, 1 << 14
    dom = plonk_amd.KzgDomain(big, log_n)
    rnd = random.Random(14)
    f = [rnd.randrange(Q) for _ in range(n)]
    cells, proofs, cm = dom.open_cells([f], 13)
    assert cm[0] == K.commit(f) and proofs[0] == [proof48(f, log_n, 13, k) for k in range(2)]
    assert dom.cells_last()["built_table"] == 1 and dom.cells_last()["table_bytes"] == 2 * n * 256
    w = M.root(log_n)
    assert [cells[0][1][i] for i in (0, 1, 8191)] == [K.evaluate(f, pow(w, 1 + 2 * i, Q)) for i in (0, 1, 8191)]
    cells, proofs, cm = dom.open_cells([f], 1)
    idx = [0, 1, 4096, 8191] + rnd.sample(range(2, 8191), 4)
    assert [proofs[0][k] for k in idx] == [proof48(f, log_n, 1, k) for k in idx]
    assert dom.cells_last()["table_bytes"] == 2 * (2 * n * 256)
    assert_last(dom, 1, 1)
    dom.close()


def test_65536_points_cells_of_64_sampled(big):
    import plonk_amd
    log_n, n, l, r = 16, 1 << 16, 64, 1 << 10
    dom = plonk_amd.KzgDomain(big, log_n)
    rnd = random.Random(16)
    raw = bytearray(rnd.randbytes(32 * n))
    for i in range(31, 32 * n, 32):
        raw[i] &= 0x3F
    f = plonk_amd.fr_from_bytes_mont(bytes(raw))
    cells, proofs, cm = dom.open_cells_bytes([bytes(raw)], 6)
    assert_last(dom, 6, 1)
    assert cm == K.commit(f)
    for k in [0, 1, r // 2, r - 1] + rnd.sample(range(2, r - 1), 12):
        assert proofs[48 * k:48 * k + 48] == proof48(f, log_n, 6, k), k
    w = M.root(log_n)
    for k in [0, r - 1] + rnd.sample(range(1, r - 1), 2):
        got = plonk_amd.fr_from_bytes_mont(cells[32 * k * l:32 * (k + 1) * l])
        assert [got[i] for i in (0, 1, l - 1)] == [K.evaluate(f, pow(w, k + r * i, Q)) for i in (0, 1, l - 1)], k
    dom.close()


# ---- a real pairing ---------------------------------------------------------------------------------------------------------
def cell_key(l, tau=K.TAU):
    """g || h || [tau^l] h: the opening key a verifier of cells of l values holds"""
    return E.g1_compress(K.g_point()) + G2.g2_compress(G2.G2_GEN) + G2.g2_compress(G2.g2_mul(G2.G2_GEN, pow(tau, l, Q)))


def verifier_b(log_n, log_cell, k, values, proof, commitment, x_k):
    """B = C - commit(r_k) + x_k proof_k from the device's bytes; r_k from the cell's values by the inverse-NTT formula"""
    c = M.remainder_from_cell(values, log_n, log_cell, k)
    commit_r = E.g1_decompress(K.scalar_commit(M.evaluate(c, K.TAU)))          # sum_j c_j s_j on the known-tau key
    b = E.g1_add(E.g1_decompress(commitment), E.g1_mul(commit_r, Q - 1) if commit_r is not None else None)
    pk = E.g1_decompress(proof)
    return E.g1_compress(E.g1_add(b, E.g1_mul(pk, x_k) if pk is not None else None))


@pytest.mark.parametrize("log_n,log_cell,sampled", [(6, 3, None), (12, 6, 8)])
def test_cells_verify_in_a_real_pairing(ctx, domains, log_n, log_cell, sampled):
    import plonk_amd
    dom, l, r = domains(log_n), 1 << log_cell, 1 << (log_n - log_cell)
    rnd = random.Random(log_n)
    f = [rnd.randrange(Q) for _ in range(dom.n)]
    cells, proofs, cm = dom.open_cells([f], log_cell)
    x, _ = dom.cell_points(log_cell)
    ks = list(range(r)) if sampled is None else [0, r - 1] + rnd.sample(range(1, r - 1), sampled - 2)
    key = plonk_amd.KzgKey(ctx, cell_key(l))
    a = [proofs[0][k] for k in ks]
    b = [verifier_b(log_n, log_cell, k, cells[0][k], proofs[0][k], cm[0], x[k]) for k in ks]
    assert key.pairing_check_each(a, b) == [OK] * len(ks)
    # one value of one cell flipped: that item alone is rejected
    bad = list(cells[0][ks[1]])
    bad[l - 1] = (bad[l - 1] + 1) % Q
    b2 = list(b)
    b2[1] = verifier_b(log_n, log_cell, ks[1], bad, proofs[0][ks[1]], cm[0], x[ks[1]])
    assert key.pairing_check_each(a, b2) == [OK, ERR_VERIFY] + [OK] * (len(ks) - 2)
    # the proof of the neighbouring cell in place of the cell's own
    other = proofs[0][(ks[2] + 1) % r]
    a3, b3 = list(a), list(b)
    a3[2] = other
    b3[2] = verifier_b(log_n, log_cell, ks[2], cells[0][ks[2]], other, cm[0], x[ks[2]])
    assert key.pairing_check_each(a3, b3) == [OK, OK, ERR_VERIFY] + [OK] * (len(ks) - 3)
    key.close()


# ---- chunking, slices, the resident form, two cell sizes ---------------------------------------------------------------------
def test_forced_chunking_and_forced_slices_give_the_same_bytes(domains, doors):
    import plonk_amd
    dom, n, log_cell = domains(6), 64, 3
    r = 8
    rnd = random.Random(6)
    raws = [plonk_amd.fr_to_bytes_mont([rnd.randrange(Q) for _ in range(m)]) for m in (64, 10, 0, 63, 64)]
    whole = dom.open_cells_bytes(raws, log_cell)
    last = assert_last(dom, log_cell, 5)
    assert last["chunks"] == 1
    per = last["slices"] * 2 * r * 256
    try:
        dom._set_workspace_cap(2 * per)
        assert dom.open_cells_bytes(raws, log_cell) == whole
        last = assert_last(dom, log_cell, 5, 2 * per)
        assert (last["chunks"], last["chunk_polys"]) == (3, 2)
        dom._set_workspace_cap(1)                              # below one polynomial: a one-polynomial chunk is always allowed
        assert dom.open_cells_bytes(raws, log_cell) == whole
        assert assert_last(dom, log_cell, 5, 1)["chunks"] == 5
    finally:
        dom._set_workspace_cap(0)
    try:
        for S in (1, 2, 4, 8):
            assert doors.dkc_set_slices(dom.handle, S) == 0
            assert dom.open_cells_bytes(raws, log_cell) == whole, S
            assert assert_last(dom, log_cell, 5, forced=S)["slices"] == S
    finally:
        doors.dkc_set_slices(dom.handle, 0)
    assert dom.open_cells_bytes(raws, log_cell) == whole
    assert_last(dom, log_cell, 5)


def test_resident_form_gives_the_bytes_of_the_host_form(ctx, domains):
    import plonk_amd
    dom, n, log_cell = domains(6), 64, 2
    r = n >> log_cell
    rnd = random.Random(66)
    lens = [64, 0, 5, 64, 1]
    raws = [plonk_amd.fr_to_bytes_mont([rnd.randrange(Q) for _ in range(m)]) for m in lens]
    raws[2] += bytes(32 * 100)                                  # trailing zeros beyond n: trimmed length 5
    whole = dom.open_cells_bytes(raws, log_cell)
    bufs = []
    for raw in raws:
        b = ctx.alloc(max(len(raw), 32))
        b.upload(raw)
        bufs.append(b)
    count = len(raws)
    cells, proofs, cm = ctx.alloc(32 * n * count), ctx.alloc(48 * r * count), ctx.alloc(48 * count)
    dom.open_cells_dev([b.ptr for b in bufs], [len(x) // 32 for x in raws], log_cell, cells.ptr, proofs.ptr, cm.ptr)
    assert (cells.download(), proofs.download(), cm.download()) == whole
    assert_last(dom, log_cell, count)
    # errors of the resident form leave the outputs untouched
    for b in (cells, proofs, cm):
        b.upload(b"\xA5" * b.nbytes)
    bad = ctx.alloc(32 * 65)
    bad.upload(plonk_amd.fr_to_bytes_mont([1] * 65))
    with pytest.raises(plonk_amd.PolynomialDegreeTooLarge):
        dom.open_cells_dev([bufs[0].ptr, bad.ptr], [64, 65], log_cell, cells.ptr, proofs.ptr, cm.ptr)
    bad.upload(b"\xff" * 32, offset=32 * 3)
    with pytest.raises(plonk_amd.PlonkError) as ei:
        dom.open_cells_dev([bufs[0].ptr, bad.ptr], [64, 64], log_cell, cells.ptr, proofs.ptr, cm.ptr)
    assert ei.value.code == ERR_DATA
    for b in (cells, proofs, cm):
        assert b.download() == b"\xA5" * b.nbytes
    for b in bufs + [cells, proofs, cm, bad]:
        b.free()


def test_two_cell_sizes_alternate_and_the_other_entry_points_keep_their_bytes(ctx):
    import plonk_amd
    dom, n = plonk_amd.KzgDomain(ctx, 6), 64
    rnd = random.Random(77)
    polys = [[rnd.randrange(Q) for _ in range(64)], [rnd.randrange(Q) for _ in range(33)]]
    z = rnd.randrange(Q)
    opened = dom.open(polys)
    info = dom.last()
    evals = dom.open_evals([opened[0][0]], z)
    evals_info = dom.evals_last()
    assert dom.cells_last() == dict.fromkeys(dom.cells_last(), 0) | {"log_n": 6}        # before the first call
    a = dom.open_cells(polys, 2)
    assert (dom.cells_last()["built_table"], dom.cells_last()["table_bytes"]) == (1, 2 * n * 256)
    b = dom.open_cells(polys, 4)
    assert (dom.cells_last()["built_table"], dom.cells_last()["table_bytes"]) == (1, 2 * 2 * n * 256)
    for _ in range(2):
        assert dom.open_cells(polys, 2) == a and dom.cells_last()["built_table"] == 0
        assert dom.open_cells(polys, 4) == b and dom.cells_last()["built_table"] == 0
    assert dom.cells_last()["table_bytes"] == 2 * 2 * n * 256
    check_all(dom, polys, 2)
    assert dom.last() == info and dom.evals_last() == evals_info
    assert dom.open(polys) == opened and dom.last() == info
    assert dom.open_evals([opened[0][0]], z) == evals
    dom.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(ctx, domains):
    import plonk_amd
    dom, n, log_cell = domains(3), 8, 1
    r = 4
    lib = ctx.lib
    mont = plonk_amd.fr_to_bytes_mont
    good, long_, noncanon = mont([1] * 8), mont([1] * 9), mont([1, 2]) + b"\xff" * 32 + mont([3])
    cells = ctypes.create_string_buffer(b"\xA5" * (32 * n * 2), 32 * n * 2)
    proofs = ctypes.create_string_buffer(b"\xA5" * (48 * r * 2), 48 * r * 2)
    cm = ctypes.create_string_buffer(b"\xA5" * 96, 96)

    def call(bufs, count=None, h=dom.handle, c=cells, p=proofs, lc=log_cell):
        keep = [ctypes.create_string_buffer(b, len(b)) for b in bufs]
        parr = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.cast(k, ctypes.c_void_p).value for k in keep])
        larr = (ctypes.c_uint64 * max(len(bufs), 1))(*[len(b) // 32 for b in bufs])
        return lib.plonk_kzg_open_cells(h, lc, parr, larr, len(bufs) if count is None else count, c, p, cm)

    assert call([good, long_]) == ERR_DEGREE
    assert call([good, noncanon]) == ERR_DATA
    assert call([long_, noncanon]) == ERR_DATA                  # the canonical-form check comes first
    assert call([good], count=65537) == ERR_ARG
    assert call([good], h=None) == ERR_ARG
    assert call([good], c=None) == ERR_ARG
    assert call([good], p=None) == ERR_ARG
    for lc in (0, 3, 4, 64, 0xffffffff):
        assert call([good], lc=lc) == ERR_ARG
        assert call([], count=0, lc=lc) == ERR_ARG
    assert call([], count=0) == OK                              # count == 0 writes nothing
    assert cells.raw == b"\xA5" * len(cells.raw) and proofs.raw == b"\xA5" * len(proofs.raw) and cm.raw == b"\xA5" * 96
    x = ctypes.create_string_buffer(b"\xA5" * (32 * r), 32 * r)
    info = plonk_amd._KzgCellsInfo()
    assert lib.plonk_kzg_cell_points(dom.handle, log_cell, None, None) == ERR_ARG
    assert lib.plonk_kzg_cell_points(None, log_cell, x, None) == ERR_ARG
    assert lib.plonk_kzg_cell_points(dom.handle, 3, x, None) == ERR_ARG and x.raw == b"\xA5" * (32 * r)
    assert lib.plonk_kzg_cell_points(dom.handle, log_cell, x, None) == OK
    assert plonk_amd.fr_from_bytes_mont(x.raw) == M.cell_points(3, log_cell)[0]
    assert lib.plonk_kzg_cells_last(dom.handle, None) == ERR_ARG and lib.plonk_kzg_cells_last(None, ctypes.byref(info)) == ERR_ARG
    assert call([good, mont([0] * 20)]) == OK                   # twenty zeros trim to the zero polynomial
    assert proofs.raw[48 * r:] == ID48 * r and cm.raw[48:] == ID48 and cells.raw[32 * n:] == bytes(32 * n)
    # a handle of log_n = 1 has no cell size at all
    d1 = domains(1)
    for lc in (0, 1, 2):
        assert call([mont([1, 2])], h=d1.handle, lc=lc) == ERR_ARG


def test_state_errors_reloaded_key_and_communicator():
    import plonk_amd
    c = plonk_amd.Context(0)
    load_key(c, 16)
    d = plonk_amd.KzgDomain(c, 3)
    before = d.open_cells([[1, 2, 3, 4, 5]], 1)
    c.comm_init(plonk_amd.Context.comm_unique_id(), 0, 1)       # a communicator: the context holds only a range of the key
    with pytest.raises(plonk_amd.PlonkError) as ei:
        d.open_cells([[1, 2, 3, 4, 5]], 1)
    assert ei.value.code == ERR_STATE
    c.comm_destroy()
    assert d.open_cells([[1, 2, 3, 4, 5]], 1) == before
    load_key(c, 16)                                             # the same key again: still another generation
    for call in (lambda: d.open_cells([[1, 2, 3, 4, 5]], 1), lambda: d.cell_points(1), d.cells_last, lambda: d.open_cells([], 1)):
        with pytest.raises(plonk_amd.PlonkError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    d.close()
    d2 = plonk_amd.KzgDomain(c, 3)
    assert d2.open_cells([[1, 2, 3, 4, 5]], 1) == before
    d2.close()
    c.close()


def test_context_left_as_found():
    """a proof and an opening made on the same context before and after a cell call are byte-identical; the tables stay"""
    import plonk_amd
    from tests import circuits as C
    c = plonk_amd.Context(0)
    comp = C.big_widget_circuit(1 << 10, seed=78)()
    case = C.compile_fast(comp, b"kzg-cells")
    srs = C.synthetic_srs(case["size"] + 7)
    c.srs_load_bytes(srs, len(srs) // 96)
    cols = C.circuit_columns(comp)
    prover = plonk_amd.Prover.compile(c, b"kzg-cells", cols["selectors"], cols["wires"], cols["witnesses"])
    rnd = random.Random(77)
    f = [rnd.randrange(Q) for _ in range(300)]
    z, v = rnd.randrange(Q), rnd.randrange(Q)
    proof = prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3))
    opening = c.kzg_open([f, f[:7]], z, v)
    tables, rows = c.table_bytes(), c.table_rows()
    dom = plonk_amd.KzgDomain(c, 6)
    check_all(dom, [[rnd.randrange(Q) for _ in range(64)], [4, 5, 6]], 3, proofs_at=[0, 1, 7], cells_at=[0, 7])
    assert prover.prove_witnesses(cols["values"], case["pi"], C.blinders(3)) == proof
    assert c.kzg_open([f, f[:7]], z, v) == opening
    assert (c.table_bytes(), c.table_rows()) == (tables, rows)
    dom.close()
    prover.close()
    c.close()
