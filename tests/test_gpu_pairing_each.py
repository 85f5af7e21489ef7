"""GPU: one pairing check per lane (plonk_kzg_pairing_check_each; pairing.hip, pairing28.cuh).  The device value of
e(-A, x_h) e(B, h) equals the host pairing's bit for bit; the verdicts are right at every position of a wave and across waves,
for the identity placements and for points that do not decode; the ladder use finds the corrupted point of a commit key."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from oracle import bls12_381 as E
from tests import circuits as C
from tests import kzg_ref as K

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g2_ref as G2   # noqa: E402

pytestmark = pytest.mark.gpu
Q, P = E.Q, E.P
OK, ERR_ARG, ERR_POINT, ERR_VERIFY = 0, -1, -10, -12
ID48 = K.IDENTITY48
HERE = os.path.dirname(os.path.abspath(__file__))
H96 = G2.g2_compress(G2.G2_GEN)
XH96 = G2.g2_compress(G2.g2_mul(G2.G2_GEN, K.TAU))


@pytest.fixture(scope="module")
def ctx():
    import plonk_amd
    c = plonk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key(ctx):
    import plonk_amd
    k = plonk_amd.KzgKey(ctx, K.opening_key())
    yield k
    k.close()


@pytest.fixture(scope="module")
def host():
    """the CPU harness of the host pairing (tests/csrc/host_verify.cpp), built as tests/test_verify_host.py builds it"""
    so = os.path.join(HERE, "_build", "libhost_verify.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_verify.cpp")
    csrc = os.path.join(HERE, "..", "plonk_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.hv_multi_pairing.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p]
    return lib


def g(s):
    """48 bytes of [s] g for the opening key's g (the identity for s = 0 mod q)"""
    return K.scalar_commit(s % Q)


def honest(rnd, count):
    rs = [rnd.randrange(1, Q) for _ in range(count)]
    return rs, [g(r) for r in rs], [g(r * K.TAU) for r in rs]


def test_device_values_equal_the_host_pairing_bit_for_bit(key, host):
    rnd = random.Random(2901)
    ra, rb = [rnd.randrange(1, Q) for _ in range(3)], [rnd.randrange(1, Q) for _ in range(3)]
    rb[1] = ra[1] * K.TAU % Q                                             # one check that holds
    a, b = [g(r) for r in ra], [g(r) for r in rb]
    got = key._pairing_each_values(a, b)
    for k in range(3):
        out = (ctypes.c_uint64 * 72)()
        assert host.hv_multi_pairing(2, g(-ra[k]) + b[k], XH96 + H96, out) == 0
        want = [sum(int(out[6 * i + j]) << (64 * j) for j in range(6)) for i in range(12)]
        assert got[k] == want
        assert (want == [1] + [0] * 11) == (k == 1)


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 129])
def test_verdicts_at_every_position_of_a_wave_and_across_waves(key, count):
    rnd = random.Random(2910 + count)
    rs, a, b = honest(rnd, count)
    verdicts, info = key.pairing_check_each_info(a, b)
    assert verdicts == [OK] * count
    assert info["proofs"] == count and info["pairing_checks"] == count and info["msm_terms"] == 0 and info["rejected"] == 0
    bad = sorted({p for p in (0, 63, 64, count - 1) if p < count})
    if count == 2:
        bad = [1]                                                         # a good item next to a bad one
    for i, p in enumerate(bad):
        b[p] = g(rs[p] * K.TAU + 1) if i % 2 == 0 else g(-rs[p] * K.TAU)  # B + g, and -B
    verdicts, info = key.pairing_check_each_info(a, b)
    assert verdicts == [ERR_VERIFY if k in bad else OK for k in range(count)]
    assert info["pairing_checks"] == count and info["rejected"] == len(bad)


def bad_points():
    """(48 bytes that are no point of the curve, 48 bytes of a curve point outside the prime-order subgroup)"""
    x = 1
    while pow((x ** 3 + 4) % P, (P - 1) // 2, P) == 1:
        x += 1
    off = bytearray(x.to_bytes(48, "big"))
    off[0] |= 0x80
    x = 5
    while True:
        y2 = (x ** 3 + 4) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2 and E.g1_add(E.g1_mul((x, y), Q - 1), (x, y)) is not None:   # [q] P != O (g1_mul reduces mod q)
            return bytes(off), E.g1_compress((x, y))
        x += 1


def test_identity_placements_and_points_that_do_not_decode(ctx, key):
    rnd = random.Random(2920)
    rs, a, b = honest(rnd, 7)
    off_curve, off_group = bad_points()
    a[0], b[0] = ID48, ID48              # (O, O) passes
    a[1] = ID48                          # (O, B != O) fails
    b[2] = ID48                          # (A != O, O) fails
    a[4] = off_curve
    b[5] = off_group
    verdicts, info = key.pairing_check_each_info(a, b)
    assert verdicts == [OK, ERR_VERIFY, ERR_VERIFY, OK, ERR_POINT, ERR_POINT, OK]
    assert info["pairing_checks"] == 5 and info["rejected"] == 4 and info["proofs"] == 7
    # argument errors
    lib = ctx.lib
    v = (ctypes.c_int32 * 7)()
    ab = b"".join(a[:1]), b"".join(b[:1])
    assert lib.plonk_kzg_pairing_check_each(None, ab[0], ab[1], 1, v, None) == ERR_ARG
    assert lib.plonk_kzg_pairing_check_each(key.handle, None, ab[1], 1, v, None) == ERR_ARG
    assert lib.plonk_kzg_pairing_check_each(key.handle, ab[0], None, 1, v, None) == ERR_ARG
    assert lib.plonk_kzg_pairing_check_each(key.handle, ab[0], ab[1], 1, None, None) == ERR_ARG
    assert lib.plonk_kzg_pairing_check_each(key.handle, ab[0], ab[1], 0, v, None) == ERR_ARG
    assert lib.plonk_kzg_pairing_check_each(key.handle, ab[0], ab[1], (1 << 24) + 1, v, None) == ERR_ARG
    assert lib.plonk_kzg_pairing_check_each(key.handle, ab[0], ab[1], 1, v, None) == OK and v[0] == OK


def test_the_ladder_finds_the_corrupted_point_of_a_commit_key(key):
    """consecutive points of a powers-of-tau key: e(P_i, x_h) == e(P_(i + 1), h); one point replaced by another point of the
    subgroup breaks exactly the two pairs that touch it"""
    n = 1 << 6
    srs = C.synthetic_srs(n)
    pts = [E.g1_compress(E.g1_from_raw96(srs[96 * i:96 * i + 96])) for i in range(n)]
    assert pts[0] == g(1) and pts[1] == g(K.TAU)
    assert key.pairing_check_each(pts[:-1], pts[1:]) == [OK] * (n - 1)
    for i in (0, 17, n - 1):
        bad = list(pts)
        bad[i] = E.g1_compress(E.g1_mul(E.G1_GEN, 123456789 + i))
        want = [ERR_VERIFY if k in (i - 1, i) else OK for k in range(n - 1)]
        assert key.pairing_check_each(bad[:-1], bad[1:]) == want
