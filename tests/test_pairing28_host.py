"""CPU: the device pairing of plonk_amd/csrc/pairing28.cuh, compiled with g++ (tests/csrc/host_pairing28.cpp), against
the host pairing of hostpairing.hpp bit for bit, and once against the plain-Python pairing of tests/pairing_ref.py."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from oracle import bls12_381 as E

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import g2_ref as G2          # noqa: E402
import kzg_ref as K          # noqa: E402
import pairing_ref as PR     # noqa: E402

SO = os.path.join(HERE, "_build", "libhost_pairing28.so")
Q = E.Q
ID48 = K.IDENTITY48
H96 = G2.g2_compress(G2.G2_GEN)
XH = G2.g2_mul(G2.G2_GEN, K.TAU)
XH96 = G2.g2_compress(XH)


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_pairing28.cpp")
    csrc = os.path.join(HERE, "..", "plonk_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    lib.hp_pairing2.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.hp_f12_inv_check.argtypes = [ctypes.c_uint64, ctypes.c_int]
    lib.hp_red_check.argtypes = [ctypes.c_uint64, ctypes.c_int]
    lib.hp_tables_roundtrip.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.hp_special_check.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]
    return lib


def comp(p):
    return ID48 if p is None else E.g1_compress(p)


def both(lib, a, b):
    """(flags, value by pairing28.cuh, value by hostpairing.hpp) of e(-a, x_h) e(b, h); 12 integers each, tower order"""
    dev, host = (ctypes.c_uint64 * 72)(), (ctypes.c_uint64 * 72)()
    rc = lib.hp_pairing2(comp(a), comp(b), XH96, H96, dev, host)
    assert rc >= 0
    ints = lambda o: [sum(int(o[6 * i + k]) << (64 * k) for k in range(6)) for i in range(12)]   # noqa: E731
    return rc, ints(dev), ints(host)


def test_random_pairs_equal_the_host_pairing_bit_for_bit_and_one_equals_the_python_pairing(lib):
    rnd = random.Random(2801)
    first = None
    for i in range(4):
        a = E.g1_mul(E.G1_GEN, rnd.randrange(1, Q))
        b = E.g1_mul(E.G1_GEN, rnd.randrange(1, Q))
        rc, dev, host = both(lib, a, b)
        assert dev == host and rc == 0 and dev != [1] + [0] * 11
        first = first or (a, b, dev)
    a, b, dev = first
    assert PR.from_tower(dev) == PR.multi_pairing([(E.g1_mul(a, Q - 1), XH), (b, G2.G2_GEN)])


def test_the_kzg_shape_passes_and_a_wrong_right_side_does_not(lib):
    r = 0x1234567ABCDEF
    a = E.g1_mul(E.G1_GEN, r)
    rc, dev, host = both(lib, a, E.g1_mul(E.G1_GEN, r * K.TAU % Q))      # e(-[r] g, [tau] h) e([r tau] g, h) = 1
    assert rc == 3 and dev == host == [1] + [0] * 11
    rc, dev, host = both(lib, a, E.g1_mul(E.G1_GEN, (r * K.TAU + 1) % Q))
    assert rc == 0 and dev == host


@pytest.mark.parametrize("a_id,b_id,one", [(True, True, True), (True, False, False), (False, True, False)])
def test_every_identity_placement(lib, a_id, b_id, one):
    p = E.g1_mul(E.G1_GEN, 77)
    rc, dev, host = both(lib, None if a_id else p, None if b_id else E.g1_mul(p, K.TAU))
    assert dev == host and rc == (3 if one else 0)


def test_inverse_reduction_and_table_round_trip(lib):
    assert lib.hp_f12_inv_check(5, 8) == 0                 # f12r_inv(x) * x == 1
    assert lib.hp_red_check(6, 20000) == 0                 # p28_red: same residue, below 2p, normalised
    size = lib.hp_tables_roundtrip(XH96, H96)              # every line and Frobenius constant converts back exactly
    assert 40000 < size < 50000                            # about 23 KB per G2 point


def test_specialised_routines_equal_the_generic_product(lib):
    """the sparse line product, the complex-method square and the cyclotomic square change the cost, never the value"""
    assert lib.hp_special_check(7, 6, XH96, H96) == 0
