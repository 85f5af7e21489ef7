"""Shared by tests/test_composer_host.py and tests/test_gpu_composer.py: the CPU harness of the gadget composer
(tests/csrc/host_composer.cpp, g++) behind the same method names as plonk_amd.Composer, the circuits A-D of the two test
files, the plain-Python meaning of every gadget output, and the bridge to the diagnosis yardstick tests/diagnose_ref.py.
Nothing here computes an expected value with the code under test."""
from __future__ import annotations

import ctypes
import json
import os
import random
import subprocess

import plonk_amd
from oracle import plonk as O
from oracle.bls12_381 import Q
from tests.widget_circuits import jj_add, jj_neg, on_curve

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_composer.so")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "composer_layouts.json")))
GEN = tuple(int(v, 16) for v in GOLDEN["jubjub"]["generator"])
ORDER = int(GOLDEN["jubjub"]["order"], 16)
IDENTITY = (0, 1)


def jj_mul(p, k):
    """[k] p by double-and-add with jj_add"""
    acc = IDENTITY
    for bit in bin(k)[2:] if k else "":
        acc = jj_add(acc, acc)
        if bit == "1":
            acc = jj_add(acc, p)
    return acc


assert on_curve(GEN) and jj_mul(GEN, ORDER) == IDENTITY


# ---- the CPU harness ------------------------------------------------------------------------------------------------------
_host = None


def host_lib():
    global _host
    if _host is not None:
        return _host
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_composer.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "plonk_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.hc_create.restype = vp
    lib.hc_destroy.argtypes = [vp]
    lib.hc_destroy.restype = None
    lib.hc_witness.argtypes = [vp, ctypes.POINTER(u32)]
    lib.hc_gate.argtypes = [vp, vp, vp, u32, ctypes.POINTER(u32)]
    lib.hc_gadget.argtypes = [vp, ctypes.c_int, u32, vp, u32, vp, u32, vp, u32, ctypes.POINTER(u32)]
    lib.hc_info.argtypes = [vp, vp]
    lib.hc_layout.argtypes = [vp, vp, vp, vp, vp]
    lib.hc_program.argtypes = [vp, vp, vp]
    lib.hc_program.restype = None
    lib.hc_fill.argtypes = [vp, vp, vp, vp, ctypes.POINTER(u64)]
    lib.hc_fill.restype = u32
    _host = lib
    return lib


class _HarnessAsLibrary:
    """the harness under the names of the C ABI: hc_gate answers for plonk_composer_gate, and so on (same signatures)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith("plonk_composer_"):
            return getattr(self._lib, "hc_" + name[len("plonk_composer_"):])
        return getattr(self._lib, name)


class HostComposer(plonk_amd.Composer):
    """plonk_amd.Composer's methods over the CPU harness: the same recorder (composer_host.hpp), no device library"""

    def __init__(self):
        self.lib = _HarnessAsLibrary(host_lib())
        self.handle = ctypes.c_void_p(self.lib.hc_create())

    def _check(self, rc):
        if rc != 0:
            raise (plonk_amd.PointMalformed if rc == -10 else plonk_amd.PlonkError)(rc, "host composer")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hc_destroy(self.handle)
            self.handle = None

    def program(self):
        """(records in scheduled order as dicts, level offsets)"""
        info = self.info()
        rec = (ctypes.c_uint32 * (11 * max(info["records"], 1)))()
        off = (ctypes.c_uint32 * (info["levels"] + 1))()
        self.lib.hc_program(self.handle, rec, off)
        names = ["kind", "width", "in0", "in1", "in2", "in3", "out0", "nout", "cst", "level", "id"]
        return [dict(zip(names, rec[11 * i:11 * i + 11])) for i in range(info["records"])], list(off)

    def fill(self, inputs):
        """the one-thread host executor: (witness table as Montgomery bytes, public-input values, error record or None)"""
        info = self.info()
        assert len(inputs) == info["inputs"]
        tab = ctypes.create_string_buffer(max(32 * info["witnesses"], 1))
        pi = ctypes.create_string_buffer(max(32 * info["public_rows"], 1))
        misses = ctypes.c_uint64()
        err = self.lib.hc_fill(self.handle, plonk_amd.fr_to_bytes_mont(inputs), tab, pi, ctypes.byref(misses))
        assert misses.value == 0, "a record read outside the table or wrote outside its own output slots"
        return tab.raw[:32 * info["witnesses"]], plonk_amd.fr_from_bytes_mont(pi.raw[:32 * info["public_rows"]]), (None if err == 0xFFFFFFFF else err)


# ---- bridge to the diagnosis yardstick ----------------------------------------------------------------------------------------
def as_oracle(layout, table_ints, pi_vals):
    """an oracle.plonk.Composer holding the recorded gates, the given witness values and public inputs (for diagnose_ref)"""
    c = O.Composer()
    c.constraints, c.public_inputs = [], {}
    c.witnesses = list(table_ints)
    c.witness_map = {w: [] for w in range(layout["witnesses"])}
    cols = {name: plonk_amd.fr_from_bytes_mont(raw) for name, raw in layout["selectors"].items()}
    pis = dict(zip(layout["pi_rows"], pi_vals))
    for i in range(len(layout["wires"][0])):
        g = O.Gate(a=layout["wires"][0][i], b=layout["wires"][1][i], c=layout["wires"][2][i], d=layout["wires"][3][i],
                   pi=pis.get(i), **{name: cols[name][i] for name in O.SELECTORS})
        c.append_custom_gate(g)
    return c


def layout_digest(layout):
    """gate_digest of the reference (support.rs:93-135), computed from the exported arrays"""
    cols = [plonk_amd.fr_from_bytes_mont(layout["selectors"][name]) for name in O.SELECTORS]
    acc = 0
    for i in range(len(layout["wires"][0])):
        for col in cols:
            acc = (acc * 1000003 + col[i]) % Q
        for w in range(4):
            acc = (acc * 1000003 + layout["wires"][w][i]) % Q
    return list(acc.to_bytes(32, "little"))


def domain_size(constraints):
    n = 1
    while n < constraints:
        n *= 2
    return n


# ---- circuits ---------------------------------------------------------------------------------------------------------------
class Case:
    """a recorded circuit: the input values of an honest proof and what plain Python says some witnesses must be"""

    def __init__(self, composer):
        self.c = composer
        self.inputs = []
        self.expect = []          # (witness index, value, what)

    def inp(self, v):
        self.inputs.append(v % Q)
        return self.c.append_witness()

    def point(self, p):
        self.inputs += [p[0], p[1]]
        return self.c.append_point()

    def want(self, w, v, what):
        self.expect.append((w, v % Q, what))

    def want_point(self, wp, p, what):
        self.want(wp[0], p[0], what + ".x")
        self.want(wp[1], p[1], what + ".y")


RANGE_WIDTHS = [0, 1, 2, 7, 8, 9, 64, 255, 256]
LOGIC_PAIRS = [0, 1, 4, 125, 127]
TRUNCATE_WIDTHS = [1, 64, 253, 254]
DECOMPOSITION_WIDTHS = [1, 8, 254]


def circuit_a(c, seed=11):
    """every gadget kind (about 2^14 gates), and one pipeline in which whole-gadget lanes feed later levels:
    mul_generator -> add_point -> select_point -> decomposition<254> of x -> logic"""
    rnd = random.Random(seed)
    k = Case(c)
    P, C3 = jj_mul(GEN, 5), jj_mul(GEN, 3)
    # composer basics
    x, y = rnd.randrange(Q), rnd.randrange(Q)
    wx, wy = k.inp(x), k.inp(y)
    k.want(c.append_constant(15), 15, "append_constant")
    wp = c.append_public()
    k.inputs.append(77)
    k.want(wp, 77, "append_public")
    c.append_gate(a=wx, b=wy, q_l=1, q_r=1, public=True)                                   # PI = -(x + y)
    k.want(c.append_evaluated_output(a=wx, b=wy, d=wp, q_m=3, q_l=5, q_r=7, q_f=11, q_c=13, q_o=2),
           -(3 * x * y + 5 * x + 7 * y + 11 * 77 + 13) * pow(2, -1, Q), "append_evaluated_output")
    assert c.append_evaluated_output(a=wx, b=wx, c=wx, q_m=1, q_o=0, q_l=Q - x) is None     # q_o = 0: a gate, no output
    s = c.gate_add(wx, wy, d=wp, q_l=2, q_r=3, q_f=4, q_c=5)
    k.want(s, 2 * x + 3 * y + 4 * 77 + 5, "gate_add")
    m = c.gate_mul(wx, wy, d=wp, q_m=2, q_f=3, q_c=4)
    k.want(m, 2 * x * y + 3 * 77 + 4, "gate_mul")
    wx2 = k.inp(x)
    c.assert_equal(wx, wx2)
    c.assert_equal_constant(c.append_constant(9), 9)
    c.assert_equal_constant(wx, 0, public=True)                                              # PI = x
    # bits and selection
    for bit in (0, 1):
        wb = k.inp(bit)
        c.component_boolean(wb)
        k.want(c.component_select(wb, wx, wy), x if bit else y, "select")
        k.want(c.component_select_one(wb, wx), x if bit else 1, "select_one")
        k.want(c.component_select_zero(wb, wx), x if bit else 0, "select_zero")
        pp, cp = k.point(P), c.append_constant_point(C3)
        k.want_point(c.component_select_identity(wb, pp), P if bit else IDENTITY, "select_identity")
        k.want_point(c.component_select_point(wb, pp, cp), P if bit else C3, "select_point")
    for n in DECOMPOSITION_WIDTHS:
        v = rnd.randrange(1 << n)
        for i, wbit in enumerate(c.component_decomposition(k.inp(v), n)):
            k.want(wbit, (v >> i) & 1, f"decomposition<{n}>[{i}]")
    # range and truncation
    for n in RANGE_WIDTHS:
        c.component_range_bits(k.inp(rnd.randrange(min(1 << n, Q))), n)
    c.component_range(k.inp(rnd.randrange(1 << 32)), 16)
    for n in TRUNCATE_WIDTHS:
        v = rnd.randrange(Q)
        k.want(c.component_truncate(k.inp(v), n), v & ((1 << n) - 1), f"truncate<{n}>")
    v = rnd.randrange(Q)
    wv, wlow, whigh = k.inp(v), k.inp(v & 1023), k.inp(v >> 10)
    c.component_range_bits(wlow, 10)
    c.bind_truncation_split(wv, wlow, 10)
    c.component_range_bits(whigh, 245)
    c.assert_canonical_truncation(whigh, wlow, 10)
    # logic
    for pairs in LOGIC_PAIRS:
        a, b = rnd.randrange(Q), rnd.randrange(Q)
        wa, wb = k.inp(a), k.inp(b)
        mask = (1 << (2 * pairs)) - 1
        k.want(c.append_logic_xor(wa, wb, pairs), (a ^ b) & mask, f"xor<{pairs}>")
        k.want(c.append_logic_and(wa, wb, pairs), (a & b) & mask, f"and<{pairs}>")
    # points
    pp = k.point(P)
    pub = c.append_public_point()
    k.inputs += [C3[0], C3[1]]
    cp = c.append_constant_point(C3)
    c.assert_equal_point(pub, cp)
    c.assert_equal_public_point(pp)
    k.want_point(c.component_neg_point(pp), jj_neg(P), "neg_point")
    k.want_point(c.component_sub_point(pp, cp), jj_mul(GEN, 2), "sub_point")
    k.want_point(c.component_add_point(pp, cp), jj_mul(GEN, 8), "add_point")
    c.assert_torsion_free_point(pp)
    k.torsion_q = (c.info()["witnesses"] - 14, jj_mul(P, pow(8, -1, ORDER)))
    k.want(k.torsion_q[0], k.torsion_q[1][0], "[1/8]P.x")
    k.want(k.torsion_q[0] + 1, k.torsion_q[1][1], "[1/8]P.y")
    # scalar multiplication
    c.assert_canonical_jubjub_scalar(k.inp(ORDER - 1))
    products = []
    for sc in (0, 1, 2, rnd.randrange(ORDER), ORDER - 1):
        g = c.component_mul_generator(k.inp(sc), GEN)
        k.want_point(g, jj_mul(GEN, sc), f"mul_generator({sc})")
        products.append((g, sc))
    for sc in (0, 1, 17, ORDER - 1):
        k.want_point(c.component_mul_point(k.inp(sc), pp), jj_mul(P, sc), f"mul_point({sc})")
    # the pipeline
    # (decomposition<254> must be satisfiable: take a product whose sum with P has an x coordinate below 2^254)
    g, sc = next((g, sc) for g, sc in products if sc > 1 and not jj_add(jj_mul(GEN, sc), P)[0] >> 254)
    sum_pt = jj_add(jj_mul(GEN, sc), P)
    added = c.component_add_point(g, pp)
    wb = k.inp(1)
    c.component_boolean(wb)
    sel = c.component_select_point(wb, added, cp)
    k.want_point(sel, sum_pt, "pipeline select")
    xv = sum_pt[0]
    bits = c.component_decomposition(sel[0], 254)
    k.want(bits[0], xv & 1, "pipeline bit 0")
    k.want(c.append_logic_xor(sel[0], bits[0], 8), (xv ^ (xv & 1)) & 0xFFFF, "pipeline xor")
    return k


def circuit_b(c, depth=3000):
    """a chain of `depth` dependent gate_mul / gate_add (2^12 gates)"""
    k = Case(c)
    x = 0x1234567
    wx = k.inp(x)
    w, v = wx, x
    for i in range(depth):
        if i & 1:
            w, v = c.gate_add(w, wx, q_c=i), (v + x + i) % Q
        else:
            w, v = c.gate_mul(w, wx), v * x % Q
    k.want(w, v, "end of the chain")
    return k


def circuit_c(c, count=5000, seed=5):
    """`count` independent component_range_bits<16> and `count` component_select over distinct inputs (2^16 gates)"""
    rnd = random.Random(seed)
    k = Case(c)
    for _ in range(count):
        c.component_range_bits(k.inp(rnd.randrange(1 << 16)), 16)
    for i in range(count):
        bit, a, b = i & 1, rnd.randrange(Q), rnd.randrange(Q)
        out = c.component_select(k.inp(bit), k.inp(a), k.inp(b))
        if i < 16:
            k.want(out, a if bit else b, "select")
    return k


def circuit_d(c, iterations=2):
    """the reference's bench circuit (benches/plonk.rs:33-82) with its default values, `iterations` rounds of the loop body"""
    k = Case(c)
    z = jj_mul(GEN, 7)
    wa, wb, wx, wy = k.inp(2), k.inp(3), k.inp(6), k.inp(7)
    wz = k.point(z)
    for _ in range(iterations):
        r = c.gate_mul(wa, wb)
        c.append_constant(15)
        c.append_constant_point(z)
        c.assert_equal(wx, r)
        c.assert_equal_point(wz, wz)
        c.gate_add(wa, wb)
        k.want_point(c.component_add_point(wz, wz), jj_mul(GEN, 14), "add_point")
        k.want(c.append_logic_and(wa, wb, 127), 2, "and")
        k.want(c.append_logic_xor(wa, wb, 127), 1, "xor")
        c.component_boolean(c.ONE)
        c.component_decomposition(wa, 254)
        k.want_point(c.component_mul_generator(wy, GEN), z, "mul_generator")
        k.want_point(c.component_mul_point(wy, wz), jj_mul(GEN, 49), "mul_point")
        c.component_range_bits(wa, 256)
        c.component_select(c.ONE, wa, wb)
        c.component_select_identity(c.ONE, wz)
        c.component_select_one(c.ONE, wa)
        c.component_select_point(c.ONE, wz, wz)
        c.component_select_zero(c.ONE, wa)
    return k


def rejected_range(c):
    """300 under component_range_bits<8>: (case, first row of the gadget, its closing assert_equal row)"""
    k = Case(c)
    w = k.inp(300)
    first = c.info()["constraints"]
    c.component_range_bits(w, 8)
    return k, first, c.info()["constraints"] - 1


def rejected_boolean(c):
    k = Case(c)
    w = k.inp(2)
    first = c.info()["constraints"]
    c.component_boolean(w)
    return k, first, first
