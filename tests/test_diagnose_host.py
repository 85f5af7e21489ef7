"""CPU: the host-callable half of witness diagnosis — plonk_amd/csrc/diagnose_core.hpp (the 17 identities of a row over plain
Fr, the decoding of sigma evaluations into wire positions) compiled with g++ (tests/csrc/host_diagnose.cpp, like
tests/csrc/host_verify.cpp) against the plain-Python yardstick tests/diagnose_ref.py; the facts about the test inputs that
keep a silent yardstick from passing; the layout of the two report structs against their ctypes mirrors."""
import ctypes
import os
import random
import subprocess

import pytest

from tests import circuits as C
from tests import diagnose_cases as DC
from tests import diagnose_ref as DR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libhost_diagnose.so")
Q = DC.Q


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "csrc", "host_diagnose.cpp")
    csrc = os.path.join(ROOT, "plonk_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".cuh"))]
    if not os.path.exists(SO) or any(os.path.getmtime(f) > os.path.getmtime(SO) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp = ctypes.c_void_p
    lib.hd_sigma_decode.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, vp]
    lib.hd_sigma_decode.restype = None
    lib.hd_report.argtypes = [ctypes.c_uint32, ctypes.c_char_p, vp, ctypes.c_char_p, vp, vp, vp]
    lib.hd_report.restype = None
    return lib


class HostCircuit:
    """the C++ evaluation of one circuit: selector columns and decoded positions prepared once, a report per assignment"""

    def __init__(self, lib, comp):
        self.lib, self.comp = lib, comp
        self.n = DC.size_of(comp)
        self.log_n = self.n.bit_length() - 1
        self.sel_keep = {k: C.fr_bytes(col) for k, col in DC.selector_columns(comp, self.n).items()}
        self.sel = (ctypes.c_void_p * 11)(*[ctypes.cast(ctypes.c_char_p(self.sel_keep[k]), ctypes.c_void_p) if k in self.sel_keep else None
                                           for k in range(11)])
        sig = DC.sigma_values(comp, self.n)
        self.pos = (ctypes.c_uint32 * (4 * self.n))()
        lib.hd_sigma_decode(self.log_n, 4 * self.n, C.fr_bytes([v for col in sig for v in col]), self.pos)
        pi = [0] * self.n
        for row, v in comp.public_inputs.items():
            pi[row] = v
        self.pi = C.fr_bytes(pi)

    def positions(self):
        return [[(p >> 30, p & ((1 << 30) - 1)) for p in self.pos[col * self.n:(col + 1) * self.n]] for col in range(4)]

    def report(self, cols):
        fam, cp = (ctypes.c_uint32 * self.n)(), (ctypes.c_uint32 * self.n)()
        self.lib.hd_report(self.log_n, C.fr_bytes([v for col in cols for v in col]), self.sel, self.pi, self.pos, fam, cp)
        return [(i, fam[i], cp[i]) for i in range(self.n) if fam[i] or cp[i]]


@pytest.fixture(scope="module")
def circuits(lib):
    return [(name, comp, HostCircuit(lib, comp)) for name, comp in DC.small_circuits()]


def test_sigma_decoding_round_trips_every_position(circuits):
    for name, comp, hc in circuits:
        want = [[tuple(p) for p in col] for col in comp.sigma_mappings(hc.n)]
        assert hc.positions() == want, name


def test_sigma_decoding_refuses_values_that_name_no_position(lib):
    rnd = random.Random(5)
    log_n = 8
    vals = [rnd.randrange(Q) for _ in range(8)] + [0, 23]        # random scalars, zero, a constant off the four cosets
    pos = (ctypes.c_uint32 * len(vals))()
    lib.hd_sigma_decode(log_n, len(vals), C.fr_bytes(vals), pos)
    assert list(pos) == [0xFFFFFFFF] * len(vals)


def test_honest_reports_are_empty_and_single_witness_mutations_match_the_yardstick(circuits):
    seen = 0
    satisfied = {}
    for name, comp, hc in circuits:
        n = hc.n
        honest = DR.columns(comp, n)
        assert DR.report(comp, n, honest) == [], name                 # the yardstick itself
        assert hc.report(honest) == [], name
        sigma = comp.sigma_mappings(n)
        satisfied[name] = 0
        for w, vals in DC.witness_mutations(comp):
            cols = DR.columns(comp, n, vals)
            want = DR.report(comp, n, cols, sigma=sigma)
            assert hc.report(cols) == want, (name, w)
            assert all(cp == 0 for _, _, cp in want), (name, w)      # a witness mutation keeps every cycle constant
            for _, fam, _ in want:
                seen |= fam
            satisfied[name] += not want
    # the mutations between them reach every identity family, and only unused / duplicated witnesses leave a circuit satisfied
    assert seen == (1 << DR.FAMILIES) - 1
    assert [len(comp.witnesses) for _, comp, _ in circuits] == [239, 635]
    assert satisfied == {"semantic": 1, "big256": 11}


def test_single_cell_forgeries_set_every_copy_bit_and_match_the_yardstick(circuits):
    rnd = random.Random(17)
    seen = 0
    for name, comp, hc in circuits:
        n = hc.n
        sigma = comp.sigma_mappings(n)
        for col, row in DC.cell_forgeries(comp, n, rnd, 48):
            cols = DR.columns(comp, n)
            cols[col][row] = (cols[col][row] + 1) % Q
            want = DR.report(comp, n, cols, sigma=sigma)
            assert hc.report(cols) == want, (name, col, row)
            for _, _, cp in want:
                seen |= cp
    assert seen == 0b1111


def test_the_last_row_reads_row_zero_when_there_is_no_padding(lib):
    comp, cols, want = DC.wraparound_case()
    assert want == [(0, 0, 0b1100), (63, 1 << 4, 0)]
    assert HostCircuit(lib, comp).report(cols) == want


def test_report_struct_layouts_match_the_c_header(tmp_path):
    """plonk_unsat_row / plonk_unsat_info as gcc lays them out against the ctypes mirrors of the binding"""
    import plonk_amd
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "plonk_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(plonk_unsat_row), offsetof(plonk_unsat_row, families),\n'
                   '  offsetof(plonk_unsat_row, copy_wires), sizeof(plonk_unsat_info), offsetof(plonk_unsat_info, family_rows),\n'
                   '  offsetof(plonk_unsat_info, first_row), offsetof(plonk_unsat_info, first_family), offsetof(plonk_unsat_info, ms));\n'
                   '  return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R, I = plonk_amd._UnsatRow, plonk_amd._UnsatInfo
    assert got == [ctypes.sizeof(R), R.families.offset, R.copy_wires.offset, ctypes.sizeof(I), I.family_rows.offset,
                   I.first_row.offset, I.first_family.offset, I.ms.offset]
    assert len(plonk_amd.IDENTITY_FAMILIES) == 18 and len(set(plonk_amd.IDENTITY_FAMILIES)) == 18
    for name in ("plonk_prover_diagnose", "plonk_prover_diagnose_dev", "plonk_prover_diagnose_witnesses"):
        assert name in plonk_amd.EXPORTS
