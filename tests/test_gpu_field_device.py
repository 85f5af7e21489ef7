"""The arithmetic layer AS THE DEVICE COMPILER BUILDS IT, against the big-int oracle at its edge operands.

tests/test_field_host.py checks the product's __host__ __device__ headers (field.cuh, curve.cuh, fp28.cuh, curve28.cuh,
fr29.cuh, fp_safegcd.cuh, g1codec.cuh, msm_recode.cuh, transcript.hpp) compiled by g++ for the host; the code that proves
is the same source compiled by hipcc -O3 for gfx950.  Here the same case bodies (tests/csrc/arith_cases.hpp) run as one
small kernel per family (tests/csrc/dev_arith.hip, built by build() into tests/_build/libdev_arith.so with the product's
flags): lane i runs case i of tests/arith_vectors.py, one launch per family, and every output record is compared bit for
bit with the expectation the host test uses.  Nothing here has a tolerance."""
import ctypes
import os

import pytest

import arith_vectors as V

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libdev_arith.so")


@pytest.fixture(scope="module")
def dev():
    assert os.path.exists(SO), "tests/_build/libdev_arith.so is missing: run build() of __graft_entry__.py first"
    return ctypes.CDLL(SO)


@pytest.mark.parametrize("name", V.FAMILIES)
def test_device_arithmetic_matches_the_oracle(dev, name):
    fam = V.family(name)
    rc, out = fam.run(dev, "d_")
    assert rc == 0, "d_case_%s: HIP error %d" % (name, rc)
    fam.check(out)
