"""Runs the per-term routine of the segmented MSM kernel (csrc/msm_seg.hpp segmsm_term: Montgomery scalar -> MSB-first double-and-add on g1.hpp's XYZZ formulas -> the lane's
accumulator) on the CPU via tests/hostcheck/segmsm_selftest.cpp -- the 64 lanes as a loop, the shuffle tree as the same pairwise order over an array -- and checks every
segment against the oracle (cref.msm_naive; oracle/pyref.py for the small ones).  A check OF the device arithmetic; CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyref
from tests import segmsm_common as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "segmsm_selftest.cpp")
R = pyref.R_MOD


@pytest.fixture(scope="module")
def sst(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sst") / "libsegmsmselftest.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    return C.CDLL(so)


def run(sst, bases, scalars, offsets):
    bases = np.ascontiguousarray(bases, dtype=np.uint64); scalars = np.ascontiguousarray(scalars, dtype=np.uint64); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.full((len(offsets) - 1, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    sst.sst_msm_segmented(p(bases), p(scalars), p(offsets), C.c_uint32(len(offsets) - 1), p(out))
    return out


def test_segment_lengths_around_the_wavefront(sst):
    """lengths 0, 1, 2, 63, 64, 65, 130 in one call: empty segments give the identity, 65 and 130 make lanes walk two and three terms"""
    bases, scalars = sc.random_terms(sum(sc.LENGTHS), 4001)
    offsets = sc.offsets_of(sc.LENGTHS)
    got = run(sst, bases, scalars, offsets)
    assert (got == sc.reference(bases, scalars, offsets)).all()
    assert not got[0].any()
    small = sc.offsets_of([0, 1, 2])
    assert (got[:3] == sc.reference_py(bases[:3], scalars[:3], small)).all()


def test_edge_scalars_on_one_point_and_on_many(sst):
    bases, _ = sc.random_terms(len(sc.EDGE_SCALARS) + 1, 4002)
    rng = np.random.default_rng(4003)
    ks = list(sc.EDGE_SCALARS) + [int(rng.integers(1, 2**62)) ** 5 % R]
    scalars = sc.fr_arr(ks)
    one_each = np.arange(len(ks) + 1, dtype=np.uint64)
    got = run(sst, bases, scalars, one_each)
    assert (got == sc.reference_py(bases, scalars, one_each)).all()
    assert not got[0].any() and (got[1] == bases[1]).all()                       # 0 P, 1 P
    assert (got[3] == sc.neg_points(bases[3:4])[0]).all()                        # (r - 1) P = -P
    together = np.array([0, len(ks)], dtype=np.uint64)
    assert (run(sst, bases, scalars, together) == sc.reference(bases, scalars, together)).all()


def test_edge_inputs_alone_at_lane_0_and_at_lane_63(sst):
    """zero scalars, identity bases, the same base twice with equal scalars (the tree must double), P and -P (the identity), r - 1, 2^253 and every adversarial point"""
    labels, bases, scalars, offsets = sc.edge_case_inputs()
    got, want = run(sst, bases, scalars, offsets), sc.edge_case_reference()
    bad = [labels[i] for i in range(len(labels)) if (got[i] != want[i]).any()]
    assert not bad, bad
    by = dict(zip(labels, got))
    assert not by["negation/alone"].any() and not by["zero_scalar/alone"].any() and not by["identity_base/alone"].any() and not by["all_zero_scalars"].any()
    assert by["duplicate/alone"].any()
    from tests import gpu_common as gc
    assert sum(l.startswith("adversarial/") and l.endswith("/alone") for l in labels) == gc.adversarial_g1_points("mont")[0].shape[0]


def test_selftest_program_under_sanitizers(tmp_path):
    """the same source as a stand-alone program (its own main, a fixed subset on multiples of the generator) under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "segmsm_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSEGMSM_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout and "FAIL" not in out.stdout
