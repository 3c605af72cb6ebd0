"""Runs the __host__ __device__ G2 code of the G2 MSM kernels (g2.hpp with the product-scanning multiplier: madd, full XYZZ addition,
doubling, normalisation, the on-twist check) on the CPU via tests/hostcheck/g2_selftest.cpp and checks it against pyref / cref, every
exceptional case included, plus a host-side bucket MSM built from the same functions.  A check OF the device arithmetic; CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import cref, pyref

HERE = os.path.dirname(os.path.abspath(__file__))
R, P = pyref.R_MOD, pyref.P_MOD
RINV_P = pow(pyref.MONT_R, -1, P)


@pytest.fixture(scope="module")
def g2s(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("g2s") / "libg2selftest.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "g2_selftest.cpp")])
    return C.CDLL(so)


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def aff(Q):
    return np.array(pyref.g2_to_limbs(Q), dtype=np.uint64)


def to_py(limbs):
    if not np.asarray(limbs).any():
        return None
    return tuple(tuple(pyref.from_limbs(limbs[8 * a + 4 * b:8 * a + 4 * b + 4]) * RINV_P % P for b in range(2)) for a in range(2))


def neg(Q):
    return (Q[0], ((-Q[1][0]) % P, (-Q[1][1]) % P))


class X:
    """an XYZZ accumulator held in a numpy buffer, driven by the compiled functions"""
    def __init__(self, lib, Q=None):
        self.lib, self.v = lib, np.zeros(32, dtype=np.uint64)
        if Q is not None:
            self.madd(Q)

    def madd(self, Q):
        self.lib.g2s_madd(p_(self.v), p_(aff(Q))); return self

    def add(self, other):
        self.lib.g2s_add(p_(self.v), p_(other.v)); return self

    def dbl(self):
        o = X(self.lib); self.lib.g2s_dbl(p_(o.v), p_(self.v)); return o

    def point(self):
        out = np.zeros(16, dtype=np.uint64); self.lib.g2s_to_affine(p_(out), p_(self.v)); return to_py(out)


def rand_pts(rng, n):
    return [pyref.g2_mul(pyref.G2_GEN, int(rng.integers(1, 2**62)) * int(rng.integers(1, 2**62)) % R) for _ in range(n)]


def test_g2_formulas_on_random_points(g2s):
    rng = np.random.default_rng(81)
    pts = rand_pts(rng, 12)
    for i in range(0, 12, 3):
        A, B, Cc = pts[i], pts[i + 1], pts[i + 2]
        a = X(g2s, A).madd(B)                                            # A + B with ZZ = 1 operand
        assert a.point() == pyref.g2_add(A, B)
        b = X(g2s, Cc).madd(A)                                           # C + A, non-trivial ZZ
        a.add(b)                                                         # full addition of two projective points
        assert a.point() == pyref.g2_add(pyref.g2_add(A, B), pyref.g2_add(Cc, A))
        assert a.dbl().point() == pyref.g2_mul(pyref.g2_add(pyref.g2_add(A, B), pyref.g2_add(Cc, A)), 2)
        for Q in (A, B, Cc):
            assert g2s.g2s_on_curve(p_(aff(Q))) == 1
        off = aff(A); off[8] ^= np.uint64(1)
        assert g2s.g2s_on_curve(p_(off)) == 0
    assert g2s.g2s_on_curve(p_(np.zeros(16, dtype=np.uint64))) == 1     # the identity passes


def test_g2_exceptional_cases(g2s):
    rng = np.random.default_rng(82)
    A, B = rand_pts(rng, 2)
    assert X(g2s).point() is None                                        # identity normalises to all zero
    assert X(g2s).madd(None).point() is None                             # identity + identity
    assert X(g2s, A).madd(None).point() == A                             # P + O (madd)
    assert X(g2s, A).madd(A).point() == pyref.g2_mul(A, 2)               # madd doubling branch
    assert X(g2s, A).madd(neg(A)).point() is None                        # madd inverse branch
    ab = X(g2s, A).madd(B)                                               # A + B (ZZ != 1)
    ab2 = X(g2s, B).madd(A)
    assert X(g2s, None).add(ab).point() == pyref.g2_add(A, B)            # O + P (add)
    assert X(g2s, A).madd(B).add(X(g2s)).point() == pyref.g2_add(A, B)   # P + O (add)
    assert ab.add(ab2).point() == pyref.g2_mul(pyref.g2_add(A, B), 2)    # add doubling branch, different representatives
    m = X(g2s, neg(A)).madd(neg(B))
    assert X(g2s, A).madd(B).add(m).point() is None                      # add inverse branch
    assert X(g2s).dbl().point() is None                                  # 2 O


@pytest.mark.parametrize("n,c", [(1, 4), (2, 3), (5, 4), (17, 5), (32, 6)])
def test_g2_bucket_msm_on_host(g2s, n, c):
    rng = np.random.default_rng(83 + n)
    pts = rand_pts(rng, n)
    if n >= 5:
        pts[1] = None                                                    # identity base
        pts[3] = neg(pts[2])                                             # P and -P
    ks = [int(rng.integers(0, 2**63)) ** 4 % R for _ in range(n)]
    ks[0] = R - 1
    if n >= 5:
        ks[3] = ks[2]; ks[4] = 0
    bases = np.stack([aff(Q) for Q in pts])
    can = np.array([pyref.to_limbs(k) for k in ks], dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint64)
    g2s.g2s_bucket_msm(p_(out), p_(bases), p_(can), C.c_uint64(n), C.c_uint32(c))
    want = None
    for Q, k in zip(pts, ks):
        want = pyref.g2_add(want, pyref.g2_mul(Q, k) if Q is not None else None)
    assert to_py(out) == want
    if n <= 5:   # and the C oracle agrees with pyref on these terms
        acc = None
        for b, k in zip(bases, ks):
            acc = pyref.g2_add(acc, to_py(cref.g2_mul(b, cref.fr_mont(k))))
        assert acc == want


def test_g2_formulas_on_adversarial_twist_points(g2s):
    """twist points whose x components are adversarial Montgomery words (tests/gpu_common.py::adversarial_g2_points: a component zero, on an edge of the
    field or of a limb grid), outside the subgroup of order r: madd, add, dbl, normalise and the on-twist check against pyref"""
    from tests import gpu_common as gc
    limbs, pts, _ = gc.adversarial_g2_points()
    m = len(pts)
    rng = np.random.default_rng(84)
    ref = rand_pts(rng, 3)
    for i, Q in enumerate(pts):
        assert g2s.g2s_on_curve(p_(limbs[i].copy())) == 1
        off = limbs[i].copy(); off[4 * int(rng.integers(0, 4))] ^= np.uint64(1)
        assert g2s.g2s_on_curve(p_(off)) == 0
        Q2 = pts[(7 * i + 11) % m]
        if Q2[0] == Q[0]:
            Q2 = pts[(7 * i + 13) % m]
        A = ref[i % 3]
        assert X(g2s, Q).point() == Q                                    # first point, normalised back
        a = X(g2s, A).madd(Q)                                            # onto a random accumulator
        assert a.point() == pyref.g2_add(A, Q)
        b = X(g2s, Q).madd(Q2)                                           # two pool points
        assert b.point() == pyref.g2_add(Q, Q2)
        assert X(g2s, Q).madd(Q).point() == pyref.g2_add(Q, Q)           # madd doubling branch
        assert X(g2s, Q).madd(neg(Q)).point() is None                    # madd inverse branch
        assert X(g2s, Q).dbl().point() == pyref.g2_add(Q, Q)
        if i % 4 == 0:                                                   # full additions and a doubling of projective points
            s = pyref.g2_add(pyref.g2_add(A, Q), pyref.g2_add(Q, Q2))
            assert a.add(b).point() == s and a.dbl().point() == pyref.g2_add(s, s)
            assert X(g2s, Q).madd(Q2).add(X(g2s, Q2).madd(Q)).point() == pyref.g2_mul(pyref.g2_add(Q, Q2), 2)
            assert X(g2s, Q).madd(Q2).add(X(g2s, neg(Q2)).madd(neg(Q))).point() is None


def test_g2_bucket_msm_on_adversarial_twist_points(g2s):
    """the host-side bucket MSM over pool points: the scalars act as integers (the points are outside the subgroup of order r)"""
    from tests import gpu_common as gc
    limbs, pts, _ = gc.adversarial_g2_points()
    rng = np.random.default_rng(85)
    for lo, c in ((0, 4), (100, 5), (len(pts) - 24, 6)):
        n = 24
        ks = [int(rng.integers(0, 2**63)) ** 4 % R for _ in range(n)]
        ks[0] = R - 1; ks[1] = pyref.FR_ZETA; ks[3] = ks[2]
        can = np.array([pyref.to_limbs(k) for k in ks], dtype=np.uint64)
        out = np.zeros(16, dtype=np.uint64)
        g2s.g2s_bucket_msm(p_(out), p_(np.ascontiguousarray(limbs[lo:lo + n])), p_(can), C.c_uint64(n), C.c_uint32(c))
        want = None
        for Q, k in zip(pts[lo:lo + n], ks):
            want = pyref.g2_add(want, pyref.g2_mul(Q, k))
        assert to_py(out) == want
