"""Runs the __host__ __device__ tower and pairing code of the pairing kernels (fq12.hpp, pairing.hpp: Fq6 / Fq12 arithmetic, the Frobenius maps and their constants,
the sparse line multiplication, the cyclotomic squaring, the Miller loop, the final exponentiation) on the CPU via tests/hostcheck/pairing_selftest.cpp and checks it
against oracle/pairing.py through the basis map: the tower coefficient a0 + a1 u at w^j v^i adds (a0 - 9 a1) at w^(2 i + j) and a1 at w^(2 i + j + 6).
A check OF the device arithmetic; CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import cref, pairing, pyref

HERE = os.path.dirname(os.path.abspath(__file__))
R, P = pyref.R_MOD, pyref.P_MOD
RINV_P = pow(pyref.MONT_R, -1, P)
F12 = pairing.F12
PS = [0, 1]   # the plain multiplier and the product-scanning one (what the kernels instantiate)


@pytest.fixture(scope="module")
def pst(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pst") / "libpairingselftest.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "pairing_selftest.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def E():
    """e(G1, G2), once per module"""
    return pairing.pairing(pyref.G2_GEN, pyref.G1_GEN)


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def mont(x):
    return pyref.mont_limbs(x % P, P)


def unmont(l):
    return pyref.from_limbs(l) * RINV_P % P


def tower_of(coeffs):
    """six Fq2 coefficients in memory order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) -> 48 u64 of Montgomery limbs"""
    out = []
    for a0, a1 in coeffs:
        out += mont(a0) + mont(a1)
    return np.array(out, dtype=np.uint64)


def coeffs_of(arr):
    return [(unmont(arr[8 * m:8 * m + 4]), unmont(arr[8 * m + 4:8 * m + 8])) for m in range(6)]


def to_oracle(arr):
    c = [0] * 12
    for m, (a0, a1) in enumerate(coeffs_of(arr)):
        j, i = divmod(m, 3)
        c[2 * i + j] += a0 - 9 * a1
        c[2 * i + j + 6] += a1
    return F12(c)


def from_oracle(x):
    co = [None] * 6
    for m in range(6):
        j, i = divmod(m, 3)
        a1 = x.c[2 * i + j + 6]
        co[m] = ((x.c[2 * i + j] + 9 * a1) % P, a1)
    return tower_of(co)


def out12():
    return np.zeros(48, dtype=np.uint64)


def fq2_arr(a):
    return np.array(mont(a[0]) + mont(a[1]), dtype=np.uint64)


def operands():
    rng = np.random.default_rng(1801)
    rnd = lambda: int(rng.integers(0, 2**63)) ** 5 % P
    ops = [[(rnd(), rnd()) for _ in range(6)] for _ in range(4)]
    ops.append([(0, 0)] * 6)                                              # 0
    ops.append([(1, 0)] + [(0, 0)] * 5)                                   # 1
    for m, half in ((0, 0), (0, 1), (2, 1), (3, 0), (5, 1)):              # p - 1 in single coefficients
        co = [(rnd(), rnd()) for _ in range(6)]
        co[m] = (P - 1, co[m][1]) if half == 0 else (co[m][0], P - 1)
        ops.append(co)
    ops.append([(P - 1, P - 1)] * 6)
    ops.append([(rnd(), rnd())] + [(0, 0)] * 5)                           # the Fq2 subfield
    ops.append([(rnd(), 0)] + [(0, 0)] * 5)                               # Fq
    ops.append([(rnd(), rnd()) for _ in range(3)] + [(0, 0)] * 3)         # the Fq6 subfield
    ops.append([(0, 0)] * 3 + [(rnd(), rnd()) for _ in range(3)])         # w * Fq6
    return [tower_of(co) for co in ops]


def test_basis_map_round_trip():
    for a in operands():
        assert (from_oracle(to_oracle(a)) == a).all()
    w = [(0, 0)] * 3 + [(1, 0)] + [(0, 0)] * 2
    assert to_oracle(tower_of(w)) == F12((0, 1) + (0,) * 10)
    v = [(0, 0), (1, 0)] + [(0, 0)] * 4
    assert to_oracle(tower_of(v)) == F12((0, 0, 1) + (0,) * 9)
    u = [(0, 1)] + [(0, 0)] * 5
    assert to_oracle(tower_of(u)) * to_oracle(tower_of(u)) == F12.of_fp(-1)


@pytest.mark.parametrize("ps", PS)
def test_fq12_ring_operations(pst, ps):
    ops = operands()
    o = out12()
    for i, a in enumerate(ops):
        A = to_oracle(a)
        b = ops[(5 * i + 3) % len(ops)]
        B = to_oracle(b)
        pst.pst_fq12_mul(ps, p_(o), p_(a), p_(b)); assert to_oracle(o) == A * B, i
        pst.pst_fq12_sqr(ps, p_(o), p_(a)); assert to_oracle(o) == A * A, i
        pst.pst_fq12_add(ps, p_(o), p_(a), p_(b)); assert to_oracle(o) == A + B, i
        pst.pst_fq12_sub(ps, p_(o), p_(a), p_(b)); assert to_oracle(o) == A - B, i
        pst.pst_fq12_neg(ps, p_(o), p_(a)); assert to_oracle(o) == -A, i
        pst.pst_fq12_conj(ps, p_(o), p_(a)); assert to_oracle(o) == F12([c if k % 2 == 0 else -c for k, c in enumerate(A.c)]), i
        pst.pst_fq12_inv(ps, p_(o), p_(a))
        if A.is_zero():
            assert not o.any()
        else:
            assert to_oracle(o) * A == F12.one(), i
            assert (o == from_oracle(A.inv())).all(), i                  # fully reduced: the same words as the oracle's value
    # results are canonical words (every limb group < p)
    pst.pst_fq12_mul(ps, p_(o), p_(ops[11]), p_(ops[11]))
    assert all(pyref.from_limbs(o[4 * k:4 * k + 4]) < P for k in range(12))


@pytest.mark.parametrize("ps", PS)
def test_fq6_mul_and_inverse(pst, ps):
    ops = [a for a in operands() if not a[24:].any()]
    assert len(ops) >= 5
    rng = np.random.default_rng(1802)
    ops += [tower_of([(int(rng.integers(0, 2**63)) ** 5 % P, int(rng.integers(0, 2**63)) ** 5 % P) for _ in range(3)] + [(0, 0)] * 3) for _ in range(3)]
    for i, a in enumerate(ops):
        b = ops[(3 * i + 1) % len(ops)]
        o = out12()
        pst.pst_fq6_mul(ps, p_(o), p_(a), p_(b)); assert to_oracle(o) == to_oracle(a) * to_oracle(b)
        o = out12()
        pst.pst_fq6_inv(ps, p_(o), p_(a))
        if a.any():
            assert to_oracle(o) * to_oracle(a) == F12.one()
        else:
            assert not o.any()


@pytest.mark.parametrize("ps", PS)
def test_frobenius_against_pow(pst, ps):
    ops = operands()
    o = out12()
    for a in (ops[0], ops[1], ops[6], ops[11], ops[12], ops[14], ops[15]):
        A = to_oracle(a)
        want = A
        for i in (1, 2, 3):
            want = want ** P
            pst.pst_fq12_frobenius(ps, i, p_(o), p_(a))
            assert to_oracle(o) == want, i


def test_frobenius_constants_against_pow(pst):
    """the table the compiled code holds == xi^(k (p^i - 1) / 6) recomputed here with square-and-multiply over Fq2"""
    def f2_pow(a, e):
        out = (1, 0)
        while e:
            if e & 1:
                out = pyref.f2_mul(out, a)
            a = pyref.f2_mul(a, a)
            e >>= 1
        return out
    g = np.zeros(8, dtype=np.uint64)
    for i in (1, 2, 3):
        for k in range(6):
            pst.pst_frob_gamma(i, k, p_(g))
            assert (unmont(g[:4]), unmont(g[4:])) == f2_pow((9, 1), k * (P**i - 1) // 6), (i, k)
    # and as elements of Fq12: w^(p^i) = gamma[i][1] w
    w = F12((0, 1) + (0,) * 10)
    pst.pst_frob_gamma(1, 1, p_(g))
    assert w ** P == F12.of_fp2((unmont(g[:4]), unmont(g[4:]))) * w


def test_constants_tool_matches_header():
    """tools/gen_pairing_constants.py regenerates the block fq12.hpp holds, and its integer checks of the exponent chain pass"""
    import importlib.util
    root = os.path.dirname(HERE)
    spec = importlib.util.spec_from_file_location("gen_pairing_constants", os.path.join(root, "tools", "gen_pairing_constants.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    mod.check_exponent()
    with open(mod.HEADER) as f:
        assert mod.block(mod.derive()) in f.read()


@pytest.mark.parametrize("ps", PS)
def test_sparse_line_multiplication_against_dense(pst, ps):
    rng = np.random.default_rng(1803)
    rnd2 = lambda: (int(rng.integers(0, 2**63)) ** 5 % P, int(rng.integers(0, 2**63)) ** 5 % P)
    lines = [(rnd2(), rnd2(), rnd2()), ((0, 0), rnd2(), rnd2()), (rnd2(), (0, 0), (0, 0)), ((P - 1, P - 1), (P - 1, 0), (0, P - 1)), ((0, 0), (0, 0), (0, 0))]
    ops = operands()
    for n, (l0, l1, l3) in enumerate(lines):
        a0, a1, a3 = fq2_arr(l0), fq2_arr(l1), fq2_arr(l3)
        dense = out12(); pst.pst_fq12_from_sparse(p_(dense), p_(a0), p_(a1), p_(a3))
        L = F12.of_fp2(l0) + F12.of_fp2(l1) * F12((0, 1) + (0,) * 10) + F12.of_fp2(l3) * F12((0, 0, 0, 1) + (0,) * 8)
        assert to_oracle(dense) == L
        for a in (ops[n], ops[6 + n], ops[14]):
            o, o2 = out12(), out12()
            pst.pst_fq12_mul_sparse(ps, p_(o), p_(a), p_(a0), p_(a1), p_(a3))
            pst.pst_fq12_mul(ps, p_(o2), p_(a), p_(dense))
            assert (o == o2).all() and to_oracle(o) == to_oracle(a) * L


def g1_arr(Pt):
    return np.zeros(8, dtype=np.uint64) if Pt is None else np.array(mont(Pt[0]) + mont(Pt[1]), dtype=np.uint64)


def g2_arr(Q):
    return np.zeros(16, dtype=np.uint64) if Q is None else np.array(pyref.g2_to_limbs(Q), dtype=np.uint64)


def run_pairing(pst, ps, Pt, Q):
    o = out12()
    pst.pst_pairing(ps, p_(o), p_(g1_arr(Pt)), p_(g2_arr(Q)))
    return o


@pytest.mark.parametrize("ps", PS)
def test_pairing_of_generators_equals_the_oracle(pst, ps, E):
    o = run_pairing(pst, ps, pyref.G1_GEN, pyref.G2_GEN)
    assert to_oracle(o) == E and (o == from_oracle(E)).all()
    # the Miller value may differ from the oracle's by subfield factors; the final exponentiation alone, on the oracle's Miller value, must agree as well
    f = pairing.miller_loop(pyref.G2_GEN, pyref.G1_GEN)
    o2 = out12(); pst.pst_final_exp(ps, p_(o2), p_(from_oracle(f)))
    assert to_oracle(o2) == E
    # cyclotomic squaring == squaring after the easy part, and differs from it before
    e1, s1, s2 = out12(), out12(), out12()
    pst.pst_final_exp_easy(ps, p_(e1), p_(from_oracle(f)))
    assert to_oracle(e1) == f ** ((P**6 - 1) * (P**2 + 1))
    pst.pst_fq12_cyclotomic_sqr(ps, p_(s1), p_(e1)); pst.pst_fq12_sqr(ps, p_(s2), p_(e1))
    assert (s1 == s2).all()
    pst.pst_fq12_cyclotomic_sqr(ps, p_(s1), p_(o)); pst.pst_fq12_sqr(ps, p_(s2), p_(o))
    assert (s1 == s2).all() and to_oracle(s1) == E * E


@pytest.mark.parametrize("ps", PS)
def test_pairing_is_bilinear_against_the_oracle(pst, ps, E):
    rng = np.random.default_rng(1804 + ps)
    for a, b in ((int(rng.integers(1, 2**62)) ** 4 % R, int(rng.integers(1, 2**62)) ** 4 % R), (R - 1, 2), (1, R - 1)):
        Pt, Q = pyref.g1_mul(pyref.G1_GEN, a), pyref.g2_mul(pyref.G2_GEN, b)
        o = run_pairing(pst, ps, Pt, Q)
        assert to_oracle(o) == E ** (a * b % R)
        n = run_pairing(pst, ps, pyref.g1_neg(Pt), Q)
        prod = out12(); pst.pst_fq12_mul(ps, p_(prod), p_(o), p_(n))
        assert to_oracle(prod) == F12.one()                               # e(P, Q) e(-P, Q) == 1
        m1, m2 = out12(), out12()                                         # and as ONE final exponentiation of the product of two Miller values
        pst.pst_miller(ps, p_(m1), p_(g1_arr(Pt)), p_(g2_arr(Q))); pst.pst_miller(ps, p_(m2), p_(g1_arr(pyref.g1_neg(Pt))), p_(g2_arr(Q)))
        pst.pst_fq12_mul(ps, p_(prod), p_(m1), p_(m2)); pst.pst_final_exp(ps, p_(prod), p_(prod.copy()))
        assert (prod == from_oracle(F12.one())).all()


@pytest.mark.parametrize("ps", PS)
def test_identity_on_either_side_gives_one(pst, ps):
    one = from_oracle(F12.one())
    Q = pyref.g2_mul(pyref.G2_GEN, 77)
    assert (run_pairing(pst, ps, None, Q) == one).all()
    assert (run_pairing(pst, ps, pyref.G1_GEN, None) == one).all()
    assert (run_pairing(pst, ps, None, None) == one).all()
    m = out12(); pst.pst_miller(ps, p_(m), p_(g1_arr(None)), p_(g2_arr(Q)))
    assert (m == one).all()


def test_pairing_of_adversarial_g1_points_equals_the_oracle(pst):
    """three G1 points with an adversarial coordinate word (zero-adjacent, on an edge of the field or of a limb grid), each against a random G2 multiple: the oracle's
    full pairing -- these points are not known multiples of the generator, so there is no cheap E^s"""
    from tests import gpu_common as gc
    abi, _, _ = gc.adversarial_g1_points("mont")
    pts, _, _ = gc.adversarial_g1_info("mont")
    rng = np.random.default_rng(1805)
    for n, i in enumerate((0, len(pts) // 2, len(pts) - 1)):
        Q = pyref.g2_mul(pyref.G2_GEN, int(rng.integers(1, 2**62)) ** 4 % R)
        assert pst.pst_g1_on_curve(p_(abi[i].copy())) == 1
        o = out12()
        pst.pst_pairing(n & 1, p_(o), p_(abi[i].copy()), p_(g2_arr(Q)))
        assert to_oracle(o) == pairing.pairing(Q, pts[i])
    off = abi[0].copy(); off[0] ^= np.uint64(1)
    assert pst.pst_g1_on_curve(p_(off)) == 0 and pst.pst_g1_on_curve(p_(np.zeros(8, dtype=np.uint64))) == 1


def test_off_subgroup_and_degenerate_inputs_do_not_trap(pst):
    """a Q outside the subgroup of order r (adversarial twist points), garbage words: the result is unspecified, the call returns"""
    from tests import gpu_common as gc
    limbs, _, _ = gc.adversarial_g2_points()
    for ps in PS:
        o = out12()
        pst.pst_pairing(ps, p_(o), p_(g1_arr(pyref.G1_GEN)), p_(limbs[3].copy()))
        junk = np.full(16, 2**64 - 1, dtype=np.uint64)
        pst.pst_pairing(ps, p_(o), p_(np.full(8, 2**64 - 1, dtype=np.uint64)), p_(junk))
        pst.pst_final_exp(ps, p_(o), p_(out12()))
        assert not o.any()                                                # 0 has no inverse: 0 in, 0 out
