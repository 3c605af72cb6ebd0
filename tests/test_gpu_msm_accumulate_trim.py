"""-m gpu: full G1 MSMs through the trimmed accumulate kernel (x held negated between additions, eight-word identity test of the gathered base) against the C oracle, byte for
byte, at the smallest sizes at which bucket starts, flushes, first entries and the doubling / annihilation path all occur in one launch: n = 2^10 and
2^12, with window tables and without them, over five scalar sets; and the same five sets once through the G2 MSM, whose accumulate shares the walk."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import cref, pyref

from gpu_common import affine_of, rand_fr

pytestmark = pytest.mark.gpu
R, P = pyref.R_MOD, pyref.P_MOD
KINDS = ["uniform", "equal", "r_minus_1", "zeros60", "meet"]
SPECIAL = 64   # leading entries of the "meet" basis: repeated points, opposite pairs and identity entries under ONE scalar


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    yield pkg
    pkg._capi.check(pkg._capi.lib().mi355_msm_set_window_bits(0))


def scalars(kind, n, seed):
    rng = np.random.default_rng(seed)
    sc = rand_fr(rng, n)
    if kind == "equal":
        sc[:] = sc[0]
    elif kind == "r_minus_1":
        sc[:] = cref.fr_mont(R - 1)
    elif kind == "zeros60":
        sc[rng.random(n) < 0.6] = 0
    elif kind == "meet":
        sc[:SPECIAL] = sc[0]
    return sc


def neg_q(words):
    return cref.f_sub(cref.FQ, np.zeros(4, dtype=np.uint64), words)


@pytest.fixture(scope="module")
def g1_cases():
    """per n: (plain basis, the "meet" basis, {kind: (scalars, expected affine)}) -- the oracle runs once per case"""
    out = {}
    for log_n in (10, 12):
        n = 1 << log_n
        rng = np.random.default_rng(900 + log_n)
        ks = rng.integers(1, 2**62, size=(n, 4), dtype=np.uint64); ks[:, 1:] = 0
        pts = cref.g1_mul_generator_vec(cref.f_from_canonical_vec(cref.FR, ks))
        meet = pts.copy()
        meet[0:16] = pts[0]                                   # one point sixteen times
        for i in range(8):                                    # eight opposite pairs
            meet[16 + 2 * i + 1, :4] = meet[16 + 2 * i, :4]; meet[16 + 2 * i + 1, 4:] = neg_q(meet[16 + 2 * i, 4:])
        meet[32:40] = 0                                       # identity entries
        meet[40:48] = pts[1]; meet[48:56, :4] = pts[1, :4]; meet[48:56, 4:] = neg_q(pts[1, 4:])   # 8 P then 8 (-P): builds 8 P, then takes it down to the identity
        cases = {}
        for kind in KINDS:
            sc = scalars(kind, n, 1000 + log_n)
            basis = meet if kind == "meet" else pts
            cases[kind] = (sc, cref.g1_to_affine(cref.best_multiexp(sc, basis)))
        out[log_n] = (pts, meet, cases)
    return out


@pytest.fixture(scope="module")
def g1_params(zk, g1_cases):
    made = {}
    for log_n, (pts, meet, _) in g1_cases.items():
        for name, basis in (("plain", pts), ("meet", meet)):
            p = zk.halo2.ParamsKZG.from_host(log_n, basis, basis)
            p.precompute(lagrange=False)
            made[(log_n, name)] = p
    yield made
    for p in made.values():
        p.release()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("log_n", [10, 12])
def test_g1_msm_matches_oracle(zk, g1_cases, g1_params, log_n, tables, kind):
    sc, want = g1_cases[log_n][2][kind]
    params = g1_params[(log_n, "meet" if kind == "meet" else "plain")]
    zk._capi.check(zk._capi.lib().mi355_msm_set_window_bits(0 if tables else -1))
    try:
        got = affine_of(params.commit(sc))
        assert got.tobytes() == want.tobytes()
        basis = g1_cases[log_n][1 if kind == "meet" else 0]
        assert affine_of(zk.halo2.best_multiexp(sc, basis)).tobytes() == want.tobytes()      # ad-hoc bases: the same kernel behind the other entry point
    finally:
        zk._capi.check(zk._capi.lib().mi355_msm_set_window_bits(0))


G2_GENS = 32


@pytest.fixture(scope="module")
def g2_basis():
    """n = 2^10 G2 points over 32 distinct multiples of the generator: gen[i] = index, sgn[i] in {+1, -1, 0 (identity entry)}"""
    n = 1 << 10
    rng = np.random.default_rng(77)
    gen = cref.g2_generator()
    gens = np.stack([cref.g2_mul(gen, s) for s in rand_fr(rng, G2_GENS, full=False)])
    idx = np.arange(n) % G2_GENS
    sgn = np.ones(n, dtype=np.int64)
    idx[0:16] = 0                                             # the same layout of the leading entries as the G1 "meet" basis
    idx[16:32] = np.repeat(np.arange(1, 9), 2); sgn[17:32:2] = -1
    sgn[32:40] = 0
    idx[40:56] = 9; sgn[48:56] = -1
    bases = gens[idx].copy()
    for i in np.nonzero(sgn < 0)[0]:
        bases[i, 8:12] = neg_q(bases[i, 8:12]); bases[i, 12:16] = neg_q(bases[i, 12:16])
    bases[sgn == 0] = 0
    return gens, idx, sgn, bases


@pytest.mark.parametrize("kind", KINDS)
def test_g2_msm_matches_oracle(zk, g2_basis, kind):
    gens, idx, sgn, bases = g2_basis
    n = bases.shape[0]
    sc = scalars(kind, n, 2000)
    can = [pyref.from_limbs(r) for r in cref.f_to_canonical_vec(cref.FR, sc)]
    tot = [0] * G2_GENS
    for i in range(n):
        tot[idx[i]] += int(sgn[i]) * can[i]
    acc = None
    for j in range(G2_GENS):
        if tot[j] % R:
            q = cref.g2_mul(gens[j], cref.fr_mont(tot[j] % R))
            c = [pyref.from_limbs(q[4 * k:4 * k + 4]) * pow(pyref.MONT_R, -1, P) % P for k in range(4)]
            acc = pyref.g2_add(acc, ((c[0], c[1]), (c[2], c[3])))
    want = np.array(pyref.g2_to_limbs(acc), dtype=np.uint64)
    got = zk.halo2.g2_msm(bases, sc)
    assert got.tobytes() == want.tobytes()
