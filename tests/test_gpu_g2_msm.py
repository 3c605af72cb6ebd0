"""G2 MSM on the device (mi355_msm_g2_*) against the oracle: sums of cref.g2_mul scalar multiples combined with pyref.g2_add (and, for
small n, pure pyref), edge cases, at-size runs over tiled bases, consistency of the three entry points, errors and the reported plan."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import cref, pyref

from gpu_common import rand_fr

pytestmark = pytest.mark.gpu

R, P = pyref.R_MOD, pyref.P_MOD
RINV_P = pow(pyref.MONT_R, -1, P)


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    yield pkg
    pkg._capi.check(pkg._capi.lib().mi355_msm_set_window_bits(0))


def to_py(limbs):
    """G2Affine limbs (Montgomery) -> pyref point (None = identity)"""
    limbs = np.asarray(limbs, dtype=np.uint64)
    if not limbs.any():
        return None
    c = [pyref.from_limbs(limbs[4 * k:4 * k + 4]) * RINV_P % P for k in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


def canon(s_mont):
    return pyref.from_limbs(s_mont) * pow(pyref.MONT_R, -1, R) % R


def expected(bases, scalars):
    acc = None
    for b, s in zip(bases, scalars):
        acc = pyref.g2_add(acc, to_py(cref.g2_mul(b, s)))
    return np.array(pyref.g2_to_limbs(acc), dtype=np.uint64)


def rand_g2(rng, n):
    gen = cref.g2_generator()
    return np.stack([cref.g2_mul(gen, s) for s in rand_fr(rng, n, full=False)]) if n else np.zeros((0, 16), dtype=np.uint64)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 64, 255, 1000, 4097])
def test_g2_msm_small_sizes_match_oracle(zk, n):
    rng = np.random.default_rng(700 + n)
    bases, sc = rand_g2(rng, n), rand_fr(rng, n)
    got = zk.halo2.g2_msm(bases, sc)
    assert (got == expected(bases, sc)).all()
    if 0 < n <= 16:
        acc = None
        for b, s in zip(bases, sc):
            acc = pyref.g2_add(acc, pyref.g2_mul(to_py(b), canon(s)))
        assert to_py(got) == acc


def test_g2_msm_edge_cases(zk, kat):
    h2 = zk.halo2
    rng = np.random.default_rng(71)
    bases, sc = rand_g2(rng, 40), rand_fr(rng, 40)
    assert (h2.g2_msm(bases, np.zeros_like(sc)) == 0).all()                                  # all-zero scalars
    mixed = bases.copy(); mixed[::3] = 0                                                     # identity bases mixed in
    assert (h2.g2_msm(mixed, sc) == expected(mixed, sc)).all()
    neg = bases.copy()
    for i in range(20):                                                                      # P and -P with equal scalars
        q = to_py(bases[i]); neg[20 + i] = pyref.g2_to_limbs((q[0], ((-q[1][0]) % P, (-q[1][1]) % P)))
    same = sc.copy(); same[20:] = sc[:20]
    assert (h2.g2_msm(neg, same) == 0).all()
    rep = np.repeat(bases[:1], 33, axis=0); eq = np.repeat(sc[:1], 33, axis=0)                # doubling inside a bucket
    assert to_py(h2.g2_msm(rep, eq)) == pyref.g2_mul(to_py(bases[0]), 33 * canon(sc[0]) % R)
    gen, s_g2 = h2.g2_generator(), cref.g2_from_words(kat["yul"]["s_g2_words"])            # the generator and the production s_g2
    two = np.stack([gen, s_g2, gen, s_g2]); s4 = rand_fr(rng, 4)
    assert (h2.g2_msm(two, s4) == expected(two, s4)).all()


def _witness_like(rng, n):
    """mostly 0 / 1, the rest below 2^16 (canonical), as Montgomery limbs"""
    v = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    r = rng.random(n)
    v[r < 0.45] = 0
    v[(r >= 0.45) & (r < 0.9)] = 1
    can = np.zeros((n, 4), dtype=np.uint64); can[:, 0] = v
    return cref.f_from_canonical_vec(cref.FR, can)


def _class_sums(sc, period):
    """S_j = sum_{i = j mod period} s_i mod r (canonical), vectorised over 16-bit chunks"""
    can = cref.f_to_canonical_vec(cref.FR, sc).reshape(-1, period, 4)
    tot = [0] * period
    for limb in range(4):
        for k in range(4):
            part = ((can[:, :, limb] >> np.uint64(16 * k)) & np.uint64(0xffff)).sum(axis=0, dtype=np.uint64)
            for j in range(period):
                tot[j] += int(part[j]) << (64 * limb + 16 * k)
    return [t % R for t in tot]


PERIOD = 1024


@pytest.fixture(scope="module")
def tiled(zk):
    rng = np.random.default_rng(72)
    return rand_g2(rng, PERIOD)


@pytest.mark.parametrize("log_n", [20, 22])
@pytest.mark.parametrize("kind", ["uniform", "witness", "equal"])
def test_g2_msm_at_size(zk, tiled, log_n, kind):
    n = 1 << log_n
    rng = np.random.default_rng(log_n * 10 + len(kind))
    if kind == "uniform":
        sc = rand_fr(rng, n)
    elif kind == "witness":
        sc = _witness_like(rng, n)
    else:
        sc = np.repeat(rand_fr(rng, 1, full=False), n, axis=0)
    bases = np.tile(tiled, (n // PERIOD, 1))
    got = zk.halo2.g2_msm(bases, sc)
    sums = _class_sums(sc, PERIOD)
    want = expected(tiled, np.stack([cref.fr_mont(s) for s in sums]))
    assert (got == want).all()
    if log_n == 20:   # a real windowed schedule: W = ceil(255 / c), the G1 plan rule (plan_pass); one entry per (scalar, window)
        c, w, e = C.c_int(), C.c_int(), C.c_uint64()
        zk._capi.check(zk._capi.lib().mi355_msm_last_plan(C.byref(c), C.byref(w), C.byref(e)))
        assert c.value >= 8 and w.value == -(-255 // c.value) and e.value == n * w.value


def test_g2_msm_entry_points_agree(zk):
    h2 = zk.halo2
    rng = np.random.default_rng(73)
    n = 3000
    bases, scs = rand_g2(rng, n), [rand_fr(rng, n) for _ in range(4)]
    host = [h2.g2_msm(bases, s) for s in scs]
    assert (host[0] == expected(bases, scs[0])).all()
    db = h2.DeviceBuffer.from_host(bases)
    ds = [h2.DeviceBuffer.from_host(s) for s in scs]
    try:
        for i in range(4):
            assert (h2.g2_msm_dev(db, ds[i], n) == host[i]).all()
        batch = h2.g2_msm_batch_dev(db, ds, n)
        assert batch.shape == (4, 16) and (batch == np.stack(host)).all()
        assert (h2.g2_msm_dev(db, ds[0], n) == host[0]).all()                                  # a repeated call
        assert (h2.g2_msm(bases, scs[0]) == host[0]).all()
    finally:
        db.free()
        for d in ds:
            d.free()


def test_g2_msm_errors(zk):
    h2, capi = zk.halo2, zk._capi
    lib = capi.lib()
    rng = np.random.default_rng(74)
    bases, sc = rand_g2(rng, 16), rand_fr(rng, 16)
    bad = bases.copy(); bad[5, 8] ^= np.uint64(1)                                            # y changed: off the twist
    with pytest.raises(zk.Mi355Error) as ei:
        h2.g2_msm(bad, sc)
    assert ei.value.code == capi.EBADARG
    assert b"base 5 " in lib.mi355_last_error() and b"twist" in lib.mi355_last_error()
    out = np.zeros(16, dtype=np.uint64)
    assert lib.mi355_msm_g2_adhoc_host(None, capi.ptr(sc), 16, capi.ptr(out)) == capi.EBADARG
    assert lib.mi355_msm_g2_adhoc_host(capi.ptr(bases), None, 16, capi.ptr(out)) == capi.EBADARG
    assert lib.mi355_msm_g2_adhoc_host(capi.ptr(bases), capi.ptr(sc), 16, None) == capi.EBADARG
    assert lib.mi355_msm_g2_dev(None, None, 16, capi.ptr(out)) == capi.EBADARG
    assert lib.mi355_msm_g2_batch_dev(None, None, 1, 16, capi.ptr(out)) == capi.EBADARG
    assert (h2.g2_msm(bases, sc) == expected(bases, sc)).all()                                # a valid call afterwards
