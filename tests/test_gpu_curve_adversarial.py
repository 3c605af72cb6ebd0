"""
-m gpu: the curve kernels on points whose coordinate WORDS are adversarial, bit-exact against the CPU oracle.

Every other G1 / G2 point of the suite is a multiple of a generator: its words are uniform in [0, p).  Here the bases come from
tests/gpu_common.py::adversarial_g1_points / adversarial_g2_points: the Montgomery (or canonical) word of x or of y is an edge of the field, of the 29-bit
or the 32-bit limb grid, an alternating bit pattern or the word whose eight low 29-bit limbs are all ones -- the inputs of from_sat, fq29_neg_loaded,
the x-only identity test and the lazy bounds of g1_29.hpp / g1fft.hpp / g1codec.hpp / g2.hpp.  The y family comes in triples P, lambda P, lambda^2 P
(equal y, different x, sum = identity).  Sizes are the smallest at which the paths occur (see test_gpu_msm_accumulate_trim.py for the MSM).
The twist points are outside the subgroup of order r; their multiples come from cref.g2_mul, which tests/test_host_logic.py checks against Python
integers on these very points, combined with pyref.g2_add.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from oracle import cref, pyref
from tests.gpu_common import (R, adversarial_fq_ints, adversarial_fq_non_lifting, adversarial_g1_info, adversarial_g1_points, adversarial_g2_points,
                              affine_of, full_range, g1_neg_words, ints_to_words, tile_words, words_to_ints)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = pyref.P_MOD
RINV_P = pow(pyref.MONT_R, -1, P)
ONE_Q = np.array(pyref.to_limbs(pyref.MONT_R % P), dtype=np.uint64)
POOL, _, _ = adversarial_g1_points("mont")
_, _, TRIPLES = adversarial_g1_info("mont")
M = POOL.shape[0]
WINDOW_BITS = (0, 2, 13, 16)
KINDS = ("uniform", "equal", "r_minus_1", "witness")
BASES = ("tiled", "spread", "opposites", "triples")


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    yield pkg
    pkg._capi.check(pkg._capi.lib().mi355_msm_set_window_bits(0))


def _up(zk, a):
    return zk.halo2.DeviceBuffer.from_host(np.ascontiguousarray(a, dtype=np.uint64))


# ------------------------------------------------------------------------------------------------ G1 MSM
def _witness_like(rng, n):
    """mostly 0 / 1, the rest below 2^16 (canonical), as Montgomery limbs (as in test_gpu_g2_msm.py)"""
    v = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    r = rng.random(n)
    v[r < 0.45] = 0
    v[(r >= 0.45) & (r < 0.9)] = 1
    can = np.zeros((n, 4), dtype=np.uint64); can[:, 0] = v
    return cref.f_from_canonical_vec(cref.FR, can)


def msm_scalars(kind, n):
    if kind == "uniform":
        return full_range("msm", n)
    if kind == "equal":
        return np.repeat(full_range("msm", 8)[7:8], n, axis=0)
    if kind == "r_minus_1":                                   # every digit negative: fq29_neg_loaded on every y of the basis
        return np.repeat(cref.fr_mont(R - 1)[None, :], n, axis=0)
    return _witness_like(np.random.default_rng(5150 + n), n)


def msm_basis(name, n):
    """tiled: the pool repeated (equal points meet in buckets).  spread: each pool point once among random points (ordinary addends onto random
    accumulators).  opposites: the pool followed by the opposites of all its points, as often as it fits, then adjacent pairs P, -P: under one
    scalar everything cancels.  triples: the y-triples P, lambda P, lambda^2 P, whole triples only, then identity entries: under one scalar each
    triple cancels."""
    if name == "tiled":
        return tile_words(POOL, n)
    if name == "spread":
        rng = np.random.default_rng(6000 + n)
        ks = rng.integers(1, 2**62, size=(n, 4), dtype=np.uint64); ks[:, 1:] = 0
        out = cref.g1_mul_generator_vec(cref.f_from_canonical_vec(cref.FR, ks))
        out[(np.arange(M) * n) // M] = POOL
        return out
    if name == "opposites":
        block = np.concatenate([POOL, g1_neg_words(POOL)])
        whole = n // (2 * M)
        rest = (n - whole * 2 * M) // 2
        pairs = np.stack([POOL[:rest], g1_neg_words(POOL[:rest])], axis=1).reshape(-1, 8)
        out = np.concatenate([block] * whole + [pairs, np.zeros((n - whole * 2 * M - 2 * rest, 8), dtype=np.uint64)])
        return np.ascontiguousarray(out)
    tri = POOL[[i for t in TRIPLES for i in t]]
    out = np.zeros((n, 8), dtype=np.uint64)
    whole = n // tri.shape[0]
    out[:whole * tri.shape[0]] = np.tile(tri, (whole, 1))
    return out


@pytest.fixture(scope="module")
def msm_cases():
    """{(log_n, basis): (points, {kind: (scalars, expected affine)})}: the oracle runs once per case"""
    out = {}
    for log_n in (10, 11):
        n = 1 << log_n
        for name in BASES:
            pts = msm_basis(name, n)
            assert pts.shape == (n, 8)
            cases = {}
            for kind in KINDS:
                sc = msm_scalars(kind, n)
                cases[kind] = (sc, cref.g1_to_affine(cref.best_multiexp(sc, pts)))
            out[(log_n, name)] = (pts, cases)
    return out


def test_the_oracle_itself_on_64_pool_points(zk):
    """n = 64 pinned to Python integers (pyref.msm) as well as to the C oracle"""
    idx = np.linspace(0, M - 1, num=64, dtype=int)
    pts = np.ascontiguousarray(POOL[idx])
    py = [adversarial_g1_info("mont")[0][i] for i in idx]
    sc = full_range("msm", 64).copy()
    sc[5] = cref.fr_mont(R - 1); sc[6] = cref.fr_mont(pyref.FR_ZETA); sc[7] = sc[8]
    can = words_to_ints(cref.f_to_canonical_vec(cref.FR, sc))
    want = pyref.msm(can, py)
    xl, yl = pyref.g1_affine_to_limbs(want)
    want = np.array(xl + yl, dtype=np.uint64)
    assert (cref.g1_to_affine(cref.best_multiexp(sc, pts)) == want).all()
    lib, check = zk._capi.lib(), zk._capi.check
    for c in WINDOW_BITS:
        check(lib.mi355_msm_set_window_bits(c))
        try:
            got = affine_of(zk.halo2.best_multiexp(sc, pts))
        finally:
            check(lib.mi355_msm_set_window_bits(0))
        assert (got == want).all(), c


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("log_n", [10, 11])
def test_g1_msm_on_adversarial_bases(zk, msm_cases, log_n, basis):
    """host pointers under four window widths, a registered basis, commit_many of 3 and 9 columns, and the window tables of precompute(), whose
    builder batch-normalises multiples of these bases"""
    h2 = zk.halo2
    lib, check = zk._capi.lib(), zk._capi.check
    n = 1 << log_n
    pts, cases = msm_cases[(log_n, basis)]
    if basis in ("opposites", "triples"):
        assert not cases["equal"][1].any() and not cases["r_minus_1"][1].any(), "one scalar everywhere: the identity"
    try:
        for c in WINDOW_BITS:
            check(lib.mi355_msm_set_window_bits(c))
            for kind in KINDS:
                sc, want = cases[kind]
                assert (affine_of(h2.best_multiexp(sc, pts)) == want).all(), ("host pointers", c, kind)
        check(lib.mi355_msm_set_window_bits(0))
        params = h2.ParamsKZG.from_host(log_n, pts, pts)
        try:
            for c in (0, 13):
                check(lib.mi355_msm_set_window_bits(c))
                for kind in KINDS:
                    sc, want = cases[kind]
                    assert (affine_of(params.commit(sc)) == want).all(), ("registered", c, kind)
            check(lib.mi355_msm_set_window_bits(0))
            cols = [cases[KINDS[j % 4]][0] for j in range(9)]
            dev = [_up(zk, col) for col in cols]
            try:
                for m in (3, 9):                                  # 9: the staged pointer array
                    got = params.commit_many(dev[:m])
                    for j in range(m):
                        assert (affine_of(got[j]) == cases[KINDS[j % 4]][1]).all(), ("commit_many", m, j)
                params.precompute(lagrange=False)
                for kind in KINDS:
                    sc, want = cases[kind]
                    assert (affine_of(params.commit(sc)) == want).all(), ("window tables", kind)
                got = params.commit_many(dev[:3])
                for j in range(3):
                    assert (affine_of(got[j]) == cases[KINDS[j]][1]).all(), ("commit_many over window tables", j)
            finally:
                for d in dev:
                    d.free()
        finally:
            params.release()
    finally:
        check(lib.mi355_msm_set_window_bits(0))


# ------------------------------------------------------------------------------------------------ MSM plan knobs (read once, at init: one child process each)
KNOB_SETTINGS = [{"MI355_FIXUP_MODE": "0"}, {"MI355_FIXUP_MODE": "1"}, {"MI355_TAIL_COOP_MASK": "0"}]
KNOB_LOG_N = 11


@pytest.fixture(scope="module")
def knob_reference(tmp_path_factory, msm_cases):
    pts, cases = msm_cases[(KNOB_LOG_N, "tiled")]
    ref = {"points": pts}
    for kind in KINDS:
        ref["sc_" + kind], ref["want_" + kind] = cases[kind]
    path = str(tmp_path_factory.mktemp("curve_knobs") / "ref.npz")
    np.savez(path, **ref)
    return path


def _knob_child(ref_path):
    """runs in the child: the tiled pool under the environment's plan knobs, bit-exact"""
    zk = ge.load_package(); zk.init(0)
    h2 = zk.halo2
    lib, check = zk._capi.lib(), zk._capi.check
    ref = np.load(ref_path)
    pts = ref["points"]
    for c in (0, 13, 16):
        check(lib.mi355_msm_set_window_bits(c))
        for kind in KINDS:
            assert (affine_of(h2.best_multiexp(ref["sc_" + kind], pts)) == ref["want_" + kind]).all(), ("host pointers", c, kind)
    check(lib.mi355_msm_set_window_bits(0))
    params = h2.ParamsKZG.from_host(KNOB_LOG_N, pts, pts)
    for kind in KINDS:
        assert (affine_of(params.commit(ref["sc_" + kind])) == ref["want_" + kind]).all(), ("registered", kind)
    params.precompute(lagrange=False)
    for kind in KINDS:
        assert (affine_of(params.commit(ref["sc_" + kind])) == ref["want_" + kind]).all(), ("window tables", kind)
    params.release()
    print("CURVE-KNOBS-OK")


@pytest.mark.parametrize("setting", KNOB_SETTINGS, ids=lambda s: ",".join("%s=%s" % (k[6:], v) for k, v in s.items()))
def test_msm_plan_knobs_on_the_tiled_pool(knob_reference, setting):
    code = "import sys; sys.path.insert(0, %r); import tests.test_gpu_curve_adversarial as t; t._knob_child(%r)" % (ROOT, knob_reference)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **setting), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CURVE-KNOBS-OK" in r.stdout, (setting, r.stdout[-500:], r.stderr[-2500:])


# ------------------------------------------------------------------------------------------------ Jacobian representatives: FFT, normalise, sum
def jacobian_reps(pts, seed):
    """[n,8] affine -> [n,12] (x z^2, y z^3, z), the word of z drawn from the Fq word pool (non-zero); identity entries stay all-zero"""
    zs = [w for w in adversarial_fq_ints() if w]
    rng = np.random.default_rng(seed)
    out = np.zeros((pts.shape[0], 12), dtype=np.uint64)
    xs, ys = words_to_ints(pts[:, :4]), words_to_ints(pts[:, 4:])
    for i, (x, y) in enumerate(zip(xs, ys)):
        if x == 0 and y == 0:
            continue
        z = zs[int(rng.integers(0, len(zs)))]                 # Montgomery words throughout: a b R^-1 is the product's word
        z2 = z * z * RINV_P % P
        out[i] = pyref.to_limbs(x * z2 * RINV_P % P) + pyref.to_limbs(y * (z2 * z * RINV_P % P) * RINV_P % P) + pyref.to_limbs(z)
    return out


def pool_with_identities(n, seed=0):
    """the pool tiled to n points, every 7th entry from index 3 on (and a run across the 256 tile edge) the identity"""
    pts = tile_words(np.roll(POOL, -seed, axis=0), n).copy()
    pts[3::7] = 0
    if n > 300:
        pts[250:262] = 0
    return pts


@pytest.fixture(scope="module")
def fft_cases():
    """{k: (Jacobian input, the oracle's transform as affine points)}; k = 8 is added to the sizes of test_g1_fft_matches_oracle"""
    out = {}
    for k in (0, 1, 2, 3, 5, 7, 8, 10):
        n = 1 << k
        jac = jacobian_reps(pool_with_identities(n, seed=k) if n > 1 else POOL[:1].copy(), 7000 + k)
        w = cref.fr_mont(pow(pyref.FR_ROOT_OF_UNITY, 1 << (28 - k), R))
        out[k] = (jac, w, cref.g1_to_affine(cref.best_fft_g1(jac, w, k)))
    return out


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 7, 8, 10])
def test_g1_fft_on_adversarial_representatives(zk, fft_cases, k):
    import torch
    h2 = zk.halo2
    n = 1 << k
    jac, w, want = fft_cases[k]
    a = jac.copy(); h2.best_fft(a, w, k)
    got = np.stack([affine_of(a[i]) for i in range(n)])
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]
    d = torch.from_numpy(jac.view(np.int64)).cuda(); h2.best_fft(d, w, k)
    assert (d.cpu().numpy().view(np.uint64) == a).all()


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 7, 8, 10])
def test_g_to_lagrange_on_adversarial_points(zk, k):
    import torch
    h2 = zk.halo2
    n = 1 << k
    g = pool_with_identities(n, seed=k + 20) if n > 1 else POOL[7:8].copy()
    w_inv = pow(pow(pyref.FR_ROOT_OF_UNITY, 1 << (28 - k), R), R - 2, R)
    want = cref.g_to_lagrange(g, k, cref.fr_mont(w_inv), cref.fr_mont(pow(n, R - 2, R)))
    d = torch.from_numpy(g.view(np.int64)).cuda()
    got = h2.g_to_lagrange(d, k).cpu().numpy().view(np.uint64).reshape(n, 8)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]
    zk._capi.check(zk._capi.lib().mi355_g_to_lagrange_dev(zk._capi.ptr(d), zk._capi.ptr(d), k, zk._capi.ptr(h2.fr(w_inv)), zk._capi.ptr(h2.fr(pow(n, R - 2, R)))))
    zk._capi.check(zk._capi.lib().mi355_synchronize())
    assert (d.cpu().numpy().view(np.uint64).reshape(n, 8) == want).all(), "in place"


@pytest.mark.parametrize("n", [1, 255, 256, 257, M])
def test_batch_normalize_on_adversarial_representatives(zk, n):
    """host pointers and device buffers (the interface refuses overlapping buffers, so there is no in-place form to run)"""
    import torch
    h2 = zk.halo2
    pts = pool_with_identities(n, seed=n) if n > 1 else POOL[M - 1:].copy()
    jac = jacobian_reps(pts, 8000 + n)
    for i in range(5, n, 11):                                 # identity as z = 0 under arbitrary x, y
        jac[i, 8:] = 0
    want = cref.g1_to_affine(jac)
    assert (want[jac[:, 8:].any(axis=1)] == pts[jac[:, 8:].any(axis=1)]).all(), "the representatives stand for the pool points"
    got = h2.batch_normalize(jac)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]
    d_in = torch.from_numpy(jac.view(np.int64)).cuda()
    d_out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    h2.batch_normalize(d_in, d_out)
    zk._capi.check(zk._capi.lib().mi355_synchronize())
    assert (d_out.cpu().numpy().view(np.uint64) == want).all()


def _sum_dev(zk, jac):
    import torch
    out = np.zeros(12, dtype=np.uint64)
    d = torch.from_numpy(np.ascontiguousarray(jac).view(np.int64)).cuda()
    zk._capi.check(zk._capi.lib().mi355_g1_sum_dev(zk._capi.ptr(d), jac.shape[0], zk._capi.ptr(out)))
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, M])
def test_g1_sum_on_adversarial_representatives(zk, n):
    h2 = zk.halo2
    pts = pool_with_identities(n, seed=n + 1) if n > 1 else POOL[M - 2:M - 1].copy()
    jac = jacobian_reps(pts, 9000 + n)
    want = np.zeros(12, dtype=np.uint64)
    for row in jac:
        want = cref.g1_add(want, row)
    want = cref.g1_to_affine(want)
    assert (affine_of(h2.g1_sum(jac)) == want).all()
    assert (affine_of(_sum_dev(zk, jac)) == want).all()


def test_g1_sum_of_the_pool_and_its_opposites_is_the_identity(zk):
    jac = jacobian_reps(np.concatenate([POOL, g1_neg_words(POOL)]), 9500)
    assert not zk.halo2.g1_sum(jac).any() and not _sum_dev(zk, jac).any()
    tri = jacobian_reps(POOL[[i for t in TRIPLES for i in t]], 9501)
    assert not zk.halo2.g1_sum(tri).any() and not _sum_dev(zk, tri).any()
    assert not zk.halo2.g1_sum(tri[:3]).any() and (affine_of(zk.halo2.g1_sum(tri[:2])) == g1_neg_words(POOL[TRIPLES[0][2]:TRIPLES[0][2] + 1])[0]).all()


# ------------------------------------------------------------------------------------------------ codec
CODEC_N = (1 << 12) + 3


def _word_of(x, sign=0):
    return np.frombuffer((x | (sign << 254)).to_bytes(32, "little"), dtype=np.uint8)


@pytest.mark.parametrize("reading", ["canonical", "mont"])
def test_codec_on_adversarial_points(zk, reading):
    """canonical: the word the codec slices (the canonical x) is the adversarial word; mont: the ABI word compress reads is.  More than one block."""
    import torch
    h2 = zk.halo2
    pool, _, _ = adversarial_g1_points(reading)
    words1 = np.stack([np.frombuffer(cref.g1_compress(p), dtype=np.uint8) for p in pool])
    for w, p in zip(words1, pool):
        assert (cref.g1_decompress(w.tobytes()) == p).all()
    idx = np.arange(CODEC_N) % pool.shape[0]
    pts, words = np.ascontiguousarray(pool[idx]), np.ascontiguousarray(words1[idx])
    pts[11::97] = 0; words[11::97] = 0                        # identities in between
    got = h2.g1_decompress(words)
    assert got.shape == (CODEC_N, 8) and (got == pts).all(), np.nonzero((got != pts).any(axis=1))[0][:8]
    assert (h2.g1_compress(pts) == words).all()
    dw = torch.from_numpy(words.reshape(-1)).cuda()
    dp = h2.g1_decompress(dw)
    assert (dp.cpu().numpy().view(np.uint64).reshape(CODEC_N, 8) == pts).all()
    dc = h2.g1_compress(dp)
    torch.cuda.synchronize()
    assert torch.equal(dc, dw)


def test_codec_rejects_the_pool_words_that_are_no_x_coordinate(zk):
    import torch
    h2, capi = zk.halo2, zk._capi
    lib, ptr = capi.lib(), capi.ptr
    pool, _, _ = adversarial_g1_points("canonical")
    words1 = np.stack([np.frombuffer(cref.g1_compress(p), dtype=np.uint8) for p in pool])
    idx = np.arange(CODEC_N) % pool.shape[0]
    pts, words = np.ascontiguousarray(pool[idx]), np.ascontiguousarray(words1[idx])
    bad = [_word_of(x, s) for x in adversarial_fq_non_lifting("canonical") for s in (0, 1) if (x, s) != (0, 0)]
    for w in bad:
        assert cref.g1_decompress(w.tobytes()) is None
    assert len(bad) >= 20
    at = np.random.default_rng(93).permutation(np.arange(300, CODEC_N))[:len(bad)]
    for i, w in zip(at, bad):
        words[int(i)] = w
    first = int(at.min())
    out = np.full((CODEC_N, 8), 0xAB, dtype=np.uint64); where = C.c_uint64(0)
    assert lib.mi355_g1_decompress_host(ptr(words), ptr(out), CODEC_N, C.byref(where)) == capi.EBADARG and where.value == first
    ok = np.ones(CODEC_N, dtype=bool); ok[at] = False
    assert not out[~ok].any() and (out[ok] == pts[ok]).all(), "rejected slots hold the identity, the others are decoded all the same"
    dw = torch.from_numpy(words.reshape(-1)).cuda(); dout = torch.empty(CODEC_N * 64, dtype=torch.uint8, device="cuda"); where = C.c_uint64(0)
    assert lib.mi355_g1_decompress_dev(ptr(dw), ptr(dout), CODEC_N, C.byref(where)) == capi.EBADARG and where.value == first
    with pytest.raises(zk.Mi355Error) as e:
        h2.g1_decompress(words)
    assert e.value.code == capi.EBADARG and e.value.index == first
    for w in (bad[0], bad[len(bad) // 2], bad[-1]):           # one planted word in the last block: that index
        one = np.ascontiguousarray(words1[idx]); one[CODEC_N - 2] = w
        assert lib.mi355_g1_decompress_host(ptr(one), ptr(out), CODEC_N, C.byref(where)) == capi.EBADARG and where.value == CODEC_N - 2


# ------------------------------------------------------------------------------------------------ G2
G2_POOL, G2_PY, _ = adversarial_g2_points()
M2 = G2_POOL.shape[0]


def g2_to_py(limbs):
    limbs = np.asarray(limbs, dtype=np.uint64)
    if not limbs.any():
        return None
    c = [pyref.from_limbs(limbs[4 * k:4 * k + 4]) * RINV_P % P for k in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


def g2_neg_words(pts):
    out = np.asarray(pts, dtype=np.uint64).reshape(-1, 16).copy()
    for half in (slice(8, 12), slice(12, 16)):
        out[:, half] = ints_to_words([(P - v) % P for v in words_to_ints(out[:, half])])
    return out


def g2_expected(bases, scalars):
    """sum of cref.g2_mul multiples (the scalar acts as an integer: these points are outside the subgroup of order r) combined with pyref.g2_add"""
    acc = None
    for b, s in zip(bases, scalars):
        acc = pyref.g2_add(acc, g2_to_py(cref.g2_mul(b, s)))
    return np.array(pyref.g2_to_limbs(acc), dtype=np.uint64)


@pytest.fixture(scope="module")
def g2_cases():
    out = {}
    for n in (64, 1000):
        bases = tile_words(G2_POOL[np.linspace(0, M2 - 1, num=64, dtype=int)], n) if n == 64 else np.ascontiguousarray(G2_POOL[np.arange(n) % M2])
        uniform = full_range("msm", n)
        equal = np.repeat(uniform[7:8], n, axis=0)
        out[n] = (bases, {"uniform": (uniform, g2_expected(bases, uniform)), "equal": (equal, g2_expected(bases, equal))})
    return out


@pytest.mark.parametrize("n", [64, 1000])
def test_g2_msm_on_adversarial_twist_points(zk, g2_cases, n):
    h2 = zk.halo2
    bases, cases = g2_cases[n]
    for kind, (sc, want) in cases.items():
        assert (h2.g2_msm(bases, sc) == want).all(), kind
    half = n // 2                                             # the base set followed by its opposites: the identity
    both = np.concatenate([bases[:half], g2_neg_words(bases[:half])])
    for kind, (sc, _) in cases.items():
        s2 = np.concatenate([sc[:half], sc[:half]])
        assert not h2.g2_msm(both, s2).any(), ("opposites", kind)
    db = h2.DeviceBuffer.from_host(bases)
    ds = [h2.DeviceBuffer.from_host(cases[k][0]) for k in ("uniform", "equal", "uniform")]
    try:
        got = h2.g2_msm_batch_dev(db, ds, n)
        assert got.shape == (3, 16)
        assert (got[0] == cases["uniform"][1]).all() and (got[1] == cases["equal"][1]).all() and (got[2] == got[0]).all()
    finally:
        for d in [db] + ds:
            d.free()
    if n == 64:                                               # one term under r - 1 is what g2_mul gives (the scalar is the integer, never r - k on -P); Python integers alone on eight terms
        for b in bases[:4]:
            assert (h2.g2_msm(b[None, :], cref.fr_mont(R - 1)[None, :]) == h2.g2_mul(b, cref.fr_mont(R - 1))).all()
        sc = cases["uniform"][0]
        can = words_to_ints(cref.f_to_canonical_vec(cref.FR, sc[:8]))
        acc = None
        for b, k in zip(bases[:8], can):
            acc = pyref.g2_add(acc, pyref.g2_mul(g2_to_py(b), k))
        assert g2_to_py(h2.g2_msm(bases[:8], sc[:8])) == acc


@pytest.mark.parametrize("scalar", ["r_minus_1", "zeta", "uniform"])
def test_g2_mul_on_every_adversarial_twist_point(zk, scalar):
    """one lane's double-and-add per call (about 16 ms), hence one case per scalar"""
    h2 = zk.halo2
    uniform = full_range("msm", M2)
    for i in range(M2):
        s = {"r_minus_1": cref.fr_mont(R - 1), "zeta": cref.fr_mont(pyref.FR_ZETA), "uniform": uniform[i]}[scalar]
        assert (h2.g2_mul(G2_POOL[i], s) == cref.g2_mul(G2_POOL[i], s)).all(), i
