"""
-m gpu: the Fr kernels over the WHOLE field and on adversarial words, bit-exact on the raw 32-byte words against the CPU oracle.

tests/gpu_common.py::rand_fr, which the older parity tests draw from, stays below 2^252 -- a third of [0, r).  Here every operand comes from
rand_fr_full (uniform over [0, r)) or from the adversarial word pool (the edges of the field and of the 29-bit / 32-bit limb grids), at the sizes
where the kernels change path: the grid of the grid-stride kernels (G = compute units * 8 * 256), the 256 * EVAL_RUN = 16384 tile of eval_polynomial
and distribute_powers, the 2048 tile of the scans, every transform size up to 2^20 and every NTT plan knob the pass driver still reads.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from oracle import cref, pyref
from tests.gpu_common import (ALL_ONES_LIMBS, R, adversarial_fr_words, affine_of, full_range, ints_to_words, pool_pairs,
                              rand_fr, rand_points, tile_words, words_to_ints)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONT = pyref.MONT_R % R                     # the word of the value one
RINV = pow(1 << 256, -1, R)
POOL = adversarial_fr_words()
PAIR_A, PAIR_B = pool_pairs(POOL)
W_ZERO, W_ONE, W_MINUS_ONE, W_ALL_ONES, W_RM1 = (ints_to_words([v])[0] for v in (0, MONT, R - MONT, ALL_ONES_LIMBS, R - 1))


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    yield pkg
    pkg._capi.check(pkg._capi.lib().mi355_msm_set_window_bits(0))


@pytest.fixture(scope="module")
def grid(zk):
    """G: threads of one sweep of the grid-stride kernels of lib_ntt.hip (multiProcessorCount * 8 blocks of 256)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


def _grid_sizes(G):
    return [1, 255, 256, 257, G - 1, G, G + 1, 2 * G + 3]


def _up(zk, a):
    return zk.halo2.DeviceBuffer.from_host(np.ascontiguousarray(a, dtype=np.uint64))


def _with_pool_pairs(a, b):
    """the two vectors with the pool's ordered pairs written over their head (as many as fit)"""
    a, b = a.copy(), b.copy()
    k = min(a.shape[0], PAIR_A.shape[0])
    a[:k] = PAIR_A[:k]; b[:k] = PAIR_B[:k]
    return a, b


# ------------------------------------------------------------------------------------------------ element-wise kernels
@pytest.mark.parametrize("kind", ["pool", "full"])
@pytest.mark.parametrize("size", range(8))
def test_fr_vec_op_over_the_whole_field(zk, grid, size, kind):
    """mi355_fr_vec_op_dev add / sub / mul: every ordered pair of pool words and uniform words, around the grid size, dst distinct and aliased."""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    n = _grid_sizes(grid)[size]
    if kind == "pool":
        a, b = tile_words(PAIR_A, n), tile_words(PAIR_B, n)
    else:
        a, b = full_range("vec_a", n), full_range("vec_b", n)
    oracle = (cref.f_add_vec, cref.f_sub_vec, cref.f_mul_vec)
    A, B, D = _up(zk, a), _up(zk, b), zk.halo2.DeviceBuffer(32 * n)
    try:
        for op in (0, 1, 2):
            want = oracle[op](cref.FR, a, b)
            want_aa = oracle[op](cref.FR, a, a)
            for alias in ("distinct", "dst=a", "dst=b", "a=b=dst"):
                A.upload(a); B.upload(b)
                dst = {"distinct": D, "dst=a": A, "dst=b": B, "a=b=dst": A}[alias]
                check(lib.mi355_fr_vec_op_dev(op, ptr(dst), ptr(A), ptr(A if alias == "a=b=dst" else B), n))
                got = dst.fr()
                exp = want_aa if alias == "a=b=dst" else want
                bad = np.flatnonzero((got != exp).any(axis=1))
                assert bad.size == 0, (op, alias, n, int(bad[0]), got[bad[0]].tolist(), exp[bad[0]].tolist())
                if alias == "distinct":
                    assert (A.fr() == a).all() and (B.fr() == b).all()
    finally:
        A.free(); B.free(); D.free()


@pytest.mark.parametrize("size", [0, 3, 6, 7])
def test_fr_vec_axpy_over_the_whole_field(zk, grid, size):
    """mi355_fr_vec_axpy_dev: dst = a + s b and dst = s b for s in {0, one, -one, the all-ones-limbs word}, dst distinct, dst = a, dst = b."""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    n = _grid_sizes(grid)[size]
    a, b = _with_pool_pairs(full_range("vec_a", n), full_range("vec_b", n))
    A, B, D = _up(zk, a), _up(zk, b), zk.halo2.DeviceBuffer(32 * n)
    try:
        for s in (W_ZERO, W_ONE, W_MINUS_ONE, W_ALL_ONES):
            sb = cref.f_mul_vec(cref.FR, b, tile_words(s[None], n))
            want = cref.f_add_vec(cref.FR, a, sb)
            if (s == W_ZERO).all():
                assert (sb == 0).all() and (want == a).all()
            if (s == W_ONE).all():
                assert (sb == b).all()
            for with_a, alias in ((True, "distinct"), (True, "dst=a"), (True, "dst=b"), (False, "distinct"), (False, "dst=b")):
                A.upload(a); B.upload(b)
                dst = {"distinct": D, "dst=a": A, "dst=b": B}[alias]
                check(lib.mi355_fr_vec_axpy_dev(ptr(dst), ptr(A) if with_a else None, ptr(B), ptr(s), n))
                got = dst.fr()
                exp = want if with_a else sb
                bad = np.flatnonzero((got != exp).any(axis=1))
                assert bad.size == 0, (hex(words_to_ints(s)[0]), with_a, alias, n, int(bad[0]), got[bad[0]].tolist(), exp[bad[0]].tolist())
    finally:
        A.free(); B.free(); D.free()


@pytest.mark.parametrize("table_kind", ["pool", "full"])
@pytest.mark.parametrize("period", [1, 2, 4, 64, 4096])
def test_fr_vec_mul_periodic_matches_oracle(zk, grid, period, table_kind):
    """mi355_fr_vec_mul_periodic_dev directly: data[i] *= table[i mod period], n below / at / not a multiple of the period and past the grid."""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    sizes = [period, 3 * period + 5, grid + 1] + ([period // 2] if period > 1 else [])
    m = POOL.shape[0]
    # a pool table takes every seventh word (7 and 54 are coprime: the short tables start at r - 1, the long ones hold the whole pool)
    table = np.ascontiguousarray(POOL[(np.arange(period) * 7 + 3) % m] if table_kind == "pool" else full_range("periodic", 4096)[-period:])
    for n in sizes:
        # against a pool table the data walks the pool one word per period: every ordered pair of pool words meets once n >= 54 * period
        data = np.ascontiguousarray(POOL[(np.arange(n) // period) % m]) if table_kind == "pool" else full_range("periodic", n)
        want = cref.f_mul_vec(cref.FR, data, table[np.arange(n) & (period - 1)])
        d = _up(zk, data)
        try:
            check(lib.mi355_fr_vec_mul_periodic_dev(ptr(d), n, ptr(table), period))
            got = d.fr()
        finally:
            d.free()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (period, n, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def test_fr_vec_mul_periodic_rejects_bad_periods(zk):
    lib, capi = zk._capi.lib(), zk._capi
    data = full_range("periodic", 64)
    d = _up(zk, data)
    try:
        table = np.ascontiguousarray(tile_words(POOL, 8192))
        for period in (0, 3, 8192):
            assert lib.mi355_fr_vec_mul_periodic_dev(capi.ptr(d), 64, capi.ptr(table), period) == capi.EBADARG, period
        assert lib.mi355_fr_vec_mul_periodic_dev(capi.ptr(d), 64, None, 4) == capi.EBADARG
        assert (d.fr() == data).all()                                  # a refused call leaves the data alone
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ distribute_powers
DIST_FACTORS = {"one": MONT, "minus_one": R - MONT, "generator": 7 * MONT % R, "all_ones_limbs": ALL_ONES_LIMBS}   # Montgomery words


@functools.lru_cache(maxsize=None)
def _power_words(factor_word, n):
    """the Montgomery words of f^i, i < n, for the value f that `factor_word` stands for: Python integers"""
    f = factor_word * RINV % R
    out, pw = [], 1
    for _ in range(n):
        out.append(pw * (1 << 256) % R); pw = pw * f % R
    return ints_to_words(out)


@pytest.mark.parametrize("factor", list(DIST_FACTORS))
@pytest.mark.parametrize("n", [1, 255, 257, 16383, 16384, 16385, 32769, 100003])
def test_distribute_powers_at_the_tile_edges(zk, n, factor):
    """mi355_distribute_powers_fr_dev in place: a[i] *= f^i on full-range data around the 256 * EVAL_RUN = 16384 block and at sizes that are no
    power of two; the powers come from Python integers."""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    data = full_range("distribute", n)
    want = cref.f_mul_vec(cref.FR, data, _power_words(DIST_FACTORS[factor], 100003)[:n])
    for i in {0, n // 2, n - 1}:                                       # the vectorised product itself against integers
        assert words_to_ints(want[i:i + 1])[0] == words_to_ints(data[i:i + 1])[0] * pow(DIST_FACTORS[factor] * RINV, i, R) % R
    d = _up(zk, data)
    try:
        check(lib.mi355_distribute_powers_fr_dev(ptr(d), n, ptr(ints_to_words([DIST_FACTORS[factor]]))))
        got = d.fr()
    finally:
        d.free()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (factor, n, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


# ------------------------------------------------------------------------------------------------ eval_polynomial
@pytest.mark.parametrize("n", [16383, 16384, 16385, 32767, 32769, 3 * 16384 + 1])
def test_eval_polynomial_at_the_tile_edges(zk, n):
    """mi355_eval_polynomial_dev / _batch_dev / _host around the 16384-coefficient block: full-range and pool-tiled coefficients, at 0, one, -one, the
    all-ones-limbs word and a uniform word; the batch call mixes every (polynomial, point) pair in one launch."""
    h2 = zk.halo2
    polys = [full_range("eval", n), tile_words(POOL, n)]
    points = [W_ZERO, W_ONE, W_MINUS_ONE, W_ALL_ONES, full_range("eval", 3 * 16384 + 2)[-1]]
    want = np.stack([cref.eval_polynomial(p, x) for p in polys for x in points])
    ints = words_to_ints(polys[1])
    for j, x in enumerate(points):                                     # Horner over Python integers pins the oracle on the pool-tiled vector
        xv, acc = words_to_ints(x[None])[0] * RINV % R, 0
        for c in reversed(ints):
            acc = (acc * xv + c) % R
        assert words_to_ints(want[len(points) + j][None])[0] == acc
    dev = [_up(zk, p) for p in polys]
    try:
        got_batch = h2.eval_polynomial_many([d for d in dev for _ in points], points * len(polys))
        assert (got_batch == want).all(), (n, np.flatnonzero((got_batch != want).any(axis=1)).tolist())
        for i, (p, d) in enumerate(zip(polys, dev)):
            for j, x in enumerate(points):
                assert (h2.eval_polynomial(d, x) == want[i * len(points) + j]).all(), (n, i, j, "dev")
                assert (h2.eval_polynomial(p, x) == want[i * len(points) + j]).all(), (n, i, j, "host")
    finally:
        for d in dev:
            d.free()


# ------------------------------------------------------------------------------------------------ the gate kernel at its stated bounds
GATE_N = 1 << 12


def _gate_run(zk, polys_h, terms, dst_h=None, dst_is_poly=None):
    """one launch of mi355_fr_gate_eval_dev and the oracle's value of it (dst_h: accumulate onto it; dst_is_poly: dst aliases that operand)"""
    h2 = zk.halo2
    coeffs = np.stack([c for c, _ in terms])
    tl = [len(f) for _, f in terms]; fp = [p for _, f in terms for p, _ in f]; fr_ = [r for _, f in terms for _, r in f]
    want = cref.gate_eval(polys_h, coeffs, tl, fp, fr_, GATE_N, dst=dst_h)
    polys_d = [_up(zk, p) for p in polys_h]
    dst = polys_d[dst_is_poly] if dst_is_poly is not None else (_up(zk, dst_h) if dst_h is not None else h2.DeviceBuffer(32 * GATE_N))
    try:
        h2.gate_eval(dst, polys_d, terms, GATE_N, accumulate=dst_h is not None)
        got = dst.fr()
    finally:
        for d in polys_d:
            d.free()
        if dst_is_poly is None:
            dst.free()
    return got, want


@pytest.mark.parametrize("word", [R - 1, ALL_ONES_LIMBS])
def test_gate_eval_sixteen_general_terms_of_the_largest_words(zk, word):
    """the bound in frpoly.hpp (16 term values + dst below reduce_small's 64 r): 16 general-coefficient terms of 3 factors each (the 48-factor limit),
    every coefficient and every factor one large word, accumulated onto a dst full of r - 1.  Expected from integers, and from the oracle."""
    w = ints_to_words([word])[0]
    polys_h = [tile_words(w[None], GATE_N) for _ in range(3)]
    terms = [(w, [(j % 3, j - 8), ((j + 1) % 3, 0), ((j + 2) % 3, 3 * j)]) for j in range(16)]
    got, want = _gate_run(zk, polys_h, terms, dst_h=tile_words(W_RM1[None], GATE_N))
    value = (16 * pow(word, 4, R) * pow(RINV, 3, R) + R - 1) % R
    assert (want == ints_to_words([value])[0]).all()
    assert (got == want).all(), (got[0].tolist(), want[0].tolist())


def test_gate_eval_unit_coefficients_keep_zero_and_negate_the_largest_word(zk):
    """16 unit-coefficient terms, +1 and -1 alternating: the first factor is 0 on some rows and r - 1 on others (the -1 path negates the first
    factor: zero must stay zero), one-factor and three-factor terms."""
    first = tile_words(np.stack([W_ZERO, W_RM1, W_RM1, W_ZERO, W_ALL_ONES]), GATE_N)
    others = [full_range("gate", 6 * GATE_N)[i * GATE_N:(i + 1) * GATE_N] for i in range(2)]
    polys_h = [first] + others
    for length in (1, 3):
        terms = [(W_ONE if j % 2 == 0 else W_MINUS_ONE, [(0, j)] + [(1 + (j + q) % 2, q - j) for q in range(length - 1)]) for j in range(16)]
        got, want = _gate_run(zk, polys_h, terms)
        assert (got == want).all(), length
        got, want = _gate_run(zk, polys_h, terms, dst_h=tile_words(W_RM1[None], GATE_N))
        assert (got == want).all(), length
    # only -1 terms over a column of zeros: every row is exactly zero
    got, want = _gate_run(zk, [tile_words(W_ZERO[None], GATE_N)], [(W_MINUS_ONE, [(0, j)]) for j in range(16)])
    assert (want == 0).all() and (got == 0).all()
    # x - x over the pool: +1 and -1 of the same word cancel to the zero word, not to r
    col = tile_words(POOL, GATE_N)
    got, want = _gate_run(zk, [col], [(W_ONE, [(0, 0)]), (W_MINUS_ONE, [(0, 0)])] * 8)
    assert (want == 0).all() and (got == 0).all()


def test_gate_eval_longest_term_most_polynomials_and_aliasing(zk):
    """one term of 16 factors over 24 distinct polynomials (both per-launch limits), dst aliasing an un-rotated operand, and the random term-list
    shape of the older test with full-range operands."""
    rng = np.random.default_rng(9106)
    pool_col = tile_words(POOL, GATE_N)
    base = full_range("gate", 6 * GATE_N).reshape(6, GATE_N, 4)
    polys_h = [np.ascontiguousarray(np.roll(base[i % 6], 17 * i, axis=0)) if i % 5 else np.ascontiguousarray(np.roll(pool_col, i, axis=0)) for i in range(24)]
    terms = [(W_ALL_ONES, [(q, (q - 8) * 37) for q in range(16)]), (W_RM1, [(16 + q, -q) for q in range(8)])]
    got, want = _gate_run(zk, polys_h, terms)
    assert (got == want).all()
    # dst IS polynomial 2, which every term reads un-rotated
    terms = [(W_RM1, [(2, 0), (1, 5), (0, -3)]), (W_MINUS_ONE, [(2, 0)]), (W_ONE, [(3, 1), (2, 0)]), (W_ALL_ONES, [(2, 0), (2, 0)])]
    got, want = _gate_run(zk, polys_h[:4], terms, dst_is_poly=2)
    assert (got == want).all()
    for trial in range(4):
        nt = [1, 5, 16, 9][trial]
        terms = []
        for j in range(nt):
            ln = 0 if (trial == 1 and j == 2) else int(rng.integers(1, 4 if nt > 9 else 6))
            c = full_range("gate", 64)[int(rng.integers(0, 64))] if j % 3 else (W_ONE if j % 2 == 0 else W_MINUS_ONE)
            terms.append((c, [(int(rng.integers(0, 6)), int(rng.integers(-3 * GATE_N, 3 * GATE_N)) if j % 3 else int(rng.integers(-2, 3))) for _ in range(ln)]))
        got, want = _gate_run(zk, polys_h[:6], terms)
        assert (got == want).all(), trial
        got2, want2 = _gate_run(zk, polys_h[:6], terms, dst_h=want)
        assert (got2 == want2).all(), trial


# ------------------------------------------------------------------------------------------------ scans
def _scan_input(kind, n):
    if kind == "full":
        return full_range("scan", n)
    if kind == "pool":
        return tile_words(POOL, n)
    if kind == "pool_nonzero":
        return tile_words(POOL[1:], n)
    a = full_range("scan", n).copy()                                   # "zero_runs": runs of zeros across the 2048-element tile edge and at both ends
    a[:3] = 0; a[n - 2:] = 0; a[2040:min(n, 2051)] = 0
    return a


@pytest.mark.parametrize("kind", ["full", "pool", "pool_nonzero", "zero_runs"])
@pytest.mark.parametrize("n", [2047, 2048, 2049, 100003])
def test_scans_over_the_whole_field(zk, n, kind):
    """mi355_fr_batch_invert_dev, _prefix_product_dev, _prefix_sum_dev and _kate_division_dev around the 2048-element tile, every output word."""
    h2 = zk.halo2
    a = _scan_input(kind, n)
    d = _up(zk, a); out = h2.DeviceBuffer(32 * n)
    try:
        h2.batch_invert(d)
        assert (d.fr() == cref.batch_invert(a)).all(), "batch_invert"
        d.upload(a)
        _, total = h2.prefix_product(d, dst=out, want_total=True)
        wz, wt = cref.prefix_product(a)
        assert (out.fr() == wz).all() and (total == wt).all(), "prefix_product"
        _, total = h2.prefix_sum(d, dst=out, want_total=True)
        wz, wt = cref.prefix_sum(a)
        assert (out.fr() == wz).all() and (total == wt).all(), "prefix_sum"
        h2.prefix_sum(d, dst=d)
        assert (d.fr() == wz).all(), "prefix_sum in place"
        for z in (W_RM1, W_ALL_ONES, W_ONE, ints_to_words([(R + 1) // 2])[0]):          # z from the pool
            d.upload(a)
            h2.kate_division(d, z, dst=out)
            assert (out.fr()[: n - 1] == cref.kate_division(a, z)).all(), ("kate_division", hex(words_to_ints(z[None])[0]))
    finally:
        d.free(); out.free()


# ------------------------------------------------------------------------------------------------ transforms
def _ntt_inputs(k):
    n = 1 << k
    rng = np.random.default_rng(9200 + k)
    return {"full": full_range("ntt", n), "pool": tile_words(POOL, n), "largest": np.ascontiguousarray(np.stack([W_RM1, W_ALL_ONES])[rng.integers(0, 2, size=n)])}


@pytest.mark.parametrize("k", range(0, 21))
def test_best_fft_and_ifft_over_the_whole_field(zk, k):
    """best_fft and EvaluationDomain::ifft at every size up to 2^20 (2^21 and 2^22 cost 1.7 s and 3.1 s, most of it the oracle) against the oracle: uniform words, the pool tiled, and a shuffle of the two
    largest words (no butterfly output is zero, unlike a constant vector)."""
    h2 = zk.halo2
    dom = h2.EvaluationDomain(2, k)
    for name, a in _ntt_inputs(k).items():
        got = a.copy()
        h2.best_fft(got, dom.omega, k)
        assert (got == cref.best_fft(a, dom.omega, k)).all(), ("best_fft", name)
        got = a.copy()
        dom.lagrange_to_coeff(got)
        assert (got == cref.ifft(a, dom.omega_inv, k, dom.ifft_divisor)).all(), ("ifft", name)


@pytest.mark.parametrize("k,j", [(4, 4), (7, 3), (10, 5), (13, 4)])
def test_coset_extension_over_the_whole_field(zk, k, j):
    h2 = zk.halo2
    dom = h2.EvaluationDomain(j, k)
    coeffs = full_range("ntt", 1 << k)
    ext = dom.coeff_to_extended(coeffs)
    want = cref.coeff_to_extended(coeffs, k, dom.extended_k, dom.g_coset, dom.g_coset_inv, dom.extended_omega)
    assert ext.shape == want.shape and (ext == want).all()
    evals = full_range("ntt", 1 << dom.extended_k)                      # any vector, not only an image of coeff_to_extended
    back = dom.extended_to_coeff(evals)
    wantb = cref.extended_to_coeff(evals, dom.extended_k, dom.g_coset, dom.g_coset_inv, dom.extended_omega_inv, dom.extended_ifft_divisor)
    assert (back == wantb[: back.shape[0]]).all()


@pytest.mark.parametrize("k", [8, 9])
def test_batched_transforms_over_the_whole_field(zk, k):
    """mi355_ntt_fr_batch_dev (with and without a divisor) and mi355_coset_ntt_fr_batch_dev on each side of the smallest batched launch: single-pass
    plans (k <= 8) run the loop of single transforms, larger ones one launch per pass with blockIdx.y = polynomial.  (Above the upper limit,
    MI355_NTT_BATCH_MAX_LOG, the same loop runs: test_ntt_plan_knobs sets it to 0.)  Batches larger than one scratch chunk or one gridDim.y slice are in
    tests/test_gpu_ntt_batch_sweep.py."""
    h2 = zk.halo2
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    n = 1 << k
    dom = h2.EvaluationDomain(2, k)
    polys = list(_ntt_inputs(k).values())
    dev = [_up(zk, p) for p in polys]
    outs = [h2.DeviceBuffer(32 * n) for _ in polys]
    try:
        h2.best_fft_many(dev, dom.omega, k)
        for d, p in zip(dev, polys):
            assert (d.fr() == cref.best_fft(p, dom.omega, k)).all()
            d.upload(p)
        h2.best_fft_many(dev, dom.omega_inv, k, divisor=dom.ifft_divisor)
        for d, p in zip(dev, polys):
            assert (d.fr() == cref.ifft(p, dom.omega_inv, k, dom.ifft_divisor)).all()
            d.upload(p)
        dst = (C.c_void_p * len(polys))(*[o.data_ptr() for o in outs]); src = (C.c_void_p * len(polys))(*[d.data_ptr() for d in dev])
        check(lib.mi355_coset_ntt_fr_batch_dev(dst, src, len(polys), k, ptr(W_ALL_ONES), ptr(dom.omega)))
        check(lib.mi355_synchronize())
        pw = _power_words(ALL_ONES_LIMBS, 100003)[:n]
        for o, d, p in zip(outs, dev, polys):
            assert (o.fr() == cref.best_fft(cref.f_mul_vec(cref.FR, p, pw), dom.omega, k)).all()
            assert (d.fr() == p).all()                                  # the coefficients are only read
    finally:
        for d in dev + outs:
            d.free()


# ------------------------------------------------------------------------------------------------ NTT plan knobs (read once, at init: one child process each)
KNOB_SIZES = (9, 12, 13, 16, 20)
KNOB_SETTINGS = [
    {"MI355_NTT_TILE_LOG": "8"}, {"MI355_NTT_TILE_LOG": "10"}, {"MI355_NTT_TILE_LOG": "12"},
    {"MI355_NTT_TWO_LEVEL_MAX_LOG": "9"}, {"MI355_NTT_TWO_LEVEL_MAX_LOG": "20"},
    {"MI355_NTT_FOLD_SCALE": "0"},
    {"MI355_NTT_BATCH_MAX_LOG": "0"},
    {"MI355_NTT_DIRECT2_MIN_LOG": "0", "MI355_NTT_DIRECT2_MAX_LOG": "28"}, {"MI355_NTT_DIRECT2_MIN_LOG": "28", "MI355_NTT_DIRECT2_MAX_LOG": "0"},
    {"MI355_NTT_COSET_FOLD_MAX_LOG": "0"},          # the coset transform takes the separate k_distribute_powers pass, src != dst (the scaled copy)
]


@pytest.fixture(scope="module")
def knob_reference(tmp_path_factory):
    """inputs and the oracle's outputs for the knob children, computed once: forward and inverse at KNOB_SIZES, the coset transform at 2^16"""
    h2 = ge.load_package().halo2                # host-side constants only
    ref = {}
    for k in KNOB_SIZES:
        dom = h2.EvaluationDomain(2, k)
        a = full_range("ntt", 1 << k)
        ref["fwd%d" % k] = cref.best_fft(a, dom.omega, k)
        ref["inv%d" % k] = cref.ifft(a, dom.omega_inv, k, dom.ifft_divisor)
    dom = h2.EvaluationDomain(2, 16)
    data = full_range("distribute", 1 << 16)
    ref["coset16"] = cref.best_fft(cref.f_mul_vec(cref.FR, data, _power_words(ALL_ONES_LIMBS, 100003)[: 1 << 16]), dom.omega, 16)
    path = str(tmp_path_factory.mktemp("knobs") / "ref.npz")
    np.savez(path, **ref)
    return path


def _knob_child(ref_path):
    """runs in the child: every transform of the reference under the environment's plan knobs, bit-exact"""
    zk = ge.load_package(); zk.init(0)
    h2 = zk.halo2
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    ref = np.load(ref_path)
    for k in KNOB_SIZES:
        dom = h2.EvaluationDomain(2, k)
        a = full_range("ntt", 1 << k)
        got = a.copy(); h2.best_fft(got, dom.omega, k)
        assert (got == ref["fwd%d" % k]).all(), ("fwd", k)
        got = a.copy(); dom.lagrange_to_coeff(got)
        assert (got == ref["inv%d" % k]).all(), ("inv", k)
        if k in (12, 13):                                               # the batch entry points: two polynomials, forward and with the divisor
            dev = [_up(zk, a), _up(zk, a)]
            h2.best_fft_many(dev, dom.omega, k)
            assert all((d.fr() == ref["fwd%d" % k]).all() for d in dev), ("batch fwd", k)
            for d in dev:
                d.upload(a)
            h2.best_fft_many(dev, dom.omega_inv, k, divisor=dom.ifft_divisor)
            assert all((d.fr() == ref["inv%d" % k]).all() for d in dev), ("batch inv", k)
            for d in dev:
                d.free()
    dom = h2.EvaluationDomain(2, 16)
    data = full_range("distribute", 1 << 16)
    src, dst = _up(zk, data), h2.DeviceBuffer(32 << 16)
    check(lib.mi355_coset_ntt_fr_dev(ptr(dst), ptr(src), 16, ptr(W_ALL_ONES), ptr(dom.omega)))
    check(lib.mi355_synchronize())
    assert (dst.fr() == ref["coset16"]).all(), "coset"
    assert (src.fr() == data).all(), "coset source"
    src.free(); dst.free()
    print("KNOBS-OK")


@pytest.mark.parametrize("setting", KNOB_SETTINGS, ids=lambda s: ",".join("%s=%s" % (k[10:], v) for k, v in s.items()))
def test_ntt_plan_knobs(knob_reference, setting):
    """every MI355_NTT_* value that lib_core.hip parses is still read by the pass driver of lib_ntt.hip (build_plan, cols_for, fold_divisor,
    coset_fold_tables, ntt_batch_inplace): each setting gives the oracle's words."""
    code = "import sys; sys.path.insert(0, %r); import tests.test_gpu_fr_full_range as t; t._knob_child(%r)" % (ROOT, knob_reference)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **setting), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "KNOBS-OK" in r.stdout, (setting, r.stdout[-500:], r.stderr[-2500:])


# ------------------------------------------------------------------------------------------------ MSM scalars above 2^252
@pytest.fixture(scope="module")
def points(zk):
    return rand_points(np.random.default_rng(42), 2048)


# ------------------------------------------------------------------------------------------------ MSM plan knobs (read once, at init: one child process each)
MSM_KNOB_N = 2048
MSM_KNOB_TAU = 0x1234567
MSM_KNOB_SETTINGS = [
    {"MI355_FIXUP_MODE": "0"},
    {"MI355_FIXUP_MODE": "1"},
    {"MI355_FIXUP_MODE": "0", "MI355_TAIL_COOP_MAX": "0"},
    {"MI355_FIXUP_MODE": "0", "MI355_FIXUP_LANES_MAX_LOG": "0", "MI355_TAIL_COOP_MASK": "14"},
    {"MI355_FIXUP_MODE": "0", "MI355_FIXUP_SERIAL_MAX": "1"},
    {"MI355_TAIL_COOP_MASK": "0"},
    {"MI355_TAIL_COOP_MAX": "16777216"},
    {"MI355_REDUCE_MIN_CHUNK": "64", "MI355_REDUCE_CHAINS": "1024"},
    {"MI355_SORT_T1": "8192"},
    {"MI355_SORT_T2": "16384"},
    {"MI355_SORT_SPLIT": "2"},
    {"MI355_SORT_FB": "9"},
    {"MI355_SEG_MIN": "1", "MI355_SEG_FILL": "100"},
    {"MI355_SEG_FACTOR": "1"},
    {"MI355_HOST_CHUNKS": "4", "MI355_HOST_SLICE_MIN_LOG": "10"},      # the host path cuts 2 048 scalars into slices with a bucket set each, then k_msm_bucket_fold
]


def _witness_like(rng, n):
    """mostly 0 / 1, the rest below 2^16 (canonical), as Montgomery limbs (as in test_gpu_g2_msm.py)"""
    v = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    r = rng.random(n)
    v[r < 0.45] = 0
    v[(r >= 0.45) & (r < 0.9)] = 1
    can = np.zeros((n, 4), dtype=np.uint64); can[:, 0] = v
    return cref.f_from_canonical_vec(cref.FR, can)


def _g2_expected(bases, scalars):
    """sum of cref.g2_mul multiples combined with pyref.g2_add (expected() of test_gpu_g2_msm.py)"""
    rinv_p = pow(pyref.MONT_R, -1, pyref.P_MOD)
    acc = None
    for b, s in zip(bases, scalars):
        limbs = np.asarray(cref.g2_mul(b, s), dtype=np.uint64)
        pt = None
        if limbs.any():
            c = [pyref.from_limbs(limbs[4 * k:4 * k + 4]) * rinv_p % pyref.P_MOD for k in range(4)]
            pt = ((c[0], c[1]), (c[2], c[3]))
        acc = pyref.g2_add(acc, pt)
    return np.array(pyref.g2_to_limbs(acc), dtype=np.uint64)


@pytest.fixture(scope="module")
def msm_knob_reference(tmp_path_factory, points):
    """inputs and the oracle's results for the MSM knob children, computed once on the CPU"""
    n = MSM_KNOB_N
    rng = np.random.default_rng(4242)
    uniform = full_range("msm", n)
    ref = {"points": points, "g1_uniform": uniform, "g1_equal": np.repeat(uniform[7:8], n, axis=0), "g1_witness": _witness_like(rng, n)}
    for kind in ("uniform", "equal", "witness"):
        ref["want_g1_" + kind] = cref.g1_to_affine(cref.best_multiexp(ref["g1_" + kind], points))
    for j in range(9):                                                  # the batch entry point: 9 polynomials of 257 scalars (the first 3 alone as well)
        ref["want_batch%d" % j] = cref.g1_to_affine(cref.best_multiexp(uniform[199 * j:199 * j + 257], points[:257]))
    can = cref.f_to_canonical_vec(cref.FR, uniform)                     # window tables: commit against p(tau) G on the synthetic SRS
    p_tau, t = 0, 1
    for row in can:
        p_tau = (p_tau + sum(int(v) << (64 * i) for i, v in enumerate(row)) * t) % R; t = t * MSM_KNOB_TAU % R
    ref["want_commit"] = cref.g1_to_affine(cref.g1_mul(cref.g1_generator(), cref.fr_mont(p_tau)))
    gen = cref.g2_generator()
    g2 = np.stack([cref.g2_mul(gen, s) for s in rand_fr(rng, 1000, full=False)])
    ref["g2_bases"] = g2
    ref["g2_uniform"] = rand_fr(rng, 1000); ref["g2_equal"] = np.repeat(rand_fr(rng, 1, full=False), 1000, axis=0)
    for kind in ("uniform", "equal"):
        ref["want_g2_" + kind] = _g2_expected(g2, ref["g2_" + kind])
    ref["g2_batch"] = rand_fr(rng, 9 * 64).reshape(9, 64, 4)
    ref["want_g2_batch"] = np.stack([_g2_expected(g2[:64], sc) for sc in ref["g2_batch"]])
    path = str(tmp_path_factory.mktemp("msm_knobs") / "ref.npz")
    np.savez(path, **ref)
    return path


def _msm_knob_child(ref_path):
    """runs in the child: every MSM of the reference under the environment's plan knobs, bit-exact"""
    zk = ge.load_package(); zk.init(0)
    h2 = zk.halo2
    lib, check = zk._capi.lib(), zk._capi.check
    ref = np.load(ref_path)
    n, pts, uniform = MSM_KNOB_N, ref["points"], ref["g1_uniform"]
    for c in (0, 13, 16):                                               # c = 13: three levels of the segmented fix-up; c = 16: 2^19 buckets, one-lane running sums, two tree passes
        check(lib.mi355_msm_set_window_bits(c))
        for kind in ("uniform", "equal", "witness"):
            assert (affine_of(h2.best_multiexp(ref["g1_" + kind], pts)) == ref["want_g1_" + kind]).all(), ("g1", kind, c)
    check(lib.mi355_msm_set_window_bits(0))
    params = h2.ParamsKZG.from_host(11, pts, pts)
    for m in (3, 9):                                                    # 9: the staged pointer array
        dev = [_up(zk, uniform[199 * j:199 * j + 257]) for j in range(m)]
        got = params.commit_many(dev)
        for j in range(m):
            assert (affine_of(got[j]) == ref["want_batch%d" % j]).all(), ("batch", m, j)
        for d in dev:
            d.free()
    assert (affine_of(h2.best_multiexp(uniform, params.g_slice(0, n))) == ref["want_g1_uniform"]).all(), "host-pointer entry point"
    params.release()
    srs = h2.ParamsKZG.setup(11, MSM_KNOB_TAU)                          # window tables: all windows share one bucket set, no Horner
    srs.precompute()
    assert (affine_of(srs.commit(uniform)) == ref["want_commit"]).all(), "window tables"
    srs.release()
    g2 = ref["g2_bases"]
    for kind in ("uniform", "equal"):
        assert (h2.g2_msm(g2, ref["g2_" + kind]) == ref["want_g2_" + kind]).all(), ("g2", kind)
    db = h2.DeviceBuffer.from_host(g2[:64]); ds = [h2.DeviceBuffer.from_host(sc) for sc in ref["g2_batch"]]
    assert (h2.g2_msm_batch_dev(db, ds, 64) == ref["want_g2_batch"]).all(), "g2 batch of 9"
    for d in [db] + ds:
        d.free()
    print("MSM-KNOBS-OK")


@pytest.mark.parametrize("setting", MSM_KNOB_SETTINGS, ids=lambda s: ",".join("%s=%s" % (k[6:], v) for k, v in s.items()))
def test_msm_plan_knobs(msm_knob_reference, setting):
    """every MI355_* value that selects between the forms of the bucket pipeline (per-bucket / segmented fix-up, one-lane / quad tail kernels,
    chunk and tile choices, segment packing, host slices) gives the oracle's points: G1 under three window widths, the batch, host-pointer and
    window-table paths, and G2, which runs the same templated kernels."""
    code = "import sys; sys.path.insert(0, %r); import tests.test_gpu_fr_full_range as t; t._msm_knob_child(%r)" % (ROOT, msm_knob_reference)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **setting), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MSM-KNOBS-OK" in r.stdout, (setting, r.stdout[-500:], r.stderr[-2500:])


MSM_SPECIAL = [R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 253, pyref.FR_ZETA, R - pyref.FR_ZETA]     # canonical values


@pytest.mark.parametrize("n", [33, 257, 2048])
def test_best_multiexp_with_scalars_over_the_whole_field(zk, points, n):
    """best_multiexp with uniform scalars and the largest canonical values (the top window's large digits and the recode carry, which scalars
    below 2^252 never reach), under forced window widths."""
    h2 = zk.halo2
    lib, check = zk._capi.lib(), zk._capi.check
    sc = full_range("msm", n).copy()
    spots = np.linspace(0, n - 1, num=len(MSM_SPECIAL), dtype=int)
    for i, v in zip(spots, MSM_SPECIAL):
        sc[i] = h2.fr(v)
    want = cref.g1_to_affine(cref.best_multiexp(sc, points[:n]))
    for c in (0, 2, 13, 16):
        check(lib.mi355_msm_set_window_bits(c))
        try:
            got = affine_of(h2.best_multiexp(sc, points[:n]))
        finally:
            check(lib.mi355_msm_set_window_bits(0))
        assert (got == want).all(), c
