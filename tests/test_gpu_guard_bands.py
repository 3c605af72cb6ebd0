"""
-m gpu: the guard-band sweep.  Every entry point of include/mi355zk.h that takes device pointers runs on INTERIOR, RAGGED views of one library block
(tests/guard_common.py): each operand starts at an odd element offset, has at least 64 KiB of poison on either side, and the sizes are the smallest at which the tail
logic of that kernel family changes.  After the call every byte of the block outside the declared write ranges must be what it was before -- the guards, the tail of a
ragged output, every read-only operand -- and the declared output must equal the CPU oracle word for word.  Every case runs under two poisons (A: 0xA5 bytes, no field
element, no curve point; B: a valid operand repeated); the oracle never sees the poison, so a result that differs under A or under B is a read past the end.

One row of TABLE per entry point (tests/test_guard_table_covers_header.py holds the table to the header), one parametrised test over the rows and their sizes.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from oracle import cref, pyref
from tests import frrand_common as fc
from tests import guard_common as gc
from tests import lookup_common as lc
from tests import perm_common as pc
from tests.gpu_common import adversarial_fr_words, affine_of, ints_to_words, rand_fr, rand_fr_full, words_to_ints

pytestmark = pytest.mark.gpu

R, P = pyref.R_MOD, pyref.P_MOD
MONT = pyref.MONT_R % R
RINV = pow(1 << 256, -1, R)
W_ONE, W_RM1 = ints_to_words([MONT])[0], ints_to_words([R - 1])[0]
ONE_Q = np.array(pyref.to_limbs(pyref.MONT_R % P), dtype=np.uint64)
KEY = bytes.fromhex("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f")
FR, AFF, JAC, G2 = 32, 64, 96, 128
GRID = "G+1"                                   # resolved on the device: multi_processor_count * 8 * 256 + 1, one word past a full sweep of the grid-stride kernels
FR_GRID = [1, 255, 257, GRID]
TILE16K = [1, 16383, 16385]                    # 256 lanes * EVAL_RUN = 16384 words per block
SCAN = [1, 2, 2047, 2049, 100003]              # 2048 words per scan tile
CURVE = [1, 255, 257]

TABLE = {}                                     # entry point -> (sizes, function(env, size))


def row(name, sizes):
    def deco(fn):
        assert name not in TABLE
        TABLE[name] = (list(sizes), fn)
        return fn
    return deco


# ------------------------------------------------------------------------------------------------ operands and oracles, computed once
@functools.lru_cache(maxsize=None)
def _fr_cached(tag, n):
    a = rand_fr_full(np.random.default_rng(abs(hash_tag(tag)) % (1 << 31)), n)
    pool = adversarial_fr_words()
    k = min(n // 2, pool.shape[0])
    a[n - k:] = pool[:k]                        # the edge words sit at the END of the vector, where the tail logic runs; r - 1 and 0 among them
    a.setflags(write=False)
    return a


def hash_tag(tag):
    return int.from_bytes(tag.encode()[:7].ljust(7, b"\0"), "little") + 7919 * len(tag)


def fr_words(tag, n):
    return _fr_cached(tag, int(n))


@functools.lru_cache(maxsize=None)
def power_words(factor_word, n):
    f = factor_word * RINV % R
    out, pw = [], MONT
    for _ in range(n):
        out.append(pw); pw = pw * f % R
    return ints_to_words(out)


@functools.lru_cache(maxsize=None)
def g1_affine(tag, n):
    """n curve points k_i G with two identities among them (n >= 8)"""
    sc = rand_fr(np.random.default_rng(hash_tag(tag) % (1 << 31)), n, full=False)
    pts = cref.g1_mul_generator_vec(sc)
    if n >= 8:
        pts[3] = 0; pts[n - 1] = 0
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def g1_jacobian(tag, n):
    """n Jacobian points in non-normalised representatives (x z^2, y z^3, z), identities (z = 0 over non-zero x, y) among them"""
    aff = g1_affine(tag, n)
    z = rand_fr(np.random.default_rng(hash_tag(tag) % (1 << 31) + 1), n, full=False)
    z[:, 3] &= np.uint64((1 << 59) - 1)                                         # below p
    z2 = cref.f_mul_vec(cref.FQ, z, z)
    jac = np.concatenate([cref.f_mul_vec(cref.FQ, np.ascontiguousarray(aff[:, :4]), z2), cref.f_mul_vec(cref.FQ, np.ascontiguousarray(aff[:, 4:]), cref.f_mul_vec(cref.FQ, z2, z)), z], axis=1)
    ident = ~aff.any(axis=1)
    jac[ident, :8] = z[ident][:, [0, 1, 2, 3, 0, 1, 2, 3]]
    jac[ident, 8:] = 0
    jac = np.ascontiguousarray(jac)
    jac.setflags(write=False)
    return jac


def normalised(aff):
    """[n,8] affine -> [n,12] as the library returns points: (x, y, R), identity all zero"""
    aff = np.asarray(aff, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((aff.shape[0], 12), dtype=np.uint64)
    out[:, :8] = aff
    out[aff.any(axis=1), 8:] = ONE_Q
    return out


@functools.lru_cache(maxsize=None)
def g2_affine(n):
    gen = cref.g2_generator()
    sc = rand_fr(np.random.default_rng(4242), 8, full=False)
    eight = np.stack([cref.g2_mul(gen, s) for s in sc])                          # eight distinct points tiled: the sum folds to eight scalar multiples
    pts = np.ascontiguousarray(eight[np.arange(n) % 8])
    pts.setflags(write=False)
    return pts


def g2_expected(bases, scalars):
    from tests.gpu_common import class_sums
    rinv_p = pow(pyref.MONT_R, -1, P)

    def to_py(l):
        c = [pyref.from_limbs(l[4 * k:4 * k + 4]) * rinv_p % P for k in range(4)]
        return ((c[0], c[1]), (c[2], c[3]))
    acc = None
    for j, s in enumerate(class_sums(scalars, 8)):
        if j < bases.shape[0]:
            acc = pyref.g2_add(acc, pyref.g2_mul(to_py(bases[j]), s))
    return np.array(pyref.g2_to_limbs(acc), dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ the environment of one case
class Env:
    def __init__(self, zk, poison, grid):
        self.zk, self.h2, self.capi, self.poison, self.grid = zk, zk.halo2, zk._capi, poison, grid
        self.lib, self.check, self.ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
        self.arenas, self.handles = [], []

    def n(self, size):
        return self.grid + 1 if size == GRID else size

    def arena(self, specs):
        ar = gc.Arena("device", gc.Arena.bytes_for(specs), self.poison, h2=self.h2, sync=lambda: self.check(self.lib.mi355_synchronize()))
        self.arenas.append(ar)
        return ar

    def table(self, views):
        """a host array of device pointers"""
        return (C.c_void_p * max(1, len(views)))(*[v if isinstance(v, int) else v.data_ptr() for v in views])

    def register(self, view, n):
        h = C.c_uint64()
        self.check(self.lib.mi355_srs_register_dev(self.ptr(view), n, 0, C.byref(h)))     # copy = 0: the library reads the view itself
        self.handles.append(h.value)
        return h.value

    def close(self):
        for h in self.handles:
            self.lib.mi355_srs_release(h)
        for ar in self.arenas:
            ar.free()


def vp(x):
    return C.c_void_p(x)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and (got == want).all(), "%s differs from the oracle: got %s, want %s" % (what, got.reshape(-1)[:12].tolist(), want.reshape(-1)[:12].tolist())


# ------------------------------------------------------------------------------------------------ grid-stride Fr kernels
@row("mi355_fr_vec_op_dev", FR_GRID)
def _vec_op(env, size):
    n = env.n(size)
    a, b = fr_words("vec_a", n), fr_words("vec_b", n)
    ar = env.arena([(n, FR)] * 3)
    A, D, B = ar.view(n, FR, a, "a"), ar.view(n, FR, None, "dst"), ar.view(n, FR, b, "b")
    for op, f in enumerate((cref.f_add_vec, cref.f_sub_vec, cref.f_mul_vec)):
        ar.run(lambda: env.check(env.lib.mi355_fr_vec_op_dev(op, env.ptr(D), env.ptr(A), env.ptr(B), n)), [(D, 0, n)], [(D, 0, f(cref.FR, a, b))])
    ar.run(lambda: env.check(env.lib.mi355_fr_vec_op_dev(2, env.ptr(A), env.ptr(A), env.ptr(B), n)), [(A, 0, n)], [(A, 0, cref.f_mul_vec(cref.FR, a, b))])      # dst aliases a


@row("mi355_fr_vec_axpy_dev", FR_GRID)
def _axpy(env, size):
    n = env.n(size)
    a, b, s = fr_words("vec_a", n), fr_words("vec_b", n), fr_words("scalar", 8)[0]
    sb = cref.f_mul_vec(cref.FR, b, np.ascontiguousarray(np.tile(s, (n, 1))))
    ar = env.arena([(n, FR)] * 3)
    B, A, D = ar.view(n, FR, b, "b"), ar.view(n, FR, a, "a"), ar.view(n, FR, None, "dst")
    ar.run(lambda: env.check(env.lib.mi355_fr_vec_axpy_dev(env.ptr(D), env.ptr(A), env.ptr(B), env.ptr(s), n)), [(D, 0, n)], [(D, 0, cref.f_add_vec(cref.FR, a, sb))])
    ar.run(lambda: env.check(env.lib.mi355_fr_vec_axpy_dev(env.ptr(D), None, env.ptr(B), env.ptr(s), n)), [(D, 0, n)], [(D, 0, sb)])


@row("mi355_fr_vec_mul_periodic_dev", FR_GRID)
def _periodic(env, size):
    n = env.n(size)
    data, table = fr_words("vec_a", n), np.ascontiguousarray(fr_words("periodic", 64)[:4])
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, data, "data")
    ar.run(lambda: env.check(env.lib.mi355_fr_vec_mul_periodic_dev(env.ptr(D), n, env.ptr(table), 4)), [(D, 0, n)], [(D, 0, cref.f_mul_vec(cref.FR, data, table[np.arange(n) & 3]))])


@row("mi355_fr_interleave_dev", FR_GRID)
def _interleave(env, size):
    n = env.n(size)
    q = 2 if size == GRID else 3                                                    # the grid-stride loop runs over the n rows of a part: two parts keep the arena at 64 MiB
    parts = [np.ascontiguousarray(np.roll(fr_words("vec_a", n), 5 * j + 1, axis=0)) for j in range(q)]
    ar = env.arena([(n, FR), (n, FR), (q * n, FR), (n, FR)][:q + 1])
    P = [None] * q
    P[1], P[0], D = ar.view(n, FR, parts[1], "part1"), ar.view(n, FR, parts[0], "part0"), ar.view(q * n, FR, None, "dst")
    if q == 3:
        P[2] = ar.view(n, FR, parts[2], "part2")
    want = np.ascontiguousarray(np.stack(parts, axis=1).reshape(q * n, 4))
    ar.run(lambda: env.check(env.lib.mi355_fr_interleave_dev(env.ptr(D), env.table(P), q, n)), [(D, 0, q * n)], [(D, 0, want)])


@row("mi355_buf_upload_packed", FR_GRID)
def _upload_packed(env, size):
    n = env.n(size)
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, None, "dst")
    rng = np.random.default_rng(77)
    for width, dt in ((1, np.uint8), (2, np.uint16), (4, np.uint32), (8, np.uint64)):
        vals = rng.integers(0, 1 << (8 * width), size=n, dtype=np.uint64, endpoint=False).astype(dt) if width < 8 else rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2 + 1
        vals[-1] = np.iinfo(dt).max
        can = np.zeros((n, 4), dtype=np.uint64); can[:, 0] = vals
        ar.run(lambda: env.check(env.lib.mi355_buf_upload_packed(env.ptr(D), env.ptr(vals), n, width)), [(D, 0, n)], [(D, 0, cref.f_from_canonical_vec(cref.FR, can))])


@row("mi355_buf_upload_sparse", FR_GRID)
def _upload_sparse(env, size):
    n = env.n(size)
    col = np.zeros((n, 4), dtype=np.uint64)
    idx = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(78).integers(0, n, size=min(n, 1000))])).astype(np.uint32)
    idx = idx[-(n - 2):] if n > 2 else idx[:0]                                     # at most n pairs are accepted, and two more follow; n = 1: only a dropped pair
    col[idx] = fr_words("vec_b", n)[idx]
    order = np.random.default_rng(79).permutation(idx.shape[0])
    # two pairs name indices n and n + 1: the contract drops them on the device -- they would land on the first words of the guard
    extra = [n, n + 1][:max(1, min(2, n - idx.shape[0]))]
    idx_x = np.ascontiguousarray(np.concatenate([idx[order], extra]).astype(np.uint32))
    vals_x = np.ascontiguousarray(np.concatenate([col[idx][order], np.tile(W_ONE, (len(extra), 1))]))
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, None, "dst")
    ar.run(lambda: env.check(env.lib.mi355_buf_upload_sparse(env.ptr(D), n, env.ptr(idx_x), env.ptr(vals_x), idx_x.shape[0])), [(D, 0, n)], [(D, 0, col)])


@row("mi355_buf_zero", FR_GRID)
def _buf_zero(env, size):
    n = env.n(size)
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, fr_words("vec_a", n), "dst")
    ar.run(lambda: env.check(env.lib.mi355_buf_zero(env.ptr(D), FR * n)), [(D, 0, n)], [(D, 0, np.zeros((n, 4), dtype=np.uint64))])


@row("mi355_buf_copy", FR_GRID)
def _buf_copy(env, size):
    n = env.n(size)
    a = fr_words("vec_a", n)
    ar = env.arena([(n, FR)] * 2)
    D, S = ar.view(n, FR, None, "dst"), ar.view(n, FR, a, "src")
    ar.run(lambda: env.check(env.lib.mi355_buf_copy(env.ptr(D), env.ptr(S), FR * n)), [(D, 0, n)], [(D, 0, a)])


@row("mi355_buf_upload", FR_GRID)
def _buf_upload(env, size):
    n = env.n(size)
    a = fr_words("vec_b", n)
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, None, "dst")
    ar.run(lambda: env.check(env.lib.mi355_buf_upload(env.ptr(D), env.ptr(a), FR * n)), [(D, 0, n)], [(D, 0, a)])


@row("mi355_buf_download", FR_GRID)
def _buf_download(env, size):
    n = env.n(size)
    a = fr_words("vec_b", n)
    ar = env.arena([(n, FR)])
    S = ar.view(n, FR, a, "src")
    out = np.full((n + 2, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)                 # the host side has its own guard words
    ar.run(lambda: env.check(env.lib.mi355_buf_download(vp(out.ctypes.data + 32), env.ptr(S), FR * n)))
    same(out[1:n + 1], a, "the downloaded words")
    assert (out[0] == 0x5A5A5A5A5A5A5A5A).all() and (out[n + 1] == 0x5A5A5A5A5A5A5A5A).all()


# ------------------------------------------------------------------------------------------------ the gate kernel
@row("mi355_fr_gate_eval_dev", [256, 257])
def _gate_eval(env, size):
    """the kernel wraps rotations modulo n, which the entry point requires to be a power of two: 257 rows are refused before any launch (and nothing may change), so the
    rotations -3, +5 and +3n - 1 run at n = 256, one row short of it.  A wrap that reads row n instead of row 0 meets poison."""
    n = size
    polys = [np.ascontiguousarray(np.roll(fr_words("gate", 257)[:n], 11 * j, axis=0)) for j in range(3)]
    ar = env.arena([(n, FR)] * 4)
    P0, D, P2, P1 = ar.view(n, FR, polys[0], "poly0"), ar.view(n, FR, None, "dst"), ar.view(n, FR, polys[2], "poly2"), ar.view(n, FR, polys[1], "poly1")
    terms = [(fr_words("scalar", 8)[1], [(0, -3), (1, 5)]), (W_ONE, [(2, 3 * n - 1)]), (W_RM1, [(1, 0), (0, 3 * n - 1), (2, -3)])]
    if n & (n - 1):
        with pytest.raises(env.capi.Mi355Error) as e:
            ar.run(lambda: env.h2.gate_eval(D, [P0, P1, P2], terms, n))
        assert e.value.code == env.capi.EBADARG
        ar.run(lambda: None)
        return
    coeffs = np.stack([c for c, _ in terms])
    tl = [len(f) for _, f in terms]; fp = [p for _, f in terms for p, _ in f]; fr_ = [r for _, f in terms for _, r in f]
    want = cref.gate_eval(polys, coeffs, tl, fp, fr_, n)
    ar.run(lambda: env.h2.gate_eval(D, [P0, P1, P2], terms, n), [(D, 0, n)], [(D, 0, want)])
    ar.run(lambda: env.h2.gate_eval(D, [P0, P1, P2], terms, n, accumulate=True), [(D, 0, n)], [(D, 0, cref.gate_eval(polys, coeffs, tl, fp, fr_, n, dst=want))])


# ------------------------------------------------------------------------------------------------ 16384-word block kernels
@row("mi355_distribute_powers_fr_dev", TILE16K)
def _distribute(env, size):
    n = size
    data, f = fr_words("distribute", n), int(words_to_ints(fr_words("scalar", 8)[2:3])[0])
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, data, "data")
    ar.run(lambda: env.check(env.lib.mi355_distribute_powers_fr_dev(env.ptr(D), n, env.ptr(ints_to_words([f])[0]))), [(D, 0, n)],
           [(D, 0, cref.f_mul_vec(cref.FR, data, np.ascontiguousarray(power_words(f, 16385)[:n])))])


@row("mi355_eval_polynomial_dev", TILE16K)
def _eval(env, size):
    n = size
    poly, x = fr_words("eval", n), fr_words("scalar", 8)[3]
    ar = env.arena([(n, FR)])
    V = ar.view(n, FR, poly, "poly")
    got, _ = ar.run(lambda: env.h2.eval_polynomial(V, x))
    same(got, cref.eval_polynomial(poly, x), "eval_polynomial")


@row("mi355_eval_polynomial_batch_dev", TILE16K)
def _eval_batch(env, size):
    n = size
    polys = [fr_words("eval", n), fr_words("eval2", n)]
    pts = [fr_words("scalar", 8)[3], W_RM1, fr_words("scalar", 8)[4]]
    ar = env.arena([(n, FR)] * 2)
    V1, V0 = ar.view(n, FR, polys[1], "poly1"), ar.view(n, FR, polys[0], "poly0")
    got, _ = ar.run(lambda: env.h2.eval_polynomial_many([V0, V1, V0], pts))
    same(got, np.stack([cref.eval_polynomial(polys[i], x) for i, x in zip((0, 1, 0), pts)]), "eval_polynomial_many")


# ------------------------------------------------------------------------------------------------ scans
@row("mi355_fr_batch_invert_dev", SCAN)
def _batch_invert(env, size):
    n = size
    a = fr_words("scan", n)
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, a, "data")
    ar.run(lambda: env.check(env.lib.mi355_fr_batch_invert_dev(env.ptr(D), n)), [(D, 0, n)], [(D, 0, cref.batch_invert(a))])


def _prefix(env, n, fn, oracle, what):
    a = fr_words("scan", n)
    want, want_total = oracle(a)
    ar = env.arena([(n, FR)] * 2)
    D, S = ar.view(n, FR, None, "dst"), ar.view(n, FR, a, "src")
    total = np.zeros(4, dtype=np.uint64)
    ar.run(lambda: env.check(fn(env.ptr(D), env.ptr(S), n, env.ptr(total))), [(D, 0, n)], [(D, 0, want)])
    same(total, want_total, what + " total")
    ar.run(lambda: env.check(fn(env.ptr(S), env.ptr(S), n, None)), [(S, 0, n)], [(S, 0, want)])                                  # in place, asynchronous


@row("mi355_fr_prefix_product_dev", SCAN)
def _prefix_product(env, size):
    _prefix(env, size, env.lib.mi355_fr_prefix_product_dev, cref.prefix_product, "prefix_product")


@row("mi355_fr_prefix_sum_dev", SCAN)
def _prefix_sum(env, size):
    _prefix(env, size, env.lib.mi355_fr_prefix_sum_dev, cref.prefix_sum, "prefix_sum")


@row("mi355_fr_kate_division_dev", SCAN)
def _kate(env, size):
    """n coefficients in, n - 1 out: word n - 1 of the destination is the first guard word"""
    n = size
    a, z = fr_words("scan", n), fr_words("scalar", 8)[5]
    want = cref.kate_division(a, z)
    ar = env.arena([(n, FR)] * 2)
    S, D = ar.view(n, FR, a, "poly"), ar.view(n, FR, None, "dst")
    ar.run(lambda: env.check(env.lib.mi355_fr_kate_division_dev(env.ptr(D) if n > 1 else None, env.ptr(S), n, env.ptr(z))), [(D, 0, n - 1)], [(D, 0, want)])
    # dst == poly + 1 element: the quotient replaces coefficients 1 .. n - 1, coefficient 0 stays
    ar.run(lambda: env.check(env.lib.mi355_fr_kate_division_dev(vp(S.at(1)) if n > 1 else None, env.ptr(S), n, env.ptr(z))), [(S, 1, n - 1)], [(S, 0, a[:1]), (S, 1, want)])


# ------------------------------------------------------------------------------------------------ transforms
def _omega(k):
    return ints_to_words([pyref.omega(k) * MONT % R])[0]


def _omega_inv(k):
    return ints_to_words([pow(pyref.omega(k), -1, R) * MONT % R])[0]


@row("mi355_ntt_fr_dev", [0, 1, 8, 9, 13, 19])
def _ntt(env, size):
    k = size
    a = fr_words("ntt", 1 << k)
    ar = env.arena([(1 << k, FR)])
    D = ar.view(1 << k, FR, a, "data")
    ar.run(lambda: env.check(env.lib.mi355_ntt_fr_dev(env.ptr(D), k, env.ptr(_omega(k)))), [(D, 0, 1 << k)], [(D, 0, cref.best_fft(a, _omega(k), k))])


@row("mi355_intt_fr_dev", [0, 1, 8, 9, 13])
def _intt(env, size):
    k = size
    a, div = fr_words("ntt", 1 << k), ints_to_words([pow(1 << k, -1, R) * MONT % R])[0]
    ar = env.arena([(1 << k, FR)])
    D = ar.view(1 << k, FR, a, "data")
    ar.run(lambda: env.check(env.lib.mi355_intt_fr_dev(env.ptr(D), k, env.ptr(_omega_inv(k)), env.ptr(div))), [(D, 0, 1 << k)], [(D, 0, cref.ifft(a, _omega_inv(k), k, div))])


def _coset_want(a, k, f):
    return cref.best_fft(cref.f_mul_vec(cref.FR, a, np.ascontiguousarray(power_words(f, 1 << 13)[:1 << k])), _omega(k), k)


@row("mi355_coset_ntt_fr_dev", [0, 1, 8, 9, 13])
def _coset_ntt(env, size):
    k = size
    n = 1 << k
    a, f = fr_words("ntt", n), int(words_to_ints(fr_words("scalar", 8)[6:7])[0])
    ar = env.arena([(n, FR)] * 2)
    D, S = ar.view(n, FR, None, "dst"), ar.view(n, FR, a, "coeffs")
    ar.run(lambda: env.check(env.lib.mi355_coset_ntt_fr_dev(env.ptr(D), env.ptr(S), k, env.ptr(ints_to_words([f])[0]), env.ptr(_omega(k)))), [(D, 0, n)], [(D, 0, _coset_want(a, k, f))])


@row("mi355_coeff_to_extended_dev", [(7, 9), (9, 11)])
def _coeff_to_extended(env, size):
    """2^k coefficients followed by poison, not by zeros: the zero padding of the extended vector is the kernel's business"""
    k, ext = size
    dom = env.h2.EvaluationDomain(5, k)
    assert dom.extended_k == ext
    a = fr_words("ntt", 1 << k)
    ar = env.arena([(1 << k, FR), (1 << ext, FR)])
    S, D = ar.view(1 << k, FR, a, "coeffs"), ar.view(1 << ext, FR, None, "dst")
    want = cref.coeff_to_extended(a, k, ext, dom.g_coset, dom.g_coset_inv, dom.extended_omega)
    ar.run(lambda: env.check(env.lib.mi355_coeff_to_extended_dev(env.ptr(D), env.ptr(S), k, ext, env.ptr(dom.g_coset), env.ptr(dom.g_coset_inv), env.ptr(dom.extended_omega))),
           [(D, 0, 1 << ext)], [(D, 0, want)])


@row("mi355_extended_to_coeff_dev", [9, 11])
def _extended_to_coeff(env, size):
    ext = size
    dom = env.h2.EvaluationDomain(5, ext - 2)
    a = fr_words("ntt", 1 << ext)
    ar = env.arena([(1 << ext, FR)])
    D = ar.view(1 << ext, FR, a, "data")
    want = cref.extended_to_coeff(a, ext, dom.g_coset, dom.g_coset_inv, dom.extended_omega_inv, dom.extended_ifft_divisor)
    ar.run(lambda: env.check(env.lib.mi355_extended_to_coeff_dev(env.ptr(D), ext, env.ptr(dom.g_coset), env.ptr(dom.g_coset_inv), env.ptr(dom.extended_omega_inv),
                                                                env.ptr(dom.extended_ifft_divisor))), [(D, 0, 1 << ext)], [(D, 0, want)])


@row("mi355_ntt_fr_batch_dev", [9])
def _ntt_batch(env, size):
    """three views of one arena, named by the pointer table in non-ascending order"""
    k = size
    n = 1 << k
    polys = [np.ascontiguousarray(np.roll(fr_words("ntt", n), 3 * j + 1, axis=0)) for j in range(3)]
    ar = env.arena([(n, FR)] * 3)
    V = [ar.view(n, FR, p, "poly%d" % j) for j, p in enumerate(polys)]
    order = [2, 0, 1]
    ar.run(lambda: env.check(env.lib.mi355_ntt_fr_batch_dev(env.table([V[j] for j in order]), 3, k, env.ptr(_omega(k)), None)), [(v, 0, n) for v in V],
           [(V[j], 0, cref.best_fft(polys[j], _omega(k), k)) for j in range(3)])
    div = ints_to_words([pow(n, -1, R) * MONT % R])[0]
    ar.run(lambda: env.check(env.lib.mi355_ntt_fr_batch_dev(env.table([V[j] for j in order]), 3, k, env.ptr(_omega_inv(k)), env.ptr(div))), [(v, 0, n) for v in V],
           [(V[j], 0, polys[j]) for j in range(3)])                                                                                   # ifft(fft(a)) = a, word for word


@row("mi355_coset_ntt_fr_batch_dev", [9])
def _coset_batch(env, size):
    k = size
    n = 1 << k
    f = int(words_to_ints(fr_words("scalar", 8)[6:7])[0])
    polys = [np.ascontiguousarray(np.roll(fr_words("ntt", n), 3 * j + 1, axis=0)) for j in range(3)]
    ar = env.arena([(n, FR)] * 6)
    S, D = [None] * 3, [None] * 3
    for j in (1, 0, 2):                                                            # sources and destinations interleaved in the arena, neither ascending
        D[j] = ar.view(n, FR, None, "dst%d" % j)
        S[j] = ar.view(n, FR, polys[j], "coeffs%d" % j)
    order = [2, 0, 1]
    ar.run(lambda: env.check(env.lib.mi355_coset_ntt_fr_batch_dev(env.table([D[j] for j in order]), env.table([S[j] for j in order]), 3, k, env.ptr(ints_to_words([f])[0]),
                                                                 env.ptr(_omega(k)))), [(d, 0, n) for d in D], [(D[j], 0, _coset_want(polys[j], k, f)) for j in range(3)])


# ------------------------------------------------------------------------------------------------ argument kernels
@row("mi355_fr_lookup_multiplicities_dev", [(300, 200, 250)])
def _lookup(env, size):
    """input_rows < n and table_rows < n: the rows behind them are POISON.  Under B that is the word of r - 1, which the table holds (a stray input row raises a count, a
    stray table row moves the last-row rule); under A it is a word the table lacks (a stray input row is reported missing)."""
    n, table_rows, input_rows = size
    rng = np.random.default_rng(31)
    table = np.ascontiguousarray(fr_words("lookup", n)[:table_rows]).copy()
    table[5] = np.frombuffer(gc.FR_B, dtype=np.uint64)                             # the word poison B repeats
    table[150] = table[7]                                                          # a repeated value: first and last row differ
    inputs = [np.ascontiguousarray(table[rng.integers(0, table_rows, size=input_rows)]) for _ in range(2)]
    inputs[1][input_rows - 1] = table[5]
    ar = env.arena([(n, FR)] * 4)
    I1, T, M, I0 = ar.view(n, FR, None, "input1"), ar.view(n, FR, None, "table"), ar.view(n, FR, None, "m"), ar.view(n, FR, None, "input0")
    T.upload(table); I0.upload(inputs[0]); I1.upload(inputs[1])                    # rows >= table_rows / input_rows stay poison
    full = lambda rows: np.concatenate([rows, np.zeros((n - rows.shape[0], 4), dtype=np.uint64)])
    for last in (0, 1):
        counts, missing = lc.reference_words(full(table), table_rows, [full(x) for x in inputs], input_rows, last=bool(last))
        assert missing is None
        miss = C.c_uint64(0)
        ar.run(lambda: env.check(env.lib.mi355_fr_lookup_multiplicities_dev(env.ptr(M), n, env.ptr(T), table_rows, env.table([I0, I1]), 2, input_rows, last, C.byref(miss))),
               [(M, 0, n)], [(M, 0, lc.counts_to_words(counts))])
        assert miss.value == lc.MISSING_NONE


@row("mi355_fr_permutation_sigma_dev", [8])
def _sigma(env, size):
    log_n = size
    n, n_cols = 1 << log_n, 3
    asm = env.h2.PermutationAssembly(n_cols, n)
    rng = np.random.default_rng(32)
    for _ in range(120):
        asm.copy(int(rng.integers(0, n_cols)), int(rng.integers(0, n)), int(rng.integers(0, n_cols)), int(rng.integers(0, n)))
    asm.copy(0, 0, 2, n - 1); asm.copy(1, n - 1, 2, 0)                             # the first and the last cell of columns
    cells, images = asm.overrides()
    omega = pyref.omega(log_n)
    ar = env.arena([(n, FR)] * n_cols)
    V = [None] * n_cols
    for j in (2, 0, 1):
        V[j] = ar.view(n, FR, None, "sigma%d" % j)
    want = pc.sigma_words(n_cols, log_n, asm.mapping, omega=omega)
    ar.run(lambda: env.h2.permutation_sigma(n_cols, log_n, ints_to_words([pc.DELTA * MONT % R])[0], ints_to_words([omega * MONT % R])[0], cells, images, out=V),
           [(v, 0, n) for v in V], [(V[j], 0, want[j]) for j in range(n_cols)])


@row("mi355_fr_nonzero_rows_dev", [1, 255, 257])
def _nonzero_rows(env, size):
    """read-only: the poison behind n is non-zero under A and under B, so a stray read changes the count"""
    n = size
    vecs = [np.zeros((n, 4), dtype=np.uint64) for _ in range(2)]
    vecs[0][n - 1] = W_ONE
    if n > 4:
        vecs[1][[0, 3, n - 2]] = fr_words("scalar", 8)[:3]; vecs[1][2, 3] = np.uint64(1 << 40)      # only the top limb set
    ar = env.arena([(n, FR)] * 2)
    V1, V0 = ar.view(n, FR, vecs[1], "vec1"), ar.view(n, FR, vecs[0], "vec0")
    (counts, rows), _ = ar.run(lambda: env.h2.nonzero_rows([V0, V1], cap=4))
    for v in range(2):
        nz = np.flatnonzero(vecs[v].any(axis=1))
        assert counts[v] == nz.size, (v, counts[v], nz.size)
        want = np.full(4, (1 << 64) - 1, dtype=np.uint64); want[:min(4, nz.size)] = nz[:4]
        same(rows[v], want, "nonzero_rows rows of vector %d" % v)


@row("mi355_fr_copy_check_dev", [8])
def _copy_check(env, size):
    log_n = size
    n = 1 << log_n
    cols = [np.ascontiguousarray(np.roll(fr_words("copy", n), j, axis=0)).copy() for j in range(3)]
    rng = np.random.default_rng(33)
    cells = np.concatenate([rng.integers(0, 3 * n, size=200), [0, n - 1, 3 * n - 1, 2 * n]]).astype(np.uint64)
    images = np.concatenate([rng.integers(0, 3 * n, size=200), [3 * n - 1, 2 * n, 0, n - 1]]).astype(np.uint64)
    flat = np.concatenate(cols)
    for t in range(0, cells.size, 2):                                              # every other pair is made to hold
        flat[int(images[t])] = flat[int(cells[t])]
    cols = [np.ascontiguousarray(flat[j * n:(j + 1) * n]) for j in range(3)]
    fails = np.flatnonzero((flat[cells.astype(np.int64)] != flat[images.astype(np.int64)]).any(axis=1))
    assert 0 < fails.size < cells.size
    ar = env.arena([(n, FR)] * 3)
    V = [None] * 3
    for j in (1, 2, 0):
        V[j] = ar.view(n, FR, cols[j], "col%d" % j)
    (n_failed, failed), _ = ar.run(lambda: env.h2.copy_check(V, cells, images, cap=8))
    assert n_failed == fails.size
    same(failed, fails[:8].astype(np.uint64), "copy_check failed pairs")


# ------------------------------------------------------------------------------------------------ randomness
@row("mi355_fr_random_dev", [65])
def _random(env, size):
    n = size
    ar = env.arena([(n, FR)])
    D = ar.view(n, FR, None, "dst")
    ar.run(lambda: env.h2.fr_random(D, KEY, 3, (1 << 32) - 7), [(D, 0, n)], [(D, 0, fc.elements(KEY, 3, (1 << 32) - 7, n))])


@row("mi355_fr_random_rows_dev", [65])
def _random_rows(env, size):
    n, rows, n_cols = size, 6, 3
    ar = env.arena([(n, FR)] * n_cols)
    V = [None] * n_cols
    for j in (1, 2, 0):
        V[j] = ar.view(n, FR, np.ascontiguousarray(np.roll(fr_words("vec_a", n), j, axis=0)), "col%d" % j)
    want = fc.elements(KEY, 1, 11, n_cols * rows).reshape(n_cols, rows, 4)
    ar.run(lambda: env.h2.fr_random_rows(V, n - rows, rows, KEY, 1, 11), [(v, n - rows, rows) for v in V], [(V[j], n - rows, want[j]) for j in range(n_cols)])


@row("mi355_fr_from_u512_dev", [65])
def _from_u512(env, size):
    n = size
    rows = fc.u512_rows(fc.extreme_u512()[:n])
    assert rows.size * rows.itemsize == 64 * n
    ar = env.arena([(n, 64), (n, FR)])
    S, D = ar.view(n, 64, rows, "src"), ar.view(n, FR, None, "dst")
    ar.run(lambda: env.h2.fr_from_u512(S, D), [(D, 0, n)], [(D, 0, fc.from_u512_bytes(rows))])


# ------------------------------------------------------------------------------------------------ curve
@row("mi355_g1_batch_normalize_dev", CURVE)
def _batch_normalize(env, size):
    n = size
    jac = g1_jacobian("norm", 257)[:n]
    ar = env.arena([(n, JAC), (n, AFF)])
    S, D = ar.view(n, JAC, jac, "jacobian", poison_b=gc.G1_JACOBIAN_B), ar.view(n, AFF, None, "affine", poison_b=gc.G1_AFFINE_B)
    ar.run(lambda: env.check(env.lib.mi355_g1_batch_normalize_dev(env.ptr(S), env.ptr(D), n)), [(D, 0, n)], [(D, 0, g1_affine("norm", 257)[:n])])


def _compressed(aff):
    return np.frombuffer(b"".join(cref.g1_compress(p) for p in aff), dtype=np.uint64).reshape(-1, 4)


@row("mi355_g1_compress_dev", CURVE)
def _compress(env, size):
    n = size
    aff = g1_affine("codec", 257)[:n]
    ar = env.arena([(n, AFF), (n, 32)])
    S, D = ar.view(n, AFF, aff, "affine", poison_b=gc.G1_AFFINE_B, align=16), ar.view(n, 32, None, "bytes", poison_b=gc.G1_COMPRESSED_B, align=16)
    ar.run(lambda: env.check(env.lib.mi355_g1_compress_dev(env.ptr(S), env.ptr(D), n)), [(D, 0, n)], [(D, 0, _compressed(aff))])


@row("mi355_g1_decompress_dev", CURVE)
def _decompress(env, size):
    n = size
    aff = g1_affine("codec", 257)[:n]
    ar = env.arena([(n, 32), (n, AFF)])
    S, D = ar.view(n, 32, _compressed(aff), "bytes", poison_b=gc.G1_COMPRESSED_B, align=16), ar.view(n, AFF, None, "affine", poison_b=gc.G1_AFFINE_B, align=16)
    bad = C.c_uint64(0)
    ar.run(lambda: env.check(env.lib.mi355_g1_decompress_dev(env.ptr(S), env.ptr(D), n, C.byref(bad))), [(D, 0, n)], [(D, 0, aff)])
    assert bad.value == (1 << 64) - 1                                              # under A the word behind the input is no point: a stray read would be reported


@row("mi355_g1_fixed_base_mul_dev", CURVE)
def _fixed_base(env, size):
    n = size
    sc = fr_words("fixed", n)
    ar = env.arena([(n, AFF), (n, FR)])
    D, S = ar.view(n, AFF, None, "points", poison_b=gc.G1_AFFINE_B), ar.view(n, FR, sc, "scalars")
    ar.run(lambda: env.check(env.lib.mi355_g1_fixed_base_mul_dev(env.ptr(D), env.ptr(S), n)), [(D, 0, n)], [(D, 0, cref.g1_mul_generator_vec(sc))])


@row("mi355_g1_fft_dev", [0, 3, 8])
def _g1_fft(env, size):
    k = size
    n = 1 << k
    jac = g1_jacobian("fft", 256)[:n]
    ar = env.arena([(n, JAC)])
    D = ar.view(n, JAC, jac, "points", poison_b=gc.G1_JACOBIAN_B)
    want = normalised(cref.g1_to_affine(cref.best_fft_g1(jac, _omega(k), k)))
    ar.run(lambda: env.check(env.lib.mi355_g1_fft_dev(env.ptr(D), k, env.ptr(_omega(k)))), [(D, 0, n)], [(D, 0, want)])


@row("mi355_g_to_lagrange_dev", [0, 3, 8])
def _g_to_lagrange(env, size):
    k = size
    n = 1 << k
    g = g1_affine("lagrange", 256)[:n]
    w_inv, n_inv = _omega_inv(k), ints_to_words([pow(n, -1, R) * MONT % R])[0]
    ar = env.arena([(n, AFF)] * 2)
    D, S = ar.view(n, AFF, None, "g_lagrange", poison_b=gc.G1_AFFINE_B), ar.view(n, AFF, g, "g", poison_b=gc.G1_AFFINE_B)
    ar.run(lambda: env.check(env.lib.mi355_g_to_lagrange_dev(env.ptr(S), env.ptr(D), k, env.ptr(w_inv), env.ptr(n_inv))), [(D, 0, n)], [(D, 0, cref.g_to_lagrange(g, k, w_inv, n_inv))])


@row("mi355_srs_setup_dev", [8])
def _srs_setup(env, size):
    k = size
    n = 1 << k
    tau = ints_to_words([0x1234567 * MONT % R])[0]
    g, gl, _, _ = cref.srs_setup(k, tau, _omega(k))
    ar = env.arena([(n, AFF)] * 2)
    GL, G = ar.view(n, AFF, None, "g_lagrange", poison_b=gc.G1_AFFINE_B), ar.view(n, AFF, None, "g", poison_b=gc.G1_AFFINE_B)
    ar.run(lambda: env.check(env.lib.mi355_srs_setup_dev(env.ptr(G), env.ptr(GL), k, env.ptr(tau), env.ptr(_omega(k)))), [(G, 0, n), (GL, 0, n)], [(G, 0, g), (GL, 0, gl)])


def _fold(jac):
    acc = np.zeros(12, dtype=np.uint64)
    for p in jac:
        acc = cref.g1_add(acc, p)
    return cref.g1_to_affine(acc)


@row("mi355_g1_sum_dev", CURVE)
def _g1_sum(env, size):
    n = size
    jac = g1_jacobian("sum", 257)[:n]
    ar = env.arena([(n, JAC)])
    S = ar.view(n, JAC, jac, "points", poison_b=gc.G1_JACOBIAN_B)
    out = np.zeros(12, dtype=np.uint64)
    ar.run(lambda: env.check(env.lib.mi355_g1_sum_dev(env.ptr(S), n, env.ptr(out))))
    same(affine_of(out), _fold(jac), "g1_sum")


# ------------------------------------------------------------------------------------------------ MSM: the basis is an arena view the library reads in place
MSM_N, MSM_OFF = 257, 3


def _msm_operands(env, n_scalars=1):
    bases = g1_affine("msm", MSM_N + MSM_OFF)
    scal = [np.ascontiguousarray(np.roll(fr_words("msm", MSM_N), 7 * j, axis=0)) for j in range(n_scalars)]
    ar = env.arena([(MSM_N, FR)] * n_scalars + [(MSM_N + MSM_OFF, AFF), (1, JAC)])
    S = [None] * n_scalars
    for j in reversed(range(n_scalars)):
        S[j] = ar.view(MSM_N, FR, scal[j], "scalars%d" % j)                        # behind them: poison; under B the scalar r - 1, which moves the sum if one more entry is read
    B = ar.view(MSM_N + MSM_OFF, AFF, bases, "bases", poison_b=gc.G1_AFFINE_B)
    return ar, bases, scal, S, B, env.register(B, MSM_N + MSM_OFF)


def _msm_want(bases, scal, off):
    return cref.g1_to_affine(cref.best_multiexp(scal, np.ascontiguousarray(bases[off:off + MSM_N]), threads=4))


@row("mi355_srs_register_dev", [MSM_N])
def _srs_register(env, size):
    """copy = 1 and copy = 0: registration reads n points and writes nothing; what the handle then serves is the view's points"""
    ar, bases, _, _, B, h0 = _msm_operands(env)
    h1 = C.c_uint64()
    ar.run(lambda: env.check(env.lib.mi355_srs_register_dev(env.ptr(B), MSM_N, 1, C.byref(h1))))
    env.handles.append(h1.value)
    for h, n in ((h0, MSM_N + MSM_OFF), (h1.value, MSM_N)):
        out = np.zeros((n, 8), dtype=np.uint64)
        ar.run(lambda: env.check(env.lib.mi355_srs_read_host(h, 0, n, env.ptr(out))))
        same(out, bases[:n], "srs_read_host")


@row("mi355_msm_g1_dev", [0, MSM_OFF])
def _msm_dev(env, size):
    off = size
    ar, bases, scal, S, B, h = _msm_operands(env)
    out = np.zeros(12, dtype=np.uint64)
    ar.run(lambda: env.check(env.lib.mi355_msm_g1_dev(h, off, env.ptr(S[0]), MSM_N, env.ptr(out))))
    same(affine_of(out), _msm_want(bases, scal[0], off), "msm_g1_dev")


@row("mi355_msm_g1_dev_async", [0, MSM_OFF])
def _msm_async(env, size):
    off = size
    ar, bases, scal, S, B, h = _msm_operands(env)
    O = ar.view(1, JAC, None, "out", poison_b=gc.G1_JACOBIAN_B)
    ar.run(lambda: env.check(env.lib.mi355_msm_g1_dev_async(h, off, env.ptr(S[0]), MSM_N, env.ptr(O))), [(O, 0, 1)], [(O, 0, normalised(_msm_want(bases, scal[0], off)))])


@row("mi355_msm_g1_batch_dev", [0, MSM_OFF])
def _msm_batch(env, size):
    off = size
    ar, bases, scal, S, B, h = _msm_operands(env, 3)
    out = np.zeros((3, 12), dtype=np.uint64)
    ar.run(lambda: env.check(env.lib.mi355_msm_g1_batch_dev(h, off, env.table([S[1], S[2], S[0]]), 3, MSM_N, env.ptr(out))))
    for i, j in enumerate((1, 2, 0)):
        same(affine_of(out[i]), _msm_want(bases, scal[j], off), "msm_g1_batch_dev vector %d" % j)


def _g2_operands(env, n_scalars):
    bases = g2_affine(MSM_N)
    scal = [np.ascontiguousarray(np.roll(fr_words("msm", MSM_N), 7 * j, axis=0)) for j in range(n_scalars)]
    ar = env.arena([(MSM_N, G2)] + [(MSM_N, FR)] * n_scalars)
    B = ar.view(MSM_N, G2, bases, "bases", poison_b=gc.G2_AFFINE_B)
    S = [ar.view(MSM_N, FR, scal[j], "scalars%d" % j) for j in range(n_scalars)]
    return ar, bases, scal, S, B


@row("mi355_msm_g2_dev", [MSM_N])
def _msm_g2(env, size):
    ar, bases, scal, S, B = _g2_operands(env, 1)
    got, _ = ar.run(lambda: env.h2.g2_msm_dev(B, S[0], MSM_N))
    same(got, g2_expected(bases, scal[0]), "msm_g2_dev")


@row("mi355_msm_g2_batch_dev", [MSM_N])
def _msm_g2_batch(env, size):
    ar, bases, scal, S, B = _g2_operands(env, 2)
    got, _ = ar.run(lambda: env.h2.g2_msm_batch_dev(B, [S[1], S[0]], MSM_N))
    for i, j in enumerate((1, 0)):
        same(got[i], g2_expected(bases, scal[j]), "msm_g2_batch_dev vector %d" % j)


# ------------------------------------------------------------------------------------------------ the sweep
def _case_id(name, size):
    s = "x".join(str(v) for v in size) if isinstance(size, tuple) else str(size)
    return "%s-%s" % (name[len("mi355_"):], s)


CASES = [(name, size) for name, (sizes, _) in TABLE.items() for size in sizes]


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    yield pkg
    pkg._capi.check(pkg._capi.lib().mi355_msm_set_window_bits(0))


@pytest.fixture(scope="module")
def grid(zk):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


def test_the_checker_sees_device_memory(zk, grid):
    """the same call with one word fewer declared than the contract writes: the arena must report exactly that word, on the device as on the host"""
    env = Env(zk, "B", grid)
    try:
        n = 257
        a, b = fr_words("vec_a", n), fr_words("vec_b", n)
        ar = env.arena([(n, FR)] * 3)
        A, D, B = ar.view(n, FR, a, "a"), ar.view(n, FR, None, "dst"), ar.view(n, FR, b, "b")
        call = lambda: env.check(env.lib.mi355_fr_vec_op_dev(0, env.ptr(D), env.ptr(A), env.ptr(B), n))
        with pytest.raises(gc.GuardViolation) as e:
            ar.run(call, [(D, 0, n - 1)])
        assert (e.value.view, e.value.anchor, e.value.offset, e.value.count <= 32) == ("dst", "start", n - 1, True)
        wrong = cref.f_add_vec(cref.FR, a, b).copy(); wrong[n - 1, 0] ^= np.uint64(1)
        with pytest.raises(gc.OracleMismatch):
            ar.run(call, [(D, 0, n)], [(D, 0, wrong)])
        ar.check_layout()
        assert all((v.data_ptr() - ar.base) % 64 == 32 for v in ar.views)           # element alignment and no more
    finally:
        env.close()


@pytest.mark.parametrize("poison", ["A", "B"])
@pytest.mark.parametrize("name,size", CASES, ids=[_case_id(n, s) for n, s in CASES])
def test_guard_bands(zk, grid, name, size, poison):
    env = Env(zk, poison, grid)
    try:
        TABLE[name][1](env, size)
    except zk._capi.Mi355Error as e:
        if e.code == zk._capi.EHIP:                                                 # the runtime reported a fault: nothing more is started on that device
            pytest.exit("HIP error in %s: %s" % (_case_id(name, size), e), returncode=3)
        raise
    finally:
        env.close()
