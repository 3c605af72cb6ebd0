"""
The mixed addition that k_msm_accumulate runs (g1_29.hpp, the NEGX form: x negated between additions, two carry passes fewer) compiled for the CPU
(tests/hostcheck/madd_trim_selftest.cpp) and compared with the C oracle, exactly and in canonical affine form.  Every addition is also checked
against the limb and value bounds g1_29.hpp documents for an accumulator.  CPU only.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cref, pyref

HERE = os.path.dirname(os.path.abspath(__file__))
P, R = pyref.P_MOD, pyref.R_MOD
M29 = (1 << 29) - 1


@pytest.fixture(scope="module")
def mt():
    src = os.path.join(HERE, "hostcheck", "madd_trim_selftest.cpp")
    so = os.path.join(HERE, "hostcheck", "libmaddtrimselftest.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    for f in (lib.mt_bucket_sums, lib.mt_madd_raw, lib.mt_madd_core_raw):
        f.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def pool():
    """4096 distinct points k G (k odd and random, so no two are equal or opposite) -- computed once"""
    rng = random.Random(2029)
    ks = rng.sample(range(1, 1 << 62), 4096)
    sc = np.stack([cref.fr_mont(k) for k in ks])
    return cref.g1_mul_generator_vec(sc)


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def neg(pt):
    r = pt.copy()
    if r.any():
        r[4:] = cref.f_sub(cref.FQ, np.zeros(4, dtype=np.uint64), pt[4:])
    return r


def oracle_sum(pts, signs):
    acc = np.zeros(12, dtype=np.uint64)
    for pt, s in zip(pts, signs):
        acc = cref.g1_add_affine(acc, neg(pt) if s else pt)
    return acc


def sums(mt, seqs):
    """seqs: list of lists of (point[8], sign) -> (device-code results, oracle results), both [n, 8] canonical affine words"""
    pts = np.ascontiguousarray(np.stack([pt for seq in seqs for pt, _ in seq]))
    signs = (C.c_uint8 * len(pts))(*[s for seq in seqs for _, s in seq])
    off = np.cumsum([0] + [len(seq) for seq in seqs]).astype(np.uint64)
    out = np.zeros((len(seqs), 8), dtype=np.uint64)
    bad = mt.mt_bucket_sums(p_(out), p_(pts), signs, p_(off), C.c_uint64(len(seqs)))
    assert bad == 0, "accumulator left its documented bounds: mask %#x" % bad
    want = cref.g1_to_affine(np.stack([oracle_sum([pt for pt, _ in seq], [s for _, s in seq]) for seq in seqs]))
    return out, want


def test_random_triples(mt, pool):
    """12 000 (accumulator, point, sign) triples: the accumulator is itself a signed sum of two points (so zz, zzz are not one and x, y are lazy)"""
    rng = random.Random(41)
    seqs = []
    for _ in range(12000):
        a, b, c = rng.sample(range(len(pool)), 3)
        seqs.append([(pool[a], rng.randrange(2)), (pool[b], rng.randrange(2)), (pool[c], rng.randrange(2))])
    got, want = sums(mt, seqs)
    assert (got == want).all()


def test_edge_cases_by_construction(mt, pool):
    A, B, Cc, D = pool[0], pool[1], pool[2], pool[3]
    Z = np.zeros(8, dtype=np.uint64)
    AB = cref.g1_to_affine(cref.g1_add_affine(cref.g1_add_affine(np.zeros(12, dtype=np.uint64), A), B))
    seqs = [
        [(A, 0)], [(A, 1)],                                      # first point into an empty accumulator, both signs
        [(A, 0), (A, 0)], [(A, 1), (A, 1)],                      # doubling (tight accumulator), both signs
        [(A, 0), (B, 0), (AB, 0)], [(A, 1), (B, 1), (AB, 1)],    # doubling with a lazy accumulator (zz != 1)
        [(A, 0), (A, 0), (B, 1), (Cc, 0)],                       # doubling, then ordinary additions on its output
        [(A, 0), (A, 1), (B, 0)], [(A, 1), (A, 0), (B, 1)],      # annihilation, then a further point (first-point path again)
        [(A, 0), (B, 0), (AB, 1), (Cc, 0), (D, 1)],              # annihilation of a lazy accumulator, then two more
        [(A, 0), (A, 1)],                                        # annihilation as the last step
        [(A, 0), (Z, 0), (B, 0)], [(A, 1), (Z, 1), (B, 1)],      # an identity addend between two real ones
        [(Z, 0), (A, 0)], [(Z, 0), (Z, 1)], [(A, 0), (B, 0), (Z, 0)],
        [(A, 0)] * 64, [(A, 1)] * 37,                            # one doubling, then a long chain on the same addend
    ]
    got, want = sums(mt, seqs)
    assert (got == want).all()
    assert not got[10].any() and not got[14].any()


def _limbs(v, fat=False):
    """9 limbs of the integer v; fat: 2^29 borrowed into every limb below the top wherever the next limb can lend it (limbs <= 2^30 - 2)"""
    l = [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]
    if fat:
        for i in range(8):
            if l[i + 1] >= 1 and l[i] + (1 << 29) <= (1 << 30) - 2:
                l[i] += 1 << 29; l[i + 1] -= 1
    assert sum(x << (29 * i) for i, x in enumerate(l)) == v
    return l


def _val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def test_accumulator_at_the_top_of_its_ranges(mt, pool):
    """x pushed to just below 14 p and y to just below 6.1 p with fat limbs (<= 2^30 - 2) -- the loosest accumulator the invariants admit -- as the
    left operand of ordinary additions, a doubling and an annihilation; chains of 300 additions alternating the sign give what the code itself reaches."""
    rng = random.Random(43)
    for trial in range(60):
        a, b, c = rng.sample(range(len(pool)), 3)
        acc = np.zeros(36, dtype=np.uint32)
        assert mt.mt_madd_raw(p_(acc), p_(pool[a]), 0) == 0 and mt.mt_madd_raw(p_(acc), p_(pool[b]), trial & 1) == 0
        base = oracle_sum([pool[a], pool[b]], [0, trial & 1])
        x, y = _val(acc[0:9]), _val(acc[9:18])
        x += (14 * P - 1 - x) // P * P
        y += (61 * P // 10 - 1 - y) // P * P
        assert 13 * P <= x < 14 * P and 5 * P <= y < 61 * P // 10
        acc[0:9] = _limbs(x); acc[9:18] = _limbs(y, fat=True)
        assert max(acc[9:17]) <= (1 << 30) - 2 and min(acc[9:17]) >= 1 << 28
        mode = trial % 4
        if mode == 2:
            add, s = cref.g1_to_affine(base), 0       # equals the accumulator: doubling
        elif mode == 3:
            add, s = cref.g1_to_affine(base), 1       # its opposite: annihilation
        else:
            add, s = pool[c], mode
        assert mt.mt_madd_raw(p_(acc), p_(add), s) == 0
        d = rng.randrange(len(pool)); assert mt.mt_madd_raw(p_(acc), p_(pool[d]), 1) == 0
        out = np.zeros(8, dtype=np.uint64); mt.mt_finish(p_(out), p_(acc))
        want = cref.g1_to_affine(cref.g1_add_affine(cref.g1_add_affine(base, neg(add) if s else add), neg(pool[d])))
        assert (out == want).all(), trial
    seqs = [[(pool[rng.randrange(len(pool))], (i + k) & 1) for i in range(300)] for k in range(4)]
    got, want = sums(mt, seqs)
    assert (got == want).all()


def test_y2_representatives(mt, pool):
    """madd_core with y2 given as different representatives of the same residue: the re-sliced ABI words, the exact residue (< p), the residue plus p
    limb by limb (every limb raised by p's limb; where the residue's limb is 0 the limb IS p's limb), p's limbs plus a residue whose low limbs are
    zero, and the 64 p - y form a negative digit loads.  All must give the same point."""
    pl = _limbs(P)
    rng = random.Random(47)
    for trial in range(40):
        a, b = rng.sample(range(len(pool)), 2)
        q = pool[b]
        x2 = np.zeros(9, dtype=np.uint32); y2 = np.zeros(9, dtype=np.uint32)
        mt.mt_from_sat(p_(x2), p_(q[:4].copy())); mt.mt_from_sat(p_(y2), p_(q[4:].copy()))
        yres = _val(y2) % P
        reps = [(_limbs(_val(y2)), 0), (_limbs(yres), 0), ([u + v for u, v in zip(_limbs(yres), pl)], 1),
                ([u + v for u, v in zip(_limbs(yres + 2 * P), pl)], 1), (_limbs(yres + 50 * P), 0)]
        want = cref.g1_to_affine(oracle_sum([pool[a], q], [0, 0]))
        for first in (False, True):           # as the second point of a bucket, and as its first (reduce_small path)
            for limbs, norm in reps:
                acc = np.zeros(36, dtype=np.uint32)
                if not first:
                    assert mt.mt_madd_raw(p_(acc), p_(pool[a]), 0) == 0
                assert mt.mt_madd_core_raw(p_(acc), p_(x2), p_(np.array(limbs, dtype=np.uint32)), norm) == 0
                out = np.zeros(8, dtype=np.uint64); mt.mt_finish(p_(out), p_(acc))
                assert (out == (q if first else want)).all(), (trial, first, limbs)
    # residues with limbs AT 0 and AT p's limbs are no curve points' y in general, so the field path alone is checked for them: acc = A, addend (x_B, y')
    # is off the curve but the formulas are polynomial identities -- compare with the same addition done with the exact residue of y' written differently
    A, B = pool[5], pool[6]
    x2 = np.zeros(9, dtype=np.uint32); mt.mt_from_sat(p_(x2), p_(B[:4].copy()))
    for yv in (0, P, 2 * P, 1, P - 1, P + 1):
        outs = []
        for limbs in (_limbs(yv), _limbs(yv + 3 * P), [u + v for u, v in zip(_limbs(yv), pl)] if yv < 3 * P else _limbs(yv)):
            acc = np.zeros(36, dtype=np.uint32)
            assert mt.mt_madd_raw(p_(acc), p_(A), 0) == 0
            assert mt.mt_madd_core_raw(p_(acc), p_(x2), p_(np.array(limbs, dtype=np.uint32)), 1) == 0
            out = np.zeros(8, dtype=np.uint64); mt.mt_finish(p_(out), p_(acc)); outs.append(out)
        assert (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all(), yv


def test_column_sum_bounds_of_the_lazy_operand():
    """Worst-case column accumulators for the limb bounds the NEGX form hands to mul_sub (second operand NOT carried: limbs <= 2^29 + 8 + fat29_4p(i))
    and to sqr / mul (Pd = U2 + xn, limbs <= 2^30 + 7), from the constants themselves: the signed accumulator must stay inside 63 bits, the unsigned one
    inside 64."""
    f4 = [0x21f3f51c, 0x241182da, 0x31ca8d3b, 0x2b548b42, 0x361765df, 0x2b6d0301, 0x229b8503, 0x397098cf, 0xc19138]
    assert _val(f4) == 4 * P
    pl = _limbs(P)
    top = lambda k10: (k10 * P // 10 >> 232) + 1

    def worst(a, b, c=None, d=None):
        pos = neg_ = w = 0
        for k in range(17):
            idx = [(i, k - i) for i in range(9) if 0 <= k - i < 9]
            pos = (pos >> 29) + sum(a[i] * b[j] for i, j in idx) + sum(M29 * pl[j] for i, j in idx)
            if c: neg_ = (neg_ >> 29) + sum(c[i] * d[j] for i, j in idx)
            w = max(w, pos, neg_)
        return w

    rd = [M29 + 9] * 8 + [top(100)]
    t = [M29 + 9 + f4[i] for i in range(8)] + [top(140) + f4[8]]
    y1 = [(1 << 30) - 2] * 8 + [top(70)]
    ppp = [M29] * 8 + [top(20)]
    assert worst(rd, t, y1, ppp) < 1 << 63
    pd = [(1 << 30) + 7] * 8 + [top(160)]
    assert worst(pd, pd) < 1 << 64 and worst(pd, [M29] * 9) < 1 << 64


# ---- addends whose coordinate WORDS are adversarial (tests/gpu_common.py::adversarial_g1_points): the edges of the field and of the 29-bit / 32-bit limb
# grids as the Montgomery word of x or of y, where from_sat, fq29_neg_loaded and the first-point path reduce_small + normalise + sub4 can be wrong without
# a random point noticing.  The pool above (4096 random points) supplies the accumulators.
@pytest.fixture(scope="module")
def adv():
    from tests import gpu_common as gc
    pts, _, _ = gc.adversarial_g1_points("mont")
    _, _, triples = gc.adversarial_g1_info("mont")
    return pts, triples


def test_adversarial_addends_in_every_position(mt, pool, adv):
    """each pool point, with both signs, as the first point of a bucket followed by two random points, and as the second and the third point onto
    random accumulators"""
    pts, _ = adv
    rng = random.Random(51)
    seqs = []
    for q in pts:
        for s in (0, 1):
            a, b = rng.sample(range(len(pool)), 2)
            ra, rb = (pool[a], rng.randrange(2)), (pool[b], rng.randrange(2))
            seqs += [[(q, s), ra, rb], [ra, (q, s), rb], [ra, rb, (q, s)], [(q, s)]]
    got, want = sums(mt, seqs)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]


def test_adversarial_addends_doubled_and_annihilated(mt, pool, adv):
    pts, _ = adv
    rng = random.Random(52)
    seqs, zero = [], []
    for q in pts:
        for s in (0, 1):
            r = (pool[rng.randrange(len(pool))], rng.randrange(2))
            zero.append(len(seqs) + 1)
            seqs += [[(q, s), (q, s)], [(q, s), (q, 1 - s)], [(q, s), (q, 1 - s), r], [(q, s), (q, s), r], [r, (q, s), (q, s)], [(q, s)] * 5]
    got, want = sums(mt, seqs)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]
    assert not got[zero].any()


def test_adversarial_y_triples_in_one_bucket(mt, adv):
    """(x, y), (beta x, y), (beta^2 x, y) are P, lambda P, lambda^2 P: equal y words and different x, so no doubling test may take one for another.  All
    three under one sign give the identity; two of the three give minus the third."""
    pts, triples = adv
    seqs, zero, minus = [], [], []
    for t in triples:
        for s in (0, 1):
            for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
                i, j, k = (t[o] for o in order)
                zero.append(len(seqs)); seqs.append([(pts[i], s), (pts[j], s), (pts[k], s)])
                minus.append((len(seqs), k, 1 - s)); seqs.append([(pts[i], s), (pts[j], s)])
                minus.append((len(seqs), k, 1 - s)); seqs.append([(pts[j], s), (pts[i], s)])
    got, want = sums(mt, seqs)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]
    assert not got[zero].any()
    for at, k, s in minus:
        assert (got[at] == (neg(pts[k]) if s else pts[k])).all(), at


def test_adversarial_addends_pairwise(mt, pool, adv):
    """400 ordered pairs of pool points (seeded sample) meeting in one bucket: alone, and on a random accumulator"""
    pts, _ = adv
    rng = random.Random(53)
    seqs = []
    for _ in range(400):
        i, j = rng.sample(range(len(pts)), 2)
        si, sj = rng.randrange(2), rng.randrange(2)
        r = (pool[rng.randrange(len(pool))], rng.randrange(2))
        seqs += [[(pts[i], si), (pts[j], sj)], [r, (pts[i], si), (pts[j], sj)]]
    got, want = sums(mt, seqs)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]


def test_adversarial_y_words_as_not_normalised_representatives(mt, pool, adv):
    """madd_core with normalise_y = 1 on the pool's y words: 64 p - y limb by limb (what a negative digit loads: the fat 64 p is rebuilt here from p
    alone), and the residue raised by p's limbs.  The word whose eight low limbs are all 0x1FFFFFFF is the one this exists for: it is the extreme of
    the column-sum argument for limbs < 2^29."""
    from tests import gpu_common as gc
    pts, _ = adv
    ys = gc.words_to_ints(pts[:, 4:])
    assert any(all((y >> (29 * i)) & M29 == M29 for i in range(8)) or all(((y + d) >> (29 * i)) & M29 == M29 for i in range(8)) for y in ys for d in range(-8, 9)), \
        "a y word at (or within the lift distance of) all-ones low limbs is in the pool"
    pl = _limbs(P)
    fat64 = _limbs(64 * P)
    for i in range(8):                                    # 2^29 lent to every limb below the top: limbs >= 2^29 - 1 wherever the limb above can lend
        fat64[i] += 1 << 29; fat64[i + 1] -= 1
    assert _val(fat64) == 64 * P and min(fat64[:8]) >= M29 and fat64[8] >= 1 << 27
    rng = random.Random(54)
    for n, q in enumerate(pts):
        x2 = np.zeros(9, dtype=np.uint32); y2 = np.zeros(9, dtype=np.uint32)
        mt.mt_from_sat(p_(x2), p_(q[:4].copy())); mt.mt_from_sat(p_(y2), p_(q[4:].copy()))
        assert max(y2[:8]) <= M29 and _val(y2) < 1 << 259
        yres = _val(y2) % P
        a = pool[rng.randrange(len(pool))]
        plus, minus = cref.g1_to_affine(oracle_sum([a, q], [0, 0])), cref.g1_to_affine(oracle_sum([a, q], [0, 1]))
        reps = [([int(c) - int(v) for c, v in zip(fat64, y2)], minus), ([u + v for u, v in zip(_limbs(yres), pl)], plus),
                ([u + v for u, v in zip(_limbs(P - yres), pl)], minus)]
        for first in (False, True):
            for limbs, want in reps:
                assert 0 <= min(limbs) and max(limbs) < 1 << 30
                acc = np.zeros(36, dtype=np.uint32)
                if not first:
                    assert mt.mt_madd_raw(p_(acc), p_(a), 0) == 0
                assert mt.mt_madd_core_raw(p_(acc), p_(x2), p_(np.array(limbs, dtype=np.uint32)), 1) == 0
                out = np.zeros(8, dtype=np.uint64); mt.mt_finish(p_(out), p_(acc))
                if first:
                    want = q if want is plus else neg(q)
                assert (out == want).all(), (n, first, limbs)
