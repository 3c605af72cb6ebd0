"""helpers shared by the -m gpu tests (TEST INFRASTRUCTURE)."""
import functools

import numpy as np

from oracle import cref, pyref

R = pyref.R_MOD


def rand_fr(rng, n, full=True):
    """n random field elements as Montgomery limbs [n,4] (uniform below 2^252, plus a few extreme values)."""
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    if full and n >= 4:
        a[0] = cref.fr_mont(R - 1); a[1] = cref.fr_mont(1); a[2] = cref.fr_mont(0); a[3] = cref.fr_mont((1 << 253) + 12345)
    return a


def rand_points(rng, n):
    """n random curve points [n,8] through the oracle (slow, ~0.4 ms each: use for n <= ~4096; device_points below makes any number)."""
    G = cref.g1_generator()
    sc = rand_fr(rng, n, full=False)
    jac = np.stack([cref.g1_mul(G, sc[i]) for i in range(n)])
    return cref.g1_to_affine(jac)


def device_points(zk, n, seed, sample=64):
    """n independent curve points k_i G made by the library's fixed-base kernel (any n: 2^21 points take well under a second), verified through the
    oracle before anything relies on them: EVERY point satisfies y^2 = x^3 + 3 (cref.f_mul_vec over Fq), and `sample` of them -- indices 0, 16383,
    16384 and n - 1 among them -- equal the oracle's own k_i G.  -> (points [n,8], the scalars k_i [n,4])"""
    import torch
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    rng = np.random.default_rng(seed)
    ks = rand_fr(rng, n, full=False)
    ks_dev = torch.from_numpy(ks.view(np.int64)).cuda()
    pts_dev = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    check(lib.mi355_g1_fixed_base_mul_dev(ptr(pts_dev), ptr(ks_dev), n))
    check(lib.mi355_synchronize())
    pts = pts_dev.cpu().numpy().view(np.uint64).reshape(n, 8)
    x, y = np.ascontiguousarray(pts[:, :4]), np.ascontiguousarray(pts[:, 4:])
    three = np.tile(np.array(pyref.to_limbs(3 * pyref.MONT_R % pyref.P_MOD), dtype=np.uint64), (n, 1))
    rhs = cref.f_add_vec(cref.FQ, cref.f_mul_vec(cref.FQ, cref.f_mul_vec(cref.FQ, x, x), x), three)
    assert (cref.f_mul_vec(cref.FQ, y, y) == rhs).all(), "a device-made point is not on the curve"
    idx = np.unique(np.concatenate([[i for i in (0, 16383, 16384, n - 1) if 0 <= i < n], rng.integers(0, n, size=sample)]))
    assert (pts[idx] == cref.g1_mul_generator_vec(ks[idx])).all(), "a device-made point is not the oracle's multiple of the generator"
    return pts, ks


def witness_like_fr(rng, n):
    """n scalars as in a witness column: 45 % zero, 45 % one, the rest below 2^16 (canonical values), as Montgomery limbs [n,4]"""
    v = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    r = rng.random(n)
    v[r < 0.45] = 0
    v[(r >= 0.45) & (r < 0.9)] = 1
    can = np.zeros((n, 4), dtype=np.uint64); can[:, 0] = v
    return cref.f_from_canonical_vec(cref.FR, can)


def class_sums(sc, period):
    """S_j = sum of sc[i] over i = j mod period, modulo r, as canonical integers (any length: the tail is zero-padded for the fold): the scalars an
    MSM over `period` bases tiled to len(sc) multiplies each distinct base by.  Vectorised over 16-bit chunks."""
    sc = np.asarray(sc, dtype=np.uint64).reshape(-1, 4)
    can = cref.f_to_canonical_vec(cref.FR, sc)
    pad = (-can.shape[0]) % period
    can = np.concatenate([can, np.zeros((pad, 4), dtype=np.uint64)]).reshape(-1, period, 4)
    tot = [0] * period
    for limb in range(4):
        for k in range(4):
            part = ((can[:, :, limb] >> np.uint64(16 * k)) & np.uint64(0xffff)).sum(axis=0, dtype=np.uint64)
            for j in range(period):
                tot[j] += int(part[j]) << (64 * limb + 16 * k)
    return [t % R for t in tot]


def affine_of(g1):
    """12-limb normalised Jacobian from the library -> 8-limb affine, checking the normalisation contract."""
    g1 = np.asarray(g1)
    one_q = np.array(pyref.to_limbs(pyref.MONT_R % pyref.P_MOD), dtype=np.uint64)
    if (g1[8:] == 0).all():
        assert (g1 == 0).all(), "identity must be returned as all-zero"
        return np.zeros(8, dtype=np.uint64)
    assert (g1[8:] == one_q).all(), "result must be normalised: z == R (Montgomery one)"
    return g1[:8].copy()


def oracle_affine(jac):
    return cref.g1_to_affine(jac)


# ---- operands over the whole field (tests/test_gpu_fr_full_range.py).  rand_fr above stays below 2^252, a third of [0, r): the words a kernel
# slices into 29-bit limbs never carry a top limb above 2^20 there, and Fr::add never has to subtract.  The generators below speak of Montgomery
# WORDS (the 32 bytes in memory), not of the values they stand for: any word below r is a legal element.
ALL_ONES_LIMBS = (0x30644D << 232) | ((1 << 232) - 1)     # the largest word below r whose eight low 29-bit limbs are all 0x1FFFFFFF
_R_LIMBS = np.array(pyref.to_limbs(R), dtype=np.uint64)


def words_to_ints(a):
    """[n,4] u64 words -> Python integers"""
    return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def ints_to_words(vals):
    """Python integers below 2^256 -> [n,4] u64 words, as they are (no Montgomery conversion)"""
    vals = list(vals)
    return np.array([pyref.to_limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def below_r(a):
    """row-wise word < r for an [n,4] u64 array (lexicographic from the top limb)"""
    lt = np.zeros(a.shape[0], dtype=bool); eq = np.ones(a.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (a[:, i] < _R_LIMBS[i]); eq &= a[:, i] == _R_LIMBS[i]
    return lt


def rand_fr_full(rng, n):
    """n Montgomery words [n,4] uniform over [0, r): rejection sampling on 254 bits (r / 2^254 = 75.6 % of the draws are kept).  Candidates are drawn
    in blocks of 4096 whatever n is, so a shorter draw from the same seed is a prefix of a longer one."""
    out = np.empty((n, 4), dtype=np.uint64)
    have = 0
    while have < n:
        c = rng.integers(0, 2**64, size=(4096, 4), dtype=np.uint64)
        c[:, 3] &= np.uint64((1 << 62) - 1)
        c = c[below_r(c)][: n - have]
        out[have:have + c.shape[0]] = c; have += c.shape[0]
    return out


def adversarial_fr_ints():
    """the pool of adversarial_fr_words as Python integers: the edges of the field, of the 29-bit and the 32-bit limb grids and of the 2^252 line that
    rand_fr never crosses, the alternating bit patterns, and the Montgomery words of 0, 1, 2, r - 1.  Fixed order, no duplicates, every word < r."""
    mont = pyref.MONT_R % R
    v = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, mont, R - mont, ALL_ONES_LIMBS]
    for i in range(1, 9):
        v += [(1 << (29 * i)) - 1, 1 << (29 * i), (1 << (29 * i)) + 1]
    for i in range(1, 8):
        v += [(1 << (32 * i)) - 1, 1 << (32 * i)]
    v += [(1 << 252) - 1, 1 << 252, 1 << 253]
    v += [int("55" * 32, 16) % R, int("AA" * 32, 16) % R]
    v += [c * mont % R for c in (0, 1, 2, R - 1)]
    return list(dict.fromkeys(v))


def adversarial_fr_words():
    """[m,4] u64: the words a kernel's from_sat / from_sat_plain slices (see adversarial_fr_ints)"""
    return ints_to_words(adversarial_fr_ints())


def pool_pairs(pool):
    """two [m*m,4] vectors in which every ordered pair of pool words meets: a[i*m + j] = pool[i], b[i*m + j] = pool[j]"""
    pool = np.asarray(pool, dtype=np.uint64); m = pool.shape[0]
    return np.ascontiguousarray(np.repeat(pool, m, axis=0)), np.ascontiguousarray(np.tile(pool, (m, 1)))


def tile_words(words, n):
    """the rows of `words` repeated in order up to length n"""
    words = np.asarray(words, dtype=np.uint64)
    return np.ascontiguousarray(words[np.arange(n) % words.shape[0]])


# seed of every rand_fr_full draw of tests/test_gpu_fr_full_range.py, and the lengths >= 1000 it is drawn at (G: multi_processor_count * 8 * 256, the
# grid of the grid-stride kernels; 256 compute units on an MI355X).  tests/test_host_logic.py checks the share of words >= 2^252 of each.
MI355X_GRID = 256 * 8 * 256
FULL_RANGE_DRAWS = {
    "vec_a": (9101, [MI355X_GRID - 1, MI355X_GRID, MI355X_GRID + 1, 2 * MI355X_GRID + 3]),
    "vec_b": (9102, [MI355X_GRID - 1, MI355X_GRID, MI355X_GRID + 1, 2 * MI355X_GRID + 3]),
    "periodic": (9103, [2048, 4096, 4096 * 3 + 5, MI355X_GRID + 1]),
    "distribute": (9104, [16383, 16384, 16385, 32769, 100003, 1 << 16]),
    "eval": (9105, [16383, 16384, 16385, 32767, 32769, 3 * 16384 + 1, 3 * 16384 + 2]),
    "gate": (9106, [6 << 12]),
    "scan": (9107, [2047, 2048, 2049, 100003]),
    "ntt": (9108, [1 << k for k in range(10, 21)]),
    "msm": (9109, [2048]),
}


def full_range(name, n):
    """the first n words of the named draw"""
    return rand_fr_full(np.random.default_rng(FULL_RANGE_DRAWS[name][0]), n)


# ---- curve points whose coordinate WORDS are adversarial (tests/test_gpu_curve_adversarial.py and the host tests of the limb code).  Every other
# point of the suite is a multiple of a generator: its words are uniform in [0, p), so nothing ever sits on an edge of the limb grids from_sat slices.
P = pyref.P_MOD
_RINV_P = pow(pyref.MONT_R, -1, P)
_T9 = (P - 1) // 9                                        # p - 1 = 9 t with 3 not dividing t
assert P % 4 == 3 and 9 * _T9 == P - 1 and _T9 % 3 != 0 and ALL_ONES_LIMBS < P <= ((0x30644E << 232) | ((1 << 232) - 1))
_ZETA9 = next(pow(g, _T9, P) for g in range(2, 50) if pow(g, 3 * _T9, P) != 1)      # a primitive 9th root of unity
FQ_BETA = pow(_ZETA9, 3, P)                               # a primitive cube root of unity: (x, y) -> (beta x, y) is the endomorphism lambda
LIFT_MAX = 8                                              # a pool word lifts to a coordinate within this distance (tests/test_host_logic.py)


def adversarial_fq_ints():
    """adversarial_fr_ints with p in place of r: words of a base-field coordinate.  Fixed order, no duplicates, every word < p."""
    mont = pyref.MONT_R % P
    v = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, mont, P - mont, ALL_ONES_LIMBS]
    for i in range(1, 9):
        v += [(1 << (29 * i)) - 1, 1 << (29 * i), (1 << (29 * i)) + 1]
    for i in range(1, 8):
        v += [(1 << (32 * i)) - 1, 1 << (32 * i)]
    v += [(1 << 252) - 1, 1 << 252, 1 << 253]
    v += [int("55" * 32, 16) % P, int("AA" * 32, 16) % P]
    v += [c * mont % P for c in (0, 1, 2, P - 1)]
    assert all(0 <= x < P for x in v)
    return list(dict.fromkeys(v))


def fq_sqrt(a):
    """a square root of a modulo p (p = 3 mod 4), or None"""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def fq_cbrt(a):
    """a cube root of a modulo p, or None: a^(1/3 mod t) is a root up to a 9th root of unity"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 3, P) != 1:
        return None
    c = pow(a, pow(3, -1, _T9), P)
    for _ in range(9):
        if pow(c, 3, P) == a:
            return c
        c = c * _ZETA9 % P
    raise AssertionError("a cube without a cube root")


def _nearest(w, lift):
    """(value of lift, signed distance) at the nearest word w + d, w - d (d = 0, 1, ..; + before -) inside [0, p) at which lift gives something"""
    for d in range(LIFT_MAX + 1):
        for s in ((0,) if d == 0 else (d, -d)):
            if 0 <= w + s < P:
                got = lift(w + s)
                if got is not None:
                    return got, s
    raise AssertionError("word %#x does not lift within %d" % (w, LIFT_MAX))


@functools.lru_cache(maxsize=None)
def _g1_pool(reading):
    assert reading in ("mont", "canonical")
    val = (lambda w: w * _RINV_P % P) if reading == "mont" else (lambda w: w)

    def lift_x(w):
        x = val(w)
        y = fq_sqrt((x * x * x + 3) % P)
        return None if y is None or x == 0 else [(x, y), (x, P - y)]

    def lift_y(w):
        y = val(w)
        x = fq_cbrt((y * y - 3) % P)
        return None if x is None or x == 0 else [(x, y), (FQ_BETA * x % P, y), (FQ_BETA * FQ_BETA * x % P, y)]

    pts, words, dist, kind, index, triples = [], [], [], [], {}, []
    for fam, lift in (("x", lift_x), ("y", lift_y)):
        for w in adversarial_fq_ints():
            got, d = _nearest(w, lift)
            ids = []
            for pt in got:
                if pt not in index:
                    index[pt] = len(pts); pts.append(pt); words.append(w); dist.append(d); kind.append(fam)
                ids.append(index[pt])
            if fam == "y" and ids not in triples:
                triples.append(ids)
    abi = np.array([pyref.mont_limbs(x, P) + pyref.mont_limbs(y, P) for x, y in pts], dtype=np.uint64)
    for a in (abi,):
        a.setflags(write=False)
    return {"points": abi, "words": ints_to_words(words), "dist": np.array(dist, dtype=np.int64), "kind": kind, "py": pts, "triples": triples}


def adversarial_g1_points(reading):
    """G1 points with an adversarial coordinate word.  reading = "mont": the pool word is the Montgomery form of the coordinate (what the MSM, FFT and
    normalise kernels slice); "canonical": it is the value (what the codec slices).  Every word of adversarial_fq_ints is taken once as an x (both
    points (x, +-y) are kept) and once as a y (all three points (x, y), (beta x, y), (beta^2 x, y) are kept: P, lambda P, lambda^2 P, which sum to
    the identity and have equal y and different x), each time at the nearest word w + d, w - d (smallest d, + first) for which the point exists.
    -> (points [m,8] u64 ABI words (Montgomery), the pool word each was built for [m,4], the signed distance d [m]); fixed order, no duplicates."""
    g = _g1_pool(reading)
    return g["points"].copy(), g["words"].copy(), g["dist"].copy()


def adversarial_g1_info(reading):
    """of the same pool: (the points as pyref tuples, "x" / "y" per point: the coordinate the word was lifted as, the index triples of the y family)"""
    g = _g1_pool(reading)
    return list(g["py"]), list(g["kind"]), [list(t) for t in g["triples"]]


def adversarial_fq_non_lifting(reading):
    """the pool words that are no x coordinate as they stand (distance != 0 in the x family), in pool order"""
    g = _g1_pool(reading)
    seen = dict()
    for w, d, k in zip(words_to_ints(g["words"]), g["dist"], g["kind"]):
        if k == "x" and d != 0:
            seen[w] = None
    return list(seen)


def g1_neg_words(pts):
    """[n,8] ABI points -> their opposites (identity entries stay all-zero)"""
    pts = np.asarray(pts, dtype=np.uint64).reshape(-1, 8)
    out = pts.copy()
    for i, y in enumerate(words_to_ints(pts[:, 4:])):
        out[i, 4:] = pyref.to_limbs((P - y) % P)
    return out


def f2_sqrt(a):
    """a square root in Fq2 = Fq[u]/(u^2 + 1) by the complex method, or None.  a = (a0, a1) canonical integers."""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        return (0, fq_sqrt(P - a0))                       # -1 is a non-residue: exactly one of a0, -a0 is a square
    s = fq_sqrt((a0 * a0 + a1 * a1) % P)                  # the norm; a is a square of Fq2 iff its norm is one of Fq
    if s is None:
        return None
    half = (P + 1) // 2
    x0 = fq_sqrt((a0 + s) * half % P)
    if x0 is None:
        x0 = fq_sqrt((a0 - s) * half % P)
    x1 = a1 * pow(2 * x0, -1, P) % P
    assert pyref.f2_mul((x0, x1), (x0, x1)) == (a0, a1)
    return (x0, x1)


@functools.lru_cache(maxsize=None)
def _g2_pool(reading):
    assert reading in ("mont", "canonical")
    val = (lambda w: w * _RINV_P % P) if reading == "mont" else (lambda w: w)
    pool = adversarial_fq_ints()
    m = len(pool)
    pts, words, dist, index = [], [], [], {}
    shapes = [(w, None) for w in pool] + [(None, w) for w in pool] + [(w, pool[(5 * i + 3) % m]) for i, w in enumerate(pool)]
    for c0w, c1w in shapes:
        c1 = 0 if c1w is None else val(c1w)

        def lift(w):
            x = (val(w), c1)
            if x == (0, 0):
                return None
            y = f2_sqrt(pyref.f2_add(pyref.f2_mul(pyref.f2_mul(x, x), x), pyref.G2_B))
            return None if y is None or y == (0, 0) else [(x, y), (x, ((-y[0]) % P, (-y[1]) % P))]

        got, d = _nearest(0 if c0w is None else c0w, lift)
        for pt in got:
            if pt not in index:
                index[pt] = len(pts); pts.append(pt); words.append((c0w or 0, c1w or 0)); dist.append(d)
    abi = np.array([pyref.g2_to_limbs(q) for q in pts], dtype=np.uint64)
    abi.setflags(write=False)
    return {"points": abi, "words": words, "dist": np.array(dist, dtype=np.int64), "py": pts}


def adversarial_g2_points(reading="mont"):
    """points of the twist y^2 = x^3 + 3 / (9 + u) with x = (w, 0), (0, w) and (w, w') over the words of adversarial_fq_ints (w' = the word 5 i + 3 places
    on, so every word is a c1 once), c0 moved to the nearest word at which x^3 + b' is a square of Fq2, both signs of y.  On the twist, NOT in the
    subgroup of order r: a scalar multiple of such a point is the multiple by the INTEGER, never by its residue modulo r.
    -> (points [m,16] u64 ABI words, the pyref tuples, the signed distances of c0 [m])"""
    g = _g2_pool(reading)
    return g["points"].copy(), list(g["py"]), g["dist"].copy()
