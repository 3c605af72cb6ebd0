"""helpers shared by the -m gpu tests (TEST INFRASTRUCTURE)."""
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
    """n random curve points [n,8] through the oracle (slow: use for n <= ~4096)."""
    G = cref.g1_generator()
    sc = rand_fr(rng, n, full=False)
    jac = np.stack([cref.g1_mul(G, sc[i]) for i in range(n)])
    return cref.g1_to_affine(jac)


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
