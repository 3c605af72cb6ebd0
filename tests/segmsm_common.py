"""Inputs and references shared by the tests of the segmented G1 MSM (mi355_msm_g1_segmented_host): the CPU run of the kernel's per-term routine
(test_msm_segmented_on_host.py) and the device (test_gpu_msm_segmented.py) see the same edge inputs and the same oracle values.
ABI forms: bases [n, 8] u64 G1Affine (Montgomery, identity = zeros), scalars [n, 4] u64 Fr (Montgomery), offsets [segments + 1] u64."""
import functools

import numpy as np

from oracle import cref, pyref

R = pyref.R_MOD
EDGE_SCALARS = (0, 1, 2, R - 1, R - 2, 1 << 253)
LENGTHS = (0, 1, 2, 63, 64, 65, 130)


def fr_arr(values):
    return np.array([pyref.mont_limbs(int(v) % R, R) for v in values], dtype=np.uint64).reshape(-1, 4)


def neg_points(pts):
    """-P for [n, 8] ABI points (the identity stays the identity)"""
    out = pts.copy()
    for i in range(pts.shape[0]):
        y = pyref.from_limbs(pts[i, 4:])
        out[i, 4:] = pyref.to_limbs((pyref.P_MOD - y) % pyref.P_MOD)
    return out


def random_terms(n, seed):
    """n random points (multiples of the generator by the oracle) with n random scalars"""
    rng = np.random.default_rng(seed)
    rnd = lambda: int(rng.integers(1, 2**62)) ** 5 % R
    pts = cref.g1_mul_generator_vec(fr_arr([rnd() for _ in range(n)]), threads=4) if n else np.zeros((0, 8), dtype=np.uint64)
    return pts, fr_arr([rnd() for _ in range(n)])


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.array(lengths, dtype=np.uint64))]).astype(np.uint64)


def reference(bases, scalars, offsets):
    """per segment: the oracle's naive sum (cref.msm_naive), affine"""
    out = np.zeros((len(offsets) - 1, 8), dtype=np.uint64)
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if hi > lo:
            out[s] = cref.g1_to_affine(cref.msm_naive(scalars[lo:hi], bases[lo:hi]))
    return out


def reference_py(bases, scalars, offsets):
    """the same with Python integers alone (oracle/pyref.py); for small totals"""
    out = np.zeros((len(offsets) - 1, 8), dtype=np.uint64)
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        pts = [pyref.g1_affine_from_limbs(b[:4], b[4:]) for b in bases[lo:hi]]
        ks = [pyref.from_mont(pyref.from_limbs(k), R) for k in scalars[lo:hi]]
        xl, yl = pyref.g1_affine_to_limbs(pyref.msm(ks, pts))
        out[s] = xl + yl
    return out


@functools.lru_cache(maxsize=None)
def _edge_case_segments():
    from tests import gpu_common as gc
    adv, _, _ = gc.adversarial_g1_points("mont")
    pool, pool_k = random_terms(80, 4101)
    P, Q = pool[0], pool[1]
    ident = np.zeros(8, dtype=np.uint64)
    rng = np.random.default_rng(4102)
    rnd = lambda: int(rng.integers(1, 2**62)) ** 5 % R
    k = rnd()
    kinds = {                                                      # name -> its terms (point, scalar)
        "zero_scalar": [(P, 0)],
        "identity_base": [(ident, rnd())],
        "identity_base_zero_scalar": [(ident, 0)],
        "duplicate": [(P, k), (P, k)],                            # equal products: the addition that meets them must double
        "negation": [(Q, k), (neg_points(Q[None])[0], k)],        # P and -P with equal scalars: the identity
        "r_minus_1": [(P, R - 1)],
        "r_minus_2": [(Q, R - 2)],
        "two_to_253": [(P, 1 << 253)],
        "one": [(Q, 1)],
        "two": [(Q, 2)],
    }
    segs = []                                                      # (label, [(point, scalar), ...])
    for name, terms in kinds.items():
        segs.append((name + "/alone", terms))
        for first, second in ((0, 63), (63, 0)):                  # inside a full wavefront: the kind's first term at lane `first`, a second one at lane `second`
            seg = [(pool[2 + i], pyref.from_mont(pyref.from_limbs(pool_k[2 + i]), R)) for i in range(64)]
            seg[first] = terms[0]
            if len(terms) > 1:
                seg[second] = terms[1]
            segs.append(("%s/lane%d" % (name, first), seg))
    segs.append(("all_zero_scalars", [(pool[i], 0) for i in range(64)]))
    segs.append(("all_identity_bases", [(ident, rnd()) for _ in range(65)]))
    segs.append(("duplicates_in_one_lane", [(P, k)] + [(pool[2 + i], 3 + i) for i in range(63)] + [(P, k)]))   # terms 0 and 64: lane 0 adds equal products
    for i in range(adv.shape[0]):                                  # every adversarial point once alone ...
        segs.append(("adversarial/%d/alone" % i, [(adv[i], rnd())]))
    for lo in range(0, adv.shape[0], 64):                          # ... and once in wavefront-sized runs (lanes 0 .. 63)
        segs.append(("adversarial/run%d" % lo, [(adv[i], EDGE_SCALARS[i % 6] if i % 5 == 0 else rnd()) for i in range(lo, min(lo + 64, adv.shape[0]))]))
    return segs


def edge_case_inputs():
    """-> (labels, bases, scalars, offsets): zero scalars, identity bases, duplicates, negations, r - 1, r - 2, 2^253 and every point of
    gpu_common.adversarial_g1_points("mont"), each kind alone in a segment, at lane 0 and at lane 63 of a full wavefront"""
    segs = _edge_case_segments()
    bases = np.array([p for _, seg in segs for p, _ in seg], dtype=np.uint64).reshape(-1, 8)
    scalars = fr_arr([k for _, seg in segs for _, k in seg])
    return [l for l, _ in segs], bases, scalars, offsets_of([len(seg) for _, seg in segs])


@functools.lru_cache(maxsize=None)
def edge_case_reference():
    """the oracle's sums for edge_case_inputs(), computed once per process"""
    _, bases, scalars, offsets = edge_case_inputs()
    return reference(bases, scalars, offsets)
