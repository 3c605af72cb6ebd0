"""mi355_msm_g1_segmented_host on the device (k_msm_g1_segmented: one wavefront per segment, a double-and-add per term, a shuffle tree): every segment against the oracle's
naive sum (cref.msm_naive), the small shapes against oracle/pyref.py as well.  Shapes: no segment, empty segments first / in the middle / last, lengths around the wavefront
(the stride loop), the verifier's shape (318 segments of 19-24 terms), the edge inputs of the host check alone and at lanes 0 and 63, one long segment against the bucket MSM."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import cref

from tests import segmsm_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def check(zk, bases, scalars, offsets, py=False):
    got = zk.halo2.msm_g1_segmented(bases, scalars, offsets)
    assert got.shape == (len(offsets) - 1, 8)
    assert (got == sc.reference(bases, scalars, offsets)).all()
    if py:
        assert (got == sc.reference_py(bases, scalars, offsets)).all()
    return got


def test_no_segment_and_one_empty_segment(zk):
    capi, ptr, lib = zk._capi, zk._capi.ptr, zk._capi.lib()
    out = np.full((1, 8), 7, dtype=np.uint64)
    assert lib.mi355_msm_g1_segmented_host(None, None, None, 0, None) == capi.OK                         # (a) segments = 0 touches nothing
    assert lib.mi355_msm_g1_segmented_host(None, None, ptr(np.zeros(1, dtype=np.uint64)), 0, ptr(out)) == capi.OK and (out == 7).all()
    empty = zk.halo2.msm_g1_segmented(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), [0, 0])   # (b) one empty segment: the identity
    assert empty.shape == (1, 8) and not empty.any()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_one_segment(zk, n):
    bases, scalars = sc.random_terms(n, 4200 + n)
    check(zk, bases, scalars, sc.offsets_of([n]), py=n <= 16)


def test_empty_segments_first_middle_last_and_the_stride_loop(zk):
    lengths = [0, 1, 0, 63, 64, 65, 130, 0]
    bases, scalars = sc.random_terms(sum(lengths), 4210)
    got = check(zk, bases, scalars, sc.offsets_of(lengths))
    assert not got[0].any() and not got[2].any() and not got[7].any() and got[1].any()
    small = [0, 1, 0, 2, 3, 0]                                                                               # 6 terms: Python integers alone
    check(zk, bases[:6], scalars[:6], sc.offsets_of(small), py=True)


def test_the_shape_of_a_batch_of_verifiers(zk):
    """318 segments of 19-24 terms (lengths from a seeded generator): about 7 000 terms"""
    rng = np.random.default_rng(4220)
    lengths = [int(v) for v in rng.integers(19, 25, size=318)]
    assert min(lengths) == 19 and max(lengths) == 24
    pool, _ = sc.random_terms(256, 4221)
    total = sum(lengths)
    bases = pool[rng.integers(0, 256, size=total)]
    scalars = sc.fr_arr([int(v) ** 5 % sc.R for v in rng.integers(1, 2**62, size=total)])
    check(zk, bases, scalars, sc.offsets_of(lengths))


def test_edge_inputs_alone_at_lane_0_and_at_lane_63(zk):
    labels, bases, scalars, offsets = sc.edge_case_inputs()
    got, want = zk.halo2.msm_g1_segmented(bases, scalars, offsets), sc.edge_case_reference()
    bad = [labels[i] for i in range(len(labels)) if (got[i] != want[i]).any()]
    assert not bad, bad
    by = dict(zip(labels, got))
    assert not by["negation/alone"].any() and not by["zero_scalar/alone"].any() and not by["identity_base/alone"].any() and by["duplicate/alone"].any()


def test_one_long_segment_equals_the_bucket_msm(zk):
    n = 4097
    pool, _ = sc.random_terms(128, 4230)
    rng = np.random.default_rng(4231)
    bases = pool[rng.integers(0, 128, size=n)]
    scalars = sc.fr_arr([int(v) ** 5 % sc.R for v in rng.integers(1, 2**62, size=n)])
    got = zk.halo2.msm_g1_segmented(bases, scalars, [0, n])
    adhoc = zk.halo2.best_multiexp(scalars, bases)
    assert (got[0] == adhoc[:8]).all()
    assert (got[0] == cref.g1_to_affine(cref.best_multiexp(scalars, bases, threads=4))).all()


def test_bad_arguments_leave_the_output_untouched(zk):
    capi, ptr, lib = zk._capi, zk._capi.ptr, zk._capi.lib()
    bases, scalars = sc.random_terms(4, 4240)
    out = np.full((2, 8), 7, dtype=np.uint64)
    call = lambda b, s, o, n, r: lib.mi355_msm_g1_segmented_host(ptr(b), ptr(s), ptr(o), n, ptr(r))
    assert call(bases, scalars, np.array([0, 3, 2], dtype=np.uint64), 2, out) == capi.EBADARG
    assert call(bases, scalars, np.array([1, 2, 4], dtype=np.uint64), 2, out) == capi.EBADARG
    off = np.array([0, 2, 4], dtype=np.uint64)
    assert call(None, scalars, off, 2, out) == capi.EBADARG and call(bases, None, off, 2, out) == capi.EBADARG
    assert call(bases, scalars, None, 2, out) == capi.EBADARG and call(bases, scalars, off, 2, None) == capi.EBADARG
    assert (out == 7).all()
    assert call(bases, scalars, off, 2, out) == capi.OK and (out == sc.reference(bases, scalars, off)).all()   # and the same arguments, intact, work
