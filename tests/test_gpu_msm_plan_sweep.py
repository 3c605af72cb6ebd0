"""
-m gpu: the AUTOMATIC plan of the bucket MSM (csrc/msm.hpp, lib_msm.hip) swept across its own switches, bit-exact against the CPU oracle.

Between 2^11 and 2^21 points the plan a caller gets by default changes its window width eight times, and with it the sorter's key split (coarse
bins appear), the form of the per-bucket fix-up (quad -> four lanes -> one lane), the form of the running sums (quad -> one lane) and the number
of level-1 sorter tiles.  The older tests reach those kernel forms by forcing c at n = 2048 (a nearly empty bucket set) or at powers of two.  Here:

  * the window choice is restated in tests/msm_plan_common.py (msm_cost / choose_c / plan); the lengths of the sweep are GENERATED from it -- both sides of every
    length at which c changes -- and after every device run mi355_msm_last_plan / _last_run must report the restated (c, W, entries, shared);
  * the bases are independent points k_i G made on the device and verified through the oracle (gpu_common.device_points), with points whose
    coordinate words are adversarial at the sorter's tile edges and at the last index of every length, two identities and a pair P, -P;
  * the scalars are uniform over the whole field (with the largest canonical values at the tile edges), witness-like, or ~24 distinct values;
  * every comparison is against oracle/cref.py (independent C), for G2 against cref.g2_mul + pyref.g2_add; none against the library itself.
Entry points: host pointers, resident scalars, the asynchronous call, batches, window tables, pipelined chunks, host slices, and the G2 MSM.
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
from tests import gpu_common as gc
from tests.gpu_common import affine_of
from tests.test_gpu_fr_full_range import MSM_SPECIAL
from tests.test_gpu_headline import last_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = pyref.P_MOD
RINV_P = pow(pyref.MONT_R, -1, P)

# ------------------------------------------------------------------------------------------------ the plan, restated
# tests/msm_plan_common.py restates csrc/msm_plan.hpp (and tests/test_msm_plan_on_host.py holds it against the C++ on the CPU).  A retune of the library changes THAT
# module; every length below follows from it.
from tests.msm_plan_common import L1_TILE, boundaries, choose_c, log2_ceil, plan, table_c, windows  # noqa: E402

BOUNDARIES = boundaries(1 << 11, 1 << 19)            # both sides of each run under three scalar kinds
BIG_BOUNDARIES = boundaries(1 << 19, 1 << 21)        # one case each: the oracle needs seconds there
G2_BOUNDARIES = [b for b in BOUNDARIES if b <= 1 << 17]
TILE_EDGES = [L1_TILE - 1, L1_TILE, L1_TILE + 1, 2 * L1_TILE + 1, 3 * L1_TILE + 1]
RAGGED = 100003
TABLE_LOG, TABLE_LENGTHS = 17, [39137, 71161, RAGGED, (1 << 17) - 1]
PIPE_LENGTHS, PIPE_TABLE_LOG = [RAGGED, (1 << 17) + 1], 18
FIRST_COARSE = next(b for b in BOUNDARIES if plan(b)["cb_bits"])                 # the first length whose sorter has coarse bins
FIRST_FOUR_LANES = next(b for b in BOUNDARIES if plan(b)["fixup"] != "quad")     # the first length past the quad fix-up
BATCHES = [(3, FIRST_COARSE - 1), (3, FIRST_COARSE), (9, BOUNDARIES[1]), (5, FIRST_FOUR_LANES)]      # (M, n); M = 9: the staged pointer array
ALL_LENGTHS = sorted({n for b in BOUNDARIES for n in (b - 1, b)} | set(BIG_BOUNDARIES) | set(TILE_EDGES) | {RAGGED} | set(TABLE_LENGTHS) | set(PIPE_LENGTHS))
N_BASES = 1 << log2_ceil(max(ALL_LENGTHS))
IDENTITY_AT, PAIR_AT = (7, 2000), (99, 100)          # two identity bases; base 100 = -(base 99), and every scalar vector has sc[100] = sc[99]
SHIFT = 4099                                         # polynomial j of a batch: the uniform draw from offset j * SHIFT on


def test_the_sweep_reaches_every_switch_of_the_plan():
    """what the lengths are generated for: should a retune move a switch out of the swept range, this says so"""
    assert len(BOUNDARIES) >= 6 and all(choose_c(b - 1) != choose_c(b) for b in BOUNDARIES + BIG_BOUNDARIES)
    plans = [plan(n) for b in BOUNDARIES for n in (b - 1, b)]
    assert {p["fixup"] for p in plans} == {"quad", "four lanes", "one lane"} and {p["sums"] for p in plans} == {"quad", "one lane"}
    assert {min(p["cb_bits"], 1) for p in plans} == {0, 1} and {min(plan(n)["tiles1"], 4) for n in TILE_EDGES} == {1, 2, 3, 4}
    assert plan(FIRST_COARSE - 1, 3)["cb_bits"] == 0 and plan(FIRST_COARSE, 3)["cb_bits"] == 1
    assert all(n & (n - 1) for n in TABLE_LENGTHS + PIPE_LENGTHS)            # log2_ceil(n), the payload shift of a table row, is exact at none of them
    assert max(ALL_LENGTHS) <= N_BASES and len(MSM_SPECIAL) == 7


# ------------------------------------------------------------------------------------------------ inputs
@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    yield pkg
    lib = pkg._capi.lib()
    pkg._capi.check(lib.mi355_msm_set_window_bits(0)); pkg._capi.check(lib.mi355_msm_set_pipeline(0, 0))


def harden(points):
    """the hard cases written over the device-made points: adversarial coordinate words at the level-1 tile edges and at the last index of every
    length of this module, two identities, one base equal to the negation of its neighbour"""
    pool, _, _ = gc.adversarial_g1_points("mont")
    spots = list(dict.fromkeys([0, L1_TILE - 1, L1_TILE, L1_TILE + 1] + [n - 1 for n in ALL_LENGTHS]))
    assert not set(spots) & set(IDENTITY_AT + PAIR_AT)
    for j, i in enumerate(spots):
        points[i] = pool[(5 * j) % pool.shape[0]]
    for i in IDENTITY_AT:
        points[i] = 0
    points[PAIR_AT[1]] = gc.g1_neg_words(points[PAIR_AT[0]:PAIR_AT[0] + 1])[0]
    return points


def register(zk, points):
    h = C.c_uint64()
    zk._capi.check(zk._capi.lib().mi355_srs_register_host(zk._capi.ptr(np.ascontiguousarray(points)), points.shape[0], C.byref(h)))
    return h.value


@pytest.fixture(scope="module")
def basis(zk):
    """N_BASES verified independent points with the hard cases, registered once; smaller cases take prefixes.  want: the oracle's results, each
    computed once and shared by the tests that need it"""
    points, _ = gc.device_points(zk, N_BASES, 20251)
    points = harden(points)
    points.setflags(write=False)
    b = {"points": points, "handle": register(zk, points), "want": {}}
    yield b
    zk._capi.check(zk._capi.lib().mi355_srs_release(b["handle"]))


def table_basis(zk, basis, log_n):
    """the first 2^log_n points as a basis of their own with window tables of the automatic width -> (handle, the tables' c)"""
    lib, check = zk._capi.lib(), zk._capi.check
    h = register(zk, basis["points"][: 1 << log_n])
    check(lib.mi355_srs_precompute(h, 0, 0))
    ptr, c, w = C.c_void_p(), C.c_int(), C.c_int()
    check(lib.mi355_srs_pre_dev_ptr(h, C.byref(ptr), C.byref(c), C.byref(w)))
    assert ptr.value and c.value == table_c(1 << log_n) and w.value == windows(c.value), (c.value, w.value)
    return h, c.value


@pytest.fixture(scope="module")
def tables(zk, basis):
    hs = {log_n: table_basis(zk, basis, log_n) for log_n in (TABLE_LOG, PIPE_TABLE_LOG)}
    yield hs
    for h, _ in hs.values():
        zk._capi.check(zk._capi.lib().mi355_srs_release(h))


_POOL = {}


def uniform_pool():
    if "u" not in _POOL:
        _POOL["u"] = gc.full_range("msm", max(ALL_LENGTHS) + 16 * SHIFT)
        _POOL["u"].setflags(write=False)
    return _POOL["u"]


def scalars(n, kind):
    """uniform: the whole-field draw with the MSM_SPECIAL values on the tile edges (and, where n has fewer edges than values, spread inside);
    shiftJ: the same draw from J * SHIFT on; witness: mostly 0 / 1; few: 24 distinct values, i.e. long buckets across the tile edges"""
    if kind == "uniform":
        sc = uniform_pool()[:n].copy()
        edges = [i for i in (0, L1_TILE - 1, L1_TILE, L1_TILE + 1, 2 * L1_TILE, 3 * L1_TILE, n - 1) if i < n]
        spots = list(dict.fromkeys(edges + [int(i) for i in np.linspace(1, n - 2, num=len(MSM_SPECIAL))]))[: len(MSM_SPECIAL)]
        for i, v in zip(spots, MSM_SPECIAL):
            sc[i] = cref.fr_mont(v)
    elif kind.startswith("shift"):
        sc = uniform_pool()[int(kind[5:]) * SHIFT:][:n].copy()
    elif kind == "witness":
        sc = gc.witness_like_fr(np.random.default_rng(7100 + n), n)
    else:
        assert kind == "few"
        sc = uniform_pool()[SHIFT:SHIFT + 24][np.random.default_rng(7200 + n).integers(0, 24, size=n)].copy()
    sc[PAIR_AT[1]] = sc[PAIR_AT[0]]
    return sc


def case(basis, n, kind):
    """(the scalars, the oracle's MSM of them over the first n bases)"""
    sc = scalars(n, kind)
    if (n, kind) not in basis["want"]:
        basis["want"][n, kind] = cref.g1_to_affine(cref.best_multiexp(sc, basis["points"][:n]))
    return sc, basis["want"][n, kind]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def check_plan(zk, want, what):
    """mi355_msm_last_plan / _last_run against the restatement; the row goes to stdout (profiles/msm_plan_sweep.md is made of these)"""
    run = last_run(zk)
    print("plan-row | %s | n=%d | c=%d | W=%d | entries=%d | shared=%d" % (what, want["n"], run["c"], run["windows"], run["entries"], run["shared"]))
    assert (run["c"], run["windows"], run["entries"], run["shared"]) == (want["c"], want["W"], want["entries"], want["shared"]), (what, want, run)
    return run


def msm_host_and_dev(zk, handle, sc, want, pl, what):
    """the host-pointer and the resident entry point over the first len(sc) points of a registered basis"""
    h2, n = zk.halo2, sc.shape[0]
    got = affine_of(h2.best_multiexp(sc, h2.SrsSlice(handle, 0, n)))
    assert (got == want).all(), (what, "host pointers", n)
    check_plan(zk, pl, what + " host")
    d = to_dev(sc)
    got = affine_of(h2.best_multiexp(d, h2.SrsSlice(handle, 0, n)))
    assert (got == want).all(), (what, "resident", n)
    check_plan(zk, pl, what + " dev")
    return d


# ------------------------------------------------------------------------------------------------ G1 sweep
@pytest.mark.parametrize("b", BOUNDARIES)
def test_g1_both_sides_of_a_boundary_uniform_scalars(zk, basis, b):
    seen = []
    for n in (b - 1, b):
        sc, want = case(basis, n, "uniform")
        msm_host_and_dev(zk, basis["handle"], sc, want, plan(n), "g1 uniform")
        seen.append(last_run(zk)["c"])
    assert seen[0] != seen[1], (b, seen)


@pytest.mark.parametrize("b", BOUNDARIES)
@pytest.mark.parametrize("kind", ["witness", "few"])
def test_g1_one_side_of_a_boundary_skewed_scalars(zk, basis, b, kind):
    """witness-like columns on the upper side, 24 distinct values (buckets of thousands of entries, the giant-bucket fix-up) on the lower"""
    n = b if kind == "witness" else b - 1
    sc, want = case(basis, n, kind)
    msm_host_and_dev(zk, basis["handle"], sc, want, plan(n), "g1 " + kind)


@pytest.mark.parametrize("n,kind", [(n, "uniform") for n in TILE_EDGES + [RAGGED]] + [(2 * L1_TILE + 1, "few"), (3 * L1_TILE + 1, "witness"), (RAGGED, "few")])
def test_g1_sorter_tile_edges(zk, basis, n, kind):
    """one entry short of a level-1 tile, a whole tile, one entry into the second, the third and the fourth, and a length with no structure"""
    sc, want = case(basis, n, kind)
    msm_host_and_dev(zk, basis["handle"], sc, want, plan(n), "g1 edge " + kind)


@pytest.mark.parametrize("n", [RAGGED, FIRST_COARSE])
def test_g1_async_entry_point(zk, basis, n):
    """mi355_msm_g1_dev_async: the result stays in device memory in stream order"""
    import torch
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    sc, want = case(basis, n, "uniform")
    d, out = to_dev(sc), torch.zeros(12, dtype=torch.int64, device="cuda")
    check(lib.mi355_msm_g1_dev_async(basis["handle"], 0, ptr(d), n, ptr(out)))
    check(lib.mi355_synchronize())
    assert (affine_of(out.cpu().numpy().view(np.uint64)) == want).all()
    check_plan(zk, plan(n), "g1 async")


@pytest.mark.parametrize("n", BIG_BOUNDARIES)
def test_g1_first_length_of_the_widest_swept_window(zk, basis, n):
    """the upper side of the boundary beyond 2^19: 2^19 buckets and more, 100 level-1 tiles, an accumulate segment above its minimum"""
    sc, want = case(basis, n, "uniform")
    assert choose_c(n) != choose_c(n - 1)
    msm_host_and_dev(zk, basis["handle"], sc, want, plan(n), "g1 big")


# ------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("M,n", BATCHES)
def test_g1_batch_over_one_basis(zk, basis, M, n):
    """mi355_msm_g1_batch_dev: (polynomial, window) pairs as windows of one bucket problem -- M times the bucket sets and sorter regions of the plan,
    each polynomial against its own oracle MSM"""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    kinds = (["uniform", "witness", "few"] + ["shift%d" % j for j in range(3, M)])[:M]
    cases = [case(basis, n, k) for k in kinds]
    dev = [to_dev(sc) for sc, _ in cases]
    arr = (C.c_void_p * M)(*[d.data_ptr() for d in dev])
    out = np.zeros((M, 12), dtype=np.uint64)
    check(lib.mi355_msm_g1_batch_dev(basis["handle"], 0, arr, M, n, ptr(out)))
    check_plan(zk, plan(n, M), "g1 batch M=%d" % M)
    for j, (_, want) in enumerate(cases):
        assert (affine_of(out[j]) == want).all(), (M, n, kinds[j])


# ------------------------------------------------------------------------------------------------ window tables
@pytest.mark.parametrize("n", TABLE_LENGTHS)
def test_g1_window_tables_and_the_table_free_plan_at_ragged_prefixes(zk, basis, tables, n):
    """prefixes of a 2^17-point basis with tables: the payload shift log2_ceil(n) is not exact at any of them.  By default the shared bucket set is
    taken; with the tables switched off the same call runs the per-window plan of the sweep"""
    lib, check = zk._capi.lib(), zk._capi.check
    h, tc = tables[TABLE_LOG]
    sc, want = case(basis, n, "uniform")
    with_tables = plan(n, tab_c=tc)
    assert with_tables["shared"] and with_tables["c"] == tc
    msm_host_and_dev(zk, h, sc, want, with_tables, "g1 tables")
    check(lib.mi355_msm_set_window_bits(-1))
    try:
        msm_host_and_dev(zk, h, sc, want, plan(n), "g1 tables off")
    finally:
        check(lib.mi355_msm_set_window_bits(0))


# ------------------------------------------------------------------------------------------------ slices
def pipeline_plan(n, chunks, tab_c=None):
    """msm_batch_impl with K = chunks slices [n k / K, n (k + 1) / K): c, W and shared of the last slice, the entries of all"""
    cuts = [n * k // chunks for k in range(chunks + 1)]
    parts = [plan(cuts[k + 1] - cuts[k], tab_c=tab_c) for k in range(chunks)]
    return dict(parts[-1], n=n, entries=sum(p["entries"] for p in parts))


@pytest.mark.parametrize("with_tables", [False, True], ids=["plain", "tables"])
@pytest.mark.parametrize("n", PIPE_LENGTHS)
def test_g1_pipelined_chunks(zk, basis, tables, n, with_tables):
    """mi355_msm_set_pipeline(3, 15): three ragged slices on three streams, each a complete MSM with its own plan; twice for the reuse of the slots"""
    lib, check = zk._capi.lib(), zk._capi.check
    h, tc = tables[PIPE_TABLE_LOG] if with_tables else (basis["handle"], None)
    sc, want = case(basis, n, "uniform")
    pl = pipeline_plan(n, 3, tc)
    assert pl["shared"] == with_tables and n // 3 >= (1 << 15) >> 2
    check(lib.mi355_msm_set_pipeline(3, 15))
    try:
        for turn in range(2):
            msm_host_and_dev(zk, h, sc, want, pl, "g1 pipelined turn %d" % turn)
    finally:
        check(lib.mi355_msm_set_pipeline(0, 0))


HOST_SLICE_ENV = {"MI355_HOST_CHUNKS": "4", "MI355_HOST_SLICE_MIN_LOG": "14"}


def host_slice_plan(n, chunks):
    """msm_host_single: a first slice of n / 16, each further one 1.7 times the last, the rest in the final slice; every slice takes the shape of the
    biggest -> (slices, that plan with the entries of all slices)"""
    w, acc, cuts = 1.0, 0.0, [0]
    for _ in range(chunks - 1):
        acc += w / 16.0; w *= 1.7
        cut = int(acc * n)
        if cuts[-1] < cut < n:
            cuts.append(cut)
    cuts.append(n)
    pl = plan(max(b - a for a, b in zip(cuts, cuts[1:])))
    return len(cuts) - 1, dict(pl, n=n, entries=n * pl["W"])


def _host_slice_child(ref_path):
    """runs in the child, under HOST_SLICE_ENV: the host-pointer MSM cut into ragged slices that share a forced shape and meet in k_msm_bucket_fold"""
    zk = ge.load_package(); zk.init(0)
    h2 = zk.halo2
    ref = np.load(ref_path)
    n = ref["sc"].shape[0]
    h = register(zk, ref["points"])
    slices, pl = host_slice_plan(n, int(HOST_SLICE_ENV["MI355_HOST_CHUNKS"]))
    assert (affine_of(h2.best_multiexp(ref["sc"], h2.SrsSlice(h, 0, n))) == ref["want"]).all(), "host slices"
    run = check_plan(zk, pl, "g1 host slices")
    assert run["host_slices"] == slices == 4, run
    assert (affine_of(h2.best_multiexp(to_dev(ref["sc"]), h2.SrsSlice(h, 0, n))) == ref["want"]).all(), "resident scalars are not sliced"
    assert check_plan(zk, plan(n), "g1 unsliced")["host_slices"] == 1
    zk._capi.check(zk._capi.lib().mi355_srs_release(h))
    print("HOST-SLICES-OK")


def test_g1_host_slices_at_a_ragged_length(basis, tmp_path):
    n = RAGGED
    sc, want = case(basis, n, "uniform")
    path = str(tmp_path / "ref.npz")
    np.savez(path, points=basis["points"][: 1 << log2_ceil(n)], sc=sc, want=want)
    code = "import sys; sys.path.insert(0, %r); import tests.test_gpu_msm_plan_sweep as t; t._host_slice_child(%r)" % (ROOT, path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **HOST_SLICE_ENV), capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "HOST-SLICES-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])


# ------------------------------------------------------------------------------------------------ G2 at the same switches
G2_PERIOD = 1021                                     # no power of two: an index error at a multiple of 1024 lands on another base


def g2_to_py(limbs):
    limbs = np.asarray(limbs, dtype=np.uint64)
    if not limbs.any():
        return None
    c = [pyref.from_limbs(limbs[4 * k:4 * k + 4]) * RINV_P % P for k in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


@pytest.fixture(scope="module")
def twist_points():
    gen = cref.g2_generator()
    return np.stack([cref.g2_mul(gen, s) for s in gc.rand_fr(np.random.default_rng(7300), G2_PERIOD, full=False)])


def g2_expected(twist_points, sc):
    """the MSM of sc over the G2_PERIOD points tiled to len(sc): the scalars folded per residue class, one oracle multiple per point, pyref sums"""
    acc = None
    for q, s in zip(twist_points, gc.class_sums(sc, G2_PERIOD)):
        if s:
            acc = pyref.g2_add(acc, g2_to_py(cref.g2_mul(q, cref.fr_mont(s))))
    return np.array(pyref.g2_to_limbs(acc), dtype=np.uint64)


@pytest.mark.parametrize("kind", ["uniform", "witness"])
@pytest.mark.parametrize("b", G2_BOUNDARIES)
def test_g2_both_sides_of_a_boundary(zk, twist_points, b, kind):
    """mi355_msm_g2_adhoc_host / _dev: the same stage A and the same templated tail under the twist's policy, with the plan of the G1 cost model"""
    h2 = zk.halo2
    seen = []
    for n in (b - 1, b):
        sc = scalars(n, kind)
        bases = np.ascontiguousarray(twist_points[np.arange(n) % G2_PERIOD])
        want = g2_expected(twist_points, sc)
        assert (h2.g2_msm(bases, sc) == want).all(), ("g2 host pointers", n, kind)
        check_plan(zk, plan(n), "g2 %s host" % kind)
        db, ds = h2.DeviceBuffer.from_host(bases), h2.DeviceBuffer.from_host(sc)
        try:
            assert (h2.g2_msm_dev(db, ds, n) == want).all(), ("g2 resident", n, kind)
        finally:
            db.free(); ds.free()
        seen.append(check_plan(zk, plan(n), "g2 %s dev" % kind)["c"])
    assert seen[0] != seen[1], (b, seen)
