"""
-m gpu: the BATCHED transform driver (csrc/lib_ntt.hip: ntt_batch_inplace, distribute_powers_batch_locked, coset_fold_tables) and the vector split of
mi355_fr_nonzero_rows_dev (csrc/lib_aux.hip) past their first chunk, bit-exact against the CPU oracle.

The single transform is pinned at every size and under every knob (tests/test_gpu_fr_full_range.py); the batches of the older tests are of 2 to 7 vectors, so
the chunk loop of ntt_batch_inplace never ran a second time, no call passed more than 65535 vectors (the gridDim.y limit), no plan saw a 17th coset factor and
the coset form never met a destination listed twice.  The prover runs these loops for every column of every proof (93 advice columns at k = 21: 6 chunks).  Here:

  * the plan of a batch is restated below (levels / batched / chunk and the ntt_pass launches that follow); the shapes are the smallest that reach each loop's
    second turn, and after every device call mi355_profile_get("ntt_pass") must report exactly the restated launch count;
  * a batch of cnt vectors is built from P distinct base vectors (vector i = base i mod P: uniform over the whole field, the adversarial pool tiled, a shuffle
    of the two largest words, further whole-field draws), P coprime to every chunk and slice size, so that a vector read or written one chunk, one slot or one
    slice off lands on different data; every vector lives in its own region of one DeviceBuffer; EVERY output vector is compared;
  * every comparison is against oracle/cref.py (best_fft, ifft, f_mul_vec; numpy for the row lists); none against the library itself.
Each device call prints one `batch-row | form | k | cnt | chunk | launches | seconds` line (profiles/ntt_batch_sweep.md is made of these).
"""
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from oracle import cref, pyref
from tests import gpu_common as gc
from tests.test_gpu_fr_full_range import W_ALL_ONES, _ntt_inputs, _power_words, _up

pytestmark = pytest.mark.gpu

R = pyref.R_MOD
RINV = pow(1 << 256, -1, R)

# ------------------------------------------------------------------------------------------------ the plan, restated
# lib_ntt.hip: build_plan (levels), batch_applies, batch_chunk and the chunk loop of ntt_batch_inplace, the slice loop of distribute_powers_batch_locked, the
# factor limit of coset_fold_tables; lib_aux.hip: the vector slices of mi355_fr_nonzero_rows_dev; with the defaults of csrc/knobs.hpp.  A retune of the library
# changes THIS block; every shape below follows from it.
SINGLE_PASS_MAX_LOG, TWO_LEVEL_MAX_LOG, BATCH_MAX_LOG = 8, 18, 22       # plan_is_multi_pass, ntt_two_level_max_log, ntt_batch_max_log
GRID_Y_MAX, SCRATCH_BYTES, WORD = 65535, 1 << 30, 32                    # gridDim.y, the batch's scratch block, sizeof(fe_t)
COSET_FACTORS_MAX = 16                                                  # folded coset factors kept per plan


def levels(k):
    return 1 if k <= SINGLE_PASS_MAX_LOG else 2 if k <= TWO_LEVEL_MAX_LOG else 3


def batched(k, cnt, dsts=None):
    """dsts: the destination addresses (None: all distinct)"""
    return cnt >= 2 and SINGLE_PASS_MAX_LOG < k <= BATCH_MAX_LOG and (dsts is None or len(set(dsts)) == len(dsts))


def chunk(k, cnt):
    return min(cnt, GRID_Y_MAX, max(1, SCRATCH_BYTES // (WORD << k)))


def chunks(k, cnt):
    """the vector counts of the batched launches of one call"""
    c = chunk(k, cnt)
    return [min(c, cnt - base) for base in range(0, cnt, c)]


def launches(k, cnt, dsts=None):
    """ntt_pass scopes of one call: one per pass and chunk when batched, one per pass and vector in the loop of single transforms"""
    return levels(k) * (len(chunks(k, cnt)) if batched(k, cnt, dsts) else cnt)


def slices(cnt):
    """the vector counts of the gridDim.y slices of distribute_powers_batch_locked and mi355_fr_nonzero_rows_dev"""
    return [min(GRID_Y_MAX, cnt - base) for base in range(0, cnt, GRID_Y_MAX)]


# (k, cnt, forms): each the smallest shape that reaches its loop or branch.  fwd: mi355_ntt_fr_batch_dev; inv: the same with the divisor (folded into the
# twiddles of a multi-pass plan); coset: mi355_coset_ntt_fr_batch_dev with the all-ones-limbs word as the factor (folded into the first pass where k >= 9)
CASES = [
    (18, 129, ("fwd", "inv", "coset")),     # chunk loop, two-level plan, a last chunk of ONE vector
    (18, 256, ("fwd",)),                    # exactly two whole chunks
    (19, 65, ("fwd", "inv", "coset")),      # chunk loop, three-level plan
    (21, 17, ("fwd",)),                     # the shape of the product's layer 3 (16 vectors per chunk)
    (9, 65536, ("fwd",)),                   # the 65535 cap of batch_chunk: 1 GiB of data, chunks of 65535 + 1
    (4, 65537, ("coset",)),                 # the 65535 split of distribute_powers_batch_locked: single-pass plan, no fold, then the loop of single transforms
]
ROWS_N, ROWS_BATCH, ROWS_CAP = 3, 65537, 2  # the 65535 split of mi355_fr_nonzero_rows_dev
FACTOR_K, DUP_K = 10, 10                    # the 17th coset factor on one plan; a destination listed twice in the coset form
BLOCK_IO_BELOW = 1 << 20                    # vectors smaller than this many bytes cross PCIe as one block per batch, larger ones one by one


def split_sizes(k, cnt, form):
    """every group size the library cuts this call into"""
    s = set(chunks(k, cnt)) if batched(k, cnt) else set()
    if form == "coset" and levels(k) < 2:
        s |= set(slices(cnt))
    return s


def bases_count(k, cnt, form):
    """P: 3 where every group is a power of two (or one vector), 7 for the 65535 splits (65535 = 3 * 5 * 17 * 257)"""
    return 7 if GRID_Y_MAX in split_sizes(k, cnt, form) else 3


FLAT_CASES = [(k, cnt, form) for k, cnt, forms in CASES for form in forms]


def test_the_sweep_reaches_every_switch_of_the_plan():
    """what the shapes are chosen for: should a retune move a switch away from them, this says so"""
    assert [chunk(k, 10 ** 6) for k in (18, 19, 20, 21, 22)] == [128, 64, 32, 16, 8] and all(chunk(k, 10 ** 6) == GRID_Y_MAX for k in range(0, 10))
    multi = [(k, cnt) for k, cnt, _ in CASES if batched(k, cnt) and len(chunks(k, cnt)) > 1]
    assert {levels(k) for k, _ in multi} == {2, 3}
    assert any(chunks(k, cnt)[-1] == 1 for k, cnt in multi if levels(k) == 2) and any(chunks(k, cnt)[-1] == 1 for k, cnt in multi if levels(k) == 3)
    assert any(len(chunks(k, cnt)) == 2 and len(set(chunks(k, cnt))) == 1 for k, cnt in multi)                 # exactly two whole chunks
    assert chunks(9, 65536) == [GRID_Y_MAX, 1] and SCRATCH_BYTES // (WORD << 9) > GRID_Y_MAX                    # the cap binds, not the scratch block
    assert chunks(21, 17) == [16, 1] and launches(21, 17) == 6 and launches(18, 256) == 4
    assert not batched(4, 65537) and launches(4, 65537) == 65537 and slices(65537) == [GRID_Y_MAX, 2] and slices(ROWS_BATCH) == [GRID_Y_MAX, 2]
    assert not batched(DUP_K, 3, [1, 2, 1]) and launches(DUP_K, 3, [1, 2, 1]) == 6 and launches(FACTOR_K, 3) == 2
    for k, cnt, form in FLAT_CASES:
        P = bases_count(k, cnt, form)
        sizes = split_sizes(k, cnt, form)
        assert sizes and all(math.gcd(P, s) == 1 for s in sizes if s > 1), (k, cnt, form, P, sizes)
        assert P == 3 or GRID_Y_MAX % P, (k, cnt, form)


# ------------------------------------------------------------------------------------------------ inputs and expected values (no device)
_DOMAINS, _BASES, _WANT = {}, {}, {}


def domain(k):
    if k not in _DOMAINS:
        _DOMAINS[k] = ge.load_package().halo2.EvaluationDomain(2, k)      # host-side constants only
    return _DOMAINS[k]


def bases(k, P):
    """P distinct read-only base vectors of 2^k words: the three kinds of _ntt_inputs, then further whole-field draws"""
    if (k, P) not in _BASES:
        out = list(_ntt_inputs(k).values())
        out += [gc.rand_fr_full(np.random.default_rng(9300 + 16 * k + j), 1 << k) for j in range(3, P)]
        out = [np.ascontiguousarray(b) for b in out[:P]]
        for b in out:
            b.setflags(write=False)
        assert all((out[i] != out[j]).any() for i in range(P) for j in range(i))
        _BASES[k, P] = out
    return _BASES[k, P]


def coset_powers(factor_word, n):
    """the Montgomery words of f^i, i < n: _power_words (Python integers) for the first 1024, then doubled through cref.f_mul_vec; the ends of every doubling are
    checked against Python's pow"""
    f = factor_word * RINV % R
    pw = _power_words(factor_word, 1024)[: min(n, 1024)]
    while pw.shape[0] < n:
        m = pw.shape[0]
        step = gc.tile_words(gc.ints_to_words([pow(f, m, R) * (1 << 256) % R]), m)
        pw = np.concatenate([pw, cref.f_mul_vec(cref.FR, pw, step)])
        assert gc.words_to_ints(pw[[m, 2 * m - 1]]) == [pow(f, m, R) * (1 << 256) % R, pow(f, 2 * m - 1, R) * (1 << 256) % R]
    return pw


def expected(k, P, form, factor_word=gc.ALL_ONES_LIMBS, omega=None):
    """the oracle's outputs for the P bases, computed once per (k, P, form, factor, omega) and shared, read-only"""
    key = (k, P, form, factor_word, None if omega is None else omega.tobytes())
    if key not in _WANT:
        dom = domain(k)
        w = dom.omega if omega is None else omega
        if form == "fwd":
            out = [cref.best_fft(b, w, k) for b in bases(k, P)]
        elif form == "inv":
            out = [cref.ifft(b, dom.omega_inv, k, dom.ifft_divisor) for b in bases(k, P)]
        else:
            pw = coset_powers(factor_word, 1 << k)
            out = [cref.best_fft(cref.f_mul_vec(cref.FR, b, pw), w, k) for b in bases(k, P)]
        for o in out:
            o.setflags(write=False)
        assert all((out[i] != out[j]).any() for i in range(P) for j in range(i)), "two bases give the same output: a misplaced vector would not show"
        _WANT[key] = out
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ the device side
_LIVE = []                                                                # the buffers of a running test: the fixture frees what a failing one leaves


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    yield pkg
    lib, check = pkg._capi.lib(), pkg._capi.check
    while _LIVE:
        _LIVE.pop().free()
    _BASES.clear(); _WANT.clear()                                         # half a GiB of host memory
    check(lib.mi355_profile_enable(0))
    check(lib.mi355_synchronize())
    check(lib.mi355_buf_trim())                                           # the 2 GiB blocks of this module do not stay pooled for later modules


def alloc(zk, regions, n):
    """one DeviceBuffer of `regions` vectors of n words"""
    b = zk.halo2.DeviceBuffer(WORD * n * regions)
    _LIVE.append(b)
    return b


def release(b):
    b.free()
    _LIVE.remove(b)


def region_ptrs(buf, first, cnt, n):
    return [buf.data_ptr() + WORD * n * (first + i) for i in range(cnt)]


def fill(buf, first, cnt, n, vecs):
    """region first + i := vecs[i mod len(vecs)]"""
    P = len(vecs)
    if WORD * n >= BLOCK_IO_BELOW:
        for i in range(cnt):
            buf.upload(vecs[i % P], WORD * n * (first + i))
    else:
        buf.upload(np.stack(vecs)[np.arange(cnt) % P], WORD * n * first)


def check_regions(buf, first, cnt, n, vecs, what):
    """region first + i == vecs[i mod len(vecs)] for EVERY i; a mismatch names the vector and, where it is one, the base whose data it holds instead"""
    P = len(vecs)

    def explain(i, got):
        other = [j for j in range(P) if (got == vecs[j]).all()]
        row = int(np.flatnonzero((got != vecs[i % P]).any(axis=1))[0])
        return "%s: vector %d of %d differs from the oracle's output of base %d at word %d%s" % (
            what, i, cnt, i % P, row, " (it holds the output of base %d)" % other[0] if other else "")

    if WORD * n >= BLOCK_IO_BELOW:
        for i in range(cnt):
            got = buf.download(WORD * n, WORD * n * (first + i)).reshape(n, 4)
            assert np.array_equal(got, vecs[i % P]), explain(i, got)
    else:
        got = buf.download(WORD * n * cnt, WORD * n * first).reshape(cnt, n, 4)
        for j in range(P):
            bad = np.flatnonzero((got[j::P] != vecs[j]).any(axis=(1, 2)))
            assert bad.size == 0, explain(j + P * int(bad[0]), got[j + P * int(bad[0])])


def counted(zk, form, k, cnt, call, dsts=None):
    """one device call between mi355_profile_reset and mi355_profile_get: the ntt_pass launches must be the restated ones"""
    lib, check = zk._capi.lib(), zk._capi.check
    check(lib.mi355_profile_enable(1)); check(lib.mi355_profile_reset())
    t0 = time.perf_counter()
    call()
    check(lib.mi355_synchronize())
    dt = time.perf_counter() - t0
    ms, got = C.c_double(), C.c_uint64()
    check(lib.mi355_profile_get(b"ntt_pass", C.byref(ms), C.byref(got)))
    want = launches(k, cnt, dsts)
    print("batch-row | %s | %d | %d | %s | %d | %.4f" % (form, k, cnt, chunk(k, cnt) if batched(k, cnt, dsts) else "-", got.value, dt))
    assert got.value == want, (form, k, cnt, "ntt_pass launches", got.value, "restated", want)


def void_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


@pytest.mark.parametrize("k,cnt,form", FLAT_CASES, ids=["%s-k%d-x%d" % (f, k, c) for k, c, f in FLAT_CASES])
def test_batches_past_one_chunk_equal_the_oracle(zk, k, cnt, form):
    """every vector of a batch that the library cuts into more than one chunk (or gridDim.y slice) against the oracle's transform of its base; the coset
    forms write to destinations of their own and leave the sources as they were"""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    n, dom = 1 << k, domain(k)
    P = bases_count(k, cnt, form)
    src, want = bases(k, P), expected(k, P, form)
    assert len(split_sizes(k, cnt, form)) > 1 or chunks(k, cnt) == [chunk(k, cnt)] * 2
    buf = alloc(zk, cnt * (2 if form == "coset" else 1), n)
    try:
        dst = void_array(region_ptrs(buf, 0, cnt, n))
        if form == "coset":
            fill(buf, cnt, cnt, n, src)
            check(lib.mi355_buf_zero(C.c_void_p(buf.data_ptr()), WORD * n * cnt))
            from_ = void_array(region_ptrs(buf, cnt, cnt, n))
            counted(zk, form, k, cnt, lambda: check(lib.mi355_coset_ntt_fr_batch_dev(dst, from_, cnt, k, ptr(W_ALL_ONES), ptr(dom.omega))))
            check_regions(buf, cnt, cnt, n, src, "the sources of %s k=%d cnt=%d" % (form, k, cnt))
        else:
            fill(buf, 0, cnt, n, src)
            w, div = (dom.omega, None) if form == "fwd" else (dom.omega_inv, dom.ifft_divisor)
            counted(zk, form, k, cnt, lambda: check(lib.mi355_ntt_fr_batch_dev(dst, cnt, k, ptr(w), ptr(div))))
        check_regions(buf, 0, cnt, n, want, "%s k=%d cnt=%d" % (form, k, cnt))
    finally:
        release(buf)


def test_nonzero_rows_past_the_grid_y_limit(zk):
    """mi355_fr_nonzero_rows_dev over 65537 vectors of 3 words, cap 2: the second slice (vectors 65535 and 65536) has its own offsets into the pointer table, the
    per-workgroup counts, the totals and the row lists.  Non-zero rows in vectors 0, 65534, 65535 and 65536 (each a different set) and in a few between,
    all-zero vectors among them; counts and rows from numpy."""
    lib, check = zk._capi.lib(), zk._capi.check
    n, batch, cap = ROWS_N, ROWS_BATCH, ROWS_CAP
    assert slices(batch) == [GRID_Y_MAX, 2]
    pool = gc.adversarial_fr_words()
    pool = pool[pool.any(axis=1)]
    data = np.zeros((batch, n, 4), dtype=np.uint64)
    hits = {0: [1], 1: [0, 1], 2: [2], 32768: [0, 2], GRID_Y_MAX - 2: [0], GRID_Y_MAX - 1: [0, 2], GRID_Y_MAX: [0, 1, 2], GRID_Y_MAX + 1: [2]}
    for j, (v, rows) in enumerate(hits.items()):
        for r in rows:
            data[v, r] = pool[(5 * j + r) % pool.shape[0]]
    data[3, 1, 3] = np.uint64(1) << np.uint64(63)                        # only the top bit of the top limb
    nz = data.any(axis=2)
    want_counts = nz.sum(axis=1).astype(np.uint64)
    want_rows = np.full((batch, cap), (1 << 64) - 1, dtype=np.uint64)
    for v in np.flatnonzero(want_counts):
        r = np.flatnonzero(nz[v])[:cap]
        want_rows[v, : r.size] = r
    assert int((want_counts == 0).sum()) == batch - len(hits) - 1 and want_counts[GRID_Y_MAX] == 3
    buf = _up(zk, data)
    _LIVE.append(buf)
    try:
        arr = void_array(region_ptrs(buf, 0, batch, n))
        counts = np.full(batch, 77, dtype=np.uint64)
        rows = np.full((batch, cap), 77, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        t0 = time.perf_counter()
        check(lib.mi355_fr_nonzero_rows_dev(arr, batch, n, cap, counts.ctypes.data_as(u64p), rows.ctypes.data_as(u64p)))
        print("batch-row | nonzero_rows | n=%d | %d | %d | - | %.4f" % (n, batch, GRID_Y_MAX, time.perf_counter() - t0))
        bad = np.flatnonzero(counts != want_counts)
        assert bad.size == 0, ("counts", bad[:8].tolist(), counts[bad[:8]].tolist(), want_counts[bad[:8]].tolist())
        bad = np.flatnonzero((rows != want_rows).any(axis=1))
        assert bad.size == 0, ("rows", bad[:8].tolist(), rows[bad[:8]].tolist(), want_rows[bad[:8]].tolist())
        assert (buf.fr().reshape(batch, n, 4) == data).all()              # the vectors are only read
    finally:
        release(buf)


def optional_table_bytes(zk):
    return zk.halo2.mem_usage()["classes"]["ntt_optional"]               # MEM_NTT_OPTIONAL of csrc/mem_budget.hpp


def test_the_seventeenth_coset_factor_on_one_plan_takes_the_separate_pass(zk):
    """coset_fold_tables keeps 16 factors per plan: each of the first 16 distinct factors builds its tables (the optional-table bytes of mi355_mem_usage grow),
    the 17th builds none and the call scales in a pass of its own -- on the same live plan, single call and batch, with a folded factor again afterwards.  The
    plan is keyed by omega: the cube of the domain's generator (a primitive 2^k-th root as well) is a plan no other test has touched."""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    h2 = zk.halo2
    k, n, P = FACTOR_K, 1 << FACTOR_K, 3
    w3 = pow(h2.FR_ROOT_OF_UNITY, 3 << (h2.FR_S - k), R)
    omega = h2.fr(w3)
    assert pow(w3, n // 2, R) == R - 1 and (omega != domain(k).omega).any()
    factors = [gc.ALL_ONES_LIMBS, R - 1, pyref.MONT_R % R] + gc.words_to_ints(gc.rand_fr_full(np.random.default_rng(9317), COSET_FACTORS_MAX - 2))
    assert len(set(factors)) == COSET_FACTORS_MAX + 1
    src = bases(k, P)
    buf = alloc(zk, 2 * P, n)
    try:
        fill(buf, P, P, n, src)
        dst, from_ = region_ptrs(buf, 0, P, n), region_ptrs(buf, P, P, n)
        held = optional_table_bytes(zk)
        for j, f in enumerate(factors):
            fw = gc.ints_to_words([f])[0]
            want = expected(k, P, "coset", f, omega)
            counted(zk, "coset factor %d" % (j + 1), k, 1,
                    lambda: check(lib.mi355_coset_ntt_fr_dev(C.c_void_p(dst[j % P]), C.c_void_p(from_[j % P]), k, ptr(fw), ptr(omega))))
            got = buf.download(WORD * n, WORD * n * (j % P)).reshape(n, 4)
            assert (got == want[j % P]).all(), ("factor", j + 1)
            now = optional_table_bytes(zk)
            assert (now > held) if j < COSET_FACTORS_MAX else (now == held), ("optional NTT table bytes after factor %d" % (j + 1), held, now)
            held = now
        for f in (factors[COSET_FACTORS_MAX], factors[0]):                # the 17th (separate scaling pass, then the plain batch), then a folded one
            check(lib.mi355_buf_zero(C.c_void_p(buf.data_ptr()), WORD * n * P))
            counted(zk, "coset batch", k, P, lambda: check(lib.mi355_coset_ntt_fr_batch_dev(void_array(dst), void_array(from_), P, k, ptr(gc.ints_to_words([f])[0]), ptr(omega))))
            check_regions(buf, 0, P, n, expected(k, P, "coset", f, omega), "coset batch, factor %#x" % f)
            assert optional_table_bytes(zk) == held
        check_regions(buf, P, P, n, src, "the sources")
    finally:
        release(buf)


def test_a_destination_listed_twice_in_the_coset_form_runs_the_serial_loop(zk):
    """dst = [A, B, A] with three different sources: no batched launch (two transforms would write A at once) but the loop of single transforms, which leaves
    in A the coset transform of the THIRD source and in B that of the second"""
    lib, check, ptr = zk._capi.lib(), zk._capi.check, zk._capi.ptr
    k, n, P = DUP_K, 1 << DUP_K, 3
    src, want = bases(k, P), expected(k, P, "coset")
    buf = alloc(zk, 2 + P, n)
    try:
        fill(buf, 2, P, n, src)
        check(lib.mi355_buf_zero(C.c_void_p(buf.data_ptr()), WORD * n * 2))
        A, B = region_ptrs(buf, 0, 2, n)
        dsts = [A, B, A]
        counted(zk, "coset dup", k, P, lambda: check(lib.mi355_coset_ntt_fr_batch_dev(void_array(dsts), void_array(region_ptrs(buf, 2, P, n)), P, k, ptr(W_ALL_ONES), ptr(domain(k).omega))), dsts=dsts)
        check_regions(buf, 0, 2, n, [want[2], want[1]], "dst = [A, B, A]")
        check_regions(buf, 2, P, n, src, "the sources")
    finally:
        release(buf)
