"""every entry point that works in ONE pooled mi355_buf block (PoolBlock, csrc/lib_common.hpp) hands the block back on every return: packed and sparse upload, lookup
multiplicities, permutation sigma, nonzero rows, copy check, random rows, pairing products.  One accepted call each at n = 2^10 (with a cheap check of what it wrote) and,
where the DEVICE finds the reason to refuse -- a lookup input that is not in the table, a pairing point off its curve -- one refused call.  After each call
mi355_mem_info's live_buffers and workspace are what they were before it; after mi355_buf_trim so is pooled.  Only invalid arguments are fed: nothing here faults."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import cref, pyref

from gpu_common import rand_fr

pytestmark = pytest.mark.gpu

N, LOG_N = 1 << 10, 10
U64P = C.POINTER(C.c_uint64)
KEY = bytes(range(32))


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def table_of(bufs):
    return (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])


def test_every_pooled_block_entry_returns_its_block(zk):
    h2, capi, lib, check = zk.halo2, zk._capi, zk._capi.lib(), zk._capi.check
    rng = np.random.default_rng(4242)
    check(lib.mi355_buf_trim())
    start = h2.mem_info(0)
    cols = [h2.DeviceBuffer(32 * N) for _ in range(4)]
    before = h2.mem_info(0)
    assert before["live_buffers"] >= start["live_buffers"] + 4 * 32 * N
    seen = []

    def settled(name):
        now = h2.mem_info(0)
        assert (now["live_buffers"], now["workspace"]) == (before["live_buffers"], before["workspace"]), name
        seen.append(name)

    # packed upload: one byte per cell, expanded to Montgomery words on the device
    small = rng.integers(0, 256, size=N, dtype=np.uint64).astype(np.uint8)
    check(lib.mi355_buf_upload_packed(C.c_void_p(cols[0].data_ptr()), capi.ptr(small), N, 1))
    want = cref.f_from_canonical_vec(cref.FR, np.stack([small.astype(np.uint64)] + [np.zeros(N, np.uint64)] * 3, axis=1))
    assert (cols[0].fr() == want).all()
    settled("upload_packed")

    # sparse upload: the non-zero cells of a mostly-zero column
    col = rand_fr(rng, N)
    col[rng.random(N) < 0.7] = 0
    idx, vals = h2.compact_nonzero(col)
    check(lib.mi355_buf_upload_sparse(C.c_void_p(cols[1].data_ptr()), N, capi.ptr(idx), capi.ptr(vals), idx.shape[0]))
    assert (cols[1].fr() == col).all()
    settled("upload_sparse")

    # lookup multiplicities: N distinct table words, the input is the table backwards -> every row is found once
    table = rand_fr(rng, N, full=False)
    table[:, 0] = np.arange(N, dtype=np.uint64)                      # distinct whatever the draw
    cols[0].upload(table); cols[1].upload(np.ascontiguousarray(table[::-1]))
    missing = C.c_uint64(0)
    check(lib.mi355_fr_lookup_multiplicities_dev(C.c_void_p(cols[2].data_ptr()), N, C.c_void_p(cols[0].data_ptr()), N, table_of(cols[1:2]), 1, N, 0, C.byref(missing)))
    assert (cols[2].fr() == cref.fr_mont(1)).all() and missing.value == (1 << 64) - 1
    settled("lookup_multiplicities")
    stray = table[::-1].copy()
    stray[77, 0] = np.uint64(N + 5)                                   # a word no table row holds
    cols[1].upload(np.ascontiguousarray(stray))
    rc = lib.mi355_fr_lookup_multiplicities_dev(C.c_void_p(cols[2].data_ptr()), N, C.c_void_p(cols[0].data_ptr()), N, table_of(cols[1:2]), 1, N, 0, C.byref(missing))
    assert rc == capi.EBADARG and missing.value == 77 and b"input 0, row 77 is not in the table" in lib.mi355_last_error()
    settled("lookup_multiplicities refused")

    # permutation sigma: sigma[j][r] = delta^j omega^r, then one swap of two cells
    delta, omega = h2.fr(7), h2.fr(5)
    cells, images = np.array([3, N + 9], dtype=np.uint64), np.array([N + 9, 3], dtype=np.uint64)
    check(lib.mi355_fr_permutation_sigma_dev(table_of(cols[:3]), 3, LOG_N, capi.ptr(delta), capi.ptr(omega), cells.ctypes.data_as(U64P), images.ctypes.data_as(U64P), 2, 0))
    s0, s1 = cols[0].fr(), cols[1].fr()
    assert (s0[0] == h2.fr(1)).all() and (s1[1] == h2.fr(35)).all() and (cols[2].fr()[2] == h2.fr(49 * 25)).all()
    assert (s0[3] == h2.fr(7 * 5 ** 9)).all() and (s1[9] == h2.fr(5 ** 3)).all()
    settled("permutation_sigma")

    # nonzero rows: three vectors with 0, 1 and 3 non-zero words
    vecs = [np.zeros((N, 4), np.uint64) for _ in range(3)]
    vecs[1][N - 1, 2] = 1
    vecs[2][[5, 600, 1023], 0] = 9
    for b, v in zip(cols, vecs):
        b.upload(v)
    counts, rows = np.zeros(3, np.uint64), np.zeros((3, 4), np.uint64)
    check(lib.mi355_fr_nonzero_rows_dev(table_of(cols[:3]), 3, N, 4, counts.ctypes.data_as(U64P), rows.ctypes.data_as(U64P)))
    assert counts.tolist() == [0, 1, 3] and rows[1, 0] == N - 1 and rows[2, :3].tolist() == [5, 600, 1023] and rows[2, 3] == (1 << 64) - 1
    settled("nonzero_rows")

    # copy check: two columns, three pairs, the middle one between cells that differ
    a, b2 = rand_fr(rng, N), rand_fr(rng, N)
    b2[10] = a[4]; b2[11] = a[4]
    cols[0].upload(a); cols[1].upload(b2)
    cells, images = np.array([4, 5, N + 10], dtype=np.uint64), np.array([N + 10, N + 12, N + 11], dtype=np.uint64)
    n_failed, failed = C.c_uint64(0), np.zeros(4, np.uint64)
    check(lib.mi355_fr_copy_check_dev(table_of(cols[:2]), 2, LOG_N, cells.ctypes.data_as(U64P), images.ctypes.data_as(U64P), 3, 4, C.byref(n_failed), failed.ctypes.data_as(U64P)))
    assert n_failed.value == 1 and failed.tolist() == [1] + [(1 << 64) - 1] * 3
    settled("copy_check")

    # random rows: rows [100, 110) of three columns = elements 0 .. 29 of the stream, the other rows untouched
    marker = np.full((N, 4), 3, np.uint64)
    for b in cols:
        b.upload(marker)
    key = (C.c_uint8 * 32).from_buffer_copy(KEY)
    check(lib.mi355_fr_random_rows_dev(table_of(cols[:3]), 3, 100, 10, key, 6, 0))
    check(lib.mi355_fr_random_dev(C.c_void_p(cols[3].data_ptr()), 30, key, 6, 0))
    flat = cols[3].fr()[:30]
    for c in range(3):
        got = cols[c].fr()
        assert (got[100:110] == flat[10 * c: 10 * c + 10]).all() and (got[:100] == 3).all() and (got[110:] == 3).all()
    settled("random_rows")

    # pairing products: e(2 G1, 5 G2) e(-2 G1, 5 G2) = 1; then the same pairs with one coordinate bit of P[1] flipped
    P = np.ascontiguousarray(cref.g1_mul_generator_vec(np.stack([cref.fr_mont(2), cref.fr_mont(pyref.R_MOD - 2)])), dtype=np.uint64).reshape(2, 8)
    q = cref.g2_mul(cref.g2_generator(), cref.fr_mont(5))
    Q = np.stack([q, q]).astype(np.uint64)
    gt, one = h2.pairing_products(P, Q, 1, 2)
    assert one.tolist() == [1]
    settled("pairing_products")
    P[1, 1] ^= np.uint64(4)
    with pytest.raises(zk.Mi355Error) as e:
        h2.pairing_products(P, Q, 1, 2)
    assert e.value.code == capi.EBADARG and "pair 1 " in str(e.value) and "P is not on the curve" in str(e.value)
    settled("pairing_products refused")

    assert len(seen) == 10
    assert h2.mem_info(0)["pooled"] > start["pooled"]                 # the blocks of the calls above sit in the pool ...
    for b in cols:
        b.free()
    check(lib.mi355_buf_trim())
    end = h2.mem_info(0)
    assert end["pooled"] == start["pooled"] and end["live_buffers"] == start["live_buffers"]   # ... and mi355_buf_trim gives them back to HIP
