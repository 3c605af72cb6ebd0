"""-m gpu: the kernels of the device randomness (csrc/frrand.hpp through mi355_fr_random_dev, mi355_fr_random_rows_dev, mi355_fr_from_u512_dev) against
tests/frrand_common.py word for word.  Every vector sits inside a larger poisoned buffer whose guard words must come back untouched.  The sizes straddle the wave
(64), the workgroup (256) and, with the workgroup count forced down, the grid: every lane then walks the grid-stride loop twice."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from tests import frrand_common as fc

pytestmark = pytest.mark.gpu
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD = 64                                   # words either side of a vector
KEY = bytes.fromhex("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f")
KEY_FF = b"\xff" * 32
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097]
STREAMS = [0, (1 << 63) | 5]
COUNTERS = [0, (1 << 32) - 3]


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


@pytest.fixture(scope="module")
def reference():
    """(stream, counter0) -> the first max(SIZES) words of the draw; computed once, read-only"""
    ref = {}
    for s in STREAMS:
        for c0 in COUNTERS:
            a = fc.elements(KEY, s, c0, max(SIZES)); a.setflags(write=False); ref[(s, c0)] = a
    return ref


def poisoned(words):
    return torch.from_numpy(np.full((words, 4), POISON, dtype=np.uint64).view(np.int64)).cuda()


def back(t):
    return t.cpu().numpy().view(np.uint64)


def guards_intact(buf, n):
    a = back(buf)
    return (a[:GUARD] == POISON).all() and (a[GUARD + n:] == POISON).all()


@pytest.mark.parametrize("n", SIZES)
def test_fr_random_matches_the_cpu_word_for_word(zk, reference, n):
    h2 = zk.halo2
    got = {}
    for s in STREAMS:
        for c0 in COUNTERS:
            buf = poisoned(n + 2 * GUARD)
            h2.fr_random(buf[GUARD:GUARD + n], KEY, s, c0)
            assert guards_intact(buf, n), (s, c0)
            got[(s, c0)] = back(buf)[GUARD:GUARD + n]
            assert (got[(s, c0)] == reference[(s, c0)][:n]).all(), (s, c0)
    assert not (got[(STREAMS[0], 0)] == got[(STREAMS[1], 0)]).all(axis=1).any()      # two streams share no word
    assert not (got[(STREAMS[0], 0)] == got[(STREAMS[0], COUNTERS[1])]).all(axis=1).any()


def test_every_lane_loops_twice_and_the_grid_does_not_show(zk, monkeypatch):
    """3 workgroups = 768 lanes for 2 * 768 + 5 words: two full sweeps and a partial third; the same words as the default grid gives"""
    h2 = zk.halo2
    n = 2 * 768 + 5
    want = fc.elements(KEY_FF, 9, (1 << 32) - 700, n)                                   # the counter crosses 2^32 in the middle of the first sweep
    out = []
    for blocks in ("3", None):
        if blocks:
            monkeypatch.setenv("MI355_FR_RANDOM_BLOCKS", blocks)
        else:
            monkeypatch.delenv("MI355_FR_RANDOM_BLOCKS")
        buf = poisoned(n + 2 * GUARD)
        h2.fr_random(buf[GUARD:GUARD + n], KEY_FF, 9, (1 << 32) - 700)
        assert guards_intact(buf, n)
        out.append(back(buf)[GUARD:GUARD + n])
    assert (out[0] == want).all() and (out[1] == want).all()
    monkeypatch.setenv("MI355_FR_RANDOM_BLOCKS", "2")
    src = torch.from_numpy(fc.u512_rows(fc.extreme_u512()[:1100]).view(np.int64).reshape(-1, 8)).cuda()
    assert (back(h2.fr_from_u512(src)) == fc.from_u512_bytes(fc.u512_rows(fc.extreme_u512()[:1100]))).all()
    cols = poisoned(3 * 512).reshape(3, 512, 4)
    h2.fr_random_rows([cols[c] for c in range(3)], 0, 512, KEY, 4, 11)                 # 1536 cells on 512 lanes
    assert (back(cols).reshape(-1, 4) == fc.elements(KEY, 4, 11, 1536)).all()


def test_fr_random_in_pieces_equals_one_call(zk, reference):
    h2 = zk.halo2
    n, s, c0 = 4097, STREAMS[1], COUNTERS[1]
    for a in (1, 255, 256, 4096):
        buf = poisoned(n + 2 * GUARD)
        h2.fr_random(buf[GUARD:GUARD + a], KEY, s, c0)
        h2.fr_random(buf[GUARD + a:GUARD + n], KEY, s, c0 + a)
        assert guards_intact(buf, n)
        assert (back(buf)[GUARD:GUARD + n] == reference[(s, c0)][:n]).all(), a


@pytest.mark.parametrize("n_cols", [1, 3, 70])
@pytest.mark.parametrize("rows", [1, 6])
def test_fr_random_rows_writes_the_last_rows_only(zk, n_cols, rows):
    h2 = zk.halo2
    n, c0, stream = 128, (1 << 32) - 5, 1
    stride = n + GUARD
    buf = poisoned(GUARD + n_cols * stride)
    cols = [buf[GUARD + c * stride:GUARD + c * stride + n] for c in range(n_cols)]
    h2.fr_random_rows(cols, n - rows, rows, KEY, stream, c0)
    a = back(buf)
    want = fc.elements(KEY, stream, c0, n_cols * rows).reshape(n_cols, rows, 4)
    mask = np.zeros(a.shape[0], dtype=bool)
    for c in range(n_cols):
        lo = GUARD + c * stride + n - rows
        assert (a[lo:lo + rows] == want[c]).all(), c
        mask[lo:lo + rows] = True
    assert (a[~mask] == POISON).all()                                                  # the rows below row0 and every guard word


def test_fr_from_u512_on_the_extreme_words_and_edge_lengths(zk):
    h2 = zk.halo2
    vals = fc.extreme_u512()
    rows = fc.u512_rows(vals)
    want = fc.from_u512_bytes(rows)
    assert all(int(x) < fc.R for x in (sum(int(v) << (64 * i) for i, v in enumerate(w)) for w in want[:64]))
    src = torch.from_numpy(rows.view(np.int64).reshape(-1, 8)).cuda()
    for n in (1, 63, 64, 65, 255, 256, 257, len(vals)):
        buf = poisoned(n + 2 * GUARD)
        h2.fr_from_u512(src[:n], buf[GUARD:GUARD + n])
        assert guards_intact(buf, n), n
        assert (back(buf)[GUARD:GUARD + n] == want[:n]).all(), n


def test_argument_checks_on_the_device(zk):
    h2, capi = zk.halo2, zk._capi
    lib = capi.lib()
    key = (C.c_uint8 * 32).from_buffer_copy(KEY)
    buf = poisoned(16)
    assert lib.mi355_fr_random_dev(capi.ptr(buf), 0, key, 0, 0) == capi.OK                                        # n = 0: no launch
    assert lib.mi355_fr_random_rows_dev((C.c_void_p * 1)(buf.data_ptr()), 0, 0, 4, key, 0, 0) == capi.OK
    assert lib.mi355_fr_from_u512_dev(capi.ptr(buf), capi.ptr(buf), 0) == capi.OK
    assert lib.mi355_fr_random_dev(capi.ptr(buf), 16, key, 0, (1 << 64) - 10) == capi.EBADARG                     # would wrap
    assert lib.mi355_fr_random_dev(C.c_void_p(buf.data_ptr() + 8), 4, key, 0, 0) == capi.EBADARG                  # misaligned
    assert lib.mi355_fr_from_u512_dev(capi.ptr(buf), capi.ptr(buf), 4) == capi.EBADARG                            # overlap
    assert (back(buf) == POISON).all()
    d = h2.DeviceBuffer(32 * 8)                                                                                   # a library block: the draw must stay inside it
    assert lib.mi355_fr_random_dev(C.c_void_p(d.data_ptr()), 9, key, 0, 0) == capi.EBADARG
    assert lib.mi355_fr_random_rows_dev((C.c_void_p * 1)(d.data_ptr()), 1, 6, 3, key, 0, 0) == capi.EBADARG
    h2.fr_random(d, KEY, 2, 7)
    assert (d.fr() == fc.elements(KEY, 2, 7, 8)).all()
    d.free()
