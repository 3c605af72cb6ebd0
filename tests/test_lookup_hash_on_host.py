"""Runs the host-visible part of the multiplicity kernels (csrc/lookup.hpp: lk_hash, lk_eq, LK_EMPTY, LK_ROUNDS, LK_HOT_MIN -- the very code the kernels call) on the
CPU via tests/hostcheck/lookup_hash_main.cpp and holds the restatements of tests/lookup_common.py equal to it: the numpy lk_hash, with which
tests/test_gpu_lookup_structured.py puts keys into chosen slots of the device's hash set, and wave_trace, with which it proves that its columns take the
hot-row and exhausted-round branches of k_lk_probe.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lookup_common as lc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "lookup_hash_main.cpp")
MASKS = (63, 4095, (1 << 27) - 1)


@pytest.fixture(scope="module")
def lkh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lkh") / "liblookuphash.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.lkh_hash.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.lkh_eq.argtypes = [C.c_void_p, C.c_void_p]
    lib.lkh_eq.restype = C.c_int
    lib.lkh_empty.restype = C.c_uint32
    lib.lkh_rounds.restype = C.c_int
    lib.lkh_hot_min.restype = C.c_uint32
    return lib


def cpp_hash(lkh, words, mask):
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    out = np.full(len(words), 0xA5A5A5A5, dtype=np.uint32)
    lkh.lkh_hash(words.ctypes.data, len(words), mask, out.ctypes.data)
    return out


def hash_words():
    """zero, every single bit 0 .. 253, every limb alone (all ones, and a pattern), r - 1, and 10 000 random reduced words"""
    rng = np.random.default_rng(5150)
    vals = [0] + [1 << b for b in range(254)]
    vals += [0xFFFFFFFF << (32 * k) for k in range(7)] + [0x30644E72 << 224] + [0x9E3779B9 >> (3 if k == 7 else 0) << (32 * k) for k in range(8)]
    vals += [lc.R_MOD - 1]
    w = rng.integers(0, 2**64, size=(10000, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)                               # below 2^252 < r
    return np.concatenate([lc.int_words(vals), w])


@pytest.mark.parametrize("mask", MASKS)
def test_numpy_hash_equals_the_header_s(lkh, mask):
    words = hash_words()
    got, want = lc.lk_hash(words, mask), cpp_hash(lkh, words, mask)
    assert got.dtype == np.uint32 and (got == want).all(), np.nonzero(got != want)[0][:5]
    assert int(want.max()) <= mask and int(want[0]) == 0
    if mask == 4095:
        assert len(np.unique(want[1:255])) > 200                      # the single-bit words spread: no bit of the word is dropped on the way to the slot


def test_montgomery_words_of_small_integers(lkh):
    vals = list(range(0, 3000)) + [lc.R_MOD - 1, lc.R_MOD - 2]
    words = lc.mont_words(vals)
    assert (words[:50] == np.stack([lc.fr_mont(v) for v in vals[:50]])).all() and (words[-1] == lc.fr_mont(lc.R_MOD - 2)).all()
    for mask in MASKS:
        assert (lc.lk_hash(words, mask) == cpp_hash(lkh, words, mask)).all()


def test_colliding_values_collide_in_the_header_s_hash(lkh):
    for S, home, count, start in ((64, 50, 25, 1), (4096, 4093, 40, 1), (64, 0, 5, 1000)):
        vals = lc.colliding_values(S, home, count, start)
        assert len(vals) == count and vals == sorted(set(vals)) and vals[0] >= start
        assert (cpp_hash(lkh, lc.mont_words(vals), S - 1) == home).all()
        others = [v for v in range(start, vals[-1]) if v not in set(vals)]       # the FIRST such integers: none in between was skipped
        assert not (cpp_hash(lkh, lc.mont_words(others), S - 1) == home).any()


def test_eq_is_false_at_every_hamming_distance_one(lkh):
    rng = np.random.default_rng(77)
    bases = [0, lc.R_MOD - 1, (1 << 252) - 1] + [int.from_bytes(rng.bytes(32), "little") >> 4 for _ in range(5)]
    for base in bases:
        a = lc.int_words([base])[0]
        assert lkh.lkh_eq(a.ctypes.data, a.ctypes.data) == 1
        for b in range(256):
            w = a.copy()
            w[b >> 6] ^= np.uint64(1 << (b & 63))                     # all 256 bits: lk_eq compares words, reduced or not
            assert lkh.lkh_eq(a.ctypes.data, w.ctypes.data) == 0 and lkh.lkh_eq(w.ctypes.data, a.ctypes.data) == 0, (hex(base), b)


def test_constants_are_the_header_s(lkh):
    assert (lkh.lkh_empty(), lkh.lkh_rounds(), lkh.lkh_hot_min()) == (lc.LK_EMPTY, lc.LK_ROUNDS, lc.LK_HOT_MIN)


def test_slots_and_wave_rows_follow_the_driver():
    src = open(os.path.join(HERE, "..", "scroll-prover_amd", "csrc", "lib_aux.hip")).read()
    assert "std::max<uint64_t>(64, 1ull << log2_ceil(2 * table_rows))" in src and "std::max<uint64_t>(2048, (ceil_div(input_rows, 8192) + 63) & ~63ull)" in src
    assert [lc.slots_for(t) for t in (0, 1, 32, 33, 263, 2048, 2049)] == [64, 64, 64, 128, 1024, 4096, 8192]
    assert [lc.wave_rows_for(r) for r in (0, 1, 2048, 4133, 1 << 24, (1 << 24) + 1, 1 << 26)] == [2048, 2048, 2048, 2048, 2048, 2112, 8192]


def test_wave_trace_counts_equal_the_reference_on_random_columns():
    rng = np.random.default_rng(31)
    seen_switch = seen_tail = 0
    for n, values, heavy in ((64, 3, 0.0), (500, 40, 0.5), (4133, 9, 0.3), (8192, 2000, 0.2), (6000, 5, 0.0), (2048, 1, 0.0)):
        t = rng.permutation(n) % values                                # every value several times: the first rule counts at its first row
        first = {int(v): int(np.nonzero(t == v)[0][0]) for v in np.unique(t)}
        for input_rows in (n, n - 27, 0):
            x = rng.integers(0, values, size=n)
            x[rng.random(n) < heavy] = int(rng.integers(0, values))    # one dominant value, in runs and scattered
            lo = int(rng.integers(0, n)); x[lo: lo + 200] = int(rng.integers(0, values))
            want, miss = lc.reference_ids(t, n, [x], input_rows, n)
            assert miss is None
            rows = np.array([first[int(v)] for v in x])
            for wave_rows in (2048, 64, 128):
                counts, switches, tails, cold = lc.wave_trace(rows, input_rows, wave_rows)
                assert (np.pad(counts, (0, n - len(counts))) == want).all(), (n, values, input_rows, wave_rows)
                assert counts.sum() == input_rows and cold <= 64
                seen_switch += switches; seen_tail += tails
    assert seen_switch > 0 and seen_tail > 0                            # the trace's own branches were all walked
    counts, switches, tails, cold = lc.wave_trace(np.array([3, -1, 3, 5]), 4, 2048)     # a miss takes no part
    assert counts.tolist() == [0, 0, 0, 2, 0, 1] and (switches, tails, cold) == (0, 0, 2)


def test_wave_trace_on_hand_made_blocks():
    a16 = [7] * 16 + list(range(100, 148))
    b17 = [8] * 17 + list(range(200, 247))
    counts, switches, tails, cold = lc.wave_trace(np.array(a16 + b17 + [7] * 64 + [8] * 20 + [9] * 15 + list(range(300, 329))), 256, 2048)
    # A becomes hot on an empty hand (no switch), B displaces it at 17 > 16, A x 64 displaces B; B x 20 and C x 15 then stay cold
    assert (switches, cold) == (2, 20) and tails == 3 and counts[7] == 80 and counts[8] == 37 and counts[9] == 15
    counts, switches, tails, cold = lc.wave_trace(np.array([1] * (lc.LK_HOT_MIN - 1) + [2] * 49), 64, 2048)
    assert (switches, tails, cold) == (0, 0, lc.LK_HOT_MIN - 1) and counts.tolist() == [0, 15, 49]          # 15 stays cold, 49 becomes hot
    counts, switches, tails, cold = lc.wave_trace(np.arange(64) % (lc.LK_ROUNDS + 1), 64, 2048)
    assert tails == 1 and counts.tolist() == [13, 13, 13, 13, 12] and cold == 13


def test_occupied_slots_and_one_limb_pairs():
    vals = lc.colliding_values(64, 62, 5)
    occ, homes, longest = lc.occupied_slots(lc.mont_words(vals + [0] * 27), 32)      # zero hashes to slot 0: the cluster 62, 63 wraps onto it
    assert (homes == 62).sum() == 5 and occ[[62, 63, 0, 1, 2, 3]].all() and occ.sum() == 6 and longest == 6
    w = lc.int_words([5, 5 ^ (1 << 40), 5 ^ (1 << 200), 9 << 64, (9 << 64) ^ 1 ^ (1 << 33)])
    assert lc.one_limb_pairs(w) == [False, True, False, False, False, False, True, False]


def test_selftest_program_under_sanitizers(tmp_path):
    """the same source as a stand-alone program (its own main) under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "lookup_hash_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DLOOKUP_HASH_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout and "FAIL" not in out.stdout
