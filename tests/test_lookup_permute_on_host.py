"""Runs the per-element bodies of csrc/lookup_permute.hpp (canonical key and digit, the pass-skipping decision, run expansion, leftover placement -- the very code
the kernels call) on the CPU via tests/hostcheck/lookup_permute_main.cpp, which walks the device's pipeline with them, and holds the result equal to the
integer restatement of halo2's permute_expression_pair in tests/lookup_permute_common.py, on the cases and sizes of the GPU test.  The same source as a
stand-alone program checks itself against std::sort + std::map under AddressSanitizer and UBSan.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lookup_permute_common as pc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "lookup_permute_main.cpp")
HOST_SIZES = [s for s in pc.SIZES if s <= 4099]      # the 65 539-row cases run in the stand-alone program below


@pytest.fixture(scope="module")
def lph(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lph") / "liblookuppermute.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.lph_permute.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.lph_permute.restype = C.c_int
    lib.lph_canonical.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.lph_pass_needed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.lph_digit.argtypes = [C.c_uint32, C.c_uint32]
    lib.lph_digit.restype = C.c_uint32
    lib.lph_leftover_of_row.argtypes = [C.c_uint32] * 4
    lib.lph_leftover_of_row.restype = C.c_uint32
    return lib


def host_permute(lph, inputs, table):
    rows = len(inputs)
    iw, tw = pc.to_words(inputs), pc.to_words(table)
    a = np.full((rows + 1, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    s = a.copy()
    missing, passes = C.c_uint64(0), C.c_uint32(0)
    rc = lph.lph_permute(iw.ctypes.data, tw.ctypes.data, rows, a.ctypes.data, s.ctypes.data, C.byref(missing), C.byref(passes))
    assert (a[rows] == 0xA5A5A5A5A5A5A5A5).all() and (s[rows] == 0xA5A5A5A5A5A5A5A5).all()
    return rc, a[:rows], s[:rows], missing.value, passes.value


def test_the_restatement_on_a_hand_made_pair():
    # sorted input 1 1 1 2 4 4; heads at rows 0, 3, 4; leftovers of the table ascending: 3, 4, 9 -> rows 5, 2, 1
    a, s, miss = pc.permute([4, 1, 2, 1, 4, 1], [9, 4, 3, 2, 1, 4])
    assert miss is None and a == [1, 1, 1, 2, 4, 4] and s == [1, 9, 4, 2, 4, 3]
    pc.check_constraints(a, s, [4, 1, 2, 1, 4, 1], [9, 4, 3, 2, 1, 4])
    assert pc.permute([4, 7, 2, 8], [9, 4, 3, 2])[2] == 1
    assert pc.from_words(pc.to_words([0, 1, pc.R_MOD - 1, 1 << 200])) == [0, 1, pc.R_MOD - 1, 1 << 200]


def test_montgomery_word_order_is_not_the_canonical_order():
    w = pc.to_words(pc.ORDER_VALUES)
    as_ints = [int.from_bytes(x.tobytes(), "little") for x in w]
    assert sorted(range(len(as_ints)), key=as_ints.__getitem__) != sorted(range(len(as_ints)), key=pc.ORDER_VALUES.__getitem__)


@pytest.mark.parametrize("rows", HOST_SIZES)
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_host_bodies_equal_the_restatement(lph, name, rows):
    rng = np.random.default_rng(1000 + rows)
    inputs, table = pc.CASES[name](rows, rng)
    a, s, miss = pc.permute(inputs, table)
    assert miss is None
    pc.check_constraints(a, s, inputs, table)
    rc, ga, gs, gmiss, passes = host_permute(lph, inputs, table)
    assert rc == 0 and gmiss == (1 << 64) - 1
    assert (ga == pc.to_words(a)).all() and (gs == pc.to_words(s)).all()
    if name == "one_digit":
        assert passes == (1 if rows > 1 else 0)
    if name == "range_zero_tail":
        assert passes == (-(-pc._range_bits(rows) // 8) if rows > 1 else 0)
    if name == "shuffle" and rows >= 4099:
        assert passes == 32


@pytest.mark.parametrize("rows", [1, 65, 4099])
def test_a_missing_value_names_the_smallest_row(lph, rows):
    rng = np.random.default_rng(7)
    inputs, table = pc.CASES["duplicated_table"](rows, rng)
    for row in sorted({0, rows // 2, rows - 1}):
        bad = pc.with_missing(inputs, table, row)
        assert pc.permute(bad, table)[2] == row
        rc, _, _, gmiss, _ = host_permute(lph, bad, table)
        assert rc == 1 and gmiss == row
    if rows > 2:
        bad = pc.with_missing(pc.with_missing(inputs, table, rows - 1), table, 1)
        assert host_permute(lph, bad, table)[3] == 1 and pc.permute(bad, table)[2] == 1


def test_bodies_one_by_one(lph):
    vals = pc.ORDER_VALUES + [int.from_bytes(np.random.default_rng(3).bytes(32), "little") % pc.R_MOD for _ in range(200)]
    w = pc.to_words(vals)
    out = np.zeros_like(w)
    lph.lph_canonical(w.ctypes.data, len(w), out.ctypes.data)
    assert [int.from_bytes(x.tobytes(), "little") for x in out] == vals
    word = 0xA1B2C3D4
    assert [lph.lph_digit(word, p) for p in (0, 1, 2, 3, 4, 31)] == [0xD4, 0xC3, 0xB2, 0xA1, 0xD4, 0xA1]
    ka = np.full(8, 0x0F0F0F0F, dtype=np.uint32); ko = ka.copy()
    ko[5] |= 0x00100000
    assert [p for p in range(32) if lph.lph_pass_needed(ka.ctypes.data, ko.ctypes.data, p)] == [22]
    assert not any(lph.lph_pass_needed(ka.ctypes.data, ka.ctypes.data, p) for p in range(32))
    # a run that starts at row 10 behind 4 earlier runs, 20 leftovers in all: row 10 is the head; row 11 is repeated row 6 from the front -> leftover 13
    assert lph.lph_leftover_of_row(10, 10, 4, 20) == 0xFFFFFFFF and lph.lph_leftover_of_row(11, 10, 4, 20) == 13 and lph.lph_leftover_of_row(12, 10, 4, 20) == 12


def test_selftest_program_under_sanitizers(tmp_path):
    """the same source as a stand-alone program (its own main) under AddressSanitizer and UBSan, every size up to 65 539 rows"""
    exe = str(tmp_path / "lookup_permute_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DLOOKUP_PERMUTE_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout and "FAIL" not in out.stdout
