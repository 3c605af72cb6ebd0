"""Runs the per-element routines of the device randomness (csrc/frrand.hpp: frrand_block, frrand_from_u512, frrand_element -- the very code the kernels call) on the
CPU via tests/hostcheck/frrand_selftest.cpp and checks them against tests/frrand_common.py (a plain-Python ChaCha20 block pinned to two published vectors, and big
integers).  A check OF the device arithmetic; CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import frrand_common as fc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "frrand_selftest.cpp")
R = fc.R
ZERO_KEY, SEQ_KEY, FF_KEY = bytes(32), bytes(range(32)), b"\xff" * 32


@pytest.fixture(scope="module")
def fst(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fst") / "libfrrandselftest.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.fst_block.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.fst_from_u512.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    lib.fst_elements.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.fst_r3.argtypes = [C.c_void_p]
    return lib


def cpp_block(fst, key, stream, counter):
    out = C.create_string_buffer(64)
    fst.fst_block(key, stream, counter, out)
    return out.raw


def test_python_block_matches_the_published_vectors():
    b = fc.block(ZERO_KEY, 0, 0)
    assert b[:16].hex() == "76b8e0ada0f13d90405d6ae55386bd28" and b[-8:].hex() == "c387b669b2ee6586"
    # RFC 8439 section 2.3.2: state words 12..15 = 1, 0x09000000, 0x4a000000, 0
    b = fc.block(SEQ_KEY, 0x4A000000, 1 | (0x09000000 << 32))
    assert b[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4" and b[-8:].hex() == "cbd083e8a2503c4e"


def test_montgomery_word_of_the_first_vector_rederived():
    v = int.from_bytes(fc.block(ZERO_KEY, 0, 0), "little")
    d0, d1 = v & ((1 << 256) - 1), v >> 256
    r2, r3 = pow(2, 512, R), pow(2, 768, R)
    halo2 = (d0 * r2 * pow(2, -256, R) + d1 * r3 * pow(2, -256, R)) % R       # two Montgomery products, summed
    assert halo2 == fc.from_u512_int(v) == fc.element(ZERO_KEY, 0, 0) == 0x2666D9070740F8385ADF55925A6EB55A81D835D88C87211EB157BE4A80F2ED3A


def test_r3_rederived(fst):
    out = np.zeros(4, dtype=np.uint64)
    fst.fst_r3(out.ctypes.data)
    assert sum(int(x) << (64 * i) for i, x in enumerate(out)) == pow(1 << 256, 3, R)


CASES = [(ZERO_KEY, 0, 0), (SEQ_KEY, 0x4A000000, 1 | (0x09000000 << 32)), (FF_KEY, 0, 0), (FF_KEY, (1 << 64) - 1, (1 << 64) - 1), (SEQ_KEY, 0xDEADBEEF00000001, 5),
         (SEQ_KEY, 1 << 63, 1 << 40)]
CASES += [(SEQ_KEY, 3, c) for c in range((1 << 32) - 3, (1 << 32) + 5)] + [(FF_KEY, 1 << 32, c) for c in range((1 << 64) - 9, (1 << 64) - 1)]


def test_blocks_match_python(fst):
    rng = np.random.default_rng(2001)
    cases = CASES + [(rng.bytes(32), int(rng.integers(0, 2**63)) * 2 + 1, int(rng.integers(0, 2**63)) * 2 + int(rng.integers(0, 2))) for _ in range(40)]
    for key, stream, counter in cases:
        assert cpp_block(fst, key, stream, counter) == fc.block(key, stream, counter), (key.hex(), stream, counter)
    assert cpp_block(fst, SEQ_KEY, 3, 1 << 32) != cpp_block(fst, SEQ_KEY, 3, 0)           # the carry into word 13 is not dropped
    assert cpp_block(fst, SEQ_KEY, 3, 0) != cpp_block(fst, SEQ_KEY, 3 | (1 << 32), 0)     # nor the high word of the stream


def test_numpy_blocks_match_the_plain_ones():
    for key, stream, c0 in ((SEQ_KEY, 0, 0), (FF_KEY, (1 << 63) | 5, (1 << 32) - 3), (SEQ_KEY, 9, (1 << 64) - 9)):
        got = fc.blocks_np(key, stream, c0, 8)
        for i in range(8):
            assert got[i].tobytes() == fc.block(key, stream, c0 + i)


@pytest.mark.parametrize("which", [0, 1], ids=["product_scanning", "cios"])
def test_from_u512_on_the_extreme_words(fst, which):
    vals = fc.extreme_u512()
    src = fc.u512_rows(vals)
    out = np.full((len(vals), 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    fst.fst_from_u512(src.ctypes.data, len(vals), out.ctypes.data, which)
    got = [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in out]
    bad = [hex(v) for v, g in zip(vals, got) if g >= R or g != fc.from_u512_int(v)]
    assert not bad, bad[:5]
    pairs = {(d0, d1) for d0 in fc.EXTREME_HALVES for d1 in fc.EXTREME_HALVES}
    assert all((v & ((1 << 256) - 1), v >> 256) in pairs for v in vals[:64]) and len(vals) > 64 + 512 + 3000


def test_elements_of_a_draw(fst):
    for key, stream, c0 in ((ZERO_KEY, 0, 0), (SEQ_KEY, 4, (1 << 32) - 3), (FF_KEY, 1 << 40, (1 << 64) - 9)):
        n = 8
        out = np.zeros((n, 4), dtype=np.uint64)
        fst.fst_elements(key, stream, c0, n, out.ctypes.data)
        assert (out == fc.elements(key, stream, c0, n)).all()
        assert [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in out] == [fc.element(key, stream, c0 + i) for i in range(n)]


def test_selftest_program_under_sanitizers(tmp_path):
    """the same source as a stand-alone program (its own main) under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "frrand_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DFRRAND_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout and "FAIL" not in out.stdout
