"""Runs the __host__ __device__ codec that k_g1_decompress / k_g1_compress execute per lane (csrc/g1codec.hpp: the square root in the 9 x 29-bit field, the
range and sign rules) on the CPU via tests/hostcheck/g1codec_selftest.cpp and checks it against cref AND pyref: the KAT A4 words, random points of both
parities, the identity, every rejected class.  Also the host-side G2 codec the Processed params loader uses for g2 / s_g2, down to a pairing check on the decoded
points.  A check OF the device arithmetic; CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import cref, pairing, pyref

HERE = os.path.dirname(os.path.abspath(__file__))
P, R = pyref.P_MOD, pyref.R_MOD


@pytest.fixture(scope="module")
def codec(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("g1c") / "libg1codecselftest.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, os.path.join(HERE, "hostcheck", "g1codec_selftest.cpp")])
    return C.CDLL(so)


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def decompress(codec, words):
    """list of 32-byte words -> ([n, 8] points, [n] accepted flags) by the compiled device routine"""
    n = len(words)
    w = np.frombuffer(b"".join(words), dtype=np.uint8).copy()
    pts = np.zeros((n, 8), dtype=np.uint64); ok = np.zeros(n, dtype=np.uint8)
    codec.g1c_decompress(p_(w), p_(pts), p_(ok), C.c_uint64(n))
    return pts, ok


def compress(codec, pts):
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    out = np.zeros(32 * pts.shape[0], dtype=np.uint8)
    codec.g1c_compress(p_(pts), p_(out), C.c_uint64(pts.shape[0]))
    return [out[32 * i:32 * i + 32].tobytes() for i in range(pts.shape[0])]


def oracle_decompress(word):
    """(cref answer or None, pyref accepts?) -- the two oracles must agree before either is used as the yardstick"""
    c = cref.g1_decompress(word)
    try:
        py = pyref.g1_decompress(word)
        py_ok = True
    except AssertionError:
        py, py_ok = None, False
    assert (c is not None) == py_ok, word.hex()
    if py_ok:
        xl, yl = pyref.g1_affine_to_limbs(py)
        assert (c == np.array(xl + yl, dtype=np.uint64)).all()
    return c


def check_words(codec, words):
    pts, ok = decompress(codec, words)
    classes = set()
    for i, w in enumerate(words):
        want = oracle_decompress(w)
        assert bool(ok[i]) == (want is not None), (i, w.hex())
        classes.add(bool(ok[i]))
        if want is None:
            assert not pts[i].any(), "a rejected slot holds the identity"
        else:
            assert (pts[i] == want).all(), (i, w.hex())
    return pts, ok, classes


def word_of(x: int, sign: int = 0, bit7: int = 0) -> bytes:
    return (x | (sign << 254) | (bit7 << 255)).to_bytes(32, "little")


@pytest.mark.parametrize("vk,npts", [("vk_chunk", 7), ("vk_batch_agg", 9)])
def test_kat_a4_words(codec, kat, vk, npts):
    raw = bytes.fromhex(kat[vk])
    words = [raw[8 + 32 * i: 40 + 32 * i] for i in range(npts)]
    pts, ok, _ = check_words(codec, words)
    assert ok.all()
    assert compress(codec, pts) == words


def test_random_points_of_both_parities(codec):
    rng = np.random.default_rng(2601)
    n = 3000
    sc = np.stack([cref.fr_mont(int(rng.integers(1, 2**62)) * int(rng.integers(1, 2**62)) % R) for _ in range(n)])
    pts = cref.g1_mul_generator_vec(sc)
    words = [cref.g1_compress(p) for p in pts]
    signs = [w[31] >> 6 & 1 for w in words]
    assert 0 in signs and 1 in signs
    for i in range(0, n, 97):   # the second oracle on a sample (python integers are slow)
        assert pyref.g1_compress(pyref.g1_affine_from_limbs(pts[i][:4], pts[i][4:])) == words[i]
    assert compress(codec, pts) == words
    got, ok = decompress(codec, words)
    assert ok.all() and (got == pts).all()
    # the other root: flipping the sign bit negates y and nothing else
    flipped = [w[:31] + bytes([w[31] ^ 0x40]) for w in words[:200]]
    neg, ok = decompress(codec, flipped)
    assert ok.all() and (neg[:, :4] == pts[:200, :4]).all()
    for i in range(200):
        assert (neg[i] == cref.g1_decompress(flipped[i])).all()
        assert (cref.f_add(cref.FQ, neg[i][4:], pts[i][4:]) == 0).all()


def test_identity_and_the_rejected_classes(codec):
    pts, ok, _ = check_words(codec, [bytes(32)])
    assert ok[0] == 1 and not pts.any()
    assert compress(codec, np.zeros((1, 8), dtype=np.uint64)) == [bytes(32)]
    _, ok, _ = check_words(codec, [word_of(0, 1)])                       # the identity with the sign bit set
    assert ok[0] == 0
    edge = [word_of(x, s) for x in (P - 1, P, P + 1, (1 << 254) - 1) for s in (0, 1)]
    _, ok, _ = check_words(codec, edge)
    assert not ok[2:].any(), "x >= q is rejected whatever the sign bit says"


def test_bit_7_of_byte_31_is_ignored_as_the_host_helper_does(codec):
    rng = np.random.default_rng(2602)
    sc = np.stack([cref.fr_mont(int(rng.integers(1, 2**62))) for _ in range(8)])
    pts = cref.g1_mul_generator_vec(sc)
    words = [cref.g1_compress(p) for p in pts]
    marked = [w[:31] + bytes([w[31] | 0x80]) for w in words] + [word_of(0, 0, 1), word_of(0, 1, 1), word_of(P, 0, 1)]
    got, ok, _ = check_words(codec, marked)
    assert ok[:8].all() and (got[:8] == pts).all() and list(ok[8:]) == [1, 0, 0]


def test_small_x_residues_and_non_residues(codec):
    words = [word_of(x, s) for x in range(1, 41) for s in (0, 1)]
    _, ok, classes = check_words(codec, words)
    assert classes == {True, False}, "x = 1..40 holds residues and non-residues"
    assert 20 < int(ok.sum()) < 60


# ---- the G2 tail of a Processed params file (host code inside the library)
def g2_limbs(Q):
    return np.array(pyref.g2_to_limbs(Q), dtype=np.uint64)


def g2_word_expected(Q) -> bytes:
    """x.c0 | x.c1 canonical little-endian, bit 6 of byte 63 = parity of canonical y.c0; identity = 64 zero bytes"""
    if Q is None:
        return bytes(64)
    b = bytearray(Q[0][0].to_bytes(32, "little") + Q[0][1].to_bytes(32, "little"))
    b[63] |= (Q[1][0] & 1) << 6
    return bytes(b)


def g2_decode(codec, word):
    w = np.frombuffer(word, dtype=np.uint8).copy(); out = np.zeros(16, dtype=np.uint64)
    ok = codec.g2c_decompress(p_(w), p_(out))
    return (out if ok else None)


def g2_encode(codec, limbs):
    out = np.zeros(64, dtype=np.uint8); codec.g2c_compress(p_(np.ascontiguousarray(limbs)), p_(out)); return out.tobytes()


def test_g2_codec_round_trips_generator_multiples(codec):
    for tau in (1, 2, 0x1234567, R - 1, 0x5343524F4C4C0001):
        Q = pyref.g2_mul(pyref.G2_GEN, tau)
        word = g2_encode(codec, g2_limbs(Q))
        assert word == g2_word_expected(Q)
        got = g2_decode(codec, word)
        assert got is not None and (got == g2_limbs(Q)).all() and cref.g2_is_on_curve(got)
    assert g2_encode(codec, np.zeros(16, dtype=np.uint64)) == bytes(64)
    assert not g2_decode(codec, bytes(64)).any()
    assert g2_decode(codec, bytes(63) + b"\x40") is None                 # the identity with the sign bit set


def test_g2_codec_rejects_x_off_the_twist_and_out_of_range(codec):
    rejected = 0
    for c0 in range(1, 12):   # x = c0 + 0 u: about half have x^3 + b' a non-square of Fq2
        word = c0.to_bytes(32, "little") + bytes(32)
        x = (c0, 0)
        rhs = pyref.f2_add(pyref.f2_mul(pyref.f2_mul(x, x), x), pyref.G2_B)
        norm = (rhs[0] * rhs[0] + rhs[1] * rhs[1]) % P
        is_square = pow(norm, (P - 1) // 2, P) == 1                      # a in Fq2 is a square iff its norm is a square in Fq
        got = g2_decode(codec, word)
        assert (got is not None) == is_square, c0
        if got is None:
            rejected += 1
        else:
            assert cref.g2_is_on_curve(got)
    assert 0 < rejected < 11
    assert g2_decode(codec, P.to_bytes(32, "little") + bytes(32)) is None
    assert g2_decode(codec, (1).to_bytes(32, "little") + P.to_bytes(32, "little")) is None


def test_g2_decoded_points_satisfy_the_srs_pairing_equation(codec):
    tau = 0x5343524F4C4C0001
    g0, g1 = pyref.G1_GEN, pyref.g1_mul(pyref.G1_GEN, tau)
    g2w = g2_encode(codec, g2_limbs(pyref.G2_GEN)); sg2w = g2_encode(codec, g2_limbs(pyref.g2_mul(pyref.G2_GEN, tau)))

    def to_py(limbs):
        rinv = pow(pyref.MONT_R, -1, P)
        return tuple(tuple(pyref.from_limbs(limbs[8 * a + 4 * b:8 * a + 4 * b + 4]) * rinv % P for b in range(2)) for a in range(2))

    g2d, sg2d = to_py(g2_decode(codec, g2w)), to_py(g2_decode(codec, sg2w))
    assert pairing.pairing_product_is_one([(g1, g2d), (pyref.g1_neg(g0), sg2d)])       # e(g[1], g2) == e(g[0], s_g2)
    flipped = sg2w[:63] + bytes([sg2w[63] ^ 0x40])
    assert not pairing.pairing_product_is_one([(g1, g2d), (pyref.g1_neg(g0), to_py(g2_decode(codec, flipped)))])


# ---- points and words from the adversarial pool (tests/gpu_common.py): x on the edges of the field and of the limb grids from_sat_plain slices
def test_adversarial_points_round_trip(codec):
    """the "canonical" pool (the canonical x, the word the codec slices, is the adversarial word) and the "mont" pool (the ABI word compress reads is)"""
    from tests import gpu_common as gc
    for reading in ("canonical", "mont"):
        pts, _, _ = gc.adversarial_g1_points(reading)
        py, _, _ = gc.adversarial_g1_info(reading)
        words = [cref.g1_compress(p) for p in pts]
        assert words == [pyref.g1_compress(q) for q in py]
        assert {w[31] >> 6 & 1 for w in words} == {0, 1}
        assert compress(codec, pts) == words
        got, ok = decompress(codec, words)
        assert ok.all() and (got == pts).all(), np.nonzero((got != pts).any(axis=1))[0][:8]
        got, ok, _ = check_words(codec, words)
        assert ok.all()


def test_adversarial_words_that_are_no_x_coordinate(codec):
    """the pool words that did not lift at distance 0 (0 among them), and every pool word's neighbours, as compressed x with either sign bit: accepted
    exactly when pyref finds a root; the first flag that is down is the first word pyref rejects"""
    from tests import gpu_common as gc
    non = gc.adversarial_fq_non_lifting("canonical")
    assert 0 in non and len(non) >= 10
    words = [word_of(x, s) for x in non for s in (0, 1)]
    _, ok, _ = check_words(codec, words)
    assert list(ok) == [1] + [0] * (len(words) - 1), "only x = 0 with the sign bit clear (the identity) is accepted"
    near = [word_of(w + d, s) for w in gc.adversarial_fq_ints() for d in range(-2, 3) if 0 <= w + d < P for s in (0, 1)]
    _, ok, classes = check_words(codec, near)
    assert classes == {True, False}
    rejected = [i for i, w in enumerate(near) if cref.g1_decompress(w) is None]
    assert int(np.argmin(ok)) == rejected[0]


def test_g2_codec_on_adversarial_twist_points(codec):
    from tests import gpu_common as gc
    for reading in ("canonical", "mont"):
        pts, py, _ = gc.adversarial_g2_points(reading)
        for limbs, Q in zip(pts, py):
            word = g2_encode(codec, limbs)
            assert word == g2_word_expected(Q)
            got = g2_decode(codec, word)
            assert got is not None and (got == limbs).all(), Q
    # x = (w, 0) and (0, w) for the pool words themselves: decoded exactly when x^3 + b' is a square of Fq2 (its norm a square of Fq)
    seen = set()
    for w in gc.adversarial_fq_ints():
        for x in ((w, 0), (0, w)):
            if x == (0, 0):
                continue
            rhs = pyref.f2_add(pyref.f2_mul(pyref.f2_mul(x, x), x), pyref.G2_B)
            is_square = pow((rhs[0] * rhs[0] + rhs[1] * rhs[1]) % P, (P - 1) // 2, P) == 1
            got = g2_decode(codec, x[0].to_bytes(32, "little") + x[1].to_bytes(32, "little"))
            assert (got is not None) == is_square, x
            seen.add(is_square)
            if got is not None:
                assert cref.g2_is_on_curve(got) and (got[:8] == np.array(pyref.mont_limbs(x[0], P) + pyref.mont_limbs(x[1], P), dtype=np.uint64)).all()
    assert seen == {True, False}
