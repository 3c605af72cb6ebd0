"""TEST INFRASTRUCTURE for the device randomness (csrc/frrand.hpp): a plain-Python ChaCha20 block function (RFC 8439, 20 rounds; state words 12..13 = the 64-bit
block counter, 14..15 = the 64-bit stream identifier), a big-integer from_u512, the extreme words the reduction is tested on, and the stream table of
plonk::create_proof restated.  Imports nothing of the code under test.  tests/test_fr_random_on_host.py pins the block to two published vectors."""
import functools

import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = 1 << 256
M32 = 0xFFFFFFFF
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)            # "expand 32-byte k"

# the streams plonk::create_proof draws from with ProofOptions::device_randomness (include/mi355zk_plonk.hpp)
STREAM_RANDOM_POLY, STREAM_ADVICE_BLIND, STREAM_M_BLIND, STREAM_Z_BLIND, STREAM_PHI_BLIND = 0, 1, 2, 3, 4
STREAM_TABLE = {"RNG_STREAM_RANDOM_POLY": 0, "RNG_STREAM_ADVICE_BLIND": 1, "RNG_STREAM_M_BLIND": 2, "RNG_STREAM_Z_BLIND": 3, "RNG_STREAM_PHI_BLIND": 4}


def _rotl(x, s):
    return ((x << s) | (x >> (32 - s))) & M32


def _qr(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def key_words(key: bytes):
    assert len(key) == 32
    return [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]


def block_words(key: bytes, stream: int, counter: int):
    """the sixteen output words of one block"""
    assert 0 <= stream < 1 << 64 and 0 <= counter < 1 << 64
    init = list(CONSTANTS) + key_words(key) + [counter & M32, counter >> 32, stream & M32, stream >> 32]
    x = list(init)
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, init)]


def block(key: bytes, stream: int, counter: int) -> bytes:
    """the 64 bytes of one block (the words serialised little-endian, as RFC 8439 does)"""
    return b"".join(w.to_bytes(4, "little") for w in block_words(key, stream, counter))


def blocks_np(key: bytes, stream: int, counter0: int, count: int):
    """[count,16] u32: the blocks counter0 .. counter0 + count - 1, the same rounds on numpy columns (checked against block_words by the host test)"""
    assert counter0 + count <= 1 << 64
    ctr = np.array([counter0 + i for i in range(count)], dtype=np.uint64)
    init = [np.full(count, c, dtype=np.uint32) for c in list(CONSTANTS) + key_words(key)]
    init += [(ctr & np.uint64(M32)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32), np.full(count, stream & M32, dtype=np.uint32), np.full(count, stream >> 32, dtype=np.uint32)]
    x = [a.copy() for a in init]

    def rotl(v, s):
        return (v << np.uint32(s)) | (v >> np.uint32(32 - s))

    def qr(a, b, c, d):
        x[a] = x[a] + x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = x[c] + x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = x[a] + x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = x[c] + x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return np.stack([a + b for a, b in zip(x, init)], axis=1)


def from_u512_int(v: int) -> int:
    """a 512-bit integer -> the Montgomery WORD of its residue: (v mod r) * 2^256 mod r"""
    assert 0 <= v < 1 << 512
    return (v % R) * MONT % R


def word_to_u64x4(w: int):
    return [(w >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def from_u512_bytes(rows) -> np.ndarray:
    """[n,64] u8 (or anything viewable as such) -> [n,4] u64 Montgomery words"""
    rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1, 64)
    return np.array([word_to_u64x4(from_u512_int(int.from_bytes(r.tobytes(), "little"))) for r in rows], dtype=np.uint64).reshape(-1, 4)


def element(key: bytes, stream: int, counter: int) -> int:
    """the Montgomery word element (key, stream, counter) of a draw"""
    return from_u512_int(int.from_bytes(block(key, stream, counter), "little"))


def elements(key: bytes, stream: int, counter0: int, count: int) -> np.ndarray:
    """[count,4] u64: the words mi355_fr_random_dev writes"""
    if count == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    return from_u512_bytes(blocks_np(key, stream, counter0, count))


def elements_canonical(key: bytes, stream: int, counter0: int, count: int):
    """the same draw as canonical integers (what oracle/plonk.py computes with)"""
    b = blocks_np(key, stream, counter0, count).view(np.uint8).reshape(count, 64) if count else []
    return [int.from_bytes(r.tobytes(), "little") % R for r in b]


# ---- the words the reduction is tested on
EXTREME_HALVES = (0, 1, R - 1, R, R + 1, 2 * R, 5 * R, (1 << 256) - 1)


@functools.lru_cache(maxsize=None)
def extreme_u512():
    """512-bit integers d0 + 2^256 d1: every pair of EXTREME_HALVES, every single-bit word, the adversarial coordinate and scalar words of tests/gpu_common.py in
    either half against the extreme halves of the other, and 3000 random words.  Fixed order."""
    from tests import gpu_common as gc
    v = [d0 | (d1 << 256) for d0 in EXTREME_HALVES for d1 in EXTREME_HALVES]
    v += [1 << i for i in range(512)]
    adv = list(dict.fromkeys(gc.adversarial_fq_ints() + gc.adversarial_fr_ints()))
    for i, w in enumerate(adv):
        other = EXTREME_HALVES[i % len(EXTREME_HALVES)]
        v += [w | (other << 256), other | (w << 256), w | (adv[(7 * i + 3) % len(adv)] << 256), w | (((1 << 256) - 1) << 256), ((1 << 256) - 1) | (w << 256)]
    rng = np.random.default_rng(2008)
    v += [int.from_bytes(rng.bytes(64), "little") for _ in range(3000)]
    return v


def u512_rows(vals) -> np.ndarray:
    """512-bit integers -> [n,64] u8"""
    vals = list(vals)
    return np.frombuffer(b"".join(x.to_bytes(64, "little") for x in vals), dtype=np.uint8).reshape(len(vals), 64).copy()
