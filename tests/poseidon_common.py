"""helpers shared by the tests of the device transcripts (TEST INFRASTRUCTURE): the job set of csrc/poseidon.hpp's contract -- every length from 0 to 9 under six squeeze
patterns, words from the edges of the field and the adversarial limb patterns of tests/gpu_common.py -- its packing into the four arrays of
mi355_poseidon_transcripts_host, and the reference: oracle.poseidon.Sponge driven by the host restatement of a job

    sp = Sponge(); prev = 0
    for p in S: sp.update(W[prev:p]); prev = p; out.append(sp.squeeze())

Words travel as Montgomery WORDS (the ABI form); the sponge of the oracle works on values, so a word w stands for w / 2^256 mod r and a challenge c comes back as c 2^256 mod r."""
import functools

import numpy as np

from oracle import poseidon, pyref
from tests.gpu_common import adversarial_fr_ints, ints_to_words, rand_fr_full, words_to_ints

R = pyref.R_MOD
MONT = pyref.MONT_R % R
RINV = pow(1 << 256, -1, R)
PATTERNS = ("end", "zero_then_end", "twice_at_one_position", "at_3_4_5", "mid_chunk_then_end", "words_behind_the_last_squeeze")
LENGTHS = tuple(range(10))
EDGES = [0, 1, R - 1, MONT, 1 << 253]                     # words: zero, the word 1, the largest word, the word of the value one, 2^253


def squeezes(length: int, pattern: str):
    c = lambda p: min(p, length)
    return {"end": [length], "zero_then_end": [0, length], "twice_at_one_position": [c(2), c(2), length], "at_3_4_5": [c(3), c(4), c(5)],
            "mid_chunk_then_end": [2 * length // 3, length], "words_behind_the_last_squeeze": [length // 2]}[pattern]


@functools.lru_cache(maxsize=None)
def word_pool():
    """edges, the adversarial words, 64 words uniform over [0, r): fixed order"""
    rnd = words_to_ints(rand_fr_full(np.random.default_rng(2101), 64))
    return tuple(dict.fromkeys(EDGES + adversarial_fr_ints())) + tuple(rnd)


def dealt_jobs(n: int, adversarial_lanes=(0, 63)):
    """n jobs, lengths and patterns dealt round-robin so that neighbouring lanes hold different scripts: job i has length (9 - i) mod 10 and pattern (i + i // 10) mod 6.
    Lanes in `adversarial_lanes` take their words from the edges and the adversarial pool alone, the others walk the whole pool."""
    pool = word_pool(); adv = tuple(dict.fromkeys(EDGES + adversarial_fr_ints()))
    jobs = []; at = 0
    for i in range(n):
        length = (9 - i) % 10
        src = adv if i in adversarial_lanes else pool
        words = [src[(at + 5 * i + k) % len(src)] for k in range(length)]
        at += length
        jobs.append((words, squeezes(length, PATTERNS[(i + i // 10) % 6])))
    return jobs


def full_job_set():
    """every length x every pattern (60 jobs), words walking the pool"""
    pool = word_pool(); jobs = []; at = 0
    for length in LENGTHS:
        for pat in PATTERNS:
            jobs.append(([pool[(at + k) % len(pool)] for k in range(length)], squeezes(length, pat)))
            at += length
    return jobs


def pack(jobs):
    """-> words [n, 4] u64, word_offsets [jobs + 1] u64, squeeze_at [m] u32, squeeze_offsets [jobs + 1] u64"""
    flat = [w for words, _ in jobs for w in words]
    words = ints_to_words(flat) if flat else np.zeros((0, 4), dtype=np.uint64)
    woff = np.cumsum([0] + [len(w) for w, _ in jobs]).astype(np.uint64)
    soff = np.cumsum([0] + [len(s) for _, s in jobs]).astype(np.uint64)
    sq = np.array([p for _, s in jobs for p in s], dtype=np.uint32)
    return np.ascontiguousarray(words), woff, sq, soff


def reference_job(words, sq):
    """the challenges of one job as Montgomery words (Python integers)"""
    sp = poseidon.Sponge(); prev = 0; out = []
    for p in sq:
        sp.update([w * RINV % R for w in words[prev:p]]); prev = p
        out.append(sp.squeeze() * (1 << 256) % R)
    return out


_CACHE = {}


def reference(jobs):
    """[m, 4] u64: the challenges of every job in order; each distinct job is hashed once per process"""
    out = []
    for words, sq in jobs:
        key = (tuple(words[:max(sq, default=0)]), tuple(sq))
        if key not in _CACHE:
            _CACHE[key] = reference_job(list(words), list(sq))
        out += _CACHE[key]
    return ints_to_words(out) if out else np.zeros((0, 4), dtype=np.uint64)
