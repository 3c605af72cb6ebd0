"""Runs the per-job routine and the table generator of the device transcripts (csrc/poseidon.hpp: poseidon_tables, poseidon_permute in both schedules, poseidon_job -- the very
code k_poseidon_transcripts calls, with the jobs as a loop) on the CPU via tests/hostcheck/poseidon_selftest.cpp and checks them against oracle/poseidon.py, the restatement
that makes the reference's released proofs verify.  A check OF the device arithmetic; CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import poseidon
from tests import poseidon_common as pc
from tests.gpu_common import ints_to_words, rand_fr_full, words_to_ints

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "poseidon_selftest.cpp")
R, RINV = pc.R, pc.RINV
T, RF, RP = 5, 8, 60


@pytest.fixture(scope="module")
def pst(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pst") / "libposeidonselftest.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.pst_tables.argtypes = [C.c_void_p, C.c_void_p]; lib.pst_tables.restype = C.c_int
    lib.pst_permute.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.pst_jobs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def tables(pst):
    n = pst.pst_tables(None, None)
    tab = np.zeros((n, 4), dtype=np.uint64); layout = np.zeros(7, dtype=np.int32)
    assert pst.pst_tables(tab.ctypes.data, layout.ctypes.data) == n
    vals = [w * RINV % R for w in words_to_ints(tab)]
    return vals, dict(zip(("rc", "mds", "prc", "row0", "what", "left", "init"), (int(x) for x in layout))), n


def test_round_constants_and_matrix_equal_the_oracle(tables):
    vals, at, n = tables
    rc, mds = poseidon.parameters(T, RF, RP)
    assert len(rc) == 340 and at["mds"] - at["rc"] == 340
    assert vals[at["rc"]:at["rc"] + 340] == list(rc)
    assert vals[at["mds"]:at["mds"] + 25] == [mds[i][j] for i in range(T) for j in range(T)]
    assert vals[at["init"]] == 1 << 64 and n == at["init"] + 1
    assert at["row0"] - at["prc"] == RP * T and at["what"] - at["row0"] == RP * T and at["left"] - at["what"] == RP * (T - 1) and at["init"] - at["left"] == T * T


def test_sparse_schedule_equals_the_plain_one_and_the_oracle(pst):
    states = np.concatenate([rand_fr_full(np.random.default_rng(2102), 5 * 62), ints_to_words([0] * 5 + [R - 1] * 5)])       # 64 states: 62 random, zero, the largest words
    a, b = states.copy(), states.copy()
    pst.pst_permute(a.ctypes.data, 64, 0); pst.pst_permute(b.ctypes.data, 64, 1)
    assert (a == b).all()
    for k in (0, 17, 62, 63):                                                   # and the permutation itself is the oracle's
        st = [w * RINV % R for w in words_to_ints(states[5 * k:5 * k + 5])]
        assert [w * RINV % R for w in words_to_ints(a[5 * k:5 * k + 5])] == poseidon.permute(st, T, RF, RP)


def run_jobs(pst, jobs):
    words, woff, sq, soff = pc.pack(jobs)
    out = np.full((len(sq) + 1, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    keep = np.zeros((1, 4), dtype=np.uint64) if words.shape[0] == 0 else words
    pst.pst_jobs(keep.ctypes.data, woff.ctypes.data, sq.ctypes.data, soff.ctypes.data, len(jobs), out.ctypes.data)
    assert (out[-1] == 0xA5A5A5A5A5A5A5A5).all()                                # nothing behind the last challenge
    return out[:-1]


def test_every_length_and_pattern_equals_the_oracle_sponge(pst):
    jobs = pc.full_job_set()
    assert len(jobs) == 60 and {len(w) for w, _ in jobs} == set(range(10))
    got, want = run_jobs(pst, jobs), pc.reference(jobs)
    assert got.shape == want.shape and (got == want).all()
    used = {w for words, _ in jobs for w in words}
    assert set(pc.EDGES) <= used and len(used & set(pc.adversarial_fr_ints())) >= 40     # the edges and the adversarial words were hashed


def test_dealt_jobs_equal_the_oracle_sponge(pst):
    """the batch the GPU test deals (130 jobs, adversarial words at lanes 0 and 63), on the CPU"""
    jobs = pc.dealt_jobs(130)
    assert len(jobs[0][0]) == 9 and len(jobs[63][0]) == 6
    got, want = run_jobs(pst, jobs), pc.reference(jobs)
    assert (got == want).all()


def test_a_squeeze_needs_no_words_and_words_behind_the_last_squeeze_are_not_read(pst):
    a = run_jobs(pst, [([], [0, 0, 0])])
    assert (a == pc.reference([([], [0, 0, 0])])).all() and len({tuple(r) for r in a.tolist()}) == 3
    w = list(pc.word_pool()[5:14])
    assert (run_jobs(pst, [(w, [4])]) == run_jobs(pst, [(w[:4] + [0] * 5, [4])])).all()
    assert run_jobs(pst, [(w, [])]).shape[0] == 0


def test_selftest_program_under_sanitizers(tmp_path):
    """the same source as a stand-alone program (its own main) under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "poseidon_selftest")
    subprocess.check_call(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPOSEIDON_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout and "FAIL" not in out.stdout
