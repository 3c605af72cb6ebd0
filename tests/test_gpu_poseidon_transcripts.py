"""mi355_poseidon_transcripts_host on the device (k_poseidon_transcripts: one lane per job, a lane walks its own script) against oracle.poseidon.Sponge driven by the host
restatement of a job (tests/poseidon_common.py).  Batches of 1, 63, 64, 65 and 130 jobs with lengths 0..9 and six squeeze patterns dealt round-robin, so that the lanes of one
wave hold different scripts and the adversarial words sit at lanes 0 and 63; one long job in the middle of a wave of silent ones (divergent trip counts); the same batch in
reverse order; two calls in a row."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import poseidon_common as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def run(zk, jobs):
    words, woff, sq, soff = pc.pack(jobs)
    return zk.halo2.poseidon_transcripts(words, woff, sq, soff)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_dealt_batches_equal_the_oracle_sponge(zk, n):
    jobs = pc.dealt_jobs(n)                                                     # a prefix of the 130-job batch: the reference of each job is computed once
    adv = set(pc.adversarial_fr_ints()) | set(pc.EDGES)
    assert set(jobs[0][0]) <= adv and len(jobs[0][0]) == 9 and (n < 64 or (set(jobs[63][0]) <= adv and len(jobs[63][0]) == 6))
    got, want = run(zk, jobs), pc.reference(jobs)
    assert got.shape == want.shape and (got == want).all(), np.argwhere((got != want).any(axis=1)).ravel()[:8]


def long_job_among_silent_ones():
    """lane 31: 400 words, a squeeze every 50.  The other 63 lanes: no words and one squeeze at 0 (even lanes), or words and NO squeeze (odd lanes: they own no output slot)"""
    pool = pc.word_pool()
    jobs = []
    for i in range(64):
        if i == 31:
            jobs.append(([pool[(7 * k) % len(pool)] for k in range(400)], list(range(50, 401, 50))))
        elif i % 2 == 0:
            jobs.append(([], [0]))
        else:
            jobs.append(([pool[(i + k) % len(pool)] for k in range(i % 7)], []))
    return jobs


def test_one_long_job_in_a_wave_of_silent_ones(zk):
    jobs = long_job_among_silent_ones()
    got, want = run(zk, jobs), pc.reference(jobs)
    assert got.shape == (32 + 8, 4) and (got == want).all()
    assert (got[:16] == got[0]).all() and (got[16:24] != got[0]).any(axis=1).all()      # sixteen empty sponges, then the long job's eight challenges in its own slots


def test_reversed_order_gives_the_same_challenge_per_job(zk):
    jobs = pc.dealt_jobs(130)
    fwd, rev = run(zk, jobs), run(zk, jobs[::-1])
    _, _, _, soff = pc.pack(jobs)
    _, _, _, roff = pc.pack(jobs[::-1])
    for j in range(130):
        a = fwd[int(soff[j]):int(soff[j + 1])]; k = 129 - j; b = rev[int(roff[k]):int(roff[k + 1])]
        assert (a == b).all(), j


def test_two_calls_in_a_row_give_identical_bytes(zk):
    jobs = pc.dealt_jobs(130)
    assert run(zk, jobs).tobytes() == run(zk, jobs).tobytes()


def test_nothing_to_squeeze_launches_nothing_and_the_kernel_reports_its_time(zk):
    capi, ptr, lib = zk._capi, zk._capi.ptr, zk._capi.lib()
    assert lib.mi355_poseidon_transcripts_host(None, None, None, None, 0, None) == capi.OK
    words, woff, sq, soff = pc.pack([([1, 2, 3], []), ([], [])])                # two silent jobs
    out = np.full((1, 4), 7, dtype=np.uint64)
    zk._capi.check(lib.mi355_profile_enable(1)); zk._capi.check(lib.mi355_profile_reset())
    try:
        assert lib.mi355_poseidon_transcripts_host(ptr(words), ptr(woff), ptr(sq), ptr(soff), 2, ptr(out)) == capi.OK and (out == 7).all()
        ms, launches = C.c_double(0), C.c_uint64(0)
        lib.mi355_profile_get(b"poseidon_transcripts", C.byref(ms), C.byref(launches))
        assert launches.value == 0
        run(zk, pc.dealt_jobs(65))
        assert lib.mi355_profile_get(b"poseidon_transcripts", C.byref(ms), C.byref(launches)) == capi.OK and launches.value == 1 and ms.value > 0
    finally:
        zk._capi.check(lib.mi355_profile_enable(0))
