"""mi355_fr_program_host (csrc/frprog.hpp, k_fr_program: one lane per job) against tests/frprog_common.py, the Python restatement tests/test_fr_program_on_host.py holds to the
host build of the same interpreter: every output word and every flag word, at 1, 63, 64, 65 and 257 jobs (one lane, a wave short of one lane, a full wave, a wave and one lane,
four waves and one), for programs of 1, 2 and about 2 000 instructions, on the adversarial operands, with a zero under INV in one job of 65, with one register named twice among
the outputs, and twice in a row (the second call takes the pooled block the first gave back)."""
import numpy as np
import pytest

import __graft_entry__ as ge

import frprog_common as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def device(zk, code, n_regs, consts, inputs, out_regs):
    iw = fc.words([v for job in inputs for v in job]).reshape(len(inputs), len(inputs[0]), 4)
    out, flags = zk.halo2.fr_program(np.array(code, dtype=np.uint32), n_regs, fc.words(consts), iw, out_regs)
    got = fc.ints(out)
    return [got[j * len(out_regs):(j + 1) * len(out_regs)] for j in range(len(inputs))], [int(f) for f in flags]


def dealt_inputs(rng, jobs, n_inputs):
    """random residues, the adversarial operands at lanes 0 and 63 and scattered elsewhere"""
    return [[fc.EDGES[(j + t) % 5] if j in (0, 63) or (j + t) % 7 == 0 else int(rng.integers(0, 1 << 62)) ** 5 % fc.R for t in range(n_inputs)] for j in range(jobs)]


@pytest.mark.parametrize("n_instr,jobs", [(1, 1), (2, 63), (2000, 64), (2, 65), (300, 257)])
def test_random_programs_equal_the_restatement(zk, n_instr, jobs):
    rng = np.random.default_rng(100 * n_instr + jobs)
    consts = [0, 1, int(rng.integers(2, 1 << 62))]
    code, n_regs, out_regs = fc.random_program(rng, len(consts), 4, 12, n_instr)
    assert out_regs[-1] == out_regs[-2]                                                              # one register named twice
    inputs = dealt_inputs(rng, jobs, 4)
    assert device(zk, code, n_regs, consts, inputs, out_regs) == fc.interpret(code, n_regs, consts, inputs, out_regs)


def test_every_op_on_every_pair_of_the_adversarial_operands(zk):
    pairs = [[a, b] for a in fc.EDGES for b in fc.EDGES]
    for op in (fc.ADD, fc.SUB, fc.MUL):
        code = [(fc.ADD, 3, 1, 0), (fc.ADD, 4, 2, 0), (op, 5, 3, 4), (op, 3, 3, 4), (op, 4, 4, 4)]      # apart, aliasing a, aliasing both
        assert device(zk, code, 6, [0], pairs, [5, 3, 4]) == fc.interpret(code, 6, [0], pairs, [5, 3, 4]), op
    code = [(fc.SQRN, 2, 1, 0), (fc.SQRN, 3, 1, 1), (fc.SQRN, 4, 1, 64), (fc.INV, 5, 1, 0), (fc.NZ, 0, 1, 31)]
    one = [[e] for e in fc.EDGES]
    assert device(zk, code, 6, [0], one, [2, 3, 4, 5, 1, 0]) == fc.interpret(code, 6, [0], one, [2, 3, 4, 5, 1, 0])     # an input and a constant among the outputs


def test_a_zero_under_inv_in_one_job_of_65_and_two_calls_in_a_row(zk):
    code = [(fc.ADD, 2, 1, 0), (fc.INV, 2, 2, 0), (fc.MUL, 3, 2, 1)]
    inputs = [[0 if j == 40 else j + 2] for j in range(65)]
    want = fc.interpret(code, 4, [0], inputs, [2, 3, 3])
    assert want[1] == [1 if j == 40 else 0 for j in range(65)] and want[0][40] == [0, 0, 0] and want[0][0][1:] == [1, 1]
    first = device(zk, code, 4, [0], inputs, [2, 3, 3])
    second = device(zk, code, 4, [0], inputs[::-1], [2, 3, 3])                                          # the block of the first call, other inputs
    assert first == want
    assert second == (want[0][::-1], want[1][::-1])


def test_no_jobs_launches_nothing_and_bad_arguments_are_refused(zk):
    out, flags = zk.halo2.fr_program(np.zeros((0, 4), dtype=np.uint32), 1, fc.words([]), np.zeros((0, 1, 4), dtype=np.uint64), [])
    assert out.shape == (0, 0, 4) and flags.shape == (0,)
    with pytest.raises(zk.Mi355Error) as e:
        zk.halo2.fr_program(np.array([[9, 1, 0, 0]], dtype=np.uint32), 2, fc.words([]), fc.words([1]).reshape(1, 1, 4), [1])
    assert "unknown op 9" in str(e.value)
