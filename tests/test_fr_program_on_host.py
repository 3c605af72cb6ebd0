"""Runs the interpreter behind mi355_fr_program_host (csrc/frprog.hpp: frprog_job -- the very code k_fr_program calls for one lane -- in the kernel's register layout, and
frprog_check, the entry point's argument checks) on the CPU.  tests/hostcheck/frprog_main.cpp holds it to a plain big-integer interpreter of its own, under AddressSanitizer and
UBSan; the same source as a shared object runs the programs the GPU test deals, against tests/frprog_common.py -- the Python restatement the device is held to.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import frprog_common as fc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "frprog_main.cpp")


def test_interpreter_program_under_sanitizers(tmp_path):
    """random programs, every op on the adversarial operands, aliased destinations, SQRN by 0 / 1 / 64, INV of zero among other jobs, every rejection of the checks"""
    exe = str(tmp_path / "frprog_main")
    subprocess.check_call(["g++", "-O1", "-g1", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout and "FAIL" not in out.stdout


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("frprog") / "libfrprog.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.frp_host_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.frp_host_run.restype = C.c_int

    def run(code, n_regs, consts, inputs, out_regs):
        code_w = np.array(code, dtype=np.uint32).reshape(-1, 4); cw = fc.words(consts); iw = fc.words([v for job in inputs for v in job]); ow = np.array(out_regs, dtype=np.uint32)
        out = np.zeros((len(inputs) * len(out_regs), 4), dtype=np.uint64); flags = np.zeros(len(inputs), dtype=np.uint32)
        assert lib.frp_host_run(code_w.ctypes.data, len(code), n_regs, cw.ctypes.data, len(consts), iw.ctypes.data, len(inputs[0]), len(inputs), ow.ctypes.data, len(out_regs),
                                out.ctypes.data, flags.ctypes.data) == 0
        got = fc.ints(out)
        return [got[j * len(out_regs):(j + 1) * len(out_regs)] for j in range(len(inputs))], [int(f) for f in flags]
    return run


@pytest.mark.parametrize("n_instr,jobs", [(1, 1), (2, 65), (2000, 5)])
def test_the_python_restatement_equals_the_interpreter(host, n_instr, jobs):
    rng = np.random.default_rng(9 + n_instr)
    consts = [0, 1, int(rng.integers(2, 1 << 62))]
    code, n_regs, out_regs = fc.random_program(rng, len(consts), 4, 12, n_instr)
    inputs = [[fc.EDGES[(j + t) % 5] if (j + t) % 3 == 0 else int(rng.integers(0, 1 << 62)) ** 4 % fc.R for t in range(4)] for j in range(jobs)]
    assert host(code, n_regs, consts, inputs, out_regs) == fc.interpret(code, n_regs, consts, inputs, out_regs)


def test_every_op_on_every_pair_of_the_adversarial_operands(host):
    pairs = [[a, b] for a in fc.EDGES for b in fc.EDGES]
    for op in (fc.ADD, fc.SUB, fc.MUL):
        code = [(fc.ADD, 3, 1, 0), (fc.ADD, 4, 2, 0), (op, 5, 3, 4), (op, 3, 3, 4), (op, 4, 4, 4)]      # apart, aliasing a, aliasing both
        assert host(code, 6, [0], pairs, [5, 3, 4]) == fc.interpret(code, 6, [0], pairs, [5, 3, 4])
    code = [(fc.SQRN, 2, 1, 0), (fc.SQRN, 3, 1, 1), (fc.SQRN, 4, 1, 64), (fc.INV, 5, 1, 0), (fc.NZ, 0, 1, 31)]
    got = host(code, 6, [0], [[e] for e in fc.EDGES], [2, 3, 4, 5])
    assert got == fc.interpret(code, 6, [0], [[e] for e in fc.EDGES], [2, 3, 4, 5])
    assert got[1][0] == (1 | 1 << 31) and got[1][1:] == [0] * 4 and got[0][0][3] == 0                     # zero: flagged by INV and by NZ, its inverse is zero
