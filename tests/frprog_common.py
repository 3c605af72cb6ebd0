"""TEST INFRASTRUCTURE: the Fr programs of mi355_fr_program_host restated with Python integers -- the reference tests/test_gpu_fr_program.py holds the device to, word for word.
Values are canonical integers here; words() / ints() convert to and from the ABI's Montgomery limbs."""
import numpy as np

from oracle import pyref

R = pyref.R_MOD
RMONT = (1 << 256) % R
RINV = pow(RMONT, -1, R)
ADD, SUB, MUL, SQRN, INV, NZ = range(6)
EDGES = [0, 1, R - 1, (1 << 255) % R, RMONT]                                  # the adversarial operands: zero, one, the largest residue, 2^255 mod r, R mod r


def interpret(code, n_regs, consts, inputs, out_regs):
    """code: [(op, dst, a, b)]; inputs: one list per job -> (outputs per job, flag word per job)"""
    outs, flags = [], []
    for job in inputs:
        reg = list(consts) + list(job) + [None] * (n_regs - len(consts) - len(job)); fl = 0
        for op, d, a, b in code:
            if op == ADD: reg[d] = (reg[a] + reg[b]) % R
            elif op == SUB: reg[d] = (reg[a] - reg[b]) % R
            elif op == MUL: reg[d] = reg[a] * reg[b] % R
            elif op == SQRN: reg[d] = pow(reg[a], 1 << b, R)
            elif op == INV:
                fl |= reg[a] == 0
                reg[d] = pow(reg[a], R - 2, R)
            else: fl |= (reg[a] == 0) << b
        outs.append([reg[r] for r in out_regs]); flags.append(fl)
    return outs, flags


def words(vals):
    """canonical integers -> [n, 4] u64 Montgomery limbs"""
    return np.array([pyref.to_limbs(v * RMONT % R) for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints(arr):
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * RINV % R for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 4)]


def random_program(rng, n_consts, n_inputs, n_temps, n_instr):
    """a program that reads nothing it has not written; every op, SQRN by 0 / 1 / 64 among them; every written register is an output, the last one twice"""
    first = n_consts + n_inputs; written = list(range(first)); code = []
    for _ in range(n_instr):
        pick = int(rng.integers(0, 40)); d = first + int(rng.integers(0, n_temps)); src = lambda: written[int(rng.integers(0, len(written)))]
        if pick < 10: code.append((ADD, d, src(), src()))
        elif pick < 18: code.append((SUB, d, src(), src()))
        elif pick < 32: code.append((MUL, d, src(), src()))
        elif pick < 36: code.append((SQRN, d, src(), [0, 1, 2, 5, 64][int(rng.integers(0, 5))]))
        elif pick == 36: code.append((INV, d, src(), 0))
        else:
            code.append((NZ, 0, src(), 1 + int(rng.integers(0, 31)))); continue
        if d not in written: written.append(d)
    return code, first + n_temps, written + [written[-1]]
