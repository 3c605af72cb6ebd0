"""the definition plonk::check_witness (include/mi355zk_plonk.hpp) is held to (TEST INFRASTRUCTURE, not a test): MockProver::verify restated in Python over oracle.plonk
on a dumped instance (tests/cpp/test_witness_check.cpp writes one on every run).

  gates     every constraint of the numerator that is neither a boundary constraint nor an l_active one, evaluated with plonk.evaluate on ALL n rows, rotations mod n;
            index = its position in the numerator's list
  copies    the copy mapping recovered from the sigma columns of `pre` (a dictionary from delta^j omega^r to (j, r): cheap at k <= 10), the cells with mapping != identity
            in cell order -- the lists halo2::PermutationAssembly::overrides gives -- and of those the pairs whose two cells differ
  lookups   table and input TUPLES over the usable rows, no theta: per lookup the smallest input row whose tuple the table lacks
"""
import os
import subprocess

import numpy as np

import __graft_entry__ as ge
from oracle import plonk

R = plonk.R


def build_instance(directory, layer, k, corrupt=(), **shape):
    """the compiled caller with --builder-only (no device): the instance with the cells of `corrupt` changed, dumped into `directory`"""
    zk = ge.load_package()
    os.makedirs(directory, exist_ok=True)
    proto = zk.protocols.write(layer, os.path.join(directory, "p.json"), k, **shape)
    cmd = [ge.build_cpp("test_witness_check"), "--protocol", proto, "--out", directory, "--builder-only", "--threads", "4"] + [x for c in corrupt for x in ("--corrupt", c)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return directory


def perm_columns(pr):
    return [c for chunk in pr.perm for c in chunk["columns"]]      # (column, sigma, delta^j) in permutation position order


def gate_indices(pr):
    """positions in the numerator's list of the constraints Protocol._recognise files under `gates`"""
    cons = pr.numerator["DistributePowers"][0]
    return [i for i, c in enumerate(cons) if any(c is g for g in pr.gates)]


class Reference:
    def __init__(self, directory):
        self._set(*plonk.ProofInputs.load(directory))

    @classmethod
    def from_inputs(cls, inp):
        """the same definition over a plonk.ProofInputs that is already in memory (plonk_capi_common.proof_inputs: the columns read back through circuit_get)"""
        ref = cls.__new__(cls)
        ref._set(inp, None)
        return ref

    def _set(self, inp, man):
        self.inp, self.man = inp, man
        pr = self.pr = self.inp.pr
        n = pr.n
        inst = list(self.inp.instances) + [0] * (n - len(self.inp.instances))
        self._cols = {}
        for i, c in enumerate(self.inp.pre):
            self._cols[i] = np.array(c, dtype=object)
        self._cols[pr.inst0] = np.array(inst, dtype=object)
        for i, c in enumerate(self.inp.advice):
            self._cols[pr.phase0[0] + i] = np.array(c, dtype=object)

    def column(self, poly):
        assert poly in self._cols, f"polynomial {poly} is neither fixed, instance nor advice"
        return self._cols[poly]

    def _eval(self, e):
        def no(*_):
            raise AssertionError("a gate / lookup expression names a challenge or a common polynomial")
        v = plonk.evaluate(e, lambda i, rot: np.roll(self.column(i), -rot), no, no, no)
        return v if isinstance(v, np.ndarray) else np.full(self.pr.n, v, dtype=object)

    def gates(self):
        """{constraint index: [failing rows, ascending]} -- only the constraints that fail somewhere"""
        cons = self.pr.numerator["DistributePowers"][0]
        out = {}
        for i in gate_indices(self.pr):
            rows = [int(r) for r in np.nonzero(self._eval(cons[i]) % R != 0)[0]]
            if rows:
                out[i] = rows
        return out

    def overrides(self):
        """(cells, images) in cell order, cell = position * n + row, from the sigma columns"""
        pr, n = self.pr, self.pr.n
        cols = perm_columns(pr)
        where = {}
        for j, (_, _, dpow) in enumerate(cols):
            v = dpow
            for r in range(n):
                where[v] = j * n + r
                v = v * pr.omega % R
        cells, images = [], []
        for j, (_, sigma, _) in enumerate(cols):
            for r, s in enumerate(self.inp.pre[sigma]):
                im = where[s]
                if im != j * n + r:
                    cells.append(j * n + r); images.append(im)
        return cells, images

    def copies(self):
        """[(t, position_a, row_a, position_b, row_b)] of the failing pairs, ascending t"""
        n = self.pr.n
        vals = [self.column(c) for c, _, _ in perm_columns(self.pr)]
        cells, images = self.overrides()
        return [(t, c // n, c % n, im // n, im % n) for t, (c, im) in enumerate(zip(cells, images)) if vals[c // n][c % n] != vals[im // n][im % n]]

    def lookups(self):
        """{lookup index: smallest usable input row whose tuple the table (usable rows) lacks}"""
        u, out = self.pr.usable, {}
        parts = lambda e: e["DistributePowers"][0] if "DistributePowers" in e else [e]
        for l, lk in enumerate(self.pr.lookups):
            table = list(zip(*[[int(x) for x in self._eval(e)[:u] % R] for e in parts(lk["table"])]))
            inputs = list(zip(*[[int(x) for x in self._eval(e)[:u] % R] for e in parts(lk["input"])]))
            have = set(table)
            miss = next((r for r, t in enumerate(inputs) if t not in have), None)
            if miss is not None:
                out[l] = miss
        return out


def first_lookup_input(pr):
    """(advice column, row) of a cell lookup 0 reads on a row where it is switched on: row 1 (the builder's in-place lookups select the middle input of block 0)"""
    found = []

    def walk(e):
        if isinstance(e, dict):
            if "Polynomial" in e and e["Polynomial"]["poly"] >= pr.phase0[0]:
                found.append(e["Polynomial"]["poly"] - pr.phase0[0])
            for v in e.values():
                walk(v)
        elif isinstance(e, list):
            for v in e:
                walk(v)
    walk(pr.lookups[0]["input"])
    return found[0], 1


def expected_failures(ref, cap=16):
    """check.json's `failures` as the definition gives them: gates (index, rows ascending, `cap` per gate), then copies (`cap` in all); lookups are compared apart"""
    out = []
    for i, rows in sorted(ref.gates().items()):
        out += [{"kind": "gate", "index": i, "row": r, "count": len(rows), "col_a": 0, "col_b": 0, "row_b": 0} for r in rows[:cap]]
    cp = ref.copies()
    out += [{"kind": "copy", "index": t, "row": ra, "count": len(cp), "col_a": ja, "col_b": jb, "row_b": rb} for t, ja, ra, jb, rb in cp[:cap]]
    return out
