"""helpers shared by the tests of the permutation sigma columns (TEST INFRASTRUCTURE): halo2::PermutationAssembly of include/mi355zk_halo2.hpp compiled with g++
(tests/hostcheck/perm_selftest.cpp) behind ctypes, an independent union-find, and the sigma words of a mapping from Python integers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
R = pyref.R_MOD
DELTA = pow(pyref.FR_GENERATOR, 1 << pyref.FR_S, R)   # halo2curves bn256::Fr::DELTA = GENERATOR^(2^S)
_lib = None


def cpp_assembly():
    global _lib
    if _lib is None:
        so = os.path.join(tempfile.mkdtemp(prefix="perm_selftest_"), "libpermselftest.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, os.path.join(HERE, "hostcheck", "perm_selftest.cpp")])
        _lib = C.CDLL(so)
        _lib.perm_assembly_run.restype = C.c_int
        _lib.perm_assembly_overrides.restype = C.c_uint64
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cpp_mapping(n_cols, n, copies, with_aux=False):
    """halo2::PermutationAssembly(n_cols, n) after copy(*c) for every c of `copies` ([m, 4]: col_a, row_a, col_b, row_b): its mapping (and aux, sizes)"""
    copies = np.ascontiguousarray(np.asarray(copies, dtype=np.uint64).reshape(-1, 4))
    out = [np.empty(n_cols * n, dtype=np.uint64) for _ in range(3)]
    ok = cpp_assembly().perm_assembly_run(C.c_uint32(n_cols), C.c_uint64(n), _p(copies), C.c_uint64(copies.shape[0]), _p(out[0]), _p(out[1]), _p(out[2]))
    assert ok == 1, "a copy names a cell outside the permutation"
    return tuple(out) if with_aux else out[0]


def cpp_overrides(n_cols, n, mapping):
    mapping = np.ascontiguousarray(mapping, dtype=np.uint64)
    cells, images = np.empty(n_cols * n, dtype=np.uint64), np.empty(n_cols * n, dtype=np.uint64)
    cnt = cpp_assembly().perm_assembly_overrides(C.c_uint32(n_cols), C.c_uint64(n), _p(mapping), _p(cells), _p(images))
    return cells[:cnt].copy(), images[:cnt].copy()


def union_find_classes(total, copies, n):
    """the classes of the equalities `copies` by a union-find that knows nothing of cycles: a sorted list of sorted tuples of cells (singletons left out)"""
    parent = list(range(total))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for ca, ra, cb, rb in copies:
        a, b = find(int(ca) * n + int(ra)), find(int(cb) * n + int(rb))
        if a != b:
            parent[max(a, b)] = min(a, b)
    cls = {}
    for c in range(total):
        cls.setdefault(find(c), []).append(c)
    return sorted(tuple(v) for v in cls.values() if len(v) > 1)


def cycles_of(mapping):
    """the cycles of a permutation given as an array, as union_find_classes lists classes; asserts that it IS a permutation"""
    m = [int(x) for x in mapping]
    assert sorted(m) == list(range(len(m))), "mapping is not a permutation"
    seen, out = [False] * len(m), []
    for c in range(len(m)):
        if seen[c]:
            continue
        cyc, x = [], c
        while not seen[x]:
            seen[x] = True; cyc.append(x); x = m[x]
        if len(cyc) > 1:
            out.append(tuple(sorted(cyc)))
    return sorted(out)


def sigma_words(n_cols, log_n, mapping, delta=DELTA, omega=None):
    """[n_cols, n, 4] u64: the Montgomery words of sigma[j][r] = delta^j' omega^r' for (j', r') = mapping[j * n + r], from Python integers"""
    n = 1 << log_n
    w = pyref.omega(log_n) if omega is None else omega
    mont = pyref.MONT_R % R
    wm = [mont] * n                                                   # omega^r in Montgomery form
    for r in range(1, n):
        wm[r] = wm[r - 1] * w % R
    ident = b"".join(b"".join((x * dj % R).to_bytes(32, "little") for x in wm) for dj in (pow(delta, j, R) for j in range(n_cols)))
    out = np.frombuffer(ident, dtype=np.uint64).reshape(n_cols * n, 4).copy()
    mapping = np.asarray(mapping, dtype=np.uint64)
    moved = np.nonzero(mapping != np.arange(n_cols * n, dtype=np.uint64))[0]
    out[moved] = out[mapping[moved].astype(np.int64)]                # the word of the image cell: delta^j' omega^r'
    return out.reshape(n_cols, n, 4)
