"""CPU-only: mi355_fr_permutation_sigma_dev (the sigma columns of the permutation argument, built on the device from the copy mapping) is declared, listed, bound and
exported, and -- without a GPU -- fails loudly with MI355_ENODEVICE, through halo2.permutation_sigma too.  PermutationAssembly in Python (scroll-prover_amd/halo2.py)
and in C++ (include/mi355zk_halo2.hpp, compiled by tests/hostcheck/perm_selftest.cpp) give the same mapping on random copy sequences over 3 columns of 2^6 rows;
each mapping is a permutation whose cycles are exactly the classes of an independent union-find; overrides() lists exactly the cells that moved."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import perm_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_fr_permutation_sigma_dev"
NC, N = 3, 1 << 6


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_declared_listed_bound_and_exported(zk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355zk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt)
    assert NAME in zk._capi.SIGNATURES
    assert re.search(r"fn\s+" + NAME + r"\s*\(", open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read())
    assert hasattr(zk._capi.lib(), NAME)
    assert callable(zk.halo2.permutation_sigma) and callable(zk.halo2.PermutationAssembly)
    assert "test_permutation_keygen" in importlib.import_module(zk.__name__ + ".build").CPP_PROGRAMS and "test_permutation_keygen" in ge.CPP_PROGRAMS
    assert callable(zk.replay.run_permutation_keygen)


def test_without_gpu_is_enodevice(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    capi = zk._capi
    lib, ptr = capi.lib(), capi.ptr
    col = np.zeros((8, 4), dtype=np.uint64)
    arr = (C.c_void_p * 1)(col.ctypes.data)
    one = zk.halo2.fr(1)
    none = C.cast(None, C.POINTER(C.c_uint64))
    assert lib.mi355_fr_permutation_sigma_dev(arr, 1, 3, ptr(one), ptr(one), none, none, 0, 0) == capi.ENODEVICE
    with pytest.raises(zk.Mi355Error) as e:
        zk.halo2.permutation_sigma(1, 3, one, one, out=[torch.zeros(8 * 32, dtype=torch.uint8)])
    assert e.value.code == capi.ENODEVICE


def copy_sequences():
    """name -> [m, 4] copies over (NC, N): random ones, repeats, copies inside a cycle, a small cycle merged into a large one and the reverse"""
    rng = np.random.default_rng(1606)

    def rand(m):
        return np.stack([rng.integers(0, NC, m), rng.integers(0, N, m), rng.integers(0, NC, m), rng.integers(0, N, m)], axis=1)

    def chain(cells):
        return [(a[0], a[1], b[0], b[1]) for a, b in zip(cells, cells[1:])]

    big = [(j, r) for j in range(NC) for r in range(0, 40, 3)]        # 42 cells across the three columns
    small = [(2, 41), (0, 43), (1, 47)]
    seqs = {
        "none": np.zeros((0, 4), dtype=np.int64),
        "sparse": rand(20),
        "dense": rand(400),                                           # far more copies than cells: most land inside a cycle
        "repeated": np.concatenate([rand(30)] * 3),
        "inside_one_cycle": np.array(chain(big) + [(0, 0, 2, 39), (1, 3, 0, 36), (2, 39, 0, 0)] + chain(big[::-1])),
        "small_into_large": np.array(chain(big) + chain(small) + [(big[5] + small[1])]),
        "large_into_small": np.array(chain(big) + chain(small) + [(small[2] + big[17])]),
        "self_copies": np.array([(1, 5, 1, 5), (0, 0, 0, 0), (1, 5, 2, 5), (1, 5, 1, 5)]),
    }
    for s in range(6):
        seqs[f"random_{s}"] = rand(int(rng.integers(1, 150)))
    return seqs


SEQS = copy_sequences()


@pytest.mark.parametrize("name", sorted(SEQS))
def test_python_and_cpp_assemblies_agree_and_follow_the_union_find(zk, name):
    copies = SEQS[name]
    py = zk.halo2.PermutationAssembly(NC, N)
    for c in copies:
        py.copy(*[int(x) for x in c])
    mapping, aux, sizes = pc.cpp_mapping(NC, N, copies, with_aux=True)
    assert (py.mapping == mapping).all(), "Python and C++ mappings differ"
    assert (py.aux == aux).all()
    named = np.unique(aux)                                            # sizes is meaningful at the cells that name a cycle
    assert (py.sizes[named] == sizes[named]).all()
    cyc = pc.cycles_of(mapping)
    assert cyc == pc.union_find_classes(NC * N, copies, N)
    for cells in cyc:                                                 # one label per cycle, and its recorded length
        assert len({int(aux[c]) for c in cells}) == 1 and int(sizes[int(aux[cells[0]])]) == len(cells)
    moved = np.nonzero(mapping != np.arange(NC * N, dtype=np.uint64))[0]
    for cells, images in (py.overrides(), pc.cpp_overrides(NC, N, mapping)):
        assert cells.dtype == np.uint64 and (cells == moved).all() and (images == mapping[moved]).all()
    assert len(moved) == sum(len(c) for c in cyc)


def test_merge_direction_decides_the_cycle_order(zk):
    """the same equalities, merged in the two directions, give the same classes but not the same mapping: why sigma must come from the caller's mapping"""
    a, b = pc.cpp_mapping(NC, N, SEQS["small_into_large"]), pc.cpp_mapping(NC, N, SEQS["large_into_small"])
    assert not (a == b).all()
    assert len(pc.cycles_of(a)) == len(pc.cycles_of(b)) == 1 and len(pc.cycles_of(a)[0]) == 45


def test_copy_outside_the_permutation_is_refused(zk):
    py = zk.halo2.PermutationAssembly(NC, N)
    for bad in ((NC, 0, 0, 0), (0, N, 0, 0), (0, 0, NC, 0), (0, 0, 0, N)):
        with pytest.raises(AssertionError):
            py.copy(*bad)
        with pytest.raises(AssertionError):
            pc.cpp_mapping(NC, N, [bad])
