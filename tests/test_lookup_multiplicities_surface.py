"""CPU-only: mi355_fr_lookup_multiplicities_dev (the multiplicity column of the mv-lookup argument, counted on the device) is declared in include/mi355zk.h, listed
in the ctypes table, bound by the Rust shim, exported by the built library and -- without a GPU -- fails loudly with MI355_ENODEVICE, through the halo2.py wrapper
too.  The numpy restatement the GPU tests compare against gives the hand-computed answers on a toy table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.lookup_common import counts_to_words, fr_mont, reference_ids, reference_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_fr_lookup_multiplicities_dev"


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
    assert callable(zk.halo2.lookup_multiplicities)


def test_without_gpu_is_enodevice(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    capi = zk._capi
    lib, ptr = capi.lib(), capi.ptr
    m, t, x = np.zeros((8, 4), dtype=np.uint64), np.zeros((8, 4), dtype=np.uint64), np.zeros((8, 4), dtype=np.uint64)
    arr = (C.c_void_p * 1)(x.ctypes.data)
    miss = C.c_uint64(0)
    assert lib.mi355_fr_lookup_multiplicities_dev(ptr(m), 8, ptr(t), 8, arr, 1, 8, 0, C.byref(miss)) == capi.ENODEVICE
    with pytest.raises(zk.Mi355Error) as e:
        zk.halo2.lookup_multiplicities(torch.zeros(8 * 32, dtype=torch.uint8), [torch.zeros(8 * 32, dtype=torch.uint8)], 8, 8)
    assert e.value.code == capi.ENODEVICE


def _words(vals):
    return np.stack([fr_mont(v) for v in vals])


# rows 6, 7 of the table hold 0 too, but lie beyond table_rows: they never receive a count
TABLE = [5, 7, 5, 0, 9, 0, 0, 0]
IN0 = [7, 5, 5, 0, 1, 1, 1, 1]
IN1 = [0, 0, 7, 5, 1, 1, 1, 1]   # rows >= input_rows = 4 hold a value the table lacks: not read


def test_reference_first_rule_two_columns():
    counts, miss = reference_words(_words(TABLE), 6, [_words(IN0), _words(IN1)], 4)
    assert miss is None and counts.tolist() == [3, 2, 0, 3, 0, 0, 0, 0]
    assert (counts_to_words(counts)[0] == fr_mont(3)).all() and (counts_to_words(counts)[2] == 0).all()


def test_reference_last_rule_two_columns():
    counts, miss = reference_words(_words(TABLE), 6, [_words(IN0), _words(IN1)], 4, last=True)
    assert miss is None and counts.tolist() == [0, 2, 3, 0, 0, 3, 0, 0]


def test_reference_missing_value_names_the_smallest_pair():
    bad0, bad1 = list(IN0), list(IN1)
    bad0[3] = 13; bad1[0] = 11                   # (column 0, row 3) and (column 1, row 0): the column decides first
    assert reference_words(_words(TABLE), 6, [_words(bad0), _words(bad1)], 4)[1] == (0, 3)
    assert reference_words(_words(TABLE), 6, [_words(IN0), _words(bad1)], 4)[1] == (1, 0)
    assert reference_words(_words(TABLE), 3, [_words(IN0)], 4)[1] == (0, 3)   # 0 sits at table row 3 only: outside table_rows = 3


def test_reference_on_ids_matches_the_word_form():
    rng = np.random.default_rng(5)
    n = 64
    ids = rng.integers(1, 20, size=n); ids[40:] = 0
    x = ids[rng.integers(0, 50, size=n)]
    for last in (False, True):
        a = reference_ids(ids, 50, [x], 60, n, last)[0]
        b = reference_words(_words(ids.tolist()), 50, [_words(x.tolist())], 60, last)[0]
        assert (a == b).all() and a.sum() == 60 and (a[50:] == 0).all()
