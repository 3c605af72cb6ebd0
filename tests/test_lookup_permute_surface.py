"""CPU-only: mi355_fr_lookup_permute_dev (the permuted columns of the classic halo2 lookup argument, built on the device) is declared in include/mi355zk.h, listed in
the ctypes table, bound by the Rust shim and exported by the built library.  Its argument checks read host memory and the buffer registry only and come before the
device is asked for, so they answer MI355_EBADARG here as well; a well-formed call -- rows == 0 included, as for every compute entry point -- fails loudly with
MI355_ENODEVICE, through the halo2.py wrapper too (no CPU fallback).  A range that leaves its block needs a registered block: tests/test_gpu_lookup_permute.py holds
that check.  Operands on different devices need two devices; that refusal is the shared one of every entry point (common_slot) and has no case of its own here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_fr_lookup_permute_dev"


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_declared_listed_bound_and_exported(zk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355zk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*void \*\w+, void \*\w+, const void \*\w+, const void \*\w+, uint64_t rows, uint64_t \*missing_out\)", txt)
    assert NAME in zk._capi.SIGNATURES and len(zk._capi.SIGNATURES[NAME][1]) == 6
    assert re.search(r"fn\s+" + NAME + r"\s*\(", open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read())
    assert hasattr(zk._capi.lib(), NAME)
    assert callable(zk.halo2.lookup_permute)


def _call(zk, pa, ps, i, t, rows, miss=None):
    miss = miss if miss is not None else C.c_uint64(0)
    return zk._capi.lib().mi355_fr_lookup_permute_dev(C.c_void_p(pa), C.c_void_p(ps), C.c_void_p(i), C.c_void_p(t), rows, C.byref(miss))


def test_bad_arguments_are_refused_before_the_device_is_asked_for(zk):
    capi, lib = zk._capi, zk._capi.lib()
    mem = np.zeros((4, 64, 4), dtype=np.uint64)                       # four columns of 64 words, 32-byte aligned or better
    base = mem.ctypes.data + (-mem.ctypes.data) % 32
    PA, PS, I, T = (base + 32 * 48 * k for k in range(4))
    for args, text in (((PA, PS, I, T, 1 << 31), b"rows must be < 2^31"), ((PA, PS, I, T, (1 << 64) - 1), b"rows must be < 2^31"),
                       ((None, PS, I, T, 8), b"null pointer"), ((PA, None, I, T, 8), b"null pointer"), ((PA, PS, None, T, 8), b"null pointer"), ((PA, PS, I, None, 8), b"null pointer"),
                       ((PA + 4, PS, I, T, 8), b"16-byte aligned"), ((PA, PS, I, T + 8, 8), b"16-byte aligned"),
                       ((PA, PA + 32 * 7, I, T, 8), b"the two outputs must not overlap"), ((PA, PA, I, T, 8), b"the two outputs must not overlap"),
                       ((I + 32 * 7, PS, I, T, 8), b"an output must not overlap an input"), ((PA, T, I, T, 8), b"an output must not overlap an input"),
                       ((PA, I, I, T, 1), b"an output must not overlap an input")):
        miss = C.c_uint64(5)
        assert _call(zk, *args, miss=miss) == capi.EBADARG and text in lib.mi355_last_error(), text
        assert miss.value == (1 << 64) - 1                            # no row is named
    assert (mem == 0).all()


def test_without_gpu_is_enodevice(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    capi = zk._capi
    mem = np.zeros((4, 16, 4), dtype=np.uint64)
    PA, PS, I, T = (mem[k].ctypes.data for k in range(4))
    assert _call(zk, PA, PS, I, T, 8) == capi.ENODEVICE
    assert _call(zk, PA, PS, I, PS + 32 * 8, 8) == capi.ENODEVICE       # ranges that touch without overlapping
    assert _call(zk, PA, PS, I, T, 0) == capi.ENODEVICE                 # the device is looked up before rows == 0 returns, as everywhere
    assert _call(zk, None, None, None, None, 0) == capi.ENODEVICE
    with pytest.raises(zk.Mi355Error) as e:
        zk.halo2.lookup_permute(torch.zeros(8 * 32, dtype=torch.uint8), torch.zeros(8 * 32, dtype=torch.uint8), 8)
    assert e.value.code == capi.ENODEVICE and e.value.row is None
