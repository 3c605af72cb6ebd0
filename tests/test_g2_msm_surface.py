"""CPU-only: the G2 MSM entry points (mi355_msm_g2_*) are declared in include/mi355zk.h, listed in the ctypes table, exported by the
built libmi355zk.so and -- without a GPU -- fail loudly with MI355_ENODEVICE (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi355_msm_g2_adhoc_host", "mi355_msm_g2_dev", "mi355_msm_g2_batch_dev")


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_g2_msm_is_declared_listed_and_exported(zk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355zk.h")).read(), flags=re.S)
    lib = zk._capi.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), f"{name} not declared in include/mi355zk.h"
        assert name in zk._capi.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported by libmi355zk.so"


def test_g2_msm_without_gpu_is_enodevice(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    capi = zk._capi
    lib, ptr = capi.lib(), capi.ptr
    bases, sc, out = np.zeros((4, 16), dtype=np.uint64), np.zeros((4, 4), dtype=np.uint64), np.zeros((4, 16), dtype=np.uint64)
    arr = (C.c_void_p * 1)(sc.ctypes.data)
    assert lib.mi355_msm_g2_adhoc_host(ptr(bases), ptr(sc), 4, ptr(out)) == capi.ENODEVICE
    assert lib.mi355_msm_g2_dev(ptr(bases), ptr(sc), 4, ptr(out)) == capi.ENODEVICE
    assert lib.mi355_msm_g2_batch_dev(ptr(bases), arr, 1, 4, ptr(out)) == capi.ENODEVICE
    with pytest.raises(zk.Mi355Error):
        zk.halo2.g2_msm(bases, sc)
