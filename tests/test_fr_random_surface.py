"""CPU-only: the three entry points of the device randomness (mi355_fr_random_dev, mi355_fr_random_rows_dev, mi355_fr_from_u512_dev) are declared, listed, bound and
exported; without a GPU they fail loudly with MI355_ENODEVICE, through scroll-prover_amd/halo2.py too; a draw whose block counters would wrap 2^64 is MI355_EBADARG
before the device is even looked at; the stream table in include/mi355zk_plonk.hpp agrees with the constants the prover uses and with tests/frrand_common.py; the
key never reaches an error text."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import frrand_common as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi355_fr_random_dev", "mi355_fr_random_rows_dev", "mi355_fr_from_u512_dev")
KEY = bytes(range(0xA0, 0xC0))


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_declared_listed_bound_and_exported(zk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355zk.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt)
        assert name in zk._capi.SIGNATURES
        assert re.search(r"fn\s+" + name + r"\s*\(", rs)
        assert hasattr(zk._capi.lib(), name)
    assert callable(zk.halo2.fr_random) and callable(zk.halo2.fr_random_rows) and callable(zk.halo2.fr_from_u512)
    assert re.search(r"pub fn random\(len: usize, slot: c_int, key: &\[u8; 32\]", rs)
    assert "test_device_randomness" in importlib.import_module(zk.__name__ + ".build").CPP_PROGRAMS and "test_device_randomness" in ge.CPP_PROGRAMS
    assert callable(zk.replay.run_device_randomness)
    hpp = open(os.path.join(ROOT, "include", "mi355zk_halo2.hpp")).read()
    for needle in ("void random(const RngKey &key, uint64_t stream, uint64_t counter0 = 0)", "inline void fr_random_rows(", "inline void fr_from_uniform_bytes_dev(", "inline Fr fr_random_reference("):
        assert needle in hpp, needle


def test_without_gpu_is_enodevice_and_a_wrapping_counter_is_ebadarg(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    capi = zk._capi
    lib, ptr = capi.lib(), capi.ptr
    buf = np.zeros((8, 4), dtype=np.uint64); src = np.zeros((8, 8), dtype=np.uint64)
    key = (C.c_uint8 * 32).from_buffer_copy(KEY)
    arr = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    top = (1 << 64) - 1
    assert lib.mi355_fr_random_dev(ptr(buf), 8, key, 0, 0) == capi.ENODEVICE
    assert lib.mi355_fr_random_dev(ptr(buf), 8, key, 7, top - 8) == capi.ENODEVICE                  # counters 2^64 - 9 .. 2^64 - 2: no wrap
    assert lib.mi355_fr_random_rows_dev(arr, 2, 4, 4, key, 1, 0) == capi.ENODEVICE
    assert lib.mi355_fr_from_u512_dev(ptr(buf), ptr(src), 8) == capi.ENODEVICE
    assert lib.mi355_fr_random_dev(ptr(buf), 0, key, 0, 0) == capi.ENODEVICE                         # the device is looked up before n == 0 returns, as everywhere
    for rc in (lib.mi355_fr_random_dev(ptr(buf), 8, key, 0, top - 6), lib.mi355_fr_random_dev(ptr(buf), 2, key, 0, top), lib.mi355_fr_random_rows_dev(arr, 2, 4, 4, key, 1, top - 6)):
        assert rc == capi.EBADARG
        err = lib.mi355_last_error()
        assert b"wraps 2^64" in err and KEY.hex().encode() not in err and KEY not in err
    t = torch.zeros((8, 4), dtype=torch.int64)
    for call in (lambda: zk.halo2.fr_random(t, KEY, 0), lambda: zk.halo2.fr_random_rows([t], 4, 4, KEY, 1), lambda: zk.halo2.fr_from_u512(torch.zeros((8, 8), dtype=torch.int64), t)):
        with pytest.raises(zk.Mi355Error) as e:
            call()
        assert e.value.code == capi.ENODEVICE
    with pytest.raises(zk.Mi355Error) as e:
        zk.halo2.fr_random(t, KEY, 0, counter0=top - 3)
    assert e.value.code == capi.EBADARG


def test_stream_table_agrees_with_the_prover_and_the_tests():
    hpp = open(os.path.join(ROOT, "include", "mi355zk_plonk.hpp")).read()
    consts = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(RNG_STREAM_[A-Z_]+) = (\d+)", hpp))
    assert consts == fc.STREAM_TABLE
    rows = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"^//\s+(RNG_STREAM_[A-Z_]+)\s+(\d+)\s", hpp, flags=re.M))   # the documented table
    assert rows == fc.STREAM_TABLE
    for name in fc.STREAM_TABLE:                                                                                              # and every constant is what create_proof passes
        assert len(re.findall(r"\b" + name + r"\b", hpp)) >= 3, name
    assert (fc.STREAM_RANDOM_POLY, fc.STREAM_ADVICE_BLIND, fc.STREAM_M_BLIND, fc.STREAM_Z_BLIND, fc.STREAM_PHI_BLIND) == (0, 1, 2, 3, 4)
    opts = re.search(r"struct ProofOptions \{.*?\};", hpp, flags=re.S).group(0)
    assert "bool device_randomness = false" in opts and "uint8_t rng_key[32]" in opts and "bool rng_key_from_os = false" in opts
    assert "double random_ms" in hpp and "getrandom(" in hpp
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in fc.STREAM_TABLE:
        assert name in design
