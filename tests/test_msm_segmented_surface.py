"""CPU-only: the surface of the segmented G1 MSM and of the batch verifier built on it.  mi355_msm_g1_segmented_host is declared in include/mi355zk.h (citing the call site it
serves), sits in the ctypes table with five arguments, is exported by the library and bound in the Rust shim; halo2.msm_g1_segmented / verify_proofs / aggregate exist; the
driver test_verify_proofs is one of the compiled programs.  Without a device the entry point fails with MI355_ENODEVICE -- after its argument checks, which read host memory
only and therefore answer MI355_EBADARG here as well (ALL of the entry point's EBADARG cases are checked before the device is asked for)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_msm_g1_segmented_host"


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_declared_bound_exported_and_in_the_rust_block(zk):
    hdr = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m and len(m.group(1).split(",")) == 5
    assert "const uint64_t *offsets_host" in m.group(1) and "uint32_t segments" in m.group(1)
    comment = hdr[:m.start()].rsplit("/*", 1)[1]
    assert "[REF integration/src/prove.rs:67]" in comment and "gen_batch_proof" in comment
    ret, args = zk._capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(args) == 5 and args[3] is C.c_uint32
    assert hasattr(zk._capi.lib(), NAME)
    rs = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rs, flags=re.S).group(1)
    assert re.search(r"fn\s+%s\s*\(" % NAME, block)


def test_python_and_cpp_surfaces_exist(zk):
    for f in ("msm_g1_segmented", "verify_proofs", "aggregate"):
        assert callable(getattr(zk.halo2, f))
    h2 = open(os.path.join(ROOT, "include", "mi355zk_halo2.hpp")).read()
    assert "msm_g1_segmented(" in h2 and NAME in h2
    pv = open(os.path.join(ROOT, "include", "mi355zk_plonk_verify.hpp")).read()
    for needle in ("struct ProofInput", "verify_proofs(const std::vector<ProofInput> &in, const G2Pair &srs)", "struct AggregateResult", "aggregate(const std::vector<ProofInput> &in, const G2Pair *srs"):
        assert needle in pv, needle
    assert "test_verify_proofs" in ge.CPP_PROGRAMS and "test_verify_proofs" in ge._build_module().CPP_PROGRAMS
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_verify_proofs.cpp"))


def _args(n=4, offsets=(0, 2, 4)):
    bs = np.zeros((n, 8), dtype=np.uint64); sc = np.zeros((n, 4), dtype=np.uint64)
    off = np.array(offsets, dtype=np.uint64); out = np.full((len(offsets) - 1, 8), 7, dtype=np.uint64)
    return bs, sc, off, out


def test_no_device_is_a_loud_failure(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for a machine without a GPU")
    capi, ptr, lib = zk._capi, zk._capi.ptr, zk._capi.lib()
    bs, sc, off, out = _args()
    assert lib.mi355_msm_g1_segmented_host(ptr(bs), ptr(sc), ptr(off), 2, ptr(out)) == capi.ENODEVICE
    assert (out == 7).all()
    assert lib.mi355_msm_g1_segmented_host(None, None, None, 0, None) == capi.ENODEVICE      # segments == 0 touches nothing, but it is still a compute entry point
    with pytest.raises(zk.Mi355Error):
        zk.halo2.msm_g1_segmented(bs, sc, off)


def test_bad_arguments_are_named_before_the_device_is_asked_for(zk):
    """every EBADARG case of the entry point: null pointers, offsets[0] != 0, decreasing offsets, segments > 2^20, more than 2^24 terms; the output stays untouched"""
    capi, ptr, lib = zk._capi, zk._capi.ptr, zk._capi.lib()
    bs, sc, off, out = _args()
    call = lambda b, s, o, n, r: lib.mi355_msm_g1_segmented_host(ptr(b), ptr(s), ptr(o), n, ptr(r))
    assert call(None, sc, off, 2, out) == capi.EBADARG and b"null" in lib.mi355_last_error()
    assert call(bs, None, off, 2, out) == capi.EBADARG
    assert call(bs, sc, None, 2, out) == capi.EBADARG
    assert call(bs, sc, off, 2, None) == capi.EBADARG
    assert call(bs, sc, np.array([1, 2, 4], dtype=np.uint64), 2, out) == capi.EBADARG and b"offsets[0]" in lib.mi355_last_error()
    assert call(bs, sc, np.array([0, 3, 2], dtype=np.uint64), 2, out) == capi.EBADARG and b"decrease" in lib.mi355_last_error()
    assert call(bs, sc, np.array([0, 2, (1 << 24) + 1], dtype=np.uint64), 2, out) == capi.EBADARG and b"2^24" in lib.mi355_last_error()
    assert call(bs, sc, off, (1 << 20) + 1, out) == capi.EBADARG and b"2^20" in lib.mi355_last_error()   # refused before a single offset is read
    assert (out == 7).all()
