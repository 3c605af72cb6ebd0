"""CPU-only: the compressed-point codec of G1 (mi355_g1_decompress_* / mi355_g1_compress_*) is declared in include/mi355zk.h, listed in the ctypes table, bound by
the Rust shim, exported by the built library and -- without a GPU -- fails loudly with MI355_ENODEVICE, through the halo2.py wrappers too; flag bit 1 of
mi355_srs_load_params_file (SerdeFormat::Processed) is documented in the header and reachable from params_from_file."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi355_g1_decompress_dev", "mi355_g1_decompress_host", "mi355_g1_compress_dev", "mi355_g1_compress_host")


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def header() -> str:
    return open(os.path.join(ROOT, "include", "mi355zk.h")).read()


def test_declared_listed_bound_and_exported(zk):
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in zk._capi.SIGNATURES, name
        assert re.search(r"fn\s+" + name + r"\s*\(", rust), name
        assert hasattr(zk._capi.lib(), name), name
    assert zk._capi.SIGNATURES["mi355_g1_decompress_dev"][1][-1] == C.POINTER(C.c_uint64)
    assert callable(zk.halo2.g1_compress) and callable(zk.halo2.g1_decompress)


def test_header_documents_the_codec_and_flag_bit_1():
    txt = " ".join(header().split())
    assert "flags bit 1" in txt and "SerdeFormat::Processed" in txt and "4 + 2 * 2^k * 32 + 128" in txt
    assert "G1Affine::from_bytes / to_bytes" in txt
    assert "NOT pinned by any fixture" in txt, "the G2 layout is recalled, and the header must say so"
    assert '"g1_decompress"' in txt and '"g1_compress"' in txt   # the profile names


def test_without_gpu_is_enodevice(zk, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    capi, h2 = zk._capi, zk.halo2
    lib, ptr = capi.lib(), capi.ptr
    words, pts = np.zeros((4, 32), dtype=np.uint8), np.zeros((4, 8), dtype=np.uint64)
    bad = C.c_uint64(0)
    assert lib.mi355_g1_decompress_host(ptr(words), ptr(pts), 4, C.byref(bad)) == capi.ENODEVICE
    assert lib.mi355_g1_decompress_dev(ptr(words), ptr(pts), 4, None) == capi.ENODEVICE
    assert lib.mi355_g1_compress_host(ptr(pts), ptr(words), 4) == capi.ENODEVICE
    assert lib.mi355_g1_compress_dev(ptr(pts), ptr(words), 4) == capi.ENODEVICE
    for call in (lambda: h2.g1_decompress(words), lambda: h2.g1_compress(pts)):
        with pytest.raises(zk.Mi355Error) as e:
            call()
        assert e.value.code == capi.ENODEVICE
    path = str(tmp_path / "params4")
    open(path, "wb").write((4).to_bytes(4, "little") + bytes(h2.params_file_size(4, "processed") - 4))
    with pytest.raises(zk.Mi355Error) as e:
        h2.params_from_file(path, format="processed")
    assert e.value.code == capi.ENODEVICE


def test_file_sizes_and_the_host_g2_word(zk):
    h2 = zk.halo2
    assert h2.params_file_size(26) == 8589934852 and h2.params_file_size(26, "raw") == 8589934852
    assert h2.params_file_size(26, "processed") == 4 + (1 << 27) * 32 + 128
    assert h2.g2_to_bytes(bytes(128)) == bytes(64)
    from oracle import pyref
    Q = pyref.g2_mul(pyref.G2_GEN, 0x1234567)
    raw = np.array(pyref.g2_to_limbs(Q), dtype=np.uint64).tobytes()
    want = bytearray(Q[0][0].to_bytes(32, "little") + Q[0][1].to_bytes(32, "little")); want[63] |= (Q[1][0] & 1) << 6
    assert h2.g2_to_bytes(raw) == bytes(want)
