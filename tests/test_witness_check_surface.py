"""CPU-only: the witness check's entry points (mi355_fr_nonzero_rows_dev, mi355_fr_copy_check_dev) are declared, bound and exported, and -- without a GPU -- fail loudly
with MI355_ENODEVICE, through halo2.nonzero_rows / halo2.copy_check and the compiled caller too; the compiled caller's --corrupt grammar."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi355_fr_nonzero_rows_dev", "mi355_fr_copy_check_dev")


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_declared_bound_and_mirrored(zk):
    hdr = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    shim = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    mirror = open(os.path.join(ROOT, "include", "mi355zk_halo2.hpp")).read()
    for name in NAMES:
        assert name in hdr and name in shim and name in mirror and name in zk._capi.SIGNATURES and hasattr(zk._capi.lib(), name)
    assert "[EXT-recalled halo2_proofs src/dev.rs, MockProver::verify: gate, lookup and permutation failures]" in hdr
    assert callable(zk.halo2.nonzero_rows) and callable(zk.halo2.copy_check) and callable(zk.replay.run_witness_check)
    plonk_hpp = open(os.path.join(ROOT, "include", "mi355zk_plonk.hpp")).read()
    for needle in ("struct VerifyFailure", "struct CheckOptions", "check_witness(const ProvingKey &pk, const Circuit &wit, const CheckOptions &opt)", "struct WitnessError : std::runtime_error", "bool check_witness = false"):
        assert needle in plonk_hpp, needle


def test_no_gpu_means_loud_failure(zk, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    lib = zk._capi.lib()
    a = np.zeros((8, 4), dtype=np.uint64)
    arr = (C.c_void_p * 1)(a.ctypes.data)
    u64p = C.POINTER(C.c_uint64)
    out = np.zeros(8, dtype=np.uint64); nf = C.c_uint64()
    assert lib.mi355_fr_nonzero_rows_dev(arr, 1, 8, 4, out.ctypes.data_as(u64p), out.ctypes.data_as(u64p)) == zk._capi.ENODEVICE
    assert lib.mi355_fr_copy_check_dev(arr, 1, 3, None, None, 0, 4, C.byref(nf), out.ctypes.data_as(u64p)) == zk._capi.ENODEVICE
    t = torch.zeros((8, 4), dtype=torch.int64)
    with pytest.raises(zk.Mi355Error):
        zk.halo2.nonzero_rows(t)
    with pytest.raises(zk.Mi355Error):
        zk.halo2.copy_check([t], [], [])
    rec = zk.replay.run_witness_check(2, 6, out_dir=str(tmp_path))
    assert not rec["ok"] and rec["returncode"] == 2 and "mi355_init" in rec["error"]
    assert os.path.exists(os.path.join(str(tmp_path), "advice.bin")), "the inputs are dumped before the device is asked for"


def test_corrupt_grammar(zk, tmp_path):
    exe = ge.build_cpp("test_witness_check")
    proto = zk.protocols.write(2, str(tmp_path / "p.json"), 6)
    run = lambda *spec: subprocess.run([exe, "--protocol", proto, "--out", str(tmp_path), "--builder-only"] + [x for s in spec for x in ("--corrupt", s)], capture_output=True, text=True, timeout=120)
    clean = run(); assert clean.returncode == 0
    base = np.fromfile(str(tmp_path / "advice.bin"), dtype=np.uint64).reshape(-1, 4)
    inst = np.fromfile(str(tmp_path / "instance.bin"), dtype=np.uint64).reshape(-1, 4)
    assert run("advice:0:3", "instance:0").returncode == 0
    got = np.fromfile(str(tmp_path / "advice.bin"), dtype=np.uint64).reshape(-1, 4)
    assert list(np.nonzero((got != base).any(axis=1))[0]) == [3]
    assert (np.fromfile(str(tmp_path / "instance.bin"), dtype=np.uint64).reshape(-1, 4) != inst).any(axis=1).tolist()[0] is True
    for bad in ("advice:0", "fixed:0:1", "advice:x:1", "instance:", "advice:99:0", "instance:100000"):
        assert run(bad).returncode == 1, bad
