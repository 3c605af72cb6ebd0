"""CPU-only: the surface of the product-side verifier.  The pairing entry point (mi355_pairing_products_host) is declared, listed, bound and exported, and fails with
MI355_ENODEVICE in a process that has bound no device.  plonk::verify_proof, through its driver in --host-only mode (no device: it stops after building the MSM list),
reproduces the challenges, numerator_at_x and the MSM scalars and points of oracle/plonk.py verify() on the released chunk, batch and bundle proofs, the MSM lists of
tests/golden/released_kats.json (19 / 24 / 19 terms), and names its failures."""
import json
import os
import re
import subprocess
import sys

import pytest

import __graft_entry__ as ge
from oracle import pyref

from verify_common import GOLD, R, ROOT, case, layout, oracle_verify, product_protocol, same_as_oracle

NAME = "mi355_pairing_products_host"


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_pairing_entry_point_is_declared_listed_bound_and_exported(zk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355zk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), f"{NAME} not declared in include/mi355zk.h"
    assert NAME in zk._capi.SIGNATURES, f"{NAME} missing from the ctypes table"
    assert len(zk._capi.SIGNATURES[NAME][1]) == 6
    assert hasattr(zk._capi.lib(), NAME), f"{NAME} not exported by libmi355zk.so"
    assert re.search(r"pub fn " + NAME + r"\(", open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read())
    assert callable(zk.halo2.pairing_products) and callable(zk.halo2.ParamsKZG.check_g2) and callable(zk.halo2.verify_proof)
    assert "lib_pairing" in ge._build_module().UNITS and "test_verify_proof" in ge.CPP_PROGRAMS
    hdr = open(os.path.join(ROOT, "include", "mi355zk_plonk_verify.hpp")).read()
    for sym in ("verify_proof", "struct VerifyResult", "struct G2Pair", "struct VerifyOptions", "struct VerifyingKeyRef"):
        assert sym in hdr


def test_pairing_without_a_bound_device_is_enodevice(zk):
    code = """
import numpy as np
import __graft_entry__ as ge
zk = ge.load_package()
capi = zk._capi
lib, ptr = capi.lib(), capi.ptr
P, Q, gt, one = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 16), dtype=np.uint64), np.zeros((1, 48), dtype=np.uint64), np.zeros(1, dtype=np.uint32)
rc = lib.mi355_pairing_products_host(ptr(P), ptr(Q), 1, 2, ptr(gt), one.ctypes.data_as(capi.C.POINTER(capi.C.c_uint32)))
assert rc == capi.ENODEVICE, rc
assert b"no gfx950 device bound" in lib.mi355_last_error()
try:
    zk.halo2.pairing_products(P, Q, 1, 2)
except zk.Mi355Error as e:
    assert e.code == capi.ENODEVICE
else:
    raise AssertionError("pairing_products returned without a device")
print("enodevice-ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "enodevice-ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("name,terms", [("chunk_proof", 19), ("batch_proof", 24), ("bundle_proof", 19)])
def test_host_only_verifier_reproduces_the_oracle_on_released_proofs(zk, name, terms):
    layer, inst, proof, okw, pkw = case(name)
    want = oracle_verify(layer, inst, proof, okw)
    assert want["ok"], want                                                  # the oracle accepts: what follows is the product's
    got = zk.halo2.verify_proof(product_protocol(layer), inst, proof, host_only=True, **pkw)
    assert got["ok"] and got["error"] == "" and got["host_only"], got
    same_as_oracle(got, want)
    assert got["has_accumulator"]
    kat = json.load(open(os.path.join(GOLD, "released_kats.json")))[name]["msm"]
    assert len(got["msm"]["scalars"]) == len(kat["scalars"]) == terms
    assert got["msm"]["scalars"] == [int(s, 16) for s in kat["scalars"]]
    assert got["msm"]["points"] == [(int(p[0], 16), int(p[1], 16)) for p in kat["points"]]
    assert got["msm"]["w_prime"] == (int(kat["w_prime"][0], 16), int(kat["w_prime"][1], 16))


def not_a_point_word(word: bytes) -> bytes:
    """the nearest change of a compressed word whose x has no y: x^3 + 3 a non-residue"""
    for d in range(1, 64):
        w = bytearray(word); w[0] = (w[0] + d) & 0xFF
        try:
            if pyref.g1_decompress(bytes(w)) is None:
                return bytes(w)
        except AssertionError:
            return bytes(w)
    raise AssertionError("no rejected word nearby")


@pytest.mark.parametrize("name", ["chunk_proof", "bundle_proof"])
def test_named_failures(zk, name):
    layer, inst, proof, okw, pkw = case(name)
    coms, evs, shp, nb = layout(layer, okw["transcript"])
    run = lambda i, p, **kw: zk.halo2.verify_proof(product_protocol(layer), i, p, host_only=True, **dict(pkw, **kw))
    # a proof one word short
    short = proof[:-32]
    assert not oracle_verify(layer, inst, short, okw)["ok"]
    got = run(inst, short); assert not got["ok"] and got["error"] == "proof_length", got
    got = run(inst, proof + bytes(32)); assert not got["ok"] and got["error"] == "proof_length", got        # and leftover bytes
    # a non-canonical evaluation word: r itself
    bad = bytearray(proof); bad[evs[3]:evs[3] + 32] = R.to_bytes(32, "big" if nb == 64 else "little")
    assert not oracle_verify(layer, inst, bytes(bad), okw)["ok"]
    got = run(inst, bytes(bad)); assert not got["ok"] and got["error"] == "non_canonical_scalar" and "evaluation 3" in got["detail"], got
    # a point word that is not on the curve
    bad = bytearray(proof)
    if nb == 64:
        bad[coms[2] + 63] ^= 1                                              # y + 1: (x, y + 1) is off the curve
    else:
        bad[coms[2]:coms[2] + 32] = not_a_point_word(proof[coms[2]:coms[2] + 32])
    assert not oracle_verify(layer, inst, bytes(bad), okw)["ok"]
    got = run(inst, bytes(bad)); assert not got["ok"] and got["error"] == "invalid_point" and "point 2 " in got["detail"], got
    # an accumulator limb of 2^88 or more
    big = list(inst); big[4] |= 1 << 88
    assert not oracle_verify(layer, big, proof, okw)["ok"]
    got = run(big, proof); assert not got["ok"] and got["error"] == "accumulator_limb" and "instance 4" in got["detail"], got
    got = run(big, proof, check_accumulator=False); assert got["ok"] and not got["has_accumulator"]        # host-only: the list is built, nothing is judged
    # accumulator limbs in range whose point is off the curve
    off = list(inst); off[0] ^= 1
    got = run(off, proof); assert not got["ok"] and got["error"] == "accumulator_point", got
