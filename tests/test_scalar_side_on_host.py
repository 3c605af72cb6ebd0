"""CPU-only: the scalar-side compiler (include/mi355zk_plonk_scalar.hpp) through tests/hostcheck/scalar_side_main.cpp.  For each of the seven layer protocols the program
compile_scalar_program records is interpreted by the code the kernel runs (csrc/frprog.hpp, on the host) over random inputs and over crafted ones (x = omega^0, u = x omega^rot,
x = 0) and held word for word to the walk over Fr itself, flags and host_finish's records included; for the ten released proofs the inputs are what vdetail::host_part hands
over.  Each program holds exactly one INV and stays under the register cap."""
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

from verify_common import ALL_TEN, case, product_protocol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "scalar_side_main.cpp")
LAYERS = list(range(7))                                                        # at their own domain sizes: the scalar side never touches a vector of that length


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def exe(zk, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("scalar_side") / "scalar_side_main")
    lib = os.path.dirname(zk._capi.LIB_PATH)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), SRC, "-o", out, "-L", lib, "-lmi355zk",
                           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def run(exe, *args):
    p = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "all passed" in p.stdout and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("layer", LAYERS)
def test_program_equals_the_host_walk_on_random_and_crafted_inputs(zk, exe, tmp_path, layer):
    path = zk.protocols.write(layer, str(tmp_path / ("layer%d.json" % layer)))
    rec = run(exe, "--protocol", path, "--jobs", "5")[0]
    assert rec["inversions"] == 1 and 0 < rec["registers"] <= 1 << 16 and 0 < rec["instructions"] <= 1 << 20
    assert rec["outputs"] >= 4 and rec["inputs"] > 8


def test_released_proofs_equal_the_host_walk(zk, exe, tmp_path):
    d = str(tmp_path)
    put = lambda name, data: (open(os.path.join(d, name), "wb").write(data), os.path.join(d, name))[1]
    man = {"proofs": []}
    for i, name in enumerate(ALL_TEN):
        layer, inst, proof, _, pkw = case(name)
        proto = product_protocol(layer)
        if isinstance(proto, dict):
            path = os.path.join(d, "protocol_layer%d.json" % layer)
            json.dump(proto, open(path, "w"), separators=(",", ":")); proto = path
        e = {"protocol": proto, "proof": put("proof%d.bin" % i, proof), "instances": put("inst%d.bin" % i, b"".join(int(v).to_bytes(32, "big") for v in inst)), "transcript": pkw["transcript"]}
        if "preprocessed" in pkw:
            e["preprocessed"] = put("pre%d.bin" % i, np.ascontiguousarray(pkw["preprocessed"], dtype=np.uint64).tobytes())
            e["initial_state"] = "%x" % pkw["initial_state"]
        man["proofs"].append(e)
    json.dump(man, open(os.path.join(d, "manifest.json"), "w"))
    recs = run(exe, "--manifest", os.path.join(d, "manifest.json"))
    assert recs[-1] == {"released": 10, "programs": 3}                       # the chunk proofs, the batch proofs, the bundle proof
    assert sorted(r["jobs"] for r in recs[:-1]) == [1, 2, 7] and all(r["inversions"] == 1 for r in recs[:-1])
