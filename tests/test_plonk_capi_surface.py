"""CPU-only: the mi355_plonk_* entry points (include/mi355zk.h; csrc/lib_plonk.cpp) through scroll-prover_amd/prover.py, as far as they go without a device: the surface
(declared, exported, bound; the headers' C++ private to the library), protocol_info against oracle/plonk.py, the handle rules, the circuit builder and circuit_set / _get byte
for byte against the dump of tests/cpp/test_plonk_replay.cpp, MI355_ENODEVICE for keygen and create_proof in a process without a device, and host-only verification in process
against the oracle and against the child-process halo2.verify_proof."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk

from plonk_capi_common import GOLD, ROOT, SMALL0, dump_bytes, fixture_dict
from verify_common import R, case, layout, oracle_verify, product_protocol, same_as_oracle
from oracle import pyref

NAMES = ["mi355_plonk_protocol_from_json", "mi355_plonk_protocol_from_file", "mi355_plonk_protocol_info", "mi355_plonk_free", "mi355_plonk_circuit_new", "mi355_plonk_circuit_synthetic",
         "mi355_plonk_circuit_set", "mi355_plonk_circuit_get", "mi355_plonk_keygen", "mi355_plonk_pk_vk", "mi355_plonk_options_new", "mi355_plonk_options_set", "mi355_plonk_create_proof",
         "mi355_plonk_check_witness", "mi355_plonk_verify_proofs", "mi355_plonk_record_json"]


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def pv(zk):
    return zk.prover


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


def raises_badarg(zk, call, *needles):
    with pytest.raises(zk.Mi355Error) as e:
        call()
    assert e.value.code == zk._capi.EBADARG, e.value
    for n in needles:
        assert n in str(e.value), (n, str(e.value))
    return str(e.value)


# ------------------------------------------------------------------------------------------------ 1. surface
def test_every_plonk_entry_point_is_declared_exported_and_bound(zk):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355zk.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(mi355_plonk_\w+)\s*\(", txt)))
    assert declared == sorted(NAMES)
    assert sorted(n for n in zk._capi.SIGNATURES if n.startswith("mi355_plonk_")) == sorted(NAMES)
    lib = zk._capi.lib()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} not exported by libmi355zk.so"
    rust = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    for n in NAMES:
        assert re.search(r"pub fn " + n + r"\(", rust), f"{n} missing from rust_shim/mi355zk.rs"
    assert "lib_plonk" in ge._build_module().UNITS


def test_the_headers_cpp_stays_private_to_the_library(zk):
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", zk._capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    leaked = [l for l in out.splitlines() if "mi355zk::plonk" in l or "mi355zk::halo2" in l]
    assert not leaked, leaked[:5]
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NAMES) <= exported


def test_the_unit_hash_covers_the_public_headers(zk):
    b = ge._build_module()
    seen = {}
    b._closure(b._unit_source("lib_plonk"), seen)
    names = {os.path.basename(p) for p in seen}
    assert {"mi355zk_plonk.hpp", "mi355zk_plonk_circuit.hpp", "mi355zk_plonk_protocol.hpp", "mi355zk_plonk_verify.hpp", "mi355zk_transcript.hpp", "mi355zk_halo2.hpp", "mi355zk.h", "plonk_capi.hpp", "fp.hpp"} <= names


# ------------------------------------------------------------------------------------------------ 2. protocol info
def check_info(pv, handle, d, layer):
    pr = plonk.Protocol(d)
    info = handle.info()
    nw = sum(pr.num_witness)
    assert (info["k"], info["n"]) == (pr.k, pr.n)
    assert info["num_preprocessed"] == pr.num_pre and info["num_instance"] == pr.num_instance[0]
    assert (info["num_advice"], info["num_lookups"], info["num_witness"]) == (pr.num_witness[0], pr.num_witness[1], nw)
    assert info["num_perm_chunks"] + info["num_lookups"] + 1 == pr.num_witness[2]
    assert (info["blind"], info["usable"], info["quotient_pieces"], info["extended_k"]) == (pr.blind, pr.usable, pr.Q, pr.ext_k)
    assert info["num_evaluations"] == len(pr.evaluations) and info["num_queries"] == len(pr.queries)
    assert info["num_commitments"] == nw + pr.Q + 2
    assert info["proof_bytes_poseidon"] == 32 * (nw + pr.Q + 2 + len(pr.evaluations)) and info["proof_bytes_evm"] == 64 * (nw + pr.Q + 2) + 32 * len(pr.evaluations)
    assert info["layer"] == layer
    root = d.get("protocol", d)
    assert info["has_initial_state"] == (1 if isinstance(root.get("transcript_initial_state"), list) else 0)
    assert info["has_accumulator"] == (1 if root.get("accumulator_indices") else 0)
    assert handle.info("num_perm_columns") >= info["num_perm_chunks"]
    return info


@pytest.mark.parametrize("layer", [2, 4])
def test_protocol_info_of_the_reference_fixtures(pv, layer):
    d = fixture_dict(layer)
    with pv.Protocol.from_file(os.path.join(GOLD, f"protocol_layer{layer}.json")) as p, pv.Protocol.from_json(d) as q:
        info = check_info(pv, p, d, d.get("protocol", d).get("layer", -1))
        assert q.info() == info                                        # the same protocol from text
        assert info["proof_bytes_poseidon"] == (896 if layer == 2 else 1312)
        assert info["has_accumulator"] == 1 and info["has_initial_state"] == 1


@pytest.mark.parametrize("layer", range(7))
def test_protocol_info_of_the_generated_layers(zk, pv, layer):
    d = zk.protocols.layer_protocol(layer, 7, **(SMALL0 if layer == 0 else {}))
    with pv.Protocol.from_json(d) as p:
        info = check_info(pv, p, d, layer)
    if layer in (2, 6):
        assert info["proof_bytes_poseidon"] == 896 and info["proof_bytes_evm"] == 1248
    if layer == 4:
        assert info["proof_bytes_poseidon"] == 1312


# ------------------------------------------------------------------------------------------------ 3. handles
def test_malformed_json_is_ebadarg_with_a_message(zk, pv):
    good = json.dumps(zk.protocols.layer_protocol(2, 6), separators=(",", ":"))
    for text in ["", "{", "[1, 2", good[:-1], good[: len(good) // 2], good + "x", "nul", '{"domain": 5}', '{"a": "unterminated', "[" * 10000, good.replace('"k":6', '"k":6.5'), good.replace('"k":6', '"k":99')]:
        msg = raises_badarg(zk, lambda: pv.Protocol.from_json(text), "mi355_plonk_protocol_from_json")
        assert len(msg) > 40
    raises_badarg(zk, lambda: pv.Protocol.from_file("/nonexistent/protocol.json"), "cannot open")
    d = zk.protocols.layer_protocol(2, 6); d["num_witness"] = [1, 1]
    raises_badarg(zk, lambda: pv.Protocol.from_json(d), "protocol:")


def test_freed_foreign_and_wrong_kind_handles_are_ebadarg(zk, pv):
    lib, capi = zk._capi.lib(), zk._capi
    p = pv.Protocol.from_json(zk.protocols.layer_protocol(2, 6))
    o = pv.Options(threads=3)
    v, h = C.c_uint64(), C.c_uint64()
    # a wrong kind, with the expected kind named
    assert lib.mi355_plonk_protocol_info(o.handle, b"k", C.byref(v)) == capi.EBADARG and b"options handle, a protocol handle is expected" in lib.mi355_last_error()
    assert lib.mi355_plonk_options_set(p.handle, b"threads", b"1") == capi.EBADARG and b"protocol handle, a options handle is expected" in lib.mi355_last_error()
    assert lib.mi355_plonk_circuit_new(o.handle, C.byref(h)) == capi.EBADARG and lib.mi355_plonk_record_json(p.handle, None, 0, C.byref(v)) == capi.EBADARG
    assert lib.mi355_plonk_circuit_get(p.handle, b"advice", 0, None, 0, C.byref(v)) == capi.EBADARG and b"circuit handle is expected" in lib.mi355_last_error()
    # never issued
    for bad in (0, 10**15, 2**64 - 1):
        assert lib.mi355_plonk_protocol_info(bad, b"k", C.byref(v)) == capi.EBADARG and b"never issued" in lib.mi355_last_error()
        assert lib.mi355_plonk_free(bad) == capi.EBADARG and b"never issued" in lib.mi355_last_error()
    # freed, then freed again
    ph = p.handle
    p.close()
    assert lib.mi355_plonk_protocol_info(ph, b"k", C.byref(v)) == capi.EBADARG and b"already freed" in lib.mi355_last_error()
    assert lib.mi355_plonk_free(ph) == capi.EBADARG and b"already freed" in lib.mi355_last_error()
    p.close()                                                          # the Python object frees once
    o.close()


def test_a_handle_value_is_never_issued_twice(zk, pv):
    seen = []
    d = zk.protocols.layer_protocol(2, 6)
    for _ in range(6):
        p = pv.Protocol.from_json(d); o = pv.Options(); c = pv.Circuit(p)
        seen += [p.handle, o.handle, c.handle]
        for x in (c, o, p):
            x.close()
    assert len(set(seen)) == len(seen) and seen == sorted(seen) and min(seen) > 0


def test_a_circuit_keeps_its_protocol_alive(zk, pv):
    p = pv.Protocol.from_json(zk.protocols.layer_protocol(2, 6))
    c = pv.Circuit.synthetic(p, seed=3)
    want = c.get_bytes("advice", 0)
    p.close()                                                          # allowed: the handle dies, the circuit holds the protocol
    assert c.get_bytes("advice", 0) == want and len(c.get_bytes("preprocessed", 0)) == 32 * 64
    c.close()


def test_unknown_option_names_fields_and_values_are_named(zk, pv):
    p = pv.Protocol.from_json(zk.protocols.layer_protocol(2, 6))
    raises_badarg(zk, lambda: p.info("no_such_field"), "no_such_field")
    o = pv.Options()
    raises_badarg(zk, lambda: o.set("no_such_option", 1), "no_such_option")
    raises_badarg(zk, lambda: o.set("rng_key", "zz" * 32), "rng_key", "64 hexadecimal digits")
    raises_badarg(zk, lambda: o.set("rng_key", "00" * 31), "rng_key")
    raises_badarg(zk, lambda: o.set("initial_state", "0x12"), "initial_state")
    raises_badarg(zk, lambda: o.set("threads", "many"), "threads")
    raises_badarg(zk, lambda: o.set("threads", 0), "threads")
    raises_badarg(zk, lambda: o.set("transcript", "sha256"), "transcript")
    raises_badarg(zk, lambda: o.set("sparse_uploads", "maybe"), "sparse_uploads")
    for name, value in [("devices", 1), ("threads", 4), ("commit_batch", 0), ("upload_threads", 2), ("early_intt", -1), ("sparse_uploads", True), ("packed_multiplicities", False),
                        ("device_multiplicities", True), ("multiplicity_rule_last", False), ("check_witness", True), ("device_randomness", False), ("rng_key", bytes(range(32))),
                        ("rng_key_from_os", False), ("coset_group_polys", 24), ("transcript", "poseidon"), ("check_accumulator", False), ("accumulator", 1), ("host_only", True),
                        ("device_transcript", False), ("initial_state", 12345), ("cap", 16), ("theta_seed", 2**64 - 1)]:
        o.set(name, value)
    o.close(); p.close()


# ------------------------------------------------------------------------------------------------ 4. the builder through the ABI
@pytest.mark.parametrize("layer,k,shape", [(2, 7, {}), (4, 8, {}), (0, 7, SMALL0)])
def test_circuit_synthetic_equals_the_replays_dump(zk, pv, tmp_path, layer, k, shape):
    rec = zk.replay.run(layer, k, out_dir=str(tmp_path), args=["--builder-only", "--dump-inputs"], **shape)
    assert rec["returncode"] == 0 and rec.get("builder_only"), rec
    with pv.Protocol.from_file(rec["protocol_path"]) as p, pv.Circuit.synthetic(p) as c, pv.Circuit.synthetic(p) as again, pv.Circuit.synthetic(p, seed=2) as other:
        got = dump_bytes(c, p.info())
        for name, data in got.items():
            with open(os.path.join(str(tmp_path), name), "rb") as f:
                want = f.read()
            assert data == want, f"{name}: circuit_get differs from the replay's dump ({len(data)} vs {len(want)} bytes)"
        assert dump_bytes(again, p.info()) == got                      # the same arguments, the same instance
        assert dump_bytes(other, p.info())["advice.bin"] != got["advice.bin"]
        man = json.load(open(os.path.join(str(tmp_path), "manifest.json")))
        assert len(c.get("copies")) == man["copy_pairs"] and len(c.get("instances")) == man["num_instance"]


def test_circuit_set_then_get_round_trips_and_sizes_are_checked(zk, pv):
    d = zk.protocols.layer_protocol(4, 6)
    rng = np.random.default_rng(7)
    with pv.Protocol.from_json(d) as p, pv.Circuit(p) as c, pv.Circuit.synthetic(p) as s:
        info = p.info(); n, blind = info["n"], info["blind"]
        assert c.get_bytes("advice", 0) == bytes(32 * n) and len(c.get("copies")) == 0 and len(c.get("instances")) == 0      # a new circuit: zero columns, nothing else
        words = lambda rows: rng.integers(0, 2**60, size=(rows, 4), dtype=np.uint64)
        sigma = [i for i in range(info["num_preprocessed"]) if c.get_bytes("preprocessed", i) != bytes(32 * n)]     # a new circuit: fixed columns zero, sigma columns the identity
        fixed = [i for i in range(info["num_preprocessed"]) if i not in sigma]
        parts = [("advice", info["num_advice"] - 1, words(n)), ("m", 0, words(n)), ("m_blind", info["num_lookups"] - 1, words(blind)), ("z_blind", info["num_perm_chunks"] - 1, words(blind)),
                 ("phi_blind", 0, words(blind)), ("random_poly", 0, words(n)), ("instances", 0, words(info["num_instance"])), ("instances", 0, words(3)), ("preprocessed", fixed[0], words(n)),
                 ("copies", 0, np.array([[0, 1, 1, 2], [info["num_perm_columns"] - 1, n - 1, 0, 0]], dtype=np.uint64))]
        for what, i, data in parts:
            c.set(what, i, data)
            assert c.get_bytes(what, i) == data.tobytes(), what
        counts = rng.integers(0, 2**31, size=n, dtype=np.uint32)
        c.set("m_counts", 0, counts); assert (c.get("m_counts", 0) == counts).all()
        # the sigma columns follow from the copies: cell (0, 1) <-> (1, 2) swapped their images
        assert len(sigma) == info["num_perm_columns"]
        before = c.get("preprocessed", sigma[0]).copy()
        c.set("copies", 0, np.zeros((0, 4), dtype=np.uint64))
        after = c.get("preprocessed", sigma[0])
        assert (before[1] != after[1]).any() and (np.delete(before, [0, 1], axis=0) == np.delete(after, [0, 1], axis=0)).all()
        # wrong sizes, indices and names
        raises_badarg(zk, lambda: c.set("advice", 0, words(n - 1)), "advice", str(32 * n))
        raises_badarg(zk, lambda: c.set("advice", info["num_advice"], words(n)), "out of range")
        raises_badarg(zk, lambda: c.set("z_blind", 0, words(blind + 1)), "z_blind")
        raises_badarg(zk, lambda: c.set("m_counts", 0, words(n)), "m_counts")
        raises_badarg(zk, lambda: c.set("instances", 0, words(info["num_instance"] + 1)), "instances")
        raises_badarg(zk, lambda: c.set("instances", 0, b"x" * 33), "instances")
        raises_badarg(zk, lambda: c.set("copies", 0, np.array([[info["num_perm_columns"], 0, 0, 0]], dtype=np.uint64)), "outside the permutation")
        raises_badarg(zk, lambda: c.set("copies", 0, np.array([[0, n, 0, 0]], dtype=np.uint64)), "outside the permutation")
        raises_badarg(zk, lambda: c.set("preprocessed", sigma[0], words(n)), "sigma column")
        raises_badarg(zk, lambda: c.set("witness", 0, words(n)), "witness")
        raises_badarg(zk, lambda: c.get_bytes("witness", 0), "witness")
        assert c.get_bytes("advice", 0) == bytes(32 * n)               # every refused call left the circuit as it was
        n_out = C.c_uint64()
        small = (C.c_uint8 * 16)()
        assert zk._capi.lib().mi355_plonk_circuit_get(c.handle, b"random_poly", 0, C.cast(small, C.c_void_p), 16, C.byref(n_out)) == zk._capi.EBADARG and n_out.value == 32 * n


# ------------------------------------------------------------------------------------------------ 5. without a device
def test_keygen_and_create_proof_without_a_device_are_enodevice():
    code = """
import ctypes as C
import __graft_entry__ as ge
zk = ge.load_package()
pv, capi, lib = zk.prover, zk._capi, zk._capi.lib()
p = pv.Protocol.from_json(zk.protocols.layer_protocol(2, 6))
c = pv.Circuit.synthetic(p)
h, n = C.c_uint64(), C.c_uint64()
buf = (C.c_uint8 * 2048)()
assert lib.mi355_plonk_keygen(p.handle, c.handle, 1, 1, 1, C.byref(h)) == capi.ENODEVICE, lib.mi355_last_error()
assert b"no gfx950 device bound" in lib.mi355_last_error()
assert lib.mi355_plonk_create_proof(1, 2, 12345, c.handle, 0, C.cast(buf, C.c_void_p), 2048, C.byref(n), None) == capi.ENODEVICE
assert lib.mi355_plonk_check_witness(12345, c.handle, 0, C.byref(n), None) == capi.ENODEVICE
try:
    pv.keygen(p, c, 1)
except zk.Mi355Error as e:
    assert e.code == capi.ENODEVICE
else:
    raise AssertionError("keygen returned without a device")
ok = (C.c_uint8 * 1)()
assert lib.mi355_plonk_verify_proofs(0, None, None, None, None, None, None, None, None, None, 0, 0, 0, ok, None) == capi.ENODEVICE
assert c.get_bytes("advice", 0) and p.info("k") == 6        # the process lives and the objects still answer
print("enodevice-ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "enodevice-ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ 6. host-only verification in process
def in_process(zk, pv, name, inst, proof, **over):
    """the released proof `name` through mi355_plonk_verify_proofs with host_only; the product keywords of verify_common.case become a key and options"""
    layer, _, _, okw, pkw = case(name)
    kw = dict(pkw); kw.update(over)
    pd = product_protocol(layer)
    p = pv.Protocol.from_file(pd) if isinstance(pd, str) else pv.Protocol.from_json(pd)
    vk = None
    if "preprocessed" in kw:                                           # the bundle proof's key: the .vkey bytes carry the same seven commitments
        kw.pop("preprocessed"); vk = bytes.fromhex(json.load(open(os.path.join(GOLD, "kat.json")))["vk_bundle"])
    opts = dict(host_only=True, **kw)
    return pv.verify_proofs([{"protocol": p, "instances": inst, "proof": proof, "vk_bytes": vk}], options=opts), p


@pytest.mark.parametrize("name", ["chunk_proof", "batch_proof", "bundle_proof"])
def test_host_only_verification_in_process_equals_the_oracle_and_the_child_process(zk, pv, name):
    layer, inst, proof, okw, pkw = case(name)
    want = oracle_verify(layer, inst, proof, okw)
    assert want["ok"], want
    (got,), p = in_process(zk, pv, name, inst, proof)
    assert got["ok"] and got["error"] == "" and got["host_only"] and got["has_accumulator"], got
    same_as_oracle(got, want)
    child = zk.halo2.verify_proof(product_protocol(layer), inst, proof, host_only=True, **pkw)
    assert got.pop("device_calls") == 0
    assert got == child                                                # field for field: ok, error, detail, challenges, numerator_at_x, msm, has_accumulator, pairing
    one, _ = pv.verify_proofs([{"protocol": p, "instances": inst, "proof": proof, "vk_bytes": bytes.fromhex(json.load(open(os.path.join(GOLD, "kat.json")))["vk_bundle"]) if name == "bundle_proof" else None}],
                              options=dict(host_only=True, **{k: v for k, v in pkw.items() if k != "preprocessed"}), one_by_one=True), None
    one[0].pop("device_calls"); assert one[0] == child                 # mode 1, the loop of verify_proof, gives the same record
    p.close()


@pytest.mark.parametrize("name", ["chunk_proof", "bundle_proof"])
def test_named_failures_stay_the_same_in_process(zk, pv, name):
    layer, inst, proof, okw, pkw = case(name)
    coms, evs, shp, nb = layout(layer, okw["transcript"])

    def both(i, pf, **over):
        (got,), p = in_process(zk, pv, name, i, pf, **over); p.close()
        child = zk.halo2.verify_proof(product_protocol(layer), i, pf, host_only=True, **dict(pkw, **over))
        got.pop("device_calls")
        assert got == child
        return got
    got = both(inst, proof[:-32]); assert not got["ok"] and got["error"] == "proof_length"
    got = both(inst, proof + bytes(32)); assert not got["ok"] and got["error"] == "proof_length"
    bad = bytearray(proof); bad[evs[3]:evs[3] + 32] = R.to_bytes(32, "big" if nb == 64 else "little")
    got = both(inst, bytes(bad)); assert not got["ok"] and got["error"] == "non_canonical_scalar" and "evaluation 3" in got["detail"]
    bad = bytearray(proof)
    if nb == 64:
        bad[coms[2] + 63] ^= 1
    else:
        bad[coms[2]:coms[2] + 32] = not_a_point_word(proof[coms[2]:coms[2] + 32])
    got = both(inst, bytes(bad)); assert not got["ok"] and got["error"] == "invalid_point" and "point 2 " in got["detail"]
    big = list(inst); big[4] |= 1 << 88
    got = both(big, proof); assert not got["ok"] and got["error"] == "accumulator_limb" and "instance 4" in got["detail"]
    got = both(big, proof, check_accumulator=False); assert got["ok"] and not got["has_accumulator"]


def test_a_batch_marks_only_the_rejected_proof(zk, pv):
    layer, inst, proof, okw, pkw = case("chunk_proof")
    with pv.Protocol.from_file(product_protocol(layer)) as p:
        cases = [{"protocol": p, "instances": inst, "proof": proof}, {"protocol": p, "instances": inst, "proof": proof[:-1]}, {"protocol": p, "instances": inst, "proof": proof}]
        recs = pv.verify_proofs(cases, options=dict(host_only=True, transcript="poseidon"))
        assert [r["ok"] for r in recs] == [True, False, True] and recs[1]["error"] == "proof_length"
        raises_badarg(zk, lambda: pv.aggregate(cases, options=dict(host_only=True)), "host_only")
        raises_badarg(zk, lambda: pv._verify_call(cases, 7, None, None, None, None, dict(host_only=True)), "mode")
