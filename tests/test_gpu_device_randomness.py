"""-m gpu: create_proof with the prover's randomness drawn on the device (ProofOptions::device_randomness, tests/cpp/test_device_randomness.cpp).

The program proves a layer with the witness's random fields emptied and a given ChaCha20 key.  Here every drawn value -- the blinding rows of the advice and
multiplicity columns, the z / phi blinding values, the random polynomial -- is recomputed from the key and the stream table (tests/frrand_common.py: plain Python),
written into the dumped inputs, and the CPU restatement of create_proof (oracle/plonk.py) must give the device's bytes; the tree-walking verifier must accept them.
Another key gives other bytes that still verify, the same key the same bytes; with the option off the program's proof is the existing replay's; a key from the
operating system gives two different verifying proofs; the option composes with sparse uploads, the witness check and several upload threads."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk
from tests import frrand_common as fc

TAU0 = 0x5343524F4C4C0001
KEY = bytes.fromhex("8f3a1c5e7b9d0f21436587a9cbed0f1e2d3c4b5a69788796a5b4c3d2e1f00112")
KEY2 = bytes(reversed(KEY))
zk = ge.load_package()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    ge.build()


def verify(rec, proof):
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
    tau = TAU0 + (rec["layer"] if rec["layer"] >= 0 else 0)
    return plonk.verify(pr, rec["vk"], inst, proof, tau, transcript=rec["transcript"])["ok"]


def inputs_with_the_device_s_draws(directory, key):
    """the dumped inputs with every random value replaced by what the device draws under `key` (the stream table of include/mi355zk_plonk.hpp)"""
    inp, _ = plonk.ProofInputs.load(directory)
    pr = inp.pr
    n, b, u = pr.n, pr.blind, pr.usable
    assert u + 1 + b == n

    def rows(stream, index):
        return fc.elements_canonical(key, stream, index * b, b)
    for a in range(len(inp.advice)):
        inp.advice[a] = list(inp.advice[a][:u + 1]) + rows(fc.STREAM_ADVICE_BLIND, a)
    for l in range(len(inp.m)):
        inp.m[l] = list(inp.m[l][:u + 1]) + rows(fc.STREAM_M_BLIND, l)
    inp.z_blind = [rows(fc.STREAM_Z_BLIND, c) for c in range(len(inp.z_blind))]
    inp.phi_blind = [rows(fc.STREAM_PHI_BLIND, l) for l in range(len(inp.phi_blind))]
    inp.random_coeffs = fc.elements_canonical(key, fc.STREAM_RANDOM_POLY, 0, n)
    return inp


CASES = [(2, 7, [], {}), (4, 8, [], {}), (6, 7, [], {}),
         (4, 8, ["--devices", "2"], {"MI355_ALLOW_DUP_DEVICES": "1", "MI355_SHARD_MIN_LOG": "6"}),
         (4, 8, ["--device-multiplicities"], {})]


@pytest.mark.parametrize("layer,k,args,env", CASES, ids=["layer2_k7", "layer4_k8", "layer6_k7_keccak", "layer4_k8_two_devices", "layer4_k8_device_multiplicities"])
def test_device_proof_equals_the_cpu_restatement_fed_with_the_recomputed_draws(tmp_path, layer, k, args, env):
    rec = zk.replay.run_device_randomness(layer, KEY, k, out_dir=str(tmp_path), args=["--key2", KEY2.hex()] + args, env=env, timeout=600)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    inp = inputs_with_the_device_s_draws(str(tmp_path), KEY)
    vk = plonk.keygen_vk(inp.pr, inp.pre, inp.tau)
    assert rec["vk"] == vk
    assert rec["transcript"] == ("evm" if layer == 6 else "poseidon")
    assert rec["proof"] == plonk.prove(inp, vk, transcript=rec["transcript"]), "the device's proof differs from the CPU restatement fed with the recomputed draws"
    assert verify(rec, rec["proof"])
    assert rec["same_key_same_bytes"] and rec["proof_again"] == rec["proof"]
    assert rec["proof_key2"] != rec["proof"] and len(rec["proof_key2"]) == len(rec["proof"]) and verify(rec, rec["proof_key2"])
    assert rec["proof_off"] != rec["proof"] and verify(rec, rec["proof_off"])
    n, b, adv = 1 << k, rec["blind"], rec["advice"]
    assert rec["on"]["witness_link_bytes"] < rec["off"]["witness_link_bytes"]                       # no random polynomial, no blinding rows
    assert rec["off"]["witness_link_bytes"] - rec["on"]["witness_link_bytes"] >= 32 * n + 32 * b * adv
    assert rec["on"]["random_ms"] > 0 and rec["off"]["random_ms"] == 0


def test_option_off_is_the_existing_replay(tmp_path):
    a, b = tmp_path / "new", tmp_path / "replay"
    rec = zk.replay.run_device_randomness(2, KEY, 7, out_dir=str(a), timeout=600)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    old = zk.replay.run(2, 7, out_dir=str(b), args=["--proofs", "1"], timeout=600)
    assert old.get("ok"), old.get("error")
    assert rec["vk"] == old["vk"] and rec["proof_off"] == old["proof"], "the default route moved"


def test_key_from_the_operating_system(tmp_path):
    rec = zk.replay.run_device_randomness(2, KEY, 7, out_dir=str(tmp_path), args=["--os-key"], timeout=600)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    assert rec["proof_os1"] != rec["proof_os2"] and rec["proof"] not in (rec["proof_os1"], rec["proof_os2"])
    assert verify(rec, rec["proof_os1"]) and verify(rec, rec["proof_os2"])


def test_composes_with_sparse_uploads_the_witness_check_and_upload_threads(tmp_path):
    """k = 12: the smallest domain whose columns take the sparse form (4 096 rows).  Same key, same bytes as the plain device-randomness proof"""
    a, b = tmp_path / "composed", tmp_path / "plain"
    rec = zk.replay.run_device_randomness(4, KEY, 12, out_dir=str(a), args=["--sparse-uploads", "--check-witness", "--upload-threads", "3"], timeout=600)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    plain = zk.replay.run_device_randomness(4, KEY, 12, out_dir=str(b), timeout=600)
    assert plain.get("ok") and plain["returncode"] == 0, plain.get("error")
    assert rec["sparse_uploads"] and rec["check_witness"] and rec["proof"] == plain["proof"] and rec["proof_off"] == plain["proof_off"]
    assert verify(rec, rec["proof"])
