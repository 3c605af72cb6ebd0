"""helpers shared by tests/test_verify_proof_surface.py and tests/test_gpu_verify_proof.py (TEST INFRASTRUCTURE): the released proofs of tests/golden/kat.json as
(protocol, instances, proof, keyword arguments) for oracle/plonk.py verify() and for halo2.verify_proof, and the oracle's verdict with its assertions caught."""
import functools
import json
import os

import numpy as np

from oracle import plonk, pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
R, P = pyref.R_MOD, pyref.P_MOD
KAT = json.load(open(os.path.join(GOLD, "kat.json")))
NEG_S_G2 = pyref.g2_from_evm_words([int(w, 16) for w in KAT["yul"]["s_g2_words"]])
NEG_S_G2_WORDS = np.array(pyref.g2_to_limbs(NEG_S_G2), dtype=np.uint64)
words = lambda b: [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def fixture_path(layer):
    return os.path.join(GOLD, f"protocol_layer{layer}.json")


@functools.lru_cache(maxsize=None)
def oracle_protocol(layer):
    if layer == 6:
        import __graft_entry__ as ge
        return plonk.Protocol(ge.load_package().protocols.layer_protocol(6))
    d = json.load(open(fixture_path(layer)))
    return plonk.Protocol(d.get("protocol", d))


def g1_abi(points):
    return np.array([pyref.mont_limbs(x, P) + pyref.mont_limbs(y, P) for x, y in points], dtype=np.uint64)


def case(name):
    """-> (layer, instances, proof, oracle keywords, product keywords without the G2 points)"""
    if name == "bundle_proof":
        pd, pi = bytes.fromhex(KAT["bundle_proof_data"]), bytes.fromhex(KAT["bundle_pi_data"])
        vk = bytes.fromhex(KAT["vk_bundle"])
        pre = [pyref.g1_decompress(vk[8 + 32 * i:8 + 32 * i + 32]) for i in range(7)]
        st = int(KAT["yul"]["transcript_initial_state"])
        return (6, words(pd[:384]) + words(pi), pd[384:], dict(transcript="evm", preprocessed=pre, initial_state=st),
                dict(transcript="evm", preprocessed=g1_abi(pre), initial_state=st, accumulator=True))
    if name.startswith("more_chunk_proofs"):
        m = KAT["more_chunk_proofs"][int(name.split(":")[1])]
        layer = 2
    else:
        m, layer = KAT[name], 2 if name == "chunk_proof" else 4
    return layer, words(bytes.fromhex(m["instances"])), bytes.fromhex(m["proof"]), dict(transcript="poseidon"), dict(transcript="poseidon")


ALL_TEN = ["chunk_proof"] + [f"more_chunk_proofs:{i}" for i in range(6)] + ["batch_proof", "batch_proof_2", "bundle_proof"]


def product_protocol(layer):
    if layer == 6:
        import __graft_entry__ as ge
        return ge.load_package().protocols.layer_protocol(6)
    return fixture_path(layer)


def oracle_verify(layer, inst, proof, okw, **over):
    """the oracle's dictionary; an assertion inside it (an invalid word, a proof cut short) is a rejection"""
    kw = dict(okw); kw.update(over)
    try:
        return plonk.verify(oracle_protocol(layer), None, inst, proof, neg_s_g2=NEG_S_G2, **kw)
    except (AssertionError, IndexError, ValueError) as e:
        return {"ok": False, "error": "assertion: %s" % e}


def layout(layer, transcript):
    """byte offsets of the proof's words: (commitment offsets, evaluation offsets, SHPLONK point offsets, point size)"""
    pr = oracle_protocol(layer)
    nb = 64 if transcript == "evm" else 32
    nc, ne = sum(pr.num_witness) + pr.Q, len(pr.evaluations)
    return [nb * i for i in range(nc)], [nb * nc + 32 * j for j in range(ne)], [nb * nc + 32 * ne, nb * nc + 32 * ne + nb], nb


def same_as_oracle(got, want):
    assert got["challenges"]["theta"] == want["challenges"]["theta"] and got["challenges"]["beta"] == want["challenges"]["beta"]
    assert got["challenges"]["gamma"] == want["challenges"]["gamma"] and got["challenges"]["y"] == want["challenges"]["y"] and got["challenges"]["x"] == want["challenges"]["x"]
    assert got["numerator_at_x"] == want["numerator_at_x"]
    assert got["msm"]["scalars"] == [s % R for s in want["msm"]["scalars"]] and got["msm"]["points"] == [tuple(p) for p in want["msm"]["points"]]
    assert got["msm"]["w_prime"] == tuple(want["msm"]["w_prime"])
