"""helpers shared by tests/test_plonk_capi_surface.py and tests/test_gpu_plonk_capi.py (TEST INFRASTRUCTURE): the circuit a mi355_plonk_* handle holds, read back through
mi355_plonk_circuit_get and handed to the CPU restatement of the prover (oracle/plonk.py ProofInputs), and the files tests/cpp/test_plonk_replay.cpp dumps for the same instance."""
import json
import os

import numpy as np

from oracle import plonk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SMALL0 = dict(advice=40, fixed=8, lookups=3, perm_columns=12, degree=5)      # layer 0's stand-in at a size a test can prove
TAU0 = 0x5343524F4C4C0001                                                      # the replay's toxic scalar is TAU0 + layer


def tau_of(layer: int) -> int:
    return TAU0 + max(layer, 0)


def dump_bytes(circuit, info: dict) -> dict:
    """the files dump_circuit writes (pre.bin, advice.bin, m.bin, instance.bin, z_blind.bin, phi_blind.bin, random.bin), rebuilt from circuit_get alone"""
    cat = lambda what, count: b"".join(circuit.get_bytes(what, i) for i in range(count))
    return {"pre.bin": cat("preprocessed", info["num_preprocessed"]), "advice.bin": cat("advice", info["num_advice"]), "m.bin": cat("m", info["num_lookups"]),
            "instance.bin": circuit.get_bytes("instances"), "z_blind.bin": cat("z_blind", info["num_perm_chunks"]), "phi_blind.bin": cat("phi_blind", info["num_lookups"]),
            "random.bin": circuit.get_bytes("random_poly")}


def proof_inputs(circuit, protocol_dict: dict, tau: int, info: dict) -> "plonk.ProofInputs":
    """oracle/plonk.py's ProofInputs from the handle: every column crosses the ABI through circuit_get (the sigma columns through sigma_column)"""
    pr = plonk.Protocol(protocol_dict)
    col = lambda what, i: plonk.mont_to_ints(circuit.get(what, i))
    L = info["num_lookups"]
    return plonk.ProofInputs(pr, [col("preprocessed", p) for p in range(info["num_preprocessed"])], col("instances", 0), [col("advice", a) for a in range(info["num_advice"])],
                             [col("m", l) for l in range(L)], [col("z_blind", c) for c in range(info["num_perm_chunks"])], [col("phi_blind", l) for l in range(L)],
                             col("random_poly", 0), tau)


def fixture_dict(layer: int) -> dict:
    return json.load(open(os.path.join(GOLD, f"protocol_layer{layer}.json")))


def to_mont(values) -> np.ndarray:
    return plonk.ints_to_mont(list(values))
