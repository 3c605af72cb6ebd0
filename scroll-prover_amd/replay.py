"""
replay.py -- host-side driver of the compiled create_proof replay (tests/cpp/test_plonk_replay.cpp): writes a layer's PlonkProtocol (protocols.py), runs the
program as its own process and returns what it wrote -- the proof, the verifying key, the instance values (bytes in the reference's layouts) and the program's
JSON record.  Used by tests/ and bench.py, which then hand the bytes to the verifier (oracle/plonk.py, checker only); nothing here imports the oracle.
"""
from __future__ import annotations

import json
import os
import subprocess
import tempfile
import time

from . import protocols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exe_path() -> str:
    from . import build
    return build.build_cpp("test_plonk_replay")


def write_protocol(layer: int, directory: str, k: int | None = None, protocol_file: str | None = None, **shape) -> str:
    """protocol_file: prove a given PlonkProtocol JSON as it stands (the reference's fixtures under tests/golden/); otherwise the layer's generated protocol"""
    if protocol_file:
        return protocol_file
    path = os.path.join(directory, f"layer{layer}_protocol.json")
    with open(path, "w") as f:
        json.dump(protocols.layer_protocol(layer, k, **shape), f, separators=(",", ":"))
    return path


def run(layer: int, k: int | None = None, out_dir: str | None = None, args=(), env=None, timeout: int = 1800, protocol_file: str | None = None, **shape) -> dict:
    """shape: what protocols.layer_protocol takes besides layer and k; lookup_argument="permuted" proves the layer's circuit under the classic halo2 lookup argument
    (the protocol file decides what the program proves: it takes no flag for it)"""
    out_dir = out_dir or tempfile.mkdtemp(prefix=f"mi355_replay_l{layer}_")
    os.makedirs(out_dir, exist_ok=True)
    proto = write_protocol(layer, out_dir, k, protocol_file, **shape)
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    out = subprocess.run([exe_path(), "--protocol", proto, "--out", out_dir] + list(args), capture_output=True, text=True, timeout=timeout, env=e)
    wall = time.perf_counter() - t0
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    rec = {"layer": layer, "ok": False, "returncode": out.returncode, "out_dir": out_dir, "protocol_path": proto, "process_wall_s": wall}
    if out.returncode != 0 or line is None:
        rec["error"] = (out.stdout + out.stderr)[-1200:]
        return rec
    rec.update(json.loads(line))
    rec["process_wall_s"] = wall
    for name in ("proof", "vk", "instances"):
        p = os.path.join(out_dir, name + ".bin")
        if os.path.exists(p):
            with open(p, "rb") as f:
                rec[name] = f.read()
    return rec


def run_process(layers, ks=None, out_dir: str | None = None, args=(), env=None, timeout: int = 2400, shapes=None) -> dict:
    """tests/cpp/test_prover_process.cpp: ONE process holding the SRS, proving keys and witnesses of several layers (a chunk prover {0, 1, 2}, a batch prover {3, 4}), under the HBM
    plan of plan_residency, proofs back to back.  Returns the program's record with, per layer, the bytes it wrote."""
    from . import build
    out_dir = out_dir or tempfile.mkdtemp(prefix="mi355_prover_process_")
    os.makedirs(out_dir, exist_ok=True)
    protos = []
    for i, layer in enumerate(layers):
        fx = os.path.join(ROOT, "tests", "golden", f"protocol_layer{layer}.json")
        k = (ks or {}).get(layer)
        protos.append(fx if (os.path.exists(fx) and not k) else write_protocol(layer, out_dir, k, None, **((shapes or {}).get(layer) or {})))
    cmd = [build.build_cpp("test_prover_process"), "--out", out_dir] + [x for p in protos for x in ("--protocol", p)] + list(args)
    e = dict(os.environ); e.update(env or {})
    t0 = time.perf_counter()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=e)
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    rec = {"ok": False, "returncode": out.returncode, "out_dir": out_dir, "protocol_paths": protos, "process_wall_s": time.perf_counter() - t0}
    if out.returncode != 0 or line is None:
        rec["error"] = (out.stdout + out.stderr)[-1200:]
        return rec
    rec.update(json.loads(line))
    for i, lay in enumerate(rec["layers"]):
        for name in ("proof", "vk", "instances"):
            with open(os.path.join(out_dir, str(i), name + ".bin"), "rb") as f:
                lay[name] = f.read()
        lay["protocol_path"] = protos[i]
    return rec


def run_lookup_multiplicities(layer: int, k: int | None = None, out_dir: str | None = None, args=(), env=None, timeout: int = 1800, protocol_file: str | None = None, **shape) -> dict:
    """tests/cpp/test_lookup_multiplicities.cpp: one layer proven by the default route (the builder's multiplicity columns handed in) and by the device route
    (ProofOptions::device_multiplicities, the m columns emptied).  Returns the program's record with `proof` (device route), `proof_default`, `vk` and `instances`;
    args: "--rule last", "--corrupt-lookup", "--devices D"."""
    from . import build
    out_dir = out_dir or tempfile.mkdtemp(prefix=f"mi355_lookup_m_l{layer}_")
    os.makedirs(out_dir, exist_ok=True)
    proto = write_protocol(layer, out_dir, k, protocol_file, **shape)
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    out = subprocess.run([build.build_cpp("test_lookup_multiplicities"), "--protocol", proto, "--out", out_dir] + list(args), capture_output=True, text=True, timeout=timeout, env=e)
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    rec = {"layer": layer, "ok": False, "returncode": out.returncode, "out_dir": out_dir, "protocol_path": proto, "process_wall_s": time.perf_counter() - t0}
    if line is None:
        rec["error"] = (out.stdout + out.stderr)[-1200:]
        return rec
    rec.update(json.loads(line))
    rec["returncode"] = out.returncode
    for name in ("proof", "proof_default", "vk", "instances"):
        p = os.path.join(out_dir, name + ".bin")
        if os.path.exists(p):
            with open(p, "rb") as f:
                rec[name] = f.read()
    return rec


def run_permutation_keygen(layer: int, k: int | None = None, out_dir: str | None = None, args=(), env=None, timeout: int = 1800, protocol_file: str | None = None, **shape) -> dict:
    """tests/cpp/test_permutation_keygen.cpp: one layer's key and one proof by the default route (Circuit::sigma_column on the host, every sigma column uploaded) and by
    the device route (keygen(..., device_sigma = true): one mi355_fr_permutation_sigma_dev call).  Returns the program's record with `vk_host`, `vk_device`,
    `proof_host`, `proof_device` and `instances`; args: "--keygen-only"."""
    from . import build
    out_dir = out_dir or tempfile.mkdtemp(prefix=f"mi355_perm_keygen_l{layer}_")
    os.makedirs(out_dir, exist_ok=True)
    proto = write_protocol(layer, out_dir, k, protocol_file, **shape)
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    out = subprocess.run([build.build_cpp("test_permutation_keygen"), "--protocol", proto, "--out", out_dir] + list(args), capture_output=True, text=True, timeout=timeout, env=e)
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    rec = {"layer": layer, "ok": False, "returncode": out.returncode, "out_dir": out_dir, "protocol_path": proto, "process_wall_s": time.perf_counter() - t0}
    if out.returncode != 0 or line is None:
        rec["error"] = (out.stdout + out.stderr)[-1200:]
        return rec
    rec.update(json.loads(line))
    for name in ("vk_host", "vk_device", "proof_host", "proof_device", "instances"):
        p = os.path.join(out_dir, name + ".bin")
        if os.path.exists(p):
            with open(p, "rb") as f:
                rec[name] = f.read()
    return rec


def run_witness_check(layer: int, k: int | None = None, out_dir: str | None = None, args=(), env=None, timeout: int = 1800, protocol_file: str | None = None, **shape) -> dict:
    """tests/cpp/test_witness_check.cpp: plonk::check_witness (MockProver::verify on the device) on the builder's instance of one layer, with the cells named by
    "--corrupt advice:<col>:<row>" / "--corrupt instance:<i>" changed first.  Returns the program's record with `check` (check.json: check_ms and the failures) and, under
    "--prove", `prove` (prove.json), `proof`, `proof_plain`, `vk` and `instances`; the dumped inputs are in `out_dir`.  args: "--builder-only" (no device), "--cap N"."""
    from . import build
    out_dir = out_dir or tempfile.mkdtemp(prefix=f"mi355_witness_check_l{layer}_")
    os.makedirs(out_dir, exist_ok=True)
    proto = write_protocol(layer, out_dir, k, protocol_file, **shape)
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    out = subprocess.run([build.build_cpp("test_witness_check"), "--protocol", proto, "--out", out_dir] + list(args), capture_output=True, text=True, timeout=timeout, env=e)
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    rec = {"layer": layer, "ok": False, "returncode": out.returncode, "out_dir": out_dir, "protocol_path": proto, "process_wall_s": time.perf_counter() - t0}
    if out.returncode != 0 or line is None:
        rec["error"] = (out.stdout + out.stderr)[-1200:]
        return rec
    rec.update(json.loads(line))
    rec["ok"] = True
    for name in ("check", "prove"):
        p = os.path.join(out_dir, name + ".json")
        if os.path.exists(p):
            with open(p) as f:
                rec[name] = json.load(f)
    for name in ("proof", "proof_plain", "vk", "instances"):
        p = os.path.join(out_dir, name + ".bin")
        if os.path.exists(p):
            with open(p, "rb") as f:
                rec[name] = f.read()
    return rec


def run_device_randomness(layer: int, key: bytes, k: int | None = None, out_dir: str | None = None, args=(), env=None, timeout: int = 1800, protocol_file: str | None = None, **shape) -> dict:
    """tests/cpp/test_device_randomness.cpp: one layer proven by the default route and, the witness's random fields emptied, with ProofOptions::device_randomness under
    `key` (32 bytes).  Returns the program's record with `proof`, `proof_again` (the same key once more), `proof_off` (default route), `vk`, `instances` and, when asked
    for, `proof_key2` ("--key2 HEX") and `proof_os1` / `proof_os2` ("--os-key"); the dumped inputs are in `out_dir`.  args: "--device-multiplicities", "--sparse-uploads",
    "--check-witness", "--devices D", "--proofs N", "--builder-key"."""
    from . import build
    assert len(key) == 32
    out_dir = out_dir or tempfile.mkdtemp(prefix=f"mi355_device_randomness_l{layer}_")
    os.makedirs(out_dir, exist_ok=True)
    proto = write_protocol(layer, out_dir, k, protocol_file, **shape)
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    out = subprocess.run([build.build_cpp("test_device_randomness"), "--protocol", proto, "--out", out_dir, "--key", key.hex()] + list(args), capture_output=True, text=True, timeout=timeout, env=e)
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    rec = {"layer": layer, "ok": False, "returncode": out.returncode, "out_dir": out_dir, "protocol_path": proto, "process_wall_s": time.perf_counter() - t0}
    if out.returncode != 0 or line is None:
        rec["error"] = (out.stdout + out.stderr)[-1200:]
        return rec
    rec.update(json.loads(line))
    for name in ("proof", "proof_again", "proof_off", "proof_key2", "proof_os1", "proof_os2", "vk", "instances"):
        p = os.path.join(out_dir, name + ".bin")
        if os.path.exists(p):
            with open(p, "rb") as f:
                rec[name] = f.read()
    return rec


def run_hbm_budget(layer: int, k: int | None = None, out_dir: str | None = None, args=(), env=None, timeout: int = 1800, protocol_file: str | None = None, **shape) -> dict:
    """tests/cpp/test_hbm_budget.cpp: one layer's instance proven in ONE process by the ungrouped route and with ProofOptions::coset_group_polys ("--group G|all"), each
    proof's high-water mark read from the library's ledger (mi355_mem_usage).  Returns the program's record with `proof_ungrouped`, `proof_grouped`, `vk` and `instances`.
    args: "--pk-cosets on-the-fly", "--devices D", "--device-multiplicities", "--fit" (the limit set midway between the two peaks: record["fit"]), "--bench N --groups 0,all,64"."""
    from . import build
    out_dir = out_dir or tempfile.mkdtemp(prefix=f"mi355_hbm_budget_l{layer}_")
    os.makedirs(out_dir, exist_ok=True)
    proto = write_protocol(layer, out_dir, k, protocol_file, **shape)
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    out = subprocess.run([build.build_cpp("test_hbm_budget"), "--protocol", proto, "--out", out_dir] + list(args), capture_output=True, text=True, timeout=timeout, env=e)
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    rec = {"layer": layer, "ok": False, "returncode": out.returncode, "out_dir": out_dir, "protocol_path": proto, "process_wall_s": time.perf_counter() - t0}
    if out.returncode != 0 or line is None:
        rec["error"] = (out.stdout + out.stderr)[-1200:]
        return rec
    rec.update(json.loads(line))
    for name in ("proof_ungrouped", "proof_grouped", "vk", "instances"):
        p = os.path.join(out_dir, name + ".bin")
        if os.path.exists(p):
            with open(p, "rb") as f:
                rec[name] = f.read()
    return rec
