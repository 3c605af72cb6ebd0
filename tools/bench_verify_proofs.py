"""Batched against one-by-one verification (plonk::verify_proofs against a loop of plonk::verify_proof) through tests/cpp/test_verify_proofs --bench, which runs both modes in
ONE process after one warm-up call of each: on the ten released proofs, and on the seven chunk proofs tiled to 318 (the number of chunk proofs the reference stores).  Wall time:
median of 5 calls per mode.  Kernel figures (mi355_profile_get, HIP events) come from one further, profiled call per mode: the segmented MSM kernel, the decompression, the
pairing kernels, and `msm_total` -- the bucket pipeline of the ad-hoc MSM calls of the loop, whose share of the loop's profiled wall time is reported as adhoc_msm_share.
Prints one JSON line.  Not part of bench.py."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
from verify_common import ALL_TEN, NEG_S_G2_WORDS, case, product_protocol

RUNS = 5
zk = ge.load_package()
exe = ge.build_cpp("test_verify_proofs")


def manifest(d, names):
    put = lambda name, data: (open(os.path.join(d, name), "wb").write(data), os.path.join(d, name))[1]
    man = {"g2": put("g2.bin", zk.halo2.g2_generator().tobytes()), "neg_s_g2": put("nsg2.bin", NEG_S_G2_WORDS.tobytes()), "proofs": []}
    for i, name in enumerate(names):
        layer, inst, proof, _, pkw = case(name)
        proto = product_protocol(layer)
        if isinstance(proto, dict):
            path = os.path.join(d, "protocol_layer%d.json" % layer)
            json.dump(proto, open(path, "w"), separators=(",", ":")); proto = path
        e = {"protocol": proto, "proof": put("proof%d.bin" % i, proof), "instances": put("inst%d.bin" % i, b"".join(int(v).to_bytes(32, "big") for v in inst)), "transcript": pkw["transcript"]}
        if "preprocessed" in pkw:
            e["preprocessed"] = put("pre%d.bin" % i, np.ascontiguousarray(pkw["preprocessed"], dtype=np.uint64).tobytes())
            e["initial_state"] = "%x" % pkw["initial_state"]; e["accumulator"] = True
        man["proofs"].append(e)
    path = os.path.join(d, "manifest.json")
    json.dump(man, open(path, "w"))
    return path


def bench(names, tile=0):
    with tempfile.TemporaryDirectory(prefix="mi355_bench_verify_") as d:
        args = [exe, "--manifest", manifest(d, names), "--bench", str(RUNS)] + (["--tile", str(tile)] if tile else [])
        out = subprocess.run(args, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stdout + out.stderr
    rec = json.loads(next(l for l in out.stdout.splitlines() if l.startswith("{")))
    assert rec["accepted_one_by_one"] == rec["accepted_batched"] == rec["proofs"], rec
    loop = rec["one_by_one"]
    rec["speedup"] = round(loop["wall_ms_median"] / rec["batched"]["wall_ms_median"], 2)
    rec["adhoc_msm_share"] = round(loop["kernels"].get("msm_total", {"ms": 0.0})["ms"] / loop["profiled_call_wall_ms"], 4)
    return rec


res = {"metric": "verify_proofs_batched_vs_one_by_one", "runs": RUNS, "released_ten": bench(ALL_TEN), "chunk_proofs_tiled_318": bench(ALL_TEN[:7], tile=318)}
print(json.dumps(res), flush=True)
