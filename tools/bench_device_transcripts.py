"""plonk::verify_proofs with the Poseidon transcripts on the host against the same call with VerifyOptions::device_transcript, through tests/cpp/test_device_transcripts --bench,
which runs both modes in ONE process after one warm-up call of each: on the ten released proofs, and on the seven chunk proofs tiled to 318 (the number of chunk proofs the
reference stores).  Per mode: the wall time of 5 calls (median and all five), its split per call (decode, record, transcript call, scalar side, MSM, pairing) and, from one
further profiled call, the kernels' own figures (mi355_profile_get: poseidon_transcripts among them).
--yardstick EXE: also runs `EXE --bench 5` on the same two workloads in the same session, EXE being a tests/cpp/test_verify_proofs binary (of the parent commit, say); its
batched figure is what the option has to beat.  Prints one JSON line.  Not part of bench.py."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
from verify_common import ALL_TEN, NEG_S_G2_WORDS, case, product_protocol

RUNS = 5
zk = ge.load_package()
exe = ge.build_cpp("test_device_transcripts")
yardstick = sys.argv[sys.argv.index("--yardstick") + 1] if "--yardstick" in sys.argv else None


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
    with tempfile.TemporaryDirectory(prefix="mi355_bench_transcripts_") as d:
        tail = ["--manifest", manifest(d, names), "--bench", str(RUNS)] + (["--tile", str(tile)] if tile else [])
        runs = {"this": [exe] + tail}
        if yardstick:
            runs["yardstick"] = [yardstick] + tail
        out = {}
        for key, args in runs.items():
            p = subprocess.run(args, capture_output=True, text=True, timeout=1500)
            assert p.returncode == 0, p.stdout + p.stderr
            out[key] = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("{")))
    rec = out["this"]
    assert rec["accepted_host_transcript"] == rec["accepted_device_transcript"] == rec["proofs"], rec
    rec["speedup"] = round(rec["host_transcript"]["wall_ms_median"] / rec["device_transcript"]["wall_ms_median"], 2)
    if yardstick:
        y = out["yardstick"]
        assert y["accepted_batched"] == y["proofs"], y
        rec["yardstick_batched"] = y["batched"]
        rec["speedup_over_yardstick"] = round(y["batched"]["wall_ms_median"] / rec["device_transcript"]["wall_ms_median"], 2)
    return rec


res = {"metric": "verify_proofs_device_transcript_vs_host_transcript", "runs": RUNS, "released_ten": bench(ALL_TEN), "chunk_proofs_tiled_318": bench(ALL_TEN[:7], tile=318)}
print(json.dumps(res), flush=True)
