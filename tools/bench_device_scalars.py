"""plonk::verify_proofs with the scalar side on the host against the same call with VerifyOptions::device_scalars, through tests/cpp/test_device_scalars --bench, which runs both
modes in ONE process after one warm-up call of each: on the ten released proofs, and on the seven chunk proofs tiled to 318 (the number of chunk proofs the reference stores);
each with the transcripts on the host and with VerifyOptions::device_transcript.  Per mode: the wall time of 5 calls (median and all five), its split per call (decode, record,
transcript call, host part, scalar call, MSM, pairing) and, from one further profiled call, the kernels' own figures (mi355_profile_get: fr_program among them).  Also prints
the instruction and register counts of the compiled programs.
--yardstick EXE: also runs `EXE --bench 5` on the same two workloads in the same session, EXE being a tests/cpp/test_device_transcripts binary of the parent commit (give its
library's directory with --yardstick-lib DIR); its figures are what the option-off call has to equal and the option-on call has to beat.  Prints one JSON line.  Not part of bench.py."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
from verify_common import ALL_TEN, NEG_S_G2_WORDS, case, product_protocol

RUNS = 5
zk = ge.load_package()
exe = ge.build_cpp("test_device_scalars")
arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
yardstick, yardstick_lib = arg("--yardstick"), arg("--yardstick-lib")


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


def one(args, env=None):
    p = subprocess.run(args, capture_output=True, text=True, timeout=1500, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def bench(names, tile=0):
    with tempfile.TemporaryDirectory(prefix="mi355_bench_scalars_") as d:
        man = manifest(d, names)
        tail = ["--manifest", man, "--bench", str(RUNS)] + (["--tile", str(tile)] if tile else [])
        out = {"programs": one([exe, "--manifest", man, "--program-info"])[:-1]}
        for key, extra in (("host_transcripts", []), ("device_transcripts", ["--device-transcript"])):
            rec = one([exe] + tail + extra)[0]
            assert rec["accepted_host_scalars"] == rec["accepted_device_scalars"] == rec["proofs"], rec
            rec["speedup"] = round(rec["host_scalars"]["wall_ms_median"] / rec["device_scalars"]["wall_ms_median"], 2)
            out[key] = rec
        if yardstick:
            env = dict(os.environ, LD_LIBRARY_PATH=yardstick_lib + os.pathsep + os.environ.get("LD_LIBRARY_PATH", "")) if yardstick_lib else None
            y = one([yardstick] + tail, env)[0]
            assert y["accepted_host_transcript"] == y["proofs"], y
            out["yardstick"] = {"host_transcript": y["host_transcript"], "device_transcript": y["device_transcript"]}
    return out


res = {"metric": "verify_proofs_device_scalars_vs_host_scalars", "runs": RUNS, "released_ten": bench(ALL_TEN), "chunk_proofs_tiled_318": bench(ALL_TEN[:7], tile=318)}
print(json.dumps(res), flush=True)
