"""bench_g1_codec.py -- the compressed-point codec of G1 on one MI355X.

  python tools/bench_g1_codec.py [--logs 20 24 26] [--loads 20 24] [--dir /tmp] [--host-threads 16] [--reps 5]

Per log2(n): mi355_g1_decompress_dev / mi355_g1_compress_dev on the Lagrange basis of a synthetic SRS -- median wall time of the synchronous call and the kernel time
from mi355_profile_get -- next to the 16-thread host loop over g1_from_bytes / g1_to_bytes (tools/g1_codec_host_bench.cpp, compiled into tools/_scratch/).
Per k of --loads: params_from_file of a Processed file against the RawBytes file of the same SRS, both freshly written, i.e. read from the page cache: the disk is
not what is measured.  One JSON line per size, then one summary line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def host_bench(words_path, n, threads):
    scratch = os.path.join(ROOT, "tools", "_scratch"); os.makedirs(scratch, exist_ok=True)
    exe = os.path.join(scratch, "g1_codec_host_bench")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "g1_codec_host_bench.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "scroll-prover_amd"), "-lmi355zk", f"-Wl,-rpath,{os.path.join(ROOT, 'scroll-prover_amd')}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, words_path, str(n), str(threads)], capture_output=True, text=True, timeout=1500)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="*", default=[20, 24, 26])
    ap.add_argument("--loads", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-max-log", type=int, default=24, help="largest size the host loop is timed at (larger sizes are scaled from it in the summary, marked so)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    zk = ge.load_package(); zk.init(0)
    h2, capi = zk.halo2, zk._capi
    lib, ptr = capi.lib(), capi.ptr
    out = []

    def prof(name):
        ms, launches = C.c_double(), C.c_uint64()
        capi.check(lib.mi355_profile_get(name, C.byref(ms), C.byref(launches)))
        return ms.value / max(1, launches.value)

    for k in a.logs:
        n = 1 << k
        g = torch.empty(n * 64, dtype=torch.uint8, device="cuda"); gl = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        w = pow(h2.FR_ROOT_OF_UNITY, 1 << (h2.FR_S - k), h2.R_MOD)
        capi.check(lib.mi355_srs_setup_dev(ptr(g), ptr(gl), k, ptr(h2.fr(0x5343524F4C4C0C0D + k)), ptr(h2.fr(w))))
        del g
        words = torch.empty(n * 32, dtype=torch.uint8, device="cuda"); back = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        wall = {"compress": [], "decompress": []}
        capi.check(lib.mi355_profile_enable(1))
        for rep in range(a.reps + 1):
            if rep == 1:
                capi.check(lib.mi355_profile_reset())
            torch.cuda.synchronize(); t0 = time.perf_counter()
            capi.check(lib.mi355_g1_compress_dev(ptr(gl), ptr(words), n)); capi.check(lib.mi355_synchronize())
            t1 = time.perf_counter()
            capi.check(lib.mi355_g1_decompress_dev(ptr(words), ptr(back), n, None))
            t2 = time.perf_counter()
            if rep:
                wall["compress"].append((t1 - t0) * 1e3); wall["decompress"].append((t2 - t1) * 1e3)
        rec = {"log_n": k, "decompress_wall_ms": statistics.median(wall["decompress"]), "decompress_kernel_ms": prof(b"g1_decompress"),
               "compress_wall_ms": statistics.median(wall["compress"]), "compress_kernel_ms": prof(b"g1_compress"), "round_trip": bool(torch.equal(back, gl))}
        capi.check(lib.mi355_profile_enable(0))
        rec["decompress_points_per_s"] = n / rec["decompress_kernel_ms"] * 1e3
        if k <= a.host_max_log:
            path = os.path.join(a.dir, f"mi355_codec_words_{os.getpid()}.bin")
            words.cpu().numpy().tofile(path)
            try:
                rec.update(host_bench(path, n, a.host_threads))
            finally:
                os.remove(path)
        del words, back, gl
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True); out.append(rec)
    for k in a.loads:
        src = h2.ParamsKZG.setup(k, 0x5343524F4C4C0C0D + k)
        raw, proc = os.path.join(a.dir, f"mi355_params{k}_{os.getpid()}.raw"), os.path.join(a.dir, f"mi355_params{k}_{os.getpid()}.processed")
        try:
            t0 = time.perf_counter(); src.write(raw); t1 = time.perf_counter(); src.write(proc, format="processed"); t2 = time.perf_counter()
            src.release()
            rec = {"load_k": k, "write_raw_ms": (t1 - t0) * 1e3, "write_processed_ms": (t2 - t1) * 1e3, "raw_bytes": os.path.getsize(raw), "processed_bytes": os.path.getsize(proc)}
            for name, path, kw in (("raw", raw, {}), ("raw_validated", raw, {"validate": True}), ("processed", proc, {"format": "processed"})):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter(); p = h2.params_from_file(path, **kw); ts.append((time.perf_counter() - t0) * 1e3); p.release()
                rec[f"load_{name}_ms"] = min(ts)
        finally:
            for p in (raw, proc):
                if os.path.exists(p):
                    os.remove(p)
        print(json.dumps(rec), flush=True); out.append(rec)
    print(json.dumps({"bench": "g1_codec", "results": out}))


if __name__ == "__main__":
    main()
