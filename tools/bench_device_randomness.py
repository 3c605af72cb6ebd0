"""The prover's randomness drawn on the device against the upload it replaces, on one machine in one run:

  * mi355_fr_random_dev at 2^20 and 2^26 elements: wall time of the call + synchronisation and the kernel alone (profile scope "fr_random"), median of 5 after a warm-up;
  * mi355_buf_upload of the same byte counts (32 MiB, 2 GiB) out of pageable and out of page-locked host memory, median of 5;
  * mi355_fr_from_u512_dev at the same two sizes;
  * a layer-4 k = 26 proof (the reference's batch protocol) and a many-column layer-0 proof (k = 20), each with ProofOptions::device_randomness off and on
    (tests/cpp/test_device_randomness.cpp: the second proof of each route in one process);
  * the default route through tests/cpp/test_plonk_replay (window tables as bench.py's proof mix has them) and, with --parent-tree DIR (a built checkout of the
    parent commit), that tree's replay program with the same arguments: the pair that shows whether the default path moved.

  python tools/bench_device_randomness.py [--sizes 20,26] [--no-proofs] [--layers 4,0] [--parent-tree DIR] [--out FILE]
"""
import ctypes as C, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge

KEY = bytes(range(1, 33))
GOLD = os.path.join(ROOT, "tests", "golden")


def med(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def kernel_ms(lib, check, scope, f):
    check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1)); f(); check(lib.mi355_synchronize())
    ms, cnt = C.c_double(), C.c_uint64(); check(lib.mi355_profile_get(scope, C.byref(ms), C.byref(cnt))); check(lib.mi355_profile_enable(0))
    return round(ms.value, 3)


def primitives(zk, log_n):
    h2, lib, check = zk.halo2, zk._capi.lib(), zk._capi.check
    n = 1 << log_n
    d = h2.DeviceBuffer(32 * n)
    sync = lambda: check(lib.mi355_synchronize())
    draw = lambda: (h2.fr_random(d, KEY, 0, 0), sync())
    rec = {"elements": n, "bytes": 32 * n, "fr_random_wall_ms": med(draw), "fr_random_kernel_ms": kernel_ms(lib, check, b"fr_random", draw)}
    src = h2.DeviceBuffer(64 * n)
    h2.fr_random(src, KEY, 1, 0)                                                     # 2 n words of anything
    red = lambda: (h2.fr_from_u512(src, d), sync())
    rec["fr_from_u512_wall_ms"] = med(red); rec["fr_from_u512_kernel_ms"] = kernel_ms(lib, check, b"fr_from_u512", red)
    src.free()
    host = np.random.default_rng(1).integers(0, 2**63, size=(n, 4), dtype=np.uint64)
    rec["upload_pageable_ms"] = med(lambda: d.upload(host))
    p = C.c_void_p(); check(lib.mi355_host_alloc(32 * n, C.byref(p)))
    C.memmove(p, host.ctypes.data, 32 * n)
    rec["upload_pinned_ms"] = med(lambda: check(lib.mi355_buf_upload(C.c_void_p(d.data_ptr()), p, 32 * n)))
    check(lib.mi355_host_free(p)); d.free(); check(lib.mi355_buf_trim())
    for k in ("upload_pageable_ms", "upload_pinned_ms"):
        rec[k.replace("_ms", "_gb_s")] = round(32 * n / rec[k] / 1e6, 1)
    return rec


def proofs(zk, layer, parent_tree):
    with tempfile.TemporaryDirectory(prefix="mi355_bench_rng_") as tmp:
        fx = os.path.join(GOLD, f"protocol_layer{layer}.json")
        args = ["--proofs", "2", "--threads", "16"] + (["--builder-key", "--upload-threads", "3"] if layer == 0 else [])
        rec = zk.replay.run_device_randomness(layer, KEY, out_dir=os.path.join(tmp, "new"), args=args, protocol_file=fx if os.path.exists(fx) else None, timeout=1700)
        out = {k: rec.get(k) for k in ("ok", "k", "advice", "lookups", "blind", "off", "on", "error") if k in rec}
        rargs = ["--proofs", "2", "--threads", "16"] + (["--upload-threads", "3"] if layer == 0 else [])
        cur = zk.replay.run(layer, out_dir=os.path.join(tmp, "replay"), args=rargs, protocol_file=rec["protocol_path"], timeout=1700)   # the default route through the replay program, as bench.py times it
        out["replay_ms"] = cur.get("resident_ms"); out["replay_ok"] = bool(cur.get("ok"))
        if parent_tree:
            exe = os.path.join(parent_tree, "tests", "cpp", "test_plonk_replay")
            pd = os.path.join(tmp, "parent"); os.makedirs(pd)
            o = subprocess.run([exe, "--protocol", rec["protocol_path"], "--out", pd] + rargs, capture_output=True, text=True, timeout=1700,
                               env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join([os.path.join(parent_tree, "scroll-prover_amd"), os.path.join(parent_tree, "oracle"), os.environ.get("LD_LIBRARY_PATH", "")])))
            line = next((l for l in o.stdout.splitlines() if l.startswith("{")), None)
            out["parent_replay_ms"] = json.loads(line)["resident_ms"] if line else None
            if not line:
                out["parent_error"] = (o.stdout + o.stderr)[-400:]
    return out


def main():
    sizes = [20, 26]; layers = [4, 0]; do_proofs = True; parent = None; out = None
    a = sys.argv[1:]
    for i, x in enumerate(a):
        if x == "--sizes": sizes = [int(v) for v in a[i + 1].split(",")]
        if x == "--layers": layers = [int(v) for v in a[i + 1].split(",")]
        if x == "--no-proofs": do_proofs = False
        if x == "--parent-tree": parent = a[i + 1]
        if x == "--out": out = a[i + 1]
    rec = {"tool": "bench_device_randomness", "primitives": {}, "proofs": {}}
    zk = ge.load_package(); zk.init(0)
    for s in sizes:
        rec["primitives"][f"2^{s}"] = primitives(zk, s)
        print(json.dumps({f"2^{s}": rec["primitives"][f"2^{s}"]}), file=sys.stderr, flush=True)
    zk.shutdown()
    if do_proofs:
        for layer in layers:
            rec["proofs"][f"layer{layer}"] = proofs(zk, layer, parent)
            print(json.dumps({f"layer{layer}": rec["proofs"][f"layer{layer}"]}), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
