"""mi355_fr_lookup_multiplicities_dev (the mv-lookup multiplicity column counted on the device) at k = 20, 22, 24, 26 against a host restatement on 16 threads
(tools/lookup_host_bench.cpp: a hash map of the table's first rows, probed by 16 threads), and -- with --proof -- step 3 of a layer-4 proof at k = 26 by the default route
(the caller's m columns uploaded) and by the device route (ProofOptions::device_multiplicities).  Prints one JSON line.  Not part of bench.py.

Cases (table_rows = input_rows = 2^k - 10, the usable rows):
  range        a range table of 2^(k-1) values (lookup_bits = k - 1) plus its zero tail; inputs drawn uniformly from the 2^(k-1) values
  tuple        a 3-column theta-compressed table: 2^(k-1) distinct words (what compression of distinct tuples gives) plus the zero tail; inputs drawn from it
  zero         the range table; an all-zero input column (the rows a selector switches off)
  mostly_zero  the range table; 90 % of the input rows zero, the rest drawn from the table
Device times: the call's wall time (it is synchronous: the error word is read back) and the kernels alone (profile scope "lookup_multiplicities"); median of 5 after a warm-up.

  python tools/bench_lookup_multiplicities.py [--ks 20,22,24,26] [--no-host] [--proof] [--out FILE]
"""
import ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge

CASES = ("range", "tuple", "zero", "mostly_zero")


def host_exe() -> str:
    src = os.path.join(ROOT, "tools", "lookup_host_bench.cpp")
    exe = os.path.join(ROOT, "tools", "_scratch", "lookup_host_bench")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", src, "-o", exe])
    return exe


def device_case(zk, k, case, rng):
    import torch
    h2, lib, check = zk.halo2, zk._capi.lib(), zk._capi.check
    n = 1 << k
    u, half = n - 10, 1 << (k - 1)
    dev = torch.device("cuda:0")
    vals = np.zeros(n, dtype=np.uint32); vals[:half] = np.arange(half, dtype=np.uint32)
    if case == "tuple":
        w = torch.randint(0, 2**62, (n, 4), dtype=torch.int64, device=dev); w[:, 3] &= (1 << 60) - 1; w[half:] = 0
        table = w
    else:
        table = torch.empty((n, 4), dtype=torch.int64, device=dev)
        b = h2.DeviceBuffer.from_packed(vals); check(lib.mi355_buf_copy(C.c_void_p(table.data_ptr()), C.c_void_p(b.data_ptr()), 32 * n)); b.free()
    idx = rng.integers(0, half, size=n)
    if case == "zero":
        idx[:] = 0
    elif case == "mostly_zero":
        idx[rng.random(n) < 0.9] = 0
    if case == "tuple":
        inp = torch.empty_like(table)
        for lo in range(0, n, 1 << 22):   # 2^22 rows per indexing call: one call over 2^26 rows is more than torch's index kernel launches
            inp[lo: lo + (1 << 22)] = table[torch.from_numpy(idx[lo: lo + (1 << 22)]).to(dev)]
    else:
        inp = torch.empty((n, 4), dtype=torch.int64, device=dev)
        b = h2.DeviceBuffer.from_packed(idx.astype(np.uint32)); check(lib.mi355_buf_copy(C.c_void_p(inp.data_ptr()), C.c_void_p(b.data_ptr()), 32 * n)); b.free()
    torch.cuda.synchronize()
    m = torch.empty_like(table)
    arr = (C.c_void_p * 1)(inp.data_ptr()); miss = C.c_uint64()
    call = lambda: check(lib.mi355_fr_lookup_multiplicities_dev(C.c_void_p(m.data_ptr()), n, C.c_void_p(table.data_ptr()), u, arr, 1, u, 0, C.byref(miss)))
    call()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter(); call(); walls.append((time.perf_counter() - t0) * 1e3)
    check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1)); call(); check(lib.mi355_synchronize())
    ms, cnt = C.c_double(), C.c_uint64(); check(lib.mi355_profile_get(b"lookup_multiplicities", C.byref(ms), C.byref(cnt))); check(lib.mi355_profile_enable(0))
    # the counts add up to the input rows (every value is in the table)
    total = int(h2.fr_to_int(m[0].cpu().numpy().view(np.uint64))) if case == "zero" else None
    del m, table, inp
    torch.cuda.empty_cache(); check(lib.mi355_buf_trim())
    return {"wall_ms": round(statistics.median(walls), 3), "kernels_ms": round(ms.value, 3), **({"m0": total} if total is not None else {})}


def main():
    ks = [20, 22, 24, 26]; host = True; proof = False; out = None
    a = sys.argv[1:]
    for i, x in enumerate(a):
        if x == "--ks": ks = [int(v) for v in a[i + 1].split(",")]
        if x == "--no-host": host = False
        if x == "--proof": proof = True
        if x == "--out": out = a[i + 1]
    rec = {"tool": "bench_lookup_multiplicities", "cases": {}}
    zk = ge.load_package(); zk.init(0)
    rng = np.random.default_rng(7)
    for k in ks:
        for case in CASES:
            r = {"device": device_case(zk, k, case, rng)}
            rec["cases"][f"{case}_k{k}"] = r
            print(json.dumps({f"{case}_k{k}": r}), file=sys.stderr, flush=True)
    zk.shutdown()
    if host:
        exe = host_exe()
        for k in ks:
            for case in CASES:
                o = subprocess.run([exe, str(k), case, "16"], capture_output=True, text=True, timeout=600)
                h = json.loads(o.stdout.strip().splitlines()[-1])
                rec["cases"][f"{case}_k{k}"]["host_16_threads"] = h
                print(json.dumps({f"{case}_k{k}_host": h}), file=sys.stderr, flush=True)
    if proof:
        r = zk.replay.run_lookup_multiplicities(4, out_dir=os.path.join(ROOT, "tools", "_scratch", "lookup_m_layer4"), protocol_file=os.path.join(ROOT, "tests", "golden", "protocol_layer4.json"), timeout=1500)
        rec["layer4_k26"] = {x: r.get(x) for x in ("ok", "k", "bytes_equal", "default_ms", "device_ms", "multiplicity_ms", "step_ms_default", "step_ms_device", "pk_cosets", "hbm", "error")}
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
