"""mi355_fr_lookup_permute_dev (the permuted columns A' and S' of the classic halo2 lookup argument, built on the device) at k = 20, 22, 24, 26 against a host
restatement of halo2's permute_expression_pair on 16 threads (tools/lookup_permute_host_bench.cpp: a parallel sort plus an ordered map).  Prints one JSON line.
Not part of bench.py.

Cases (rows = 2^k - 7, the usable rows):
  range   a range table of 2^(k-1) values (lookup_bits = k - 1) plus its zero tail; inputs drawn uniformly from the 2^(k-1) values
  tuple   a 3-column theta-compressed table: 2^(k-1) distinct random words (what compression of distinct tuples gives) plus the zero tail; inputs drawn from it
  zero    the range table; an all-zero input column (the rows a selector switches off): one run, every other row repeated
Device times: the call's wall time (it is synchronous) and the kernels alone (profile scope "lookup_permute"); median of 5 after a warm-up.  `passes`: the radix
passes that ran (profile scope "lookup_permute_pass"; 32 digits less the ones every key shares).

  python tools/bench_classic_lookup.py [--ks 20,22,24,26] [--no-host] [--out FILE]
"""
import ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge

CASES = ("range", "tuple", "zero")


def host_exe() -> str:
    src = os.path.join(ROOT, "tools", "lookup_permute_host_bench.cpp")
    exe = os.path.join(ROOT, "tools", "_scratch", "lookup_permute_host_bench")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", src, "-o", exe])
    return exe


def device_case(zk, k, case, rng):
    import torch
    h2, lib, check = zk.halo2, zk._capi.lib(), zk._capi.check
    n = 1 << k
    u, half = n - 7, 1 << (k - 1)
    dev = torch.device("cuda:0")
    packed = lambda vals: h2.DeviceBuffer.from_packed(vals.astype(np.uint32))
    vals = np.zeros(n, dtype=np.uint32); vals[:half] = np.arange(half, dtype=np.uint32)
    idx = rng.integers(0, half, size=n)
    if case == "zero":
        idx[:] = 0
    if case == "tuple":
        table = torch.randint(0, 2**62, (n, 4), dtype=torch.int64, device=dev); table[:, 3] &= (1 << 60) - 1; table[half:] = 0
        inp = torch.empty_like(table)
        for lo in range(0, n, 1 << 22):
            inp[lo: lo + (1 << 22)] = table[torch.from_numpy(idx[lo: lo + (1 << 22)]).to(dev)]
    else:
        table = torch.empty((n, 4), dtype=torch.int64, device=dev); inp = torch.empty_like(table)
        for dst, v in ((table, vals), (inp, idx)):
            b = packed(v); check(lib.mi355_buf_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(b.data_ptr()), 32 * n)); b.free()
    torch.cuda.synchronize()
    a, s = torch.empty_like(table), torch.empty_like(table)
    miss = C.c_uint64()
    call = lambda: check(lib.mi355_fr_lookup_permute_dev(C.c_void_p(a.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(inp.data_ptr()), C.c_void_p(table.data_ptr()), u, C.byref(miss)))
    call()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter(); call(); walls.append((time.perf_counter() - t0) * 1e3)
    check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1)); call(); check(lib.mi355_synchronize())
    ms, cnt, pms, passes = C.c_double(), C.c_uint64(), C.c_double(), C.c_uint64()
    check(lib.mi355_profile_get(b"lookup_permute", C.byref(ms), C.byref(cnt))); check(lib.mi355_profile_get(b"lookup_permute_pass", C.byref(pms), C.byref(passes))); check(lib.mi355_profile_enable(0))
    # A'[0] = S'[0], and the first and last rows of A' are the smallest and the largest input
    head_equal = bool((a[0] == s[0]).all().item())
    del a, s, table, inp
    torch.cuda.empty_cache(); check(lib.mi355_buf_trim())
    return {"wall_ms": round(statistics.median(walls), 3), "kernels_ms": round(ms.value, 3), "sort_passes_ms": round(pms.value, 3), "passes": passes.value, "head_equal": head_equal}


def main():
    ks = [20, 22, 24, 26]; host = True; out = None
    a = sys.argv[1:]
    for i, x in enumerate(a):
        if x == "--ks": ks = [int(v) for v in a[i + 1].split(",")]
        if x == "--no-host": host = False
        if x == "--out": out = a[i + 1]
    rec = {"tool": "bench_classic_lookup", "cases": {}}
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
                o = subprocess.run([exe, str(k), case, "16"], capture_output=True, text=True, timeout=900)
                h = json.loads(o.stdout.strip().splitlines()[-1])
                rec["cases"][f"{case}_k{k}"]["host_16_threads"] = h
                print(json.dumps({f"{case}_k{k}_host": h}), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
