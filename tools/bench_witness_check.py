"""the two reductions of the witness check alone (csrc/check.hpp) against their algorithmic bytes, and plonk::check_witness against create_proof of the same process.

Kernels: mi355_fr_nonzero_rows_dev on one vector of 2^20 / 2^24 / 2^26 words (32 B per row), clean and with every row failing; mi355_fr_copy_check_dev on 2 columns
of that size with every cell of column 0 paired with its row in column 1 (64 B of gathers + 16 B of list per pair), clean and with every pair failing.  Per case the
call's wall time (synchronous: staging uploads, three launches, the read-back) and the kernels alone (profile scopes "nonzero_rows" / "copy_check"), median of 5 after
a warm-up, and GB/s of algorithmic bytes over the kernel time.
Driver (--layers): tests/cpp/test_witness_check.cpp --prove --no-dump per layer at its own k, clean and with advice cell (0, 3) off by one: check_ms next to the
create_proof total of the same process without the check.

  python tools/bench_witness_check.py [--logs 20,24,26] [--layers 0:20,2:25,4:26] [--out FILE]
"""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge

STANDIN = dict(advice=40, fixed=8, lookups=3, perm_columns=12, degree=5)


def timed(zk, call, scope):
    lib, check = zk._capi.lib(), zk._capi.check
    call()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter(); call(); walls.append((time.perf_counter() - t0) * 1e3)
    check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1)); call(); check(lib.mi355_synchronize())
    ms, cnt = C.c_double(), C.c_uint64(); check(lib.mi355_profile_get(scope, C.byref(ms), C.byref(cnt))); check(lib.mi355_profile_enable(0))
    return round(statistics.median(walls), 3), round(ms.value, 4)


def kernels(zk, log_n):
    import torch
    h2 = zk.halo2
    n = 1 << log_n
    out = {}
    zero = torch.zeros((n, 4), dtype=torch.int64, device="cuda:0")
    full = torch.randint(1, 1 << 62, (n, 4), dtype=torch.int64, device="cuda:0")
    for name, vec in (("clean", zero), ("all_failing", full)):
        wall, ker = timed(zk, lambda: h2.nonzero_rows(vec, 16), b"nonzero_rows")
        out[f"nonzero_rows_{name}"] = {"wall_ms": wall, "kernels_ms": ker, "algorithmic_gb_s": round(32 * n / ker / 1e6, 1) if ker else None}
    cells = np.arange(n, dtype=np.uint64); images = cells + np.uint64(n)
    for name, other in (("clean", zero.clone()), ("all_failing", full)):
        wall, ker = timed(zk, lambda: h2.copy_check([zero, other], cells, images, 16), b"copy_check")
        out[f"copy_check_{name}"] = {"pairs": n, "wall_ms": wall, "kernels_ms": ker, "algorithmic_gb_s": round(80 * n / ker / 1e6, 1) if ker else None}
    del zero, full
    torch.cuda.empty_cache(); zk._capi.check(zk._capi.lib().mi355_buf_trim())
    print(json.dumps({f"2^{log_n}": out}), file=sys.stderr, flush=True)
    return out


def main():
    logs = [20, 24, 26]; layers = []; out = None
    a = sys.argv[1:]
    for i, x in enumerate(a):
        if x == "--logs": logs = [int(v) for v in a[i + 1].split(",") if v]
        if x == "--layers": layers = [tuple(int(v) for v in s.split(":")) for s in a[i + 1].split(",") if s]
        if x == "--out": out = a[i + 1]
    rec = {"tool": "bench_witness_check", "kernels": {}, "driver": {}}
    zk = ge.load_package()
    if logs:
        zk.init(0)
        for log_n in logs:
            rec["kernels"][f"2^{log_n}"] = kernels(zk, log_n)
        zk.shutdown()
    for layer, k in layers:
        for name, extra in (("clean", []), ("one_cell_off", ["--corrupt", "advice:0:3"])):
            r = zk.replay.run_witness_check(layer, k, args=["--no-dump", "--threads", "16"] + extra + (["--prove"] if name == "clean" else []), timeout=1500, **(STANDIN if layer == 0 else {}))
            keep = {x: r.get(x) for x in ("ok", "k", "gates", "lookups", "perm_columns", "copy_pairs", "failures", "check_ms", "proof_ms", "pk_cosets", "error")}
            rec["driver"][f"layer{layer}_k{k}_{name}"] = keep
            print(json.dumps({f"layer{layer}_k{k}_{name}": keep}), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
