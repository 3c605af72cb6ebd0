"""mi355_fr_permutation_sigma_dev (the sigma columns of the permutation argument built on the device from the copy mapping) at (n_cols, log_n) = (150, 20), (32, 24),
(8, 26) with 0, 10 % and 100 % of the cells overridden, against the default keygen route's sigma stage on the same machine (Circuit::sigma_column on 8 host threads +
one 32-byte-per-cell upload per column: tests/cpp/test_permutation_keygen.cpp --sigma-only, 0 and 10 % of the cells in copy pairs).

Device times: the call's wall time (it is synchronous; host validation, staging uploads and kernels) and the kernels alone (profile scope "permutation_sigma");
median of 5 after a warm-up.  The override lists are one cycle through every k-th cell.

  python tools/bench_permutation_sigma.py [--shapes 150x20,32x24,8x26] [--no-host] [--out FILE]
"""
import ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge

DENSITIES = (0, 10, 100)


def device_shape(zk, n_cols, log_n):
    import torch
    h2, lib, check = zk.halo2, zk._capi.lib(), zk._capi.check
    total = n_cols << log_n
    delta, omega = h2.fr(pow(7, 1 << 28, h2.R_MOD)), h2.fr(pow(h2.FR_ROOT_OF_UNITY, 1 << (h2.FR_S - log_n), h2.R_MOD))
    cols = [torch.empty((1 << log_n, 4), dtype=torch.int64, device="cuda:0") for _ in range(n_cols)]
    out = {}
    for pct in DENSITIES:
        cells = np.arange(0, total, 100 // pct, dtype=np.uint64) if pct else np.zeros(0, dtype=np.uint64)
        images = np.roll(cells, -1)
        call = lambda: h2.permutation_sigma(n_cols, log_n, delta, omega, cells, images, out=cols)
        call()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter(); call(); walls.append((time.perf_counter() - t0) * 1e3)
        check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1)); call(); check(lib.mi355_synchronize())
        ms, cnt = C.c_double(), C.c_uint64(); check(lib.mi355_profile_get(b"permutation_sigma", C.byref(ms), C.byref(cnt))); check(lib.mi355_profile_enable(0))
        out[f"{pct}pct"] = {"overrides": int(cells.size), "wall_ms": round(statistics.median(walls), 3), "kernels_ms": round(ms.value, 3)}
        print(json.dumps({f"{n_cols}x2^{log_n}_{pct}pct": out[f"{pct}pct"]}), file=sys.stderr, flush=True)
    del cols
    torch.cuda.empty_cache(); check(lib.mi355_buf_trim())
    return out


def main():
    shapes = [(150, 20), (32, 24), (8, 26)]; host = True; out = None
    a = sys.argv[1:]
    for i, x in enumerate(a):
        if x == "--shapes": shapes = [tuple(int(v) for v in s.split("x")) for s in a[i + 1].split(",")]
        if x == "--no-host": host = False
        if x == "--out": out = a[i + 1]
    rec = {"tool": "bench_permutation_sigma", "shapes": {}}
    zk = ge.load_package(); zk.init(0)
    for n_cols, log_n in shapes:
        rec["shapes"][f"{n_cols}x2^{log_n}"] = {"device": device_shape(zk, n_cols, log_n)}
    zk.shutdown()
    if host:
        exe = ge.build_cpp("test_permutation_keygen")
        for n_cols, log_n in shapes:
            h = {}
            for pct in (0, 10):
                o = subprocess.run([exe, "--sigma-only", str(n_cols), str(log_n), str(pct)], capture_output=True, text=True, timeout=900)
                line = next((l for l in o.stdout.splitlines() if l.startswith("{")), None)
                h[f"{pct}pct"] = json.loads(line) if line else {"ok": False, "error": (o.stdout + o.stderr)[-400:]}
                print(json.dumps({f"{n_cols}x2^{log_n}_{pct}pct_host": h[f"{pct}pct"]}), file=sys.stderr, flush=True)
            rec["shapes"][f"{n_cols}x2^{log_n}"]["host_route"] = h
    line = json.dumps(rec)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
