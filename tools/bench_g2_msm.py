"""G2 against G1 MSM time (mi355_msm_g2_adhoc_host / mi355_msm_g1_adhoc_host) at 2^16, 2^20 and 2^22 in one process: uniform scalars over
random bases (1024 distinct points of each group, tiled), warm-up, median of 5, and the per-phase mi355_profile_get figures of one more
profiled call.  Prints one JSON line.  Not part of bench.py."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
from oracle import cref
from gpu_common import rand_fr, rand_points

zk = ge.load_package(); zk.init(0); h2 = zk.halo2; lib = zk._capi.lib(); check = zk._capi.check; ptr = zk._capi.ptr
rng = np.random.default_rng(5)
gen2 = cref.g2_generator()
g2_pts = np.stack([cref.g2_mul(gen2, s) for s in rand_fr(rng, 1024, full=False)])
g1_pts = rand_points(rng, 1024)
PHASES = {"g1": ("msm_total", "msm_digits", "msm_sort", "msm_accumulate", "msm_reduce"),
          "g2": ("msm_g2_total", "msm_g2_validate", "msm_g2_digits", "msm_g2_sort", "msm_g2_accumulate", "msm_g2_fixup", "msm_g2_reduce")}


def prof(name):
    ms, cnt = C.c_double(), C.c_uint64(); check(lib.mi355_profile_get(name.encode(), C.byref(ms), C.byref(cnt))); return round(ms.value, 3)


def run(kind, bases, sc, n):
    out = np.zeros(16 if kind == "g2" else 12, dtype=np.uint64)
    fn = lib.mi355_msm_g2_adhoc_host if kind == "g2" else lib.mi355_msm_g1_adhoc_host
    call = lambda: check(fn(ptr(bases), ptr(sc), n, ptr(out)))
    call()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1)); call(); check(lib.mi355_profile_enable(0))
    c, w, e = C.c_int(), C.c_int(), C.c_uint64(); check(lib.mi355_msm_last_plan(C.byref(c), C.byref(w), C.byref(e)))
    return {"ms": round(statistics.median(ts), 3), "c": c.value, "windows": w.value, "phases_ms": {p: prof(p) for p in PHASES[kind]}}


res = {"metric": "g2_vs_g1_msm_adhoc_host", "sizes": {}}
for log_n in (16, 20, 22):
    n = 1 << log_n
    sc = rand_fr(rng, n)
    r2 = run("g2", np.ascontiguousarray(np.tile(g2_pts, (n // 1024, 1))), sc, n)
    r1 = run("g1", np.ascontiguousarray(np.tile(g1_pts, (n // 1024, 1))), sc, n)
    res["sizes"][str(log_n)] = {"g2": r2, "g1": r1, "ratio": round(r2["ms"] / r1["ms"], 2)}
print(json.dumps(res), flush=True)
