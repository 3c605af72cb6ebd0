#!/usr/bin/env python3
"""bench_hbm_budget.py -- what the quotient in coset groups (ProofOptions::coset_group_polys) costs and saves, on one MI355X.

Drives tests/cpp/test_hbm_budget (--bench): per shape and key mode ONE process builds the circuit and the key once and then, for every entry of --groups (0 = the ungrouped
route, all, or G), proves once to warm up and --proofs times more; each proof runs between two mi355_buf_trim calls with the ledger's high-water mark reset, so `high_water` is one
proof's peak on top of what the process holds anyway (SRS, key, workspace).  Prints one JSON line per process and a markdown table (the one profiles/hbm_budget.md keeps).

  python tools/bench_hbm_budget.py                          # the layer-0 stand-in at k = 20 and layer 3 at k = 21, key resident and lean, G in {0, all, 256, 64, 24}
  python tools/bench_hbm_budget.py --shapes 3:12 --proofs 3 # a small run
  --parent-exe PATH --parent-libdir DIR                     # the parent commit's test_plonk_replay and the directory of its libmi355zk.so: the same shapes, ungrouped, for comparison
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

STANDIN = dict(advice=40, fixed=8, lookups=3, perm_columns=12, degree=5)   # the layer-0 stand-in of the prover tests
GiB = float(1 << 30)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="0:20,3:21", help="layer:k pairs; layer 0 is the 40-column stand-in")
    ap.add_argument("--groups", default="0,all,256,64,24")
    ap.add_argument("--proofs", type=int, default=5)
    ap.add_argument("--keys", default="resident,on-the-fly")
    ap.add_argument("--parent-exe", default="")
    ap.add_argument("--parent-libdir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ge.build()
    zk = ge.load_package()
    rows, lines = [], []
    for shape in a.shapes.split(","):
        layer, k = (int(x) for x in shape.split(":"))
        kw = STANDIN if layer == 0 else {}
        for key in a.keys.split(","):
            with tempfile.TemporaryDirectory(prefix="mi355_hbm_bench_") as tmp:
                rec = zk.replay.run_hbm_budget(layer, k, out_dir=tmp, args=["--bench", str(a.proofs), "--groups", a.groups, "--pk-cosets", key], timeout=1500, **kw)
                lines.append(json.dumps({k_: v for k_, v in rec.items() if k_ not in ("out_dir", "protocol_path")}))
                print(lines[-1], flush=True)
                if not rec.get("ok"):
                    continue
                for r in rec["runs"]:
                    rows.append((layer, k, key, r["group"], r["coset_groups"], r["coset_retransforms"], r["coset_ntt"], r["high_water"] / GiB, r["step7_ms_median"], r["step7_ms_min"], r["step7_ms_max"],
                                 r["total_ms_median"], r["total_ms_min"], r["total_ms_max"]))
                if a.parent_exe:
                    proto = zk.replay.write_protocol(layer, tmp, k, None, **kw)
                    env = dict(os.environ, LD_LIBRARY_PATH=a.parent_libdir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
                    out = subprocess.run([a.parent_exe, "--protocol", proto, "--out", tmp, "--proofs", str(a.proofs + 1), "--pk-cosets", key, "--tables", "off"], capture_output=True, text=True, timeout=1500, env=env)
                    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
                    if out.returncode == 0 and line:
                        p = json.loads(line)
                        rows.append((layer, k, key, "parent", 0, 0, p["coset_ntt"], float("nan"), p["step_ms"]["7_quotient"], float("nan"), float("nan"), p["resident_ms"], float("nan"), float("nan")))
                        lines.append(json.dumps({"parent": True, "layer": layer, "k": k, "pk_cosets": key, "coset_ntt": p["coset_ntt"], "step7_ms_last": p["step_ms"]["7_quotient"], "total_ms_last": p["resident_ms"], "proofs": a.proofs + 1}))
                        print(lines[-1], flush=True)
                    else:
                        print(json.dumps({"parent": True, "error": (out.stdout + out.stderr)[-600:]}), flush=True)
    table = ["| layer | k | key | G | groups / part | re-transforms | coset transforms | high-water GiB | step 7 ms median (min – max) | proof ms median (min – max) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        table.append("| %d | %d | %s | %s | %d | %d | %d | %.3f | %.1f (%.1f – %.1f) | %.1f (%.1f – %.1f) |" % r)
    print("\n".join(table))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n\n" + "\n".join(table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
