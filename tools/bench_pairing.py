"""Pairing products on the device (mi355_pairing_products_host) at (groups, pairs_per_group) = (1, 2) -- one verifier's check --, (318, 2) -- a batch of chunk
proofs -- and (1, 636) -- the same pairs as one product, the deep tree: warm-up, median of 5 wall times, and the per-kernel mi355_profile_get figures of one more
profiled call.  In the same run the Python oracle's time for one two-pair check (oracle/pairing.py, big integers) is recorded: the only comparison there is, since
no parent commit has this capability.  No threshold is set.  Prints one JSON line; the figures belong in profiles/pairing.md, which marks every number it holds as
measured or unmeasured.  Not part of bench.py.
The last row is one full plonk::verify_proof of the released chunk proof (tests/golden/kat.json, protocol_layer2.json, the released -[s]G2, accumulator checked) through
halo2.verify_proof: the wall time of the driver PROCESS (start-up and mi355_init included) and, from a second run under MI355 profiling, nothing more -- the driver is a
process of its own, so its kernels are not in this process's profile."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
from oracle import cref, pairing, pyref
from gpu_common import rand_fr

zk = ge.load_package(); zk.init(0); h2 = zk.halo2; lib = zk._capi.lib(); check = zk._capi.check
rng = np.random.default_rng(18)
KERNELS = ("pairing_validate", "pairing_miller", "pairing_reduce", "pairing_final_exp")
gen2 = cref.g2_generator()
g2_pts = np.stack([cref.g2_mul(gen2, s) for s in rand_fr(rng, 12, full=False)])
g1_pts = cref.g1_mul_generator_vec(rand_fr(rng, 636, full=False))


def prof(name):
    ms, cnt = C.c_double(), C.c_uint64(); check(lib.mi355_profile_get(name.encode(), C.byref(ms), C.byref(cnt))); return {"ms": round(ms.value, 3), "launches": cnt.value}


def run(groups, ppg):
    n = groups * ppg
    P, Q = np.ascontiguousarray(g1_pts[:n]), np.ascontiguousarray(g2_pts[np.arange(n) % len(g2_pts)])
    call = lambda: h2.pairing_products(P, Q, groups, ppg)
    call()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
    check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1)); call(); check(lib.mi355_profile_enable(0))
    return {"wall_ms": round(statistics.median(ts), 3), "kernels": {k: prof(k) for k in KERNELS}}


res = {"metric": "pairing_products_host", "shapes": {}}
for groups, ppg in ((1, 2), (318, 2), (1, 636)):
    res["shapes"]["%dx%d" % (groups, ppg)] = run(groups, ppg)
A, B = pyref.g1_mul(pyref.G1_GEN, 5), pyref.g2_mul(pyref.G2_GEN, 7)
t0 = time.perf_counter()
ok = pairing.pairing_product_is_one([(A, B), (pyref.g1_neg(pyref.g1_mul(pyref.G1_GEN, 35)), pyref.G2_GEN)])
res["oracle_two_pair_check_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
assert ok
from verify_common import NEG_S_G2_WORDS, case, fixture_path
layer, inst, proof, okw, pkw = case("chunk_proof")
h2.verify_proof(fixture_path(layer), inst, proof, neg_s_g2=NEG_S_G2_WORDS, **pkw)          # warm-up: builds the driver when it is stale
ts = []
for _ in range(3):
    t0 = time.perf_counter(); rec = h2.verify_proof(fixture_path(layer), inst, proof, neg_s_g2=NEG_S_G2_WORDS, **pkw); ts.append((time.perf_counter() - t0) * 1e3)
assert rec["ok"] and rec["pairing"] == [1, 1]
t0 = time.perf_counter(); h2.verify_proof(fixture_path(layer), inst, proof, host_only=True, **pkw); host_ms = (time.perf_counter() - t0) * 1e3
res["verify_proof_chunk_process_ms"] = round(statistics.median(ts), 1)
res["verify_proof_chunk_host_only_process_ms"] = round(host_ms, 1)
print(json.dumps(res), flush=True)
