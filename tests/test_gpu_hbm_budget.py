"""-m gpu: the memory limit the library keeps (mi355_mem_set_limit / _usage / _reset_peak over csrc/mem_budget.hpp) and the quotient in coset groups
(ProofOptions::coset_group_polys, tests/cpp/test_hbm_budget.cpp).

  * the limit holds: three 32 MiB blocks fit a limit of held + 3 blocks, the fourth is refused ON THE HOST (MI355_EOOM naming the limit; the refused counter grows, held does
    not, hipMemGetInfo's free figure stays where it was), succeeds from the pool after one free, and any size succeeds once the limit is lifted;
  * the optional NTT tables are counted and reclaimed: coset transforms at 2^12 and 2^16 with three factors each and an inverse with a divisor leave optional tables; held is
    the sum of what mi355_mem_info reports and the table / SRS classes, to the byte; an allocation that only fits without the tables gets them reclaimed; the same transforms
    then run table-free and, with the limit lifted, with rebuilt tables -- every word equal to the oracle's each time;
  * grouped proofs are the same proofs: bytes equal to the ungrouped route's and accepted by oracle/plonk.py, key resident and lean, on two device slots, with the
    multiplicities made on the device; coset_ntt is the ungrouped count plus the re-transforms;
  * it fits where the other does not: with the limit midway between the two routes' high-water marks the grouped proof succeeds below it, the ungrouped one is refused naming
    the limit, and a grouped proof after that still succeeds.
No test approaches the device's real memory and no refusal here is a HIP error: every one is the ledger's own, made before any HIP call.  The byte-exact cases run in a child
process under MI355_BUF_ARENA=0 (one allocation per block: the 1 GiB slabs would blur small shapes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import cref, plonk, pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU0 = 0x5343524F4C4C0001
zk = ge.load_package()
pytestmark = pytest.mark.gpu
MiB = 1 << 20


def child(name):
    """tests.test_gpu_hbm_budget.<name>() in a process of its own, slabs off; returns the JSON line it printed"""
    ge.build()
    code = "import sys; sys.path.insert(0, %r); import tests.test_gpu_hbm_budget as t; t.%s()" % (ROOT, name)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, MI355_BUF_ARENA="0"))
    line = next((l for l in r.stdout.splitlines() if l.startswith("{")), None)
    assert r.returncode == 0 and line, (r.stdout[-800:], r.stderr[-2500:])
    return json.loads(line)


# ---------------------------------------------------------------------------------------------------------------- the limit holds
def _limit_child():
    h2 = zk.halo2
    zk.init(0)
    out = {}
    warm = h2.DeviceBuffer(4096); warm.free()                                 # the runtime's own first-allocation overheads are behind us
    zk._capi.check(zk._capi.lib().mi355_buf_trim())
    B = 32 * MiB
    free0 = h2.mem_info()["free"]
    u0 = h2.mem_usage()
    h2.mem_set_limit(u0["held"] + 3 * B)
    blocks = [h2.DeviceBuffer(B) for _ in range(3)]
    u3 = h2.mem_usage()
    try:
        h2.DeviceBuffer(B); out["fourth"] = "allocated"
    except zk.Mi355Error as e:
        out["fourth"] = {"code": e.code, "msg": str(e)}
    u4 = h2.mem_usage()
    free4 = h2.mem_info()["free"]
    blocks.pop().free()
    again = h2.DeviceBuffer(B)                                                # the freed block, from the pool: nothing is asked of the allocator
    u5 = h2.mem_usage()
    h2.mem_set_limit(0)
    big = h2.DeviceBuffer(8 * B)
    u6 = h2.mem_usage()
    free6 = h2.mem_info()["free"]
    for b in blocks + [again, big]:
        b.free()
    zk._capi.check(zk._capi.lib().mi355_buf_trim())
    out.update(B=B, u0=u0, u3=u3, u4=u4, u5=u5, u6=u6, free0=free0, free4=free4, free6=free6, u_end=h2.mem_usage())
    zk.shutdown()
    print(json.dumps(out))


def test_the_limit_holds():
    r = child("_limit_child")
    B, u0, u3, u4, u5, u6 = r["B"], r["u0"], r["u3"], r["u4"], r["u5"], r["u6"]
    limit = u0["held"] + 3 * B
    assert u3["held"] == limit and u3["limit"] == limit and u3["classes"]["buffers"] == u0["classes"]["buffers"] + 3 * B
    assert r["fourth"] != "allocated" and r["fourth"]["code"] == zk._capi.EOOM, r["fourth"]
    assert str(limit) in r["fourth"]["msg"] and "limit" in r["fourth"]["msg"] and str(B) in r["fourth"]["msg"], r["fourth"]["msg"]
    assert u4["refused"] == u3["refused"] + B and u4["held"] == u3["held"] and u4["high_water"] == limit
    assert u5["held"] == limit and u5["refused"] == u4["refused"]
    assert u6["held"] == limit + 8 * B and u6["limit"] == 0
    # the refusal never reached the allocator: between the start and the refused call the device lost the three blocks (and the allocator's rounding), no more
    assert r["free0"] - r["free4"] <= 3 * B + 8 * MiB, (r["free0"], r["free4"])
    assert r["free0"] - r["free6"] <= 11 * B + 16 * MiB
    assert r["u_end"]["held"] == u0["held"] and r["u_end"]["high_water"] >= u6["held"]


# ---------------------------------------------------------------------------------------------------------------- tables are counted and reclaimed
def _powers_mont(f, n):
    out = np.empty((n, 4), dtype=np.uint64); v = pyref.MONT_R % pyref.R_MOD
    for i in range(n):
        out[i] = pyref.to_limbs(v); v = v * f % pyref.R_MOD
    return out


def _tables_child():
    h2 = zk.halo2
    zk.init(0)
    rng = np.random.default_rng(5)
    cases = []
    for k in (12, 16):
        dom = h2.EvaluationDomain(4, k); n = 1 << k
        a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64); a[:, 3] &= np.uint64((1 << 60) - 1)
        want = []
        for part in range(3):
            f = h2.FR_ZETA * pow(dom._extended_omega, part, pyref.R_MOD) % pyref.R_MOD
            want.append(cref.best_fft(cref.f_mul_vec(cref.FR, a, _powers_mont(f, n)), dom.omega, k, threads=4))
        inv = cref.f_mul_vec(cref.FR, cref.best_fft(a, dom.omega_inv, k, threads=4), np.tile(dom.ifft_divisor, (n, 1)))
        cases.append((dom, a, want, inv))

    def run_all():
        ok = True
        for dom, a, want, inv in cases:
            d = h2.DeviceBuffer.from_host(a); o = h2.DeviceBuffer(a.nbytes)
            for part in range(3):
                dom.coeff_to_extended_part(d, part, o)
                ok = ok and bool((o.fr() == want[part]).all())
            dom.lagrange_to_coeff(d)
            ok = ok and bool((d.fr() == inv).all())
            d.free(); o.free()
        zk._capi.check(zk._capi.lib().mi355_buf_trim())
        return ok

    out = {"first_equal": run_all()}
    u1, i1 = h2.mem_usage(), h2.mem_info()
    B = 4 * MiB
    h2.mem_set_limit(u1["held"] + B - 4096)                                   # just below held + one block: the block fits only without the tables
    blk = h2.DeviceBuffer(B)
    u2 = h2.mem_usage()
    out["second_equal"] = run_all()                                           # table-free forms (what does not fit the limit is not built)
    u3 = h2.mem_usage()
    h2.mem_set_limit(0)
    out["third_equal"] = run_all()                                            # the tables are rebuilt
    u4 = h2.mem_usage()
    blk.free()
    out.update(B=B, u1=u1, i1=i1, u2=u2, u3=u3, u4=u4)
    zk.shutdown()
    print(json.dumps(out))


def test_tables_are_counted_and_reclaimed():
    r = child("_tables_child")
    u1, i1, u2, u3, u4, B = r["u1"], r["i1"], r["u2"], r["u3"], r["u4"], r["B"]
    assert r["first_equal"] and r["second_equal"] and r["third_equal"]
    c1 = u1["classes"]
    assert c1["ntt_optional"] >= 3 * 36 * (1 << 16) and c1["ntt_required"] > 0                    # at least the three [k][column] tables of the 2^16 coset factors
    assert u1["held"] == sum(c1.values())
    assert u1["held"] == i1["live_buffers"] + i1["pooled"] + i1["workspace"] + c1["ntt_required"] + c1["ntt_optional"] + c1["srs"] + c1["window_tables"] + c1["fixed_tables"]
    assert c1["buffers"] == i1["live_buffers"] + i1["pooled"] and c1["workspace"] == i1["workspace"] and c1["srs"] == 0
    assert c1["ntt_optional"] > B                                                                  # so that giving them back makes room for the block
    # the block was served only by reclaiming: the optional class is empty, a reclaim is counted, nothing was refused, the limit held
    assert u2["classes"]["ntt_optional"] == 0 and u2["reclaims"] > u1["reclaims"] and u2["refused"] == u1["refused"]
    assert u2["held"] <= u2["limit"] and u2["classes"]["buffers"] == c1["buffers"] + B
    assert u3["held"] <= u3["limit"] == u2["limit"]                                                 # the second run stayed below it: what did not fit was not built
    # rebuilt: at least the three coset tables of 2^16 again.  (Not necessarily every byte of the first run: a plan that was rebuilt under the limit without its 2-D level
    # table keeps the lo x hi pair until it is rebuilt the next time.)
    assert u4["classes"]["ntt_optional"] >= 3 * 36 * (1 << 16) and u4["classes"]["ntt_optional"] >= u3["classes"]["ntt_optional"]
    assert u4["limit"] == 0


# ---------------------------------------------------------------------------------------------------------------- grouped proofs are the same proofs
def verify(rec, proof):
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
    tau = TAU0 + (rec["layer"] if rec["layer"] >= 0 else 0)
    return plonk.verify(pr, rec["vk"], inst, proof, tau, transcript=rec["transcript"])["ok"]


STANDIN = dict(advice=40, fixed=8, lookups=3, perm_columns=12, degree=5)     # the layer-0 stand-in of the other prover tests: 40 advice columns
DUP = {"MI355_ALLOW_DUP_DEVICES": "1", "MI355_SHARD_MIN_LOG": "6"}
LEAN = ["--pk-cosets", "on-the-fly"]
# layer, k, group, arguments, environment, shape, cut (the plan has more than G operands: at least two groups and one re-transform)
SAME = [
    (3, 8, "24", [], {}, {}, True), (3, 8, "24", LEAN, {}, {}, True),
    (0, 7, "24", [], {}, STANDIN, True), (0, 8, "24", LEAN, {}, STANDIN, True),
    (0, 8, "40", [], {}, STANDIN, True), (0, 7, "40", LEAN, {}, STANDIN, True),
    (2, 8, "24", [], {}, {}, False), (2, 8, "24", LEAN, {}, {}, False),                           # one group: the degenerate case
    (3, 8, "24", ["--devices", "2"], DUP, {}, True),
    (0, 8, "24", LEAN + ["--devices", "2"], DUP, STANDIN, True),
    (0, 8, "24", ["--device-multiplicities"], {}, STANDIN, True),
]


@pytest.mark.parametrize("layer,k,group,args,env,shape,cut", SAME)
def test_grouped_proof_is_the_ungrouped_proof(tmp_path, layer, k, group, args, env, shape, cut):
    rec = zk.replay.run_hbm_budget(layer, k, out_dir=str(tmp_path), args=["--group", group] + args, env=env, timeout=600, **shape)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    a, b = rec["ungrouped"], rec["grouped"]
    print(json.dumps({"ungrouped": a, "grouped": b}))
    assert rec["equal"] and rec["proof_grouped"] == rec["proof_ungrouped"] and len(rec["proof_grouped"]) == b["proof_bytes"] > 0
    assert verify(rec, rec["proof_grouped"])
    assert a["coset_groups"] == 0 and a["coset_retransforms"] == 0
    if cut:
        assert b["coset_groups"] >= 2 and b["coset_retransforms"] >= 1
    else:
        assert b["coset_groups"] == 1 and b["coset_retransforms"] == 0
    assert b["coset_ntt"] == a["coset_ntt"] + b["coset_retransforms"]
    assert b["gate_launches"] == a["gate_launches"]


def test_group_below_one_launch_is_refused(tmp_path):
    rec = zk.replay.run_hbm_budget(2, 7, out_dir=str(tmp_path), args=["--group", "23"], timeout=600)
    assert not rec.get("ok") and "coset_group_polys must be 0 or at least 24" in rec.get("error", ""), rec


# ---------------------------------------------------------------------------------------------------------------- it fits where the other does not
FIT_K = 12


def test_grouped_fits_where_ungrouped_does_not(tmp_path):
    """layer 3, lean key, G = 24, slabs off, at k = 12: the smallest k tried, and the margin is already 238 vectors of 128 KiB.  Measured once on one MI355X (high-water marks of
    one proof; key, SRS and workspace included): ungrouped 317 666 011 bytes, grouped 286 470 875 bytes, so the limit sits at 302 068 443.  The ungrouped route holds one coset
    part of each of its 330 operands (330 x 128 KiB = 41 MiB at k = 12), the grouped one at most 24."""
    rec = zk.replay.run_hbm_budget(3, FIT_K, out_dir=str(tmp_path), args=["--group", "24", "--fit"] + LEAN, env={"MI355_BUF_ARENA": "0"}, timeout=600)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    a, b, f = rec["ungrouped"], rec["grouped"], rec["fit"]
    print(json.dumps({"ungrouped_high_water": a["high_water"], "grouped_high_water": b["high_water"], "fit": f}))
    per = 32 << FIT_K
    # a clear margin.  Step 7 holds 330 part buffers ungrouped and at most 24 grouped; another step may set the grouped route's peak instead -- step 4 holds, beside what step 7
    # also holds, at most one early coefficient copy of each of the ~140 witness polynomials and a few temporaries -- so at least 330 - 24 - 140 - 16 = 150 buffers separate the two
    assert a["high_water"] - b["high_water"] >= 150 * per
    assert b["high_water"] < f["limit"] < a["high_water"]
    assert rec["equal"] and verify(rec, rec["proof_grouped"])
    assert f["grouped_ok"] and f["grouped_equal"] and f["grouped_high_water"] <= f["limit"], f
    assert f["ungrouped_code"] == zk._capi.EOOM and "limit" in f["ungrouped_error"] and str(f["limit"]) in f["ungrouped_error"] and f["refused_grew"], f
    assert f["grouped_again_ok"] and f["grouped_again_equal"], f
