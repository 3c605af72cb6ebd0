"""-m gpu: the multiplicity column of the mv-lookup argument counted on the MI355X.

  * mi355_fr_lookup_multiplicities_dev (through halo2.lookup_multiplicities) against the numpy restatement (tests/lookup_common.py), every word of m: 2^4 .. 2^24 and
    2^26, random tables with scattered duplicates and a zero tail under both duplicate rules, 1 to 3 input columns, table_rows / input_rows below n, an all-zero input
    column, an all-equal table; a missing value is MI355_EBADARG with exactly the smallest (column, row); two calls give the same words.
  * create_proof with ProofOptions::device_multiplicities (tests/cpp/test_lookup_multiplicities.cpp): under the first-occurrence rule the proof bytes equal the default
    route's, where the builder's own m columns are handed in; the last-occurrence rule gives another proof that still verifies; a lookup input outside its table
    emits no proof and names the lookup and the row; one layer at k = 26."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk
from tests.lookup_common import counts_to_words, reference_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TAU0 = 0x5343524F4C4C0001
zk = ge.load_package()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    ge.build()
    zk.init(0)
    yield torch.device("cuda:0")
    zk.shutdown()


def pool_words(torch, dev, size, seed):
    """size distinct reduced words: id 0 is zero, the rest uniform below 2^252 (distinct with overwhelming probability)"""
    w = np.random.default_rng(seed).integers(0, 2**64, size=(size, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)
    w[0] = 0
    return torch.from_numpy(w.view(np.int64)).to(dev)


def gather(pool, ids, dev):
    """pool[ids] on the device, 2^22 rows per indexing call (one call over 2^26 rows is more than torch's index kernel launches)"""
    import torch
    out = torch.empty((len(ids), 4), dtype=torch.int64, device=dev)
    for lo in range(0, len(ids), 1 << 22):
        out[lo: lo + (1 << 22)] = pool[torch.from_numpy(np.ascontiguousarray(ids[lo: lo + (1 << 22)])).to(dev)]
    return out


def run_case(dev, n, table_rows, input_rows, table_ids, input_ids, pool, last):
    import torch
    table = gather(pool, table_ids, dev)
    inputs = [gather(pool, x, dev) for x in input_ids]
    m = zk.halo2.lookup_multiplicities(table, inputs, table_rows, input_rows, last=last)
    counts, miss = reference_ids(table_ids, table_rows, input_ids, input_rows, n, last)
    assert miss is None
    want = torch.from_numpy(counts_to_words(counts).view(np.int64)).to(dev)
    assert torch.equal(m, want), f"n={n} last={last}: {int((m != want).any(dim=1).sum())} rows differ"
    assert not m[table_rows:].any()
    return m, table, inputs


SIZES = [(4, 1), (10, 2), (16, 3), (20, 2), (24, 1)]


@pytest.mark.parametrize("log_n,cols", SIZES)
@pytest.mark.parametrize("last", [False, True])
def test_entry_point_matches_the_reference(dev, log_n, cols, last):
    import torch
    rng = np.random.default_rng(log_n * 7 + cols + (100 if last else 0))
    n = 1 << log_n
    tr, ir = n - max(1, n // 16), n - max(1, n // 8)
    P = max(4, n // 4)
    pool = pool_words(torch, dev, P + 1, log_n)
    t = rng.integers(1, P, size=n)                                   # scattered duplicates (about 4 rows per value)
    t[tr - max(1, tr // 8): tr] = 0                                  # the zero tail of a range table
    t[tr:] = P                                                       # beyond table_rows: a value no input below input_rows may find
    xs = []
    for c in range(cols):
        x = t[rng.integers(0, tr, size=n)]
        x[ir:] = P                                                   # beyond input_rows: not in the table, never read
        xs.append(x)
    m, table, inputs = run_case(dev, n, tr, ir, t, xs, pool, last)
    m2 = zk.halo2.lookup_multiplicities(table, inputs, tr, ir, last=last)
    assert torch.equal(m, m2), "two calls differ"


@pytest.mark.parametrize("log_n", [10, 20])
def test_all_zero_input_and_all_equal_table(dev, log_n):
    import torch
    n = 1 << log_n
    pool = pool_words(torch, dev, 8, 3)
    zeros = np.zeros(n, dtype=np.int64)
    mostly = np.where(np.random.default_rng(2).random(n) < 0.9, 0, 5)
    t = np.arange(n) % 7; t[n // 2:] = 0                             # 0 .. 6 repeating, then the zero tail
    for last in (False, True):
        run_case(dev, n, n, n, t, [zeros, mostly], pool, last)
        m, _, _ = run_case(dev, n, n - 3, n, np.full(n, 5), [np.full(n, 5), np.full(n, 5)], pool, last)   # one value everywhere
        row = n - 4 if last else 0
        assert m[row].any() and int((m.any(dim=1)).sum()) == 1


def test_missing_value_names_the_smallest_column_and_row(dev):
    import torch
    rng = np.random.default_rng(9)
    n = 1 << 12
    pool = pool_words(torch, dev, 1025, 4)
    t = rng.integers(0, 1000, size=n)
    xs = [t[rng.integers(0, n, size=n)] for _ in range(3)]
    xs[2][17] = 1024; xs[1][300] = 1024; xs[1][2000] = 1024; xs[2][5] = 1024
    table = gather(pool, t, dev)
    ins = [gather(pool, x, dev) for x in xs]
    for last in (False, True):
        with pytest.raises(zk.Mi355Error) as e:
            zk.halo2.lookup_multiplicities(table, ins, n, n, last=last)
        assert e.value.code == zk._capi.EBADARG and (e.value.column, e.value.row) == (1, 300), str(e.value)
    with pytest.raises(zk.Mi355Error) as e:                           # a miss beyond input_rows is not read; one beyond table_rows is not in the table
        zk.halo2.lookup_multiplicities(table, ins[2:], n, 10)
    assert (e.value.column, e.value.row) == (0, 5)
    assert reference_ids(t, n, xs, n, n)[1] == (1, 300)


def test_entry_point_at_2_26(dev):
    import torch
    n = 1 << 26
    rng = np.random.default_rng(26)
    P = 1 << 20
    pool = pool_words(torch, dev, P + 1, 26)
    tr = n - 9
    t = rng.integers(1, P, size=n, dtype=np.int64)                   # every value about 64 times, scattered
    t[1 << 25: tr] = 0
    x = t[rng.integers(0, tr, size=n)]
    m, table, inputs = run_case(dev, n, tr, n - 9, t, [x], pool, False)
    assert zk.halo2.mem_info(0)["pooled"] >= (1 << 27) * 4 + n * 4   # the call's workspace (hash slots + counts, ~12 B per row) is a pooled block, visible here
    del m, table, inputs, pool
    torch.cuda.empty_cache()
    zk._capi.check(zk._capi.lib().mi355_buf_trim())                  # the workspace block went back to the pool; the prover tests below run in other processes


# ---------------------------------------------------------------------------------------------------------------- the prover
def verify(rec):
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
    tau = TAU0 + (rec["layer"] if rec["layer"] >= 0 else 0)
    return plonk.verify(pr, rec["vk"], inst, rec["proof"], tau, transcript=rec["transcript"])["ok"]


STANDIN = dict(advice=40, fixed=8, lookups=3, perm_columns=12, degree=5)
FIRST_RULE = [(2, 7, [], {}, {}), (4, 8, [], {}, {}), (3, 9, [], {}, {}), (0, 8, [], {}, STANDIN),
              (4, 9, ["--devices", "2"], {"MI355_ALLOW_DUP_DEVICES": "1", "MI355_SHARD_MIN_LOG": "6"}, {})]


@pytest.mark.parametrize("layer,k,args,env,shape", FIRST_RULE)
def test_prover_first_rule_gives_the_default_route_s_bytes(tmp_path, layer, k, args, env, shape):
    rec = zk.replay.run_lookup_multiplicities(layer, k, out_dir=str(tmp_path), args=args, env=env, timeout=600, **shape)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    assert rec["bytes_equal"] and rec["proof"] == rec["proof_default"] and rec["rule"] == "first"
    assert rec["multiplicity_ms"] > 0
    assert verify(rec)


def test_prover_last_rule_differs_and_verifies(tmp_path):
    rec = zk.replay.run_lookup_multiplicities(4, 8, out_dir=str(tmp_path), args=["--rule", "last"], timeout=600)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    assert rec["rule"] == "last" and not rec["bytes_equal"] and rec["proof"] != rec["proof_default"]
    assert verify(rec)


def test_prover_refuses_a_lookup_input_outside_the_table(tmp_path):
    rec = zk.replay.run_lookup_multiplicities(4, 8, out_dir=str(tmp_path), args=["--corrupt-lookup"], timeout=600)
    assert rec.get("ok") and rec["returncode"] == 0, rec
    assert not rec["proof_emitted"] and rec["error_code"] == zk._capi.EBADARG
    assert "lookup 0: input row 1 is not in the table" in rec["error"]
    assert "proof" not in rec


def test_prover_full_size_layer4_k26(tmp_path):
    rec = zk.replay.run_lookup_multiplicities(4, out_dir=str(tmp_path), protocol_file=os.path.join(GOLD, "protocol_layer4.json"), timeout=1500)
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    assert rec["k"] == 26 and rec["bytes_equal"] and rec["proof"] == rec["proof_default"] and len(rec["proof"]) == 1312
