"""-m gpu: a witness judged on the MI355X -- MockProver::verify for a PlonkProtocol (csrc/check.hpp, mi355_fr_nonzero_rows_dev, mi355_fr_copy_check_dev,
plonk::check_witness, ProofOptions::check_witness).

  * mi355_fr_nonzero_rows_dev against numpy at n = 1, 63, 64, 65, 1 000, 2^16 + 3 and once at 2^20 with a batch of 3: all zero; one non-zero row at 0, at n - 1 and on
    both sides of 64 / 256 / 1 024 (the wave, the workgroup, the tile of CHECK_ITEMS x 256 words); words non-zero only in the top 32-bit limb, only in limb 0; every row
    non-zero with cap 8; cap 0; cap above the count (unused slots ~0); clean vectors between failing neighbours in one batch; two calls agree.
  * mi355_fr_copy_check_dev at (log_n, n_cols) = (1, 1), (4, 3), (10, 7), (16, 5) over the mappings of tests/test_gpu_permutation_sigma.py: columns constant on every
    cycle pass; one cell of the 17-cycle changed fails exactly the two pairs that touch it; a difference in the top limb only; count = 0; cap below the failures; a list
    over two staged pieces (2^23 pairs) with failures either side of the piece boundary; a cell out of range is EBADARG before anything is launched, and a valid call
    follows; the workspace is one pooled block that mi355_buf_trim returns.
  * the driver (tests/cpp/test_witness_check.cpp) on layers 2, 4, 3 and the layer-0 stand-in at small k against tests/witness_check_common.py: gates and copies EXACTLY
    (kinds, indices, rows, counts), lookups by their smallest missing pair -- clean, advice:0:3, a lookup input pushed out of its table, instance:0, two at once, cap 1.
  * create_proof under check_witness: throws on a corrupted witness (the message names the first failure, nothing is written), and on a clean one gives the bytes of
    the run without the check, which verify.
  * once at full size: layer 4 at k = 26 with one advice cell off; the gate rows are the ones the four-cell neighbourhood gives on the host.  check_ms is printed."""
import ctypes as C
import json

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk
from tests import perm_common as pc
from tests import witness_check_common as wc
from tests.test_gpu_permutation_sigma import mappings

TAU0 = 0x5343524F4C4C0001
NONE = (1 << 64) - 1
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


# ---------------------------------------------------------------------------------------------------------------- nonzero_rows
def expect_rows(a, cap):
    nz = np.nonzero((a != 0).any(axis=1))[0].astype(np.uint64)
    rows = np.full(cap, NONE, dtype=np.uint64)
    rows[:min(cap, nz.size)] = nz[:cap]
    return nz.size, rows


def vectors_for(n, rng):
    """name -> [n, 4] u64: every kind of vector this n has the rows for"""
    z = lambda: np.zeros((n, 4), dtype=np.uint64)
    out = {"all_zero": z()}
    for p in sorted({0, n - 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} & set(range(n))):
        v = z(); v[p, 1] = 5; out[f"single_{p}"] = v
    v = z(); v[::3, 3] = 1 << 32; v[n - 1, 3] = 1 << 63; out["top_limb_only"] = v
    v = z(); v[1::2, 0] = 1; out["limb0_only"] = v
    out["clean_between"] = z()
    v = rng.integers(1, 1 << 63, size=(n, 4), dtype=np.uint64); out["every_row"] = v
    v = z(); idx = rng.choice(n, size=max(1, n // 50), replace=False); v[idx, 2] = 7; out["sparse"] = v
    return out


def run_nonzero(dev, arrays, cap):
    import torch
    ts = [torch.from_numpy(a.view(np.int64)).to(dev) for a in arrays]
    counts, rows = zk.halo2.nonzero_rows(ts, cap)
    for v, a in enumerate(arrays):
        want_n, want_rows = expect_rows(a, cap)
        assert int(counts[v]) == want_n, (v, int(counts[v]), want_n)
        assert (rows[v] == want_rows).all(), (v, rows[v][:8], want_rows[:8])
    return counts, rows, ts


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, (1 << 16) + 3])
def test_nonzero_rows_match_numpy(dev, n):
    rng = np.random.default_rng(n)
    kinds = vectors_for(n, rng)
    arrays = list(kinds.values())
    counts, rows, ts = run_nonzero(dev, arrays, 8)
    names = list(kinds)
    assert int(counts[names.index("every_row")]) == n and list(rows[names.index("every_row")][:min(n, 8)]) == list(range(min(n, 8)))
    assert int(counts[names.index("clean_between")]) == 0 and (rows[names.index("clean_between")] == NONE).all()
    again = zk.halo2.nonzero_rows(ts, 8)
    assert (again[0] == counts).all() and (again[1] == rows).all(), "two calls differ"
    c0, r0 = zk.halo2.nonzero_rows(ts, 0)                                  # counts only
    assert (c0 == counts).all() and r0.shape == (len(arrays), 0)
    run_nonzero(dev, arrays, min(65536, 2 * n + 5))                        # cap above every count: the whole list, then ~0
    run_nonzero(dev, [kinds["sparse"]], 1)


def test_nonzero_rows_at_2_20_with_a_batch_of_3(dev):
    n = 1 << 20
    rng = np.random.default_rng(20)
    a = np.zeros((n, 4), dtype=np.uint64); a[rng.choice(n, size=1000, replace=False), 3] = 1 << 40
    b = np.zeros((n, 4), dtype=np.uint64)
    c = rng.integers(1, 1 << 63, size=(n, 4), dtype=np.uint64); c[12345] = 0
    run_nonzero(dev, [a, b, c], 16)
    run_nonzero(dev, [a], 2000)                                            # more failures than one workgroup holds: ranks across many workgroups


def test_nonzero_rows_rejects_bad_arguments(dev):
    import torch
    lib = zk._capi.lib()
    t = torch.zeros((8, 4), dtype=torch.int64, device=dev)
    arr = (C.c_void_p * 1)(t.data_ptr())
    counts = np.full(1, 77, dtype=np.uint64); rows = np.full(8, 77, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    cp, rp = counts.ctypes.data_as(u64p), rows.ctypes.data_as(u64p)
    assert lib.mi355_fr_nonzero_rows_dev(arr, 0, 8, 8, cp, rp) == zk._capi.EBADARG        # batch == 0
    assert lib.mi355_fr_nonzero_rows_dev(arr, 1, 0, 8, cp, rp) == zk._capi.EBADARG        # n == 0
    assert lib.mi355_fr_nonzero_rows_dev(arr, 1, 8, 65537, cp, rp) == zk._capi.EBADARG    # cap > 65536
    assert (counts == 77).all() and (rows == 77).all()
    assert lib.mi355_fr_nonzero_rows_dev(arr, 1, 8, 0, cp, None) == zk._capi.OK and counts[0] == 0


# ---------------------------------------------------------------------------------------------------------------- copy_check
def cycle_labels(mapping):
    """the smallest cell of every cell's cycle (pointer doubling)"""
    lab = np.arange(mapping.size, dtype=np.int64); m = mapping.astype(np.int64)
    for _ in range(max(1, int(mapping.size).bit_length())):
        lab = np.minimum(lab, lab[m]); m = m[m]
    return lab


def words_of(labels):
    w = np.zeros((labels.size, 4), dtype=np.uint64)
    w[:, 0] = labels.astype(np.uint64) + 1
    w[:, 3] = (labels.astype(np.uint64) * np.uint64(2654435761)) & np.uint64((1 << 60) - 1)
    return w


def run_copy(dev, n_cols, log_n, words, cells, images, cap):
    import torch
    n = 1 << log_n
    cols = [torch.from_numpy(words[j * n:(j + 1) * n].view(np.int64).copy()).to(dev) for j in range(n_cols)]
    n_failed, failed = zk.halo2.copy_check(cols, cells, images, cap)
    ci, ii = np.asarray(cells, dtype=np.int64), np.asarray(images, dtype=np.int64)
    bad = np.nonzero((words[ci] != words[ii]).any(axis=1))[0].astype(np.uint64) if ci.size else np.zeros(0, dtype=np.uint64)
    want = np.full(cap, NONE, dtype=np.uint64); want[:min(cap, bad.size)] = bad[:cap]
    assert n_failed == bad.size and (failed == want).all(), (n_failed, bad.size, failed[:8], want[:8])
    return bad


@pytest.mark.parametrize("log_n,n_cols", [(1, 1), (4, 3), (10, 7), (16, 5)])
def test_copy_check_over_the_mappings_of_the_sigma_tests(dev, log_n, n_cols):
    n = 1 << log_n
    for name, copies in mappings(n_cols, log_n).items():
        mapping = pc.cpp_mapping(n_cols, n, copies)
        cells, images = pc.cpp_overrides(n_cols, n, mapping)
        words = words_of(cycle_labels(mapping))
        assert run_copy(dev, n_cols, log_n, words, cells, images, 16).size == 0, name           # constant on every cycle (count = 0 for no_copies)
        if name == "cycle_17":
            x = int(cells[5])
            w = words.copy(); w[x, 1] ^= 9
            bad = run_copy(dev, n_cols, log_n, w, cells, images, 16)
            assert sorted(bad) == sorted([int(np.nonzero(cells == x)[0][0]), int(np.nonzero(images == x)[0][0])]) and len(bad) == 2
            run_copy(dev, n_cols, log_n, w, cells, images, 1)                                    # cap below the failures
            run_copy(dev, n_cols, log_n, w, cells, images, 0)
            w = words.copy(); w[x, 3] ^= 1 << 63                                                 # the two cells differ in the top limb only
            assert run_copy(dev, n_cols, log_n, w, cells, images, 16).size == 2
        if name == "whole_column" and n > 1:
            w = words_of(np.arange(n_cols * n))                                                  # every cell its own value: every pair fails
            bad = run_copy(dev, n_cols, log_n, w, cells, images, 8)
            assert bad.size == len(cells) == n


def test_copy_check_over_two_staged_pieces(dev):
    log_n, n_cols = 20, 8
    total = n_cols << log_n                                                                      # 2^23 pairs: two pieces of 2^22
    cells = np.arange(total, dtype=np.uint64); images = (cells + np.uint64(1)) % np.uint64(total)
    words = np.zeros((total, 4), dtype=np.uint64); words[:, 0] = 3
    for x in (5, (1 << 22) - 1, 1 << 22, 6_000_000, total - 1):
        words[x, 2] = x
    bad = run_copy(dev, n_cols, log_n, words, cells, images, 16)
    # pair t compares cells t and t + 1: a changed cell x fails pairs x - 1 and x; the neighbours 2^22 - 1 and 2^22 share pair 2^22 - 1, so 5 cells give 9 pairs
    assert list(bad) == [4, 5, (1 << 22) - 2, (1 << 22) - 1, 1 << 22, 5_999_999, 6_000_000, total - 2, total - 1]
    run_copy(dev, n_cols, log_n, words, cells, images, 3)


def test_copy_check_rejects_a_cell_out_of_range_and_leaves_one_pooled_block(dev):
    import torch
    log_n, n_cols = 10, 3
    n, total = 1 << log_n, 3 << 10
    lib = zk._capi.lib()
    cols = [torch.zeros((n, 4), dtype=torch.int64, device=dev) for _ in range(n_cols)]
    arr = (C.c_void_p * n_cols)(*[c.data_ptr() for c in cols])
    u64p = C.POINTER(C.c_uint64)
    nf = C.c_uint64(77); failed = np.full(4, 77, dtype=np.uint64)
    for cells, images, where in (([5, total, 9], [9, 5, 5], "pair 1"), ([5, 9, 12], [9, 5, NONE], "pair 2")):
        c, i = np.array(cells, dtype=np.uint64), np.array(images, dtype=np.uint64)
        assert lib.mi355_fr_copy_check_dev(arr, n_cols, log_n, c.ctypes.data_as(u64p), i.ctypes.data_as(u64p), 3, 4, C.byref(nf), failed.ctypes.data_as(u64p)) == zk._capi.EBADARG
        assert where in lib.mi355_last_error().decode() and nf.value == 77 and (failed == 77).all()
    assert lib.mi355_fr_copy_check_dev(arr, 0, log_n, None, None, 0, 4, C.byref(nf), failed.ctypes.data_as(u64p)) == zk._capi.EBADARG      # n_cols == 0
    assert lib.mi355_fr_copy_check_dev(arr, n_cols, 29, None, None, 0, 4, C.byref(nf), failed.ctypes.data_as(u64p)) == zk._capi.EBADARG   # log_n > 28
    assert lib.mi355_fr_copy_check_dev(arr, n_cols, log_n, None, None, 0, 65537, C.byref(nf), failed.ctypes.data_as(u64p)) == zk._capi.EBADARG
    assert nf.value == 77 and (failed == 77).all()
    zk._capi.check(lib.mi355_buf_trim())
    before = zk.halo2.mem_info(0)
    cols[1][9, 0] = 1
    n_failed, ft = zk.halo2.copy_check(cols, [5, n + 9], [n + 9, 5], 4)                         # a valid call afterwards
    assert n_failed == 2 and list(ft) == [0, 1, NONE, NONE]
    after = zk.halo2.mem_info(0)
    assert after["live_buffers"] == before["live_buffers"] and after["workspace"] == before["workspace"], "the call left something live behind"
    assert after["pooled"] > before["pooled"], "the workspace block is not visible as pooled memory"
    zk._capi.check(lib.mi355_buf_trim())
    assert zk.halo2.mem_info(0)["pooled"] == before["pooled"]


# ---------------------------------------------------------------------------------------------------------------- the driver
STANDIN = dict(advice=40, fixed=8, lookups=3, perm_columns=12, degree=5)
LAYERS = [(2, 7, {}), (4, 8, {}), (3, 9, {}), (0, 8, STANDIN)]
CASES = ["clean", "advice", "lookup_input", "instance", "two", "cap1"]


def corruptions(case, layer, k, shape):
    if case == "lookup_input":                                                                   # far outside every table of the builder (at most 2^16 rows)
        col, row = wc.first_lookup_input(plonk.Protocol(zk.protocols.layer_protocol(layer, k, **shape)))
        return [f"advice:{col}:{row}:{1 << 40}"]
    return {"clean": [], "advice": ["advice:0:3"], "instance": ["instance:0"], "two": ["advice:0:3", "instance:0"], "cap1": ["advice:0:3", "instance:0"]}[case]


def check_against_reference(rec, cap):
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    ref = wc.Reference(rec["out_dir"])
    got = rec["check"]["failures"]
    assert [f for f in got if f["kind"] != "lookup"] == wc.expected_failures(ref, cap), "gates / copies differ from the definition"
    assert {f["index"]: (f["col_a"], f["row"], f["count"]) for f in got if f["kind"] == "lookup"} == {l: (0, row, 1) for l, row in ref.lookups().items()}
    assert rec["check"]["check_ms"] > 0 and rec["failures"] == len(got)
    return ref, got


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("layer,k,shape", LAYERS)
def test_driver_reports_what_the_definition_reports(tmp_path, layer, k, shape, case):
    cap = 1 if case == "cap1" else 16
    args = [x for c in corruptions(case, layer, k, shape) for x in ("--corrupt", c)] + ["--cap", str(cap)]
    ref, got = check_against_reference(zk.replay.run_witness_check(layer, k, out_dir=str(tmp_path), args=args, timeout=600, **shape), cap)
    kinds = {f["kind"] for f in got}
    if case == "clean":
        assert got == []
    if case in ("advice", "two", "cap1"):
        assert "gate" in kinds
    if case == "lookup_input":
        assert "lookup" in kinds
    if case in ("instance", "two", "cap1"):
        assert "copy" in kinds and (case != "instance" or "gate" not in kinds)
    if case == "cap1":
        cp = [f for f in got if f["kind"] == "copy"]
        assert len(cp) == 1 and cp[0]["count"] == 2, "cap bounds the list, not the count"


# ---------------------------------------------------------------------------------------------------------------- create_proof under check_witness
def test_create_proof_refuses_a_corrupted_witness(tmp_path):
    rec = zk.replay.run_witness_check(4, 8, out_dir=str(tmp_path), args=["--corrupt", "advice:0:3", "--prove"], timeout=600)
    ref, got = check_against_reference(rec, 16)
    first = got[0]
    assert rec["prove"]["threw"] is True and rec["prove"]["proof_written"] is False and "proof" not in rec
    assert f"gate constraint {first['index']} fails at row {first['row']} ({first['count']} rows in all)" in rec["prove"]["message"]


def test_create_proof_of_a_clean_witness_is_unchanged_by_the_check(tmp_path):
    rec = zk.replay.run_witness_check(4, 8, out_dir=str(tmp_path), args=["--prove"], timeout=600)
    check_against_reference(rec, 16)
    assert rec["prove"] == {"threw": False, "message": "", "proof_written": True}
    assert rec["proof"] == rec["proof_plain"] and len(rec["proof"]) == 1312 and rec["proofs_equal"] is True
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
    assert plonk.verify(pr, rec["vk"], inst, rec["proof"], TAU0 + 4, transcript=rec["transcript"])["ok"]


# ---------------------------------------------------------------------------------------------------------------- full size, once
def test_layer4_at_k26_names_the_rows_around_one_corrupted_cell(tmp_path):
    """advice cell (0, 3) is the output of the vertical gate q (a + a(wX) a(w^2 X) - a(w^3 X)) at row 0 and an operand at rows 1 .. 3; q is 1 on the first row of every
    used block only (rows 0, 4, ..), so of the four rows whose gate reads the cell exactly row 0 is switched on: the first gate constraint fails there and nowhere else.
    The dump is not read back here (gigabytes): the expectation is this host-side reasoning, which the small-k cases hold equal to the definition."""
    rec = zk.replay.run_witness_check(4, None, out_dir=str(tmp_path), args=["--corrupt", "advice:0:3", "--no-dump", "--threads", "16"], timeout=1500)
    assert rec.get("ok") and rec["k"] == 26, rec.get("error")
    got = rec["check"]["failures"]
    print("check_ms at layer 4, k = 26:", rec["check"]["check_ms"])
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    first = wc.gate_indices(pr)[0]
    assert [(f["kind"], f["index"], f["row"], f["count"]) for f in got] == [("gate", first, 0, 1)]
