"""-m gpu: the sigma columns of the permutation argument built on the MI355X from the copy mapping.

  * mi355_fr_permutation_sigma_dev (through halo2.permutation_sigma) against the definition: sigma[j][r] = delta^j' omega^r' for (j', r') = mapping[j][r], the words
    computed from Python integers (tests/perm_common.py sigma_words, oracle.pyref's constants), EVERY word of every column, at (log_n, n_cols) = (1, 1), (4, 3), (10, 7),
    (13, 2), (16, 5), (4, 17), (6, 33) (more columns than one tile of k_perm_identity) and once at (20, 8).  Mappings come from halo2::PermutationAssembly (the C++ one, which tests/test_permutation_sigma_surface.py holds equal to
    the Python one): no copies, 2-cycles, cycles of 3 and 17 across columns, one cycle through a whole column, a cycle through (0, 0), (last column, n - 1) and the
    rows next to every power of two (where the high / low split of the omega table could go wrong), lists of 1, 255, 256, 257 and n_cols * n overrides -- every kind
    the size has the cells for.  Two calls give the same words; count == 0 equals distribute_powers of the constant column delta^j.
  * rejected lists (a cell out of range, a cell twice, images that are not the cells) leave marker-filled columns untouched -- no kernel is launched for them -- and a
    valid call afterwards succeeds; the call leaves nothing live behind but a pooled block, which mi355_buf_trim returns.
  * keygen(..., device_sigma = true) (tests/cpp/test_permutation_keygen.cpp): the verifying key and the proof are the default route's bytes, and the proof verifies."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk, pyref
from tests import perm_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def consts(log_n):
    return zk.halo2.fr(pc.DELTA), zk.halo2.fr(pyref.omega(log_n))


@functools.lru_cache(maxsize=2)
def identity_words(n_cols, log_n):
    """computed once per size and shared (read-only) by the cases of that size"""
    w = pc.sigma_words(n_cols, log_n, np.arange(n_cols << log_n, dtype=np.uint64))
    w.setflags(write=False)
    return w


def expected(n_cols, log_n, mapping):
    ident = identity_words(n_cols, log_n).reshape(-1, 4)
    out = ident.copy()
    moved = np.nonzero(mapping != np.arange(mapping.size, dtype=np.uint64))[0]
    out[moved] = ident[mapping[moved].astype(np.int64)]
    return out.reshape(n_cols, 1 << log_n, 4)


def chain(cells):
    return [(a[0], a[1], b[0], b[1]) for a, b in zip(cells, cells[1:])]


def mappings(n_cols, log_n):
    """name -> copies ([m, 4]) for every kind of mapping this size has the cells for"""
    n, last = 1 << log_n, n_cols - 1
    total = n_cols * n
    cell = lambda c: (c // n, c % n)
    out = {"no_copies": []}
    if total >= 4:
        out["two_cycles"] = [(0, 0, last, n - 1), (0, 1, last, n - 2)] + [(j % n_cols, (7 * j + 2) % n, (j + 1) % n_cols, (11 * j + 3) % n) for j in range(min(40, n // 4)) if n >= 16]
    for length in (3, 17):
        if total >= 2 * length:
            out[f"cycle_{length}"] = chain([((3 * i) % n_cols, (5 * i + 1) % n) for i in range(length)] if n * n_cols >= 64 else [cell(i) for i in range(length)])
    out["whole_column"] = chain([(last, r) for r in range(n)])       # the rotation of the last column
    edge = [(0, 0), (last, n - 1)]
    for i in range(1, log_n + 1):
        for r in ((1 << i) - 1, (1 << i) + 1 if i < log_n else None, 1 << i if i < log_n else None):
            if r is not None and 0 < r < n - 1:
                edge.append(((i + r) % n_cols, r))
    edge = list(dict.fromkeys(edge))
    if len(edge) >= 2:
        out["powers_of_two_edges"] = chain(edge)
    for count in (255, 256, 257):
        if total >= count:
            stride = max(1, total // count)
            out[f"count_{count}"] = chain([cell(i * stride) for i in range(count)])
    return out


def run(dev, n_cols, log_n, mapping, cells=None, images=None, trusted=False):
    import torch
    delta, omega = consts(log_n)
    if cells is None:
        cells, images = pc.cpp_overrides(n_cols, 1 << log_n, mapping)
    cols = zk.halo2.permutation_sigma(n_cols, log_n, delta, omega, cells, images, device=dev, trusted=trusted)
    want = torch.from_numpy(expected(n_cols, log_n, mapping).view(np.int64)).to(dev)
    for j in range(n_cols):
        assert torch.equal(cols[j], want[j]), f"(log_n {log_n}, n_cols {n_cols}) column {j}: {int((cols[j] != want[j]).any(dim=1).sum())} rows differ"
    return cols, len(cells)


SIZES = [(1, 1), (4, 3), (10, 7), (13, 2), (16, 5), (4, 17), (6, 33)]   # the last two: a second and a third column tile of k_perm_identity (PERM_COL_TILE = 16), both clamped


@pytest.mark.parametrize("log_n,n_cols", SIZES)
def test_entry_point_matches_the_definition(dev, log_n, n_cols):
    import torch
    n, total = 1 << log_n, n_cols << log_n
    kinds = mappings(n_cols, log_n)
    assert log_n < 10 or {"two_cycles", "cycle_3", "cycle_17", "whole_column", "powers_of_two_edges", "count_255", "count_256", "count_257"} <= set(kinds)
    for name, copies in kinds.items():
        mapping = pc.cpp_mapping(n_cols, n, copies)
        cols, count = run(dev, n_cols, log_n, mapping)
        if name.startswith("count_"):
            assert count == int(name[6:])
        if name == "whole_column":
            assert count == (n if n > 1 else 0)
            again, _ = run(dev, n_cols, log_n, mapping)
            assert all(torch.equal(a, b) for a, b in zip(cols, again)), "two calls differ"
    # one override (a cell listed with itself), and the dense list: every cell listed, most with themselves
    ident = np.arange(total, dtype=np.uint64)
    run(dev, n_cols, log_n, ident, cells=ident[total - 1:], images=ident[total - 1:])
    both = [c for k in ("two_cycles", "cycle_17", "powers_of_two_edges") if k in kinds for c in kinds[k]] or kinds["whole_column"]
    mapping = pc.cpp_mapping(n_cols, n, both)
    run(dev, n_cols, log_n, mapping, cells=ident, images=mapping)
    run(dev, n_cols, log_n, mapping, cells=ident, images=mapping, trusted=True)


def test_entry_point_at_2_20_with_8_columns(dev):
    log_n, n_cols = 20, 8
    n = 1 << log_n
    kinds = mappings(n_cols, log_n)
    kinds.pop("no_copies")
    whole = kinds.pop("whole_column")
    copies = [c for k in sorted(kinds) for c in kinds[k]]             # every sparse kind at once (they may share cells: the assembly merges their cycles)
    mapping = pc.cpp_mapping(n_cols, n, copies + whole)
    cols, count = run(dev, n_cols, log_n, mapping)
    assert count > n
    del cols
    ident = np.arange(n_cols * n, dtype=np.uint64)
    run(dev, n_cols, log_n, mapping, cells=ident, images=mapping)     # count == n_cols * n: two staged pieces


@pytest.mark.parametrize("log_n,n_cols", [(4, 3), (16, 5)])
def test_no_overrides_is_distribute_powers_of_the_delta_column(dev, log_n, n_cols):
    import torch
    n = 1 << log_n
    delta, omega = consts(log_n)
    cols = zk.halo2.permutation_sigma(n_cols, log_n, delta, omega, device=dev)
    lib, ptr = zk._capi.lib(), zk._capi.ptr
    for j in range(n_cols):
        const = torch.from_numpy(np.tile(zk.halo2.fr(pow(pc.DELTA, j, pc.R)), (n, 1)).view(np.int64)).to(dev)
        zk._capi.check(lib.mi355_distribute_powers_fr_dev(ptr(const), n, ptr(omega)))
        zk._capi.check(lib.mi355_synchronize())
        assert torch.equal(cols[j], const), j


def test_rejected_lists_leave_the_columns_untouched(dev):
    import torch
    log_n, n_cols = 10, 3
    n, total = 1 << log_n, 3 << 10
    delta, omega = consts(log_n)
    marker = 0x5A5A5A5A5A5A5A5A
    cols = [torch.full((n, 4), marker, dtype=torch.int64, device=dev) for _ in range(n_cols)]
    bad = {
        "cell out of range": ([5, total, 9], [9, 5, total], "override 1"),
        "image out of range": ([5, 9, 12], [9, 5, (1 << 64) - 1], "override 2"),
        "cell twice": ([5, 9, 5], [9, 5, 9], "override 2"),
        "images are not the cells": ([5, 9, 12], [9, 5, 13], "override 2"),
    }
    for name, (cells, images, where) in bad.items():
        with pytest.raises(zk.Mi355Error) as e:
            zk.halo2.permutation_sigma(n_cols, log_n, delta, omega, cells, images, out=cols)
        assert e.value.code == zk._capi.EBADARG and where in str(e.value), (name, str(e.value))
        zk._capi.check(zk._capi.lib().mi355_synchronize())
        assert all(bool((c == marker).all()) for c in cols), name
    lib, ptr = zk._capi.lib(), zk._capi.ptr
    arr = (C.c_void_p * n_cols)(*[c.data_ptr() for c in cols])
    assert lib.mi355_fr_permutation_sigma_dev(arr, 0, log_n, ptr(delta), ptr(omega), None, None, 0, 0) == zk._capi.EBADARG        # n_cols == 0
    assert lib.mi355_fr_permutation_sigma_dev(arr, n_cols, 29, ptr(delta), ptr(omega), None, None, 0, 0) == zk._capi.EBADARG   # log_n > 28
    assert lib.mi355_fr_permutation_sigma_dev(arr, n_cols, log_n, ptr(delta), ptr(omega), None, None, 0, 2) == zk._capi.EBADARG   # an unknown flag bit
    zk._capi.check(lib.mi355_synchronize())
    assert all(bool((c == marker).all()) for c in cols)
    mapping = pc.cpp_mapping(n_cols, n, [(0, 5, 1, 9), (2, 12, 0, 5)])
    cells, images = pc.cpp_overrides(n_cols, n, mapping)
    zk.halo2.permutation_sigma(n_cols, log_n, delta, omega, cells, images, out=cols)
    want = torch.from_numpy(expected(n_cols, log_n, mapping).view(np.int64)).to(dev)
    assert all(torch.equal(cols[j], want[j]) for j in range(n_cols))


def test_workspace_is_one_pooled_block_that_trim_returns(dev):
    import torch
    log_n, n_cols = 16, 5
    delta, omega = consts(log_n)
    lib = zk._capi.lib()
    zk._capi.check(lib.mi355_buf_trim())
    before = zk.halo2.mem_info(0)
    cols = zk.halo2.permutation_sigma(n_cols, log_n, delta, omega, [3, 70000], [70000, 3], device=dev)
    after = zk.halo2.mem_info(0)
    assert after["live_buffers"] == before["live_buffers"], "the call left a live library block behind"
    assert after["workspace"] == before["workspace"], "the call grew a workspace role"
    assert after["pooled"] > before["pooled"], "the staging block is not visible as pooled memory"
    zk._capi.check(lib.mi355_buf_trim())
    assert zk.halo2.mem_info(0)["pooled"] == before["pooled"]
    del cols


# ---------------------------------------------------------------------------------------------------------------- keygen
def verify(rec, proof):
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
    tau = TAU0 + (rec["layer"] if rec["layer"] >= 0 else 0)
    return plonk.verify(pr, rec["vk_device"], inst, proof, tau, transcript=rec["transcript"])["ok"]


def check_routes(rec):
    assert rec.get("ok") and rec["returncode"] == 0, rec.get("error")
    assert rec["vk_equal"] and rec["vk_device"] == rec["vk_host"] and len(rec["vk_device"]) > 8
    assert rec["proof_equal"] and rec["proof_device"] == rec["proof_host"] and len(rec["proof_device"]) > 0
    assert rec["copy_pairs"] > 0 and rec["sigma_ms"]["device"] > 0 and rec["sigma_ms"]["host"] > 0
    assert verify(rec, rec["proof_device"])


STANDIN = dict(advice=40, fixed=8, lookups=3, perm_columns=12, degree=5)
ROUTES = [(2, 7, {}), (4, 8, {}), (3, 9, {}), (0, 8, STANDIN), (0, 13, STANDIN)]   # the small configurations of the byte-equality tests of the prover, k = 7 .. 13


@pytest.mark.parametrize("layer,k,shape", ROUTES)
def test_keygen_device_route_gives_the_default_route_s_key_and_proof(tmp_path, layer, k, shape):
    check_routes(zk.replay.run_permutation_keygen(layer, k, out_dir=str(tmp_path), timeout=600, **shape))


def test_keygen_device_route_layer5_at_its_own_k(tmp_path):
    rec = zk.replay.run_permutation_keygen(5, out_dir=str(tmp_path), timeout=1500)
    assert rec.get("k") == 21, rec.get("error")
    check_routes(rec)
