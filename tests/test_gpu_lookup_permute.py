"""-m gpu: mi355_fr_lookup_permute_dev (the permuted columns A' and S' of the classic halo2 lookup argument, csrc/lookup_permute.hpp) against the integer
restatement of permute_expression_pair in tests/lookup_permute_common.py, every output word compared.

Every case runs on INTERIOR, RAGGED views of one library block (tests/guard_common.py): the four operands start at odd word offsets with at least 64 KiB of poison
around each, and after the call every byte outside rows < `rows` of the two outputs must be what it was -- the guards, the inputs, the rows behind `rows`.  Sizes:
one row, two, either side of a wave (63, 64, 65), past a workgroup (257), past a radix chunk and a scan tile (4 099), past 32 of them (65 539: the scans recurse).
Cases: tests/lookup_permute_common.py CASES; a value the table lacks at the first, a middle and the last row; calls in a row with different `rows` through the same
pooled workspace; the same call twice for equal bytes; the argument checks; the workspace in the memory ledger."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from tests import guard_common as gc
from tests import lookup_permute_common as pc

pytestmark = pytest.mark.gpu

FR = 32
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


@functools.lru_cache(maxsize=None)
def case(name, rows):
    """(input words, table words, A' words, S' words) of one case, computed once"""
    inputs, table = pc.CASES[name](rows, np.random.default_rng(1000 + rows))
    a, s, miss = pc.permute(inputs, table)
    assert miss is None
    pc.check_constraints(a, s, inputs, table)
    return tuple(pc.to_words(x) for x in (inputs, table, a, s))


class Operands:
    """input, perm_table, table, perm_input as views of `cap` words in one arena (the outputs between the inputs)"""

    def __init__(self, zk, cap, poison="A"):
        self.zk, self.lib, self.capi = zk, zk._capi.lib(), zk._capi
        self.ar = gc.Arena("device", gc.Arena.bytes_for([(cap, FR)] * 4), poison, h2=zk.halo2, sync=lambda: zk._capi.check(self.lib.mi355_synchronize()))
        self.I, self.PS, self.T, self.PA = (self.ar.view(cap, FR, None, n) for n in ("input", "perm_table", "table", "perm_input"))

    def call(self, rows, miss):
        return self.lib.mi355_fr_lookup_permute_dev(self.capi.ptr(self.PA), self.capi.ptr(self.PS), self.capi.ptr(self.I), self.capi.ptr(self.T), rows, C.byref(miss))

    def run(self, iw, tw, aw, sw):
        """upload the columns, run under the arena's check, hold rows < len(iw) of both outputs to (aw, sw)"""
        rows = len(iw)
        self.I.upload(iw); self.T.upload(tw)
        miss = C.c_uint64(0)
        rc, after = self.ar.run(lambda: self.call(rows, miss), [(self.PA, 0, rows), (self.PS, 0, rows)], [(self.PA, 0, aw), (self.PS, 0, sw)])
        assert rc == 0, self.lib.mi355_last_error()
        assert miss.value == NONE
        return after

    def free(self):
        self.ar.free()


@pytest.mark.parametrize("rows", pc.SIZES)
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_every_word_equals_the_restatement(zk, name, rows):
    ops = Operands(zk, rows + 3)                                     # three more rows than the call may touch: ragged views
    try:
        ops.run(*case(name, rows))
    finally:
        ops.free()


@pytest.mark.parametrize("rows", [65, 4099])
@pytest.mark.parametrize("name", ["range_zero_tail", "duplicated_table"])
def test_rows_behind_the_columns_are_not_read(zk, name, rows):
    """poison B is the word of r - 1, a valid element: were a row >= `rows` of the table or the input read, a count and with it an output word would move"""
    ops = Operands(zk, rows + 70, poison="B")
    try:
        ops.run(*case(name, rows))
    finally:
        ops.free()


@pytest.mark.parametrize("rows", [1, 65, 4099])
def test_a_missing_value_names_the_smallest_row_and_the_next_call_is_right(zk, rows):
    iw, tw, aw, sw = case("duplicated_table", rows)
    inputs, table = pc.from_words(iw), pc.from_words(tw)
    ops = Operands(zk, rows + 3)
    try:
        ops.T.upload(tw)
        for row in sorted({0, rows - 1, rows // 2}, key=lambda r: (r == rows // 2, r)):      # the middle row last
            bad = pc.with_missing(inputs, table, row)
            if rows > 2 and row == rows // 2:
                bad = pc.with_missing(bad, table, rows - 1)          # two misses: the smaller row is named
            assert pc.permute(bad, table)[2] == row
            ops.I.upload(pc.to_words(bad))
            miss = C.c_uint64(0)
            rc, _ = ops.ar.run(lambda: ops.call(rows, miss), [(ops.PA, 0, rows), (ops.PS, 0, rows)])
            assert rc == zk._capi.EBADARG and miss.value == row
            assert ("input row %d is not in the table" % row).encode() in ops.lib.mi355_last_error()
        ops.run(iw, tw, aw, sw)                                      # after the refused call: the valid one
    finally:
        ops.free()


def test_calls_in_a_row_with_different_rows_share_the_workspace(zk):
    ops = Operands(zk, 65539 + 3)
    try:
        for name, rows in (("shuffle", 65539), ("straddling_run", 257), ("all_equal", 4099), ("montgomery_order", 65539), ("one_digit", 63)):
            ops.run(*case(name, rows))
    finally:
        ops.free()


def test_the_same_call_twice_gives_the_same_bytes(zk):
    rows = 65539
    ops = Operands(zk, rows + 3)
    try:
        first = ops.run(*case("duplicated_table", rows))
        second = ops.run(*case("duplicated_table", rows))
        assert (first == second).all()
    finally:
        ops.free()


def test_the_pass_count_follows_the_keys(zk):
    """a range table of 16 bits sorts in two passes, keys that differ in one digit in one, random keys in all 32 (the profile counts one span per pass)"""
    lib, check = zk._capi.lib(), zk._capi.check
    for name, rows, want in (("range_zero_tail", 65539, 2), ("one_digit", 4099, 1), ("shuffle", 4099, 32), ("all_equal", 1, 0)):
        ops = Operands(zk, rows + 3)
        try:
            check(lib.mi355_profile_reset()); check(lib.mi355_profile_enable(1))
            ops.run(*case(name, rows))
            ms, cnt = C.c_double(), C.c_uint64()
            rc = lib.mi355_profile_get(b"lookup_permute_pass", C.byref(ms), C.byref(cnt))
            check(lib.mi355_profile_enable(0))
            assert (cnt.value if rc == 0 else 0) == want, (name, rows)
        finally:
            lib.mi355_profile_enable(0)
            ops.free()


def test_argument_checks_and_rows_zero(zk):
    capi, lib = zk._capi, zk._capi.lib()
    ops = Operands(zk, 300)
    lone = zk.halo2.DeviceBuffer(FR * 100)                             # a block of its own, shorter than the call's rows
    try:
        iw, tw, aw, sw = case("range_zero_tail", 257)
        ops.I.upload(iw); ops.T.upload(tw)
        miss = C.c_uint64(0)
        vp = C.c_void_p
        I, T, PA, PS = (v.data_ptr() for v in (ops.I, ops.T, ops.PA, ops.PS))
        call = lambda pa, ps, i, t, rows: lib.mi355_fr_lookup_permute_dev(vp(pa), vp(ps), vp(i), vp(t), rows, C.byref(miss))
        for args, text in (((PA, PS, I, T, 1 << 31), b"rows must be < 2^31"),
                           ((None, PS, I, T, 257), b"null pointer"), ((PA, PS, I, None, 257), b"null pointer"),
                           ((PA + 8, PS, I, T, 257), b"16-byte aligned"),
                           ((PA, PA + FR * 100, I, T, 257), b"the two outputs must not overlap"),
                           ((I + FR * 256, PS, I, T, 257), b"an output must not overlap an input"), ((PA, T, I, T, 257), b"an output must not overlap an input"),
                           ((lone.data_ptr(), PS, I, T, 257), b"range exceeds the block"), ((PA, PS, lone.data_ptr(), T, 257), b"range exceeds the block")):
            rc, _ = ops.ar.run(lambda: call(*args), [])                # refused before any launch: not a byte moves
            assert rc == capi.EBADARG and text in lib.mi355_last_error(), (text, rc, lib.mi355_last_error())
        rc, _ = ops.ar.run(lambda: call(PA, PS, I, T, 0), [])          # rows == 0: MI355_OK, nothing written
        assert rc == 0 and call(None, None, None, None, 0) == 0 and miss.value == NONE
        ops.run(iw, tw, aw, sw)
    finally:
        lone.free()
        ops.free()


def test_the_workspace_goes_back_to_the_pool_and_to_hip(zk):
    h2, lib, check = zk.halo2, zk._capi.lib(), zk._capi.check
    rows = 65539
    ops = Operands(zk, rows + 3)
    try:
        check(lib.mi355_buf_trim())
        before = h2.mem_info(0)
        ops.run(*case("shuffle", rows))
        now = h2.mem_info(0)
        assert (now["live_buffers"], now["workspace"]) == (before["live_buffers"], before["workspace"])      # the block went back ...
        assert h2.mem_usage()["classes"]["buffers"] >= now["live_buffers"] + now["pooled"]                   # ... and the ledger holds what the pool holds
        check(lib.mi355_buf_trim())
        assert h2.mem_info(0)["pooled"] == before["pooled"]
    finally:
        ops.free()


def test_a_workspace_past_the_limit_is_refused_on_the_host(zk):
    """2^25 rows need a workspace of about 2 GiB, more than a slab: under a limit of held + 1 GiB the call is MI355_EOOM before anything is launched (the operands are
    never initialised, and never read)"""
    h2, capi, lib, check = zk.halo2, zk._capi, zk._capi.lib(), zk._capi.check
    rows = 1 << 25
    bufs = [h2.DeviceBuffer(FR * rows) for _ in range(4)]
    try:
        check(lib.mi355_buf_trim())
        u0 = h2.mem_usage()
        h2.mem_set_limit(u0["held"] + (1 << 30))
        miss = C.c_uint64(0)
        rc = lib.mi355_fr_lookup_permute_dev(*[C.c_void_p(b.data_ptr()) for b in bufs], rows, C.byref(miss))
        u1 = h2.mem_usage()
        assert rc == capi.EOOM and u1["refused"] > u0["refused"] and u1["held"] <= u0["held"], (rc, lib.mi355_last_error())
    finally:
        h2.mem_set_limit(0)
        for b in bufs:
            b.free()
