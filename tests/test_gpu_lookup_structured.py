"""-m gpu: mi355_fr_lookup_multiplicities_dev (through halo2.lookup_multiplicities) on columns BUILT to take the branches of k_lk_insert / k_lk_probe (csrc/lookup.hpp)
that random words never take.  Every word of m is compared with the numpy restatement (tests/lookup_common.py reference_ids), under both duplicate rules unless a
case says otherwise, two calls must agree, and a miss must be MI355_EBADARG with exactly the reference's (column, row).  All shapes have n <= 2^13.

Each case first asserts its own PREMISE on the CPU -- with the restatements of the hash and of the wave counter that tests/test_lookup_hash_on_host.py holds equal to
the header -- so that a retune of the hash, of the slot count or of the thresholds fails here loudly instead of silently losing the coverage:

  a  near-equal words: W, W ^ (1 << b) for every b in 0 .. 253, zero and the words 1 << 32 k; for each of the eight limbs a pair that differs in that limb only
  b  table_rows = 32 (64 slots): 24 keys with home slot 50, one cluster 50 .. 63, 0 .. 9 in any order of arrival; the 25th such value walks all of it and misses
  c  table_rows = 2048 (4096 slots): 40 keys with home slot 4093, each at two scattered rows, so the atomicMin / atomicMax fold happens at a displaced slot past the wrap
  d  one wave whose hot row is displaced three times while it holds a count; a group of 20 and one of 16 that stay cold; a group of LK_HOT_MIN - 1
  e  blocks with more than 1 + LK_ROUNDS groups (the one-by-one adds), of 64 distinct rows, of 63 equal + 1 and of 64 equal rows
  f  input_rows = 4096 + 37: a last wave of one ragged block whose idle lanes' cells hold that wave's hot value; misses on either side of a wave boundary and
     in a later column at an earlier row
  g  runs across table_rows, a value only beyond table_rows, A A B B A A, table_rows of 1 and 0, and 512 inserts contending for each of two slots
  h  permuting an input column's rows within input_rows leaves m unchanged (the columns of d and e)

The measured premise numbers and times are in profiles/lookup_structured.md."""
import numpy as np
import pytest

import __graft_entry__ as ge
from tests import lookup_common as lc

zk = ge.load_package()
pytestmark = pytest.mark.gpu
RULES = (False, True)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    ge.build()
    zk.init(0)
    yield torch.device("cuda:0")
    zk.shutdown()


def random_words(rng, count):
    """distinct uniform words below 2^252 (distinct with overwhelming probability; asserted where it matters)"""
    w = rng.integers(0, 2**64, size=(count, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)
    return w


class Case:
    """pool: [P, 4] uint64 distinct words; table_ids / input_ids: indices into it per row (n rows each)"""

    def __init__(self, pool, table_ids, table_rows, input_ids, input_rows):
        self.pool = np.ascontiguousarray(pool, dtype=np.uint64)
        assert len(np.unique(self.pool, axis=0)) == len(self.pool), "the pool's words are not distinct"
        self.table_ids, self.table_rows = np.asarray(table_ids, dtype=np.int64), int(table_rows)
        self.input_ids, self.input_rows = [np.asarray(x, dtype=np.int64) for x in input_ids], int(input_rows)
        self.n = len(self.table_ids)
        assert self.n <= 1 << 13 and all(len(x) == self.n for x in self.input_ids)

    def table_words(self):
        return self.pool[self.table_ids]

    def found_rows(self, column, last=False):
        """the table row each input row of one column finds (-1: none), for wave_trace"""
        t = self.table_ids[: self.table_rows]
        where = {}
        for r, v in enumerate(t.tolist()):
            where[v] = r if last or v not in where else where[v]
        return np.array([where.get(v, -1) for v in self.input_ids[column].tolist()])

    def trace(self, column=0, last=False):
        return lc.wave_trace(self.found_rows(column, last), self.input_rows, lc.wave_rows_for(self.input_rows))

    def with_inputs(self, input_ids):
        return Case(self.pool, self.table_ids, self.table_rows, input_ids, self.input_rows)


def upload(case, dev):
    import torch
    to = lambda ids: torch.from_numpy(case.pool[ids].view(np.int64)).to(dev)
    return to(case.table_ids), [to(x) for x in case.input_ids]


def check(case, dev, rules=RULES):
    """every word of m against the reference under each rule, twice; returns the reference's counts per rule"""
    import torch
    table, inputs = upload(case, dev)
    out = {}
    for last in rules:
        counts, miss = lc.reference_ids(case.table_ids, case.table_rows, case.input_ids, case.input_rows, case.n, last)
        assert miss is None and counts.sum() == case.input_rows * len(case.input_ids)
        m = zk.halo2.lookup_multiplicities(table, inputs, case.table_rows, case.input_rows, last=last)
        want = torch.from_numpy(lc.counts_to_words(counts).view(np.int64)).to(dev)
        bad = (m != want).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, f"last={last}: {bad.numel()} rows of m differ, the first at row {int(bad[0])}"
        m2 = zk.halo2.lookup_multiplicities(table, inputs, case.table_rows, case.input_rows, last=last)
        assert torch.equal(m, m2), "two calls differ"
        out[last] = counts
    return out


def check_miss(case, dev, where, rules=RULES):
    table, inputs = upload(case, dev)
    for last in rules:
        assert lc.reference_ids(case.table_ids, case.table_rows, case.input_ids, case.input_rows, case.n, last) == (None, where)
        for _ in range(2):
            with pytest.raises(zk.Mi355Error) as e:
                zk.halo2.lookup_multiplicities(table, inputs, case.table_rows, case.input_rows, last=last)
            assert e.value.code == zk._capi.EBADARG and (e.value.column, e.value.row) == where, str(e.value)


def spread(ids_with_counts, columns, rng):
    """every id as often as asked, shuffled over `columns` columns of equal length"""
    flat = np.repeat([i for i, _ in ids_with_counts], [c for _, c in ids_with_counts])
    assert len(flat) % columns == 0
    return np.split(rng.permutation(flat), columns)


def pad(x, n, fill):
    return np.concatenate([x, np.full(n - len(x), fill, dtype=np.int64)])


# ------------------------------------------------------------------------------------------------------------------------------------------- a
W_NEAR = 0x0A5C3F19E2D4B687_13579BDF02468ACE_F0E1D2C3B4A59687_89ABCDEF01234567        # < 2^252, no limb zero
assert W_NEAR < 1 << 252 and all((W_NEAR >> (32 * k)) & 0xFFFFFFFF for k in range(8))


def case_near_equal():
    """n = 512.  The table is W, its 254 one-bit neighbours, zero and the eight words 1 << 32 k: 1 + 254 + 1 + 8 = 264 distinct values, so table_rows = 264
    (one more than the 263 a count without W itself gives).  Pool id 264 is W ^ (1 << 253) ^ 1: two bits from W, one bit from two table values, in no table."""
    rng = np.random.default_rng(0xA)
    vals = [W_NEAR] + [W_NEAR ^ (1 << b) for b in range(254)] + [0] + [1 << (32 * k) for k in range(8)]
    assert len(vals) == 264 and max(vals) < (1 << 253) + (1 << 252) < lc.R_MOD
    pool = lc.int_words(vals + [W_NEAR ^ (1 << 253) ^ 1])
    n, tr = 512, 264
    order = rng.permutation(tr)                                        # value j sits at table row order[j]
    t = np.full(n, 264); t[order] = np.arange(tr)
    cols = spread([(j, j % 5 + 1) for j in range(tr)], 2, rng)
    ir = len(cols[0])
    assert ir == 395
    return Case(pool, t, tr, [pad(x, n, 264) for x in cols], ir), order


def test_near_equal_words(dev):
    case, order = case_near_equal()
    assert all(lc.one_limb_pairs(case.table_words()[: case.table_rows])), "premise: a pair differing in one limb only, for each limb"
    counts = check(case, dev)
    for last in RULES:
        assert (counts[last][order] == np.arange(264) % 5 + 1).all()      # value j exactly (j % 5) + 1 times, at its own row
    x = [c.copy() for c in case.input_ids]
    x[1][17] = 264
    check_miss(case.with_inputs(x), dev, (1, 17))
    x[0][394] = 264                                                     # the last row read of the earlier column wins
    check_miss(case.with_inputs(x), dev, (0, 394))


# ------------------------------------------------------------------------------------------------------------------------------------------- b
def case_small_chain():
    rng = np.random.default_rng(0xB)
    S, home, tr, n = 64, 50, 32, 64
    coll = lc.colliding_values(S, home, 25)
    cand = np.arange(1, 4000)
    h = lc.lk_hash(lc.mont_words(cand.tolist()), S - 1)
    quiet = [int(v) for v in cand[(h >= 12) & (h <= 38)] if int(v) not in coll][:8]      # homes well inside the slots the cluster leaves free
    pool = lc.mont_words(coll[:24] + quiet + coll[24:])                # ids 0 .. 23 collide, 24 .. 31 do not, 32 is the 25th colliding value
    t = pad(rng.permutation(32), n, 32)                                # beyond table_rows the 25th value: there, and only there
    cols = spread([(j, j % 7 + 1) for j in range(32)], 2, rng)
    ir = len(cols[0])
    assert ir == 61
    return Case(pool, t, tr, [pad(x, n, 32) for x in cols], ir)


def test_collision_chain_in_a_small_table(dev):
    case = case_small_chain()
    assert lc.slots_for(case.table_rows) == 64
    occ, homes, longest = lc.occupied_slots(case.table_words(), case.table_rows)
    cluster = [(50 + i) & 63 for i in range(24)]
    assert (homes == 50).sum() == 24 and occ[cluster].all() and not occ[10] and not occ[49] and longest == 24, "premise: one cluster 50 .. 63, 0 .. 9"
    assert lc.lk_hash(case.pool[32:33], 63)[0] == 50
    counts = check(case, dev)
    assert sorted(counts[False][:32].tolist()) == sorted(j % 7 + 1 for j in range(32))
    x = [c.copy() for c in case.input_ids]
    x[0][40] = 32                                                       # home 50, 24 occupied slots of other values, then the empty slot 10
    check_miss(case.with_inputs(x), dev, (0, 40))
    x[0][40] = case.input_ids[0][40]; x[1][60] = 32
    check_miss(case.with_inputs(x), dev, (1, 60))


# ------------------------------------------------------------------------------------------------------------------------------------------- c
def case_mid_chain():
    rng = np.random.default_rng(0xC)
    S, home, tr, n, k = 4096, 4093, 2048, 4096, 40
    coll = lc.mont_words(lc.colliding_values(S, home, k))
    pool = np.concatenate([coll, random_words(rng, tr - 2 * k + 1)])   # ids 0 .. 39 collide; the last id is in no table
    absent = len(pool) - 1
    t = np.full(n, absent)
    spots = rng.permutation(np.arange(0, tr, 2))[: 2 * k]              # even rows: no two of them adjacent
    t[: tr] = -1
    t[spots[:k]] = np.arange(k); t[spots[k:]] = np.arange(k)
    t[: tr][t[: tr] < 0] = rng.permutation(np.arange(k, absent))
    ir = 4000
    xs = []
    for c in range(2):
        x = t[rng.integers(0, tr, size=n)]
        x[rng.permutation(ir)[:800]] = rng.integers(0, k, size=800)    # the colliding values well represented
        x[ir:] = absent
        xs.append(x)
    return Case(pool, t, tr, xs, ir), spots[:k], spots[k:]


def test_collision_chain_across_the_wrap_in_a_mid_table(dev):
    case, s0, s1 = case_mid_chain()
    S = lc.slots_for(case.table_rows)
    occ, homes, longest = lc.occupied_slots(case.table_words(), case.table_rows)
    k = int((homes == 4093).sum())
    assert S == 4096 and k >= 40 and 4093 + k > S and occ[[(4093 + i) & (S - 1) for i in range(k)]].all() and longest >= 40, "premise: 40 keys of home 4093, past the wrap"
    assert (np.abs(s0 - s1) > 1).all()                                  # the two rows of a colliding value are not one run: both insert, the later one folds
    counts = check(case, dev)
    for j in range(40):                                                 # the count sits on the smallest / the largest row of the value
        lo, hi = min(s0[j], s1[j]), max(s0[j], s1[j])
        assert counts[False][lo] > 0 and counts[False][hi] == 0 and counts[True][hi] == counts[False][lo] and counts[True][lo] == 0
    x = [c.copy() for c in case.input_ids]
    x[1][3999] = case.table_ids[4095]
    check_miss(case.with_inputs(x), dev, (1, 3999))


# ------------------------------------------------------------------------------------------------------------------------------------------- d, e
def table_with_repeats(rng, n):
    """n rows over n - 100 values: ids 0 .. 99 (A, B, C, D among them) stand at a second, later row too, so the two rules count on different rows"""
    return np.concatenate([rng.permutation(n - 100), rng.permutation(100)]), n - 100      # the later rows of 0 .. 99 close the table


def case_hot_switching():
    """one column, one wave of 32 blocks.  A x 16 becomes hot on an empty hand; B x 17, C x 18 and A x 64 each displace a hot row that holds a count (after A x 64
    the wave holds 64 and nothing can displace it again, so the third switch needs the C x 18 block before it); then B x 20 and C x 16 go through a round and
    stay cold, and C x 15 is a group of LK_HOT_MIN - 1."""
    rng = np.random.default_rng(0xD)
    n = 2048
    t, values = table_with_repeats(rng, n)
    pool = random_words(rng, values)
    A, B, C, D = 0, 1, 2, 3
    fresh = iter(rng.permutation(np.arange(4, values)).tolist())
    distinct = lambda c: [next(fresh) for _ in range(c)]
    blocks = [[A] * 16 + distinct(48), [B] * 17 + distinct(47), [C] * 18 + distinct(46), [A] * 64, [B] * 20 + [C] * 15 + distinct(29), [C] * 16 + [D] * 16 + distinct(32)]
    while len(blocks) < 32:                                             # filler: the hot value scattered among few others
        blocks.append(rng.choice([A, B, 7, 8, 9, 10, 11], size=64, p=[.4, .1, .1, .1, .1, .1, .1]).tolist())
    assert all(len(b) == 64 for b in blocks)
    return Case(pool, t, n, [np.array(sum(blocks, []))], n)


def case_exhausted_rounds():
    rng = np.random.default_rng(0xE)
    n = 2048
    t, values = table_with_repeats(rng, n)
    pool = random_words(rng, values)
    blocks = []
    for i in range(8):
        g = rng.permutation(values)[:64]
        blocks.append(rng.permutation(np.concatenate([np.repeat(g[:7], 8), g[7:15]])))    # 7 groups of 8 + 8 single rows: 15 groups
        blocks.append(g)                                                                   # 64 distinct rows
        blocks.append(rng.permutation(np.concatenate([np.full(63, g[20]), g[21:22]])))    # 63 equal + 1
        blocks.append(np.full(64, g[i]))                                                   # 64 equal
    return Case(pool, t, n, [np.concatenate(blocks)], n)


def test_hot_row_switching(dev):
    case = case_hot_switching()
    assert lc.wave_rows_for(case.input_rows) == 2048 == case.input_rows
    for last in RULES:
        counts, switches, tails, cold = case.trace(0, last)
        assert switches >= 3 and cold >= lc.LK_HOT_MIN, "premise: three displaced hot rows that held a count, and a cold group of at least LK_HOT_MIN"
    x = case.input_ids[0].reshape(-1, 64)
    sizes = [np.unique(b, return_counts=True)[1] for b in x]
    assert any((s == lc.LK_HOT_MIN - 1).any() for s in sizes) and any((s == lc.LK_HOT_MIN).any() for s in sizes), "premise: groups of LK_HOT_MIN - 1 and of LK_HOT_MIN"
    counts = check(case, dev)
    assert not (counts[False] == counts[True]).all()                    # the rules count on different rows here


def test_exhausted_rounds(dev):
    case = case_exhausted_rounds()
    counts, switches, tails, cold = case.trace()
    assert tails >= 16 and switches >= 1, "premise: blocks that leave lanes to the one-by-one adds after LK_ROUNDS rounds"
    check(case, dev)


@pytest.mark.parametrize("which", ["hot_switching", "exhausted_rounds"])
def test_permuting_the_input_rows_leaves_m_unchanged(dev, which):
    case = case_hot_switching() if which == "hot_switching" else case_exhausted_rounds()
    rng = np.random.default_rng(0x11)
    base = check(case, dev)
    short = Case(case.pool, case.table_ids, case.table_rows, case.input_ids, case.input_rows - 100)      # within input_rows: the rows beyond stay where they are
    base_short = check(short, dev)
    for _ in range(2):
        x = case.input_ids[0]
        got = check(case.with_inputs([x[rng.permutation(case.n)]]), dev)
        y = x.copy(); y[: short.input_rows] = x[rng.permutation(short.input_rows)]
        got_short = check(short.with_inputs([y]), dev)
        for last in RULES:
            assert (got[last] == base[last]).all() and (got_short[last] == base_short[last]).all()
    assert case.trace()[1:] != case.with_inputs([np.sort(case.input_ids[0])]).trace()[1:]               # the waves did take other branches


# ------------------------------------------------------------------------------------------------------------------------------------------- f
def case_ragged():
    """three waves (2048, 2048, 37 rows), two columns; H is the hot value of the last wave and fills every cell from input_rows on"""
    rng = np.random.default_rng(0xF)
    n, tr, ir = 8192, 5000, 4096 + 37
    values = 3000
    pool = random_words(rng, values + 1)                                # the last id is in no table
    t = pad(np.concatenate([rng.permutation(values), rng.integers(0, values, size=tr - values)]), n, values)
    H = 5
    xs = []
    for c in range(2):
        x = rng.integers(0, values, size=n)
        x[rng.random(n) < 0.3] = 11 + c                                 # a hot value in the full waves
        x[4096: ir] = rng.permutation(np.concatenate([np.full(20, H), rng.integers(0, values, size=17)]))
        x[ir:] = H
        xs.append(x)
    return Case(pool, t, tr, xs, ir), H, values


def test_ragged_last_wave_with_table_values_beyond_input_rows(dev):
    case, H, absent = case_ragged()
    assert lc.wave_rows_for(case.input_rows) == 2048 and case.input_rows % 2048 == 37
    for c in range(2):
        tail = case.found_rows(c)[4096:]
        hot_row = tail[case.input_rows - 4096]
        assert (tail[case.input_rows - 4096:] == hot_row).all() and (tail[: case.input_rows - 4096] == hot_row).sum() >= lc.LK_HOT_MIN, "premise: H is hot in the last wave"
        assert lc.wave_trace(tail, 37, 2048)[0][hot_row] + 27 == lc.wave_trace(tail, 64, 2048)[0][hot_row]      # counting the idle lanes would show: 27 more
    counts = check(case, dev)
    for last in RULES:
        row = case.found_rows(0, last)[case.input_rows]                 # H's row: it counts the cells below input_rows only
        assert counts[last][row] == sum(int((x[: case.input_rows] == H).sum()) for x in case.input_ids) < 100
    for cells, where in (([(0, 2047), (0, 2048)], (0, 2047)), ([(0, 2048)], (0, 2048)), ([(1, 0), (0, 4132)], (0, 4132)), ([(1, 2048), (1, 4132), (1, 2047)], (1, 2047)),
                         ([(0, 4133), (1, 4132)], (1, 4132))):
        x = [c.copy() for c in case.input_ids]
        for c, r in cells:
            x[c][r] = absent
        check_miss(case.with_inputs(x), dev, where)


# ------------------------------------------------------------------------------------------------------------------------------------------- g
def test_runs_across_table_rows(dev):
    rng = np.random.default_rng(0x6)
    n, tr = 128, 61
    pool = random_words(rng, n + 2)
    V, ONLY_BEYOND = n, n + 1
    t = np.arange(n)
    t[tr - 3: tr + 6] = V                                               # rows tr - 3 .. tr + 5
    t[tr + 10] = ONLY_BEYOND
    x = [pad(np.array([V] * 9 + [3, 4, V]), n, V), pad(np.array([0, V, tr - 4] + [7] * 9), n, V)]
    case = Case(pool, t, tr, x, 12)
    counts = check(case, dev)
    assert counts[False][tr - 3] == 11 and counts[True][tr - 1] == 11 and counts[False][tr - 1] == 0 and counts[True][tr - 3] == 0
    t2 = t.copy(); t2[5] = V                                            # an earlier first row
    counts = check(Case(pool, t2, tr, x, 12), dev)
    assert counts[False][5] == 11 and counts[True][tr - 1] == 11 and counts[False][tr - 3] == 0
    y = [c.copy() for c in x]
    y[1][11] = ONLY_BEYOND                                              # in the table tensor, but only beyond table_rows: a miss
    check_miss(case.with_inputs(y), dev, (1, 11))
    y[0][3] = tr + 20                                                   # the word that stands at table row tr + 20 and nowhere else
    check_miss(case.with_inputs(y), dev, (0, 3))


def test_a_a_b_b_a_a(dev):
    rng = np.random.default_rng(0x7)
    pool = random_words(rng, 3)
    t = np.array([0, 0, 1, 1, 0, 0, 2, 2])
    case = Case(pool, t, 6, [np.array([0, 1, 0, 0, 1, 2, 2, 2]), np.array([1, 1, 1, 1, 0, 2, 2, 2])], 5)
    counts = check(case, dev)
    assert counts[False].tolist() == [4, 0, 6, 0, 0, 0, 0, 0] and counts[True].tolist() == [0, 0, 0, 6, 0, 4, 0, 0]
    check_miss(Case(pool, t, 6, case.input_ids, 6), dev, (0, 5))        # value 2 stands at rows 6, 7 only


def test_table_rows_of_one_and_of_zero(dev):
    import torch
    rng = np.random.default_rng(0x8)
    n = 64
    pool = random_words(rng, 2)
    t = pad(np.array([0]), n, 1)
    ins = [np.zeros(n, dtype=np.int64), pad(np.zeros(50, dtype=np.int64), n, 1)]
    counts = check(Case(pool, t, 1, ins, 50), dev)
    assert counts[False].tolist() == [100] + [0] * 63 and counts[True].tolist() == [100] + [0] * 63
    check_miss(Case(pool, t, 1, ins, 51), dev, (1, 50))
    counts = check(Case(pool, t, 0, ins, 0), dev)                       # no table, nothing read: m is all zero words
    assert not counts[False].any()
    table, inputs = upload(Case(pool, t, 0, ins, 0), dev)
    assert not zk.halo2.lookup_multiplicities(table, inputs, 0, 0).any()
    check_miss(Case(pool, t, 0, ins, 1), dev, (0, 0))                   # no table, one row read: every slot is empty


def test_alternating_table_contends_on_two_slots(dev):
    rng = np.random.default_rng(0x9)
    n = 1024
    pool = random_words(rng, 3)
    t = np.arange(n) % 2                                                # no two adjacent rows equal: all 1024 rows insert, 512 per slot
    assert (t[1:] != t[:-1]).all()
    ins = [rng.integers(0, 2, size=n), np.zeros(n, dtype=np.int64), (np.arange(n) // 3) % 2]
    case = Case(pool, t, n, ins, n - 5)
    counts = check(case, dev)
    assert np.nonzero(counts[False])[0].tolist() == [0, 1] and np.nonzero(counts[True])[0].tolist() == [n - 2, n - 1]
    x = [c.copy() for c in ins]
    x[2][n - 6] = 2
    check_miss(case.with_inputs(x), dev, (2, n - 6))
