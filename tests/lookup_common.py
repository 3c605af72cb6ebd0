"""the multiplicity column of the mv-lookup argument, restated in numpy for the tests of mi355_fr_lookup_multiplicities_dev (TEST INFRASTRUCTURE).
halo2's `prepare` [EXT-recalled halo2_proofs src/plonk/mv_lookup/prover.rs] maps every compressed table value to a row of the usable range and adds 1 to m[row] per
compressed input cell; a value missing from the table fails the proof.  Here the row a repeated value maps to is its first (or last) row of the table."""
import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
_M64 = (1 << 64) - 1
MISSING_NONE = (1 << 64) - 1


def fr_mont(v: int) -> np.ndarray:
    x = (v % R_MOD) * (1 << 256) % R_MOD
    return np.array([(x >> (64 * i)) & _M64 for i in range(4)], dtype=np.uint64)


def reference_ids(table_ids, table_rows, input_ids, input_rows, n, last=False):
    """table_ids / input_ids[c]: integer value ids per row (equal ids = equal words).  Returns (counts int64[n], missing) with missing = (column, row) of the smallest
    pair whose value the table lacks, or None."""
    t = np.asarray(table_ids[:table_rows])
    if last:
        uid, idx = np.unique(t[::-1], return_index=True)
        idx = table_rows - 1 - idx
    else:
        uid, idx = np.unique(t, return_index=True)
    counts = np.zeros(n, dtype=np.int64)
    for c, ids in enumerate(input_ids):
        x = np.asarray(ids[:input_rows])
        pos = np.searchsorted(uid, x)
        pos_c = np.minimum(pos, max(len(uid) - 1, 0))
        found = (pos < len(uid)) & (uid[pos_c] == x) if len(uid) else np.zeros(len(x), dtype=bool)
        if not found.all():
            return None, (c, int(np.argmin(found)))
        counts += np.bincount(idx[pos_c], minlength=n)[:n]
    return counts, None


def reference_words(table, table_rows, inputs, input_rows, last=False):
    """the same on 32-byte words: table [n, 4] uint64, inputs a list of [n, 4] arrays"""
    n = len(table)
    allw = np.concatenate([np.asarray(table)] + [np.asarray(x) for x in inputs]).reshape(-1, 4)
    _, inv = np.unique(allw, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return reference_ids(inv[:n], table_rows, [inv[n * (c + 1): n * (c + 2)] for c in range(len(inputs))], input_rows, n, last)


def mont_words(vals) -> np.ndarray:
    """[len(vals), 4] Montgomery words of many integers at once (fr_mont row by row, without an array per value)"""
    r1 = (1 << 256) % R_MOD
    raw = b"".join((v % R_MOD * r1 % R_MOD).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def int_words(vals) -> np.ndarray:
    """[len(vals), 4] words whose 256 bits ARE the integers (each below r: a reduced word the ABI accepts)"""
    assert all(0 <= v < R_MOD for v in vals)
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


# ---- the device's hash set and wave counter restated (csrc/lookup.hpp); tests/test_lookup_hash_on_host.py holds these equal to the header's own
LK_EMPTY = 0xFFFFFFFF
LK_ROUNDS = 4
LK_HOT_MIN = 16


def slots_for(table_rows: int) -> int:
    """S of mi355_fr_lookup_multiplicities_dev: the next power of two >= 2 x table_rows, at least 64"""
    s = 64
    while s < 2 * table_rows:
        s *= 2
    return s


def lk_hash(words, mask: int) -> np.ndarray:
    """lk_hash of csrc/lookup.hpp on [n, 4] uint64 words (word k = limbs 2k + 1 : 2k), wrapping 64-bit arithmetic"""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    u = np.uint64
    with np.errstate(over="ignore"):
        h = w[:, 0].copy()
        h = (h ^ (h >> u(31))) * u(0x9E3779B97F4A7C15) ^ w[:, 1]
        h = (h ^ (h >> u(29))) * u(0xBF58476D1CE4E5B9) ^ w[:, 2]
        h = (h ^ (h >> u(32))) * u(0x94D049BB133111EB) ^ w[:, 3]
        h = (h ^ (h >> u(30))) * u(0xBF58476D1CE4E5B9)
        h = (h ^ (h >> u(27))) * u(0x94D049BB133111EB)
        h ^= h >> u(31)
    return (h & u(0xFFFFFFFF) & u(mask)).astype(np.uint32)


def colliding_values(S: int, home: int, count: int, start: int = 1):
    """the first `count` integers i >= start whose Montgomery word hashes to `home` under mask S - 1 (the values of a range table)"""
    out, lo, step = [], start, max(4096, 8 * S)
    while len(out) < count:
        h = lk_hash(mont_words(range(lo, lo + step)), S - 1)
        out += [lo + int(i) for i in np.nonzero(h == home)[0]]
        lo += step
    return out[:count]


def occupied_slots(table, table_rows: int):
    """the slots the table's distinct values occupy after k_lk_insert (linear probing fills the same set of slots in any order of arrival).
    Returns (occupied bool[S], homes uint32 per distinct value, longest circular run of occupied slots)."""
    S = slots_for(table_rows)
    keys = np.unique(np.asarray(table)[:table_rows].reshape(-1, 4), axis=0)
    homes = lk_hash(keys, S - 1)
    occ = np.zeros(S, dtype=bool)
    for h in homes.tolist():
        while occ[h]:
            h = (h + 1) & (S - 1)
        occ[h] = True
    assert not occ.all()
    first_free = int(np.argmin(occ))
    longest = run = 0
    for i in range(1, S + 1):
        run = run + 1 if occ[(first_free + i) & (S - 1)] else 0
        longest = max(longest, run)
    return occ, homes, longest


def one_limb_pairs(words):
    """for each of the eight 32-bit limbs: is there a pair of distinct words that differ in that limb only"""
    l = np.unique(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4), axis=0).view(np.uint32).reshape(-1, 8)
    return [bool((np.unique(np.delete(l, k, axis=1), axis=0, return_counts=True)[1] > 1).any()) for k in range(8)]


def wave_trace(row_ids, input_rows: int, wave_rows: int):
    """the bookkeeping of k_lk_probe for one input column, lane by lane in plain Python.  row_ids[r] is the table row that input row r finds (negative: a miss,
    which takes no part).  Returns (counts, switches, tail_blocks, largest_cold): counts[row] as the atomics add them up (length max row + 1); the number of
    times a group displaced a hot row that held a non-zero count; the number of 64-row blocks that left lanes to the one-by-one adds after LK_ROUNDS rounds;
    the largest group that went through a round without becoming the hot row."""
    ids = [int(x) for x in row_ids[:input_rows]]
    counts = [0] * (max(ids, default=-1) + 1)
    switches = tail_blocks = largest_cold = 0
    for lo in range(0, input_rows, wave_rows):
        hi = min(lo + wave_rows, input_rows)
        hot, hot_cnt = None, 0
        for base in range(lo, hi, 64):
            lanes = [x for x in ids[base: min(base + 64, hi)] if x >= 0]        # the active lanes' rows, in lane order
            if hot is not None:
                hot_cnt += lanes.count(hot)
                lanes = [x for x in lanes if x != hot]
            for _ in range(LK_ROUNDS):
                if not lanes:
                    break
                lead = lanes[0]
                c = lanes.count(lead)
                if c >= LK_HOT_MIN and hot_cnt < c:
                    if hot_cnt:
                        counts[hot] += hot_cnt
                        switches += 1
                    hot, hot_cnt = lead, c
                else:
                    counts[lead] += c
                    largest_cold = max(largest_cold, c)
                lanes = [x for x in lanes if x != lead]
            if lanes:
                tail_blocks += 1
            for x in lanes:
                counts[x] += 1
        if hot_cnt:
            counts[hot] += hot_cnt
    return np.array(counts, dtype=np.int64), switches, tail_blocks, largest_cold


def wave_rows_for(input_rows: int) -> int:
    """wave_rows of mi355_fr_lookup_multiplicities_dev: 2048 until a column has more than 8192 waves of that"""
    return max(2048, (-(-input_rows // 8192) + 63) & ~63)


def counts_to_words(counts) -> np.ndarray:
    """u64 counts -> [n, 4] Montgomery words (what the device's m holds)"""
    counts = np.asarray(counts)
    u, inv = np.unique(counts, return_inverse=True)
    tab = np.stack([fr_mont(int(v)) for v in u]) if len(u) else np.zeros((0, 4), dtype=np.uint64)
    return tab[inv.reshape(-1)]
