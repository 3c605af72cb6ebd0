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


def counts_to_words(counts) -> np.ndarray:
    """u64 counts -> [n, 4] Montgomery words (what the device's m holds)"""
    counts = np.asarray(counts)
    u, inv = np.unique(counts, return_inverse=True)
    tab = np.stack([fr_mont(int(v)) for v in u]) if len(u) else np.zeros((0, 4), dtype=np.uint64)
    return tab[inv.reshape(-1)]
