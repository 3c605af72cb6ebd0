"""the permuted columns of the classic halo2 lookup argument, restated on Python integers for the tests of mi355_fr_lookup_permute_dev (TEST INFRASTRUCTURE;
nothing here looks at the C++).  halo2's `permute_expression_pair` [EXT-recalled halo2_proofs src/plonk/lookup/prover.rs]: A' is the input sorted ascending by
the canonical integer; the row that starts a run of equal values of A' takes that value in S' and uses up one copy of it in the table (a value the table lacks
fails the proof); the copies left over, walked in ascending order, are pop()ed into the other rows from the back."""
import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
_R1 = (1 << 256) % R_MOD
_RINV = pow(1 << 256, -1, R_MOD)


def permute(inputs, table):
    """inputs, table: equally long lists of integers in [0, r).  Returns (A', S', None), or (None, None, row) with the smallest row of `inputs` whose value the
    table lacks."""
    assert len(inputs) == len(table)
    leftover = {}
    for v in table:
        leftover[v] = leftover.get(v, 0) + 1
    for row, v in enumerate(inputs):
        if v not in leftover:
            return None, None, row
    a = sorted(inputs)
    s = [None] * len(a)
    repeated = []
    for i, v in enumerate(a):
        if i == 0 or a[i - 1] != v:
            s[i] = v
            leftover[v] -= 1
        else:
            repeated.append(i)
    for v in sorted(leftover):
        for _ in range(leftover[v]):
            s[repeated.pop()] = v
    assert not repeated
    return a, s, None


def to_words(vals) -> np.ndarray:
    """[len(vals), 4] uint64 Montgomery words (what the ABI holds) of integers"""
    raw = b"".join((v % R_MOD * _R1 % R_MOD).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def from_words(words) -> list:
    """the integers that [n, 4] uint64 Montgomery words stand for"""
    raw = np.ascontiguousarray(words, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i: i + 32], "little") * _RINV % R_MOD for i in range(0, len(raw), 32)]


def check_constraints(a, s, inputs, table):
    """what the argument's constraints 4 and 5 and its grand product ask of the two columns, on integers: A'[0] = S'[0]; every other row has A' = S' or
    A' = A' of the row above; the two columns are permutations of the input and the table"""
    assert sorted(a) == sorted(inputs) and sorted(s) == sorted(table)
    assert not a or a[0] == s[0]
    for i in range(1, len(a)):
        assert a[i] == s[i] or a[i] == a[i - 1], i


# ---- the cases of the device and host tests: name -> function(rows, rng) -> (inputs, table[, missing row])
def _range_bits(rows):
    return max(1, (rows // 2).bit_length())


def case_range_zero_tail(rows, rng):
    """a range table 0 .. 2^b - 1 with a zero tail, inputs drawn from it"""
    b = _range_bits(rows)
    t = [i if i < (1 << b) and i < rows else 0 for i in range(rows)]
    return [t[int(i)] for i in rng.integers(0, rows, size=rows)], t


def case_all_equal(rows, rng):
    """one run: every row but the first is a repeated row"""
    t = [(7 * i + 3) % R_MOD for i in range(rows)]
    return [t[rows // 2]] * rows, t


def case_shuffle(rows, rng):
    """the inputs are the table's distinct values in another order: no repeated row, no leftover"""
    t = [int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(rows)]
    while len(set(t)) != rows:
        t = [int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(rows)]
    return [t[int(i)] for i in rng.permutation(rows)], t


def case_duplicated_table(rows, rng):
    """every table value several times, not in adjacent rows: the leftovers carry duplicates"""
    d = max(1, rows // 5)
    vals = [int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(d)]
    t = [vals[i % d] for i in range(rows)]
    return [vals[int(i)] for i in rng.integers(0, max(1, d // 2), size=rows)], t


ORDER_VALUES = [0, 1, R_MOD - 1, R_MOD - 2, 1 << 64, 1 << 128, 1 << 192, (1 << 64) + 1, (1 << 192) + 1, (5 << 224) + 9, (5 << 224) + 10, (6 << 224) + 9,
                (1 << 253) + 77, (1 << 253) + 78, (1 << 32) - 1, 1 << 32, (1 << 224) - 1, 1 << 224]


def case_montgomery_order(rows, rng):
    """values whose Montgomery words order differently from the integers: the ends of the field, single set bits, pairs that differ in the lowest / highest limb only"""
    t = [ORDER_VALUES[i % len(ORDER_VALUES)] for i in range(rows)]
    return [t[int(i)] for i in rng.integers(0, rows, size=rows)], t


def case_straddling_run(rows, rng):
    """short runs, then one run that crosses row 64 and row 256 of A' (a wave and a workgroup boundary), then short runs"""
    t = list(range(1, rows + 1))
    long_run = min(rows, max(2, min(rows - rows // 4, 300)))
    head = min(50, (rows - long_run) // 2)
    x = [1 + i for i in range(head)] + [head + 1] * long_run
    x += [head + 2 + i // 2 for i in range(rows - len(x))]
    return [x[int(i)] for i in rng.permutation(rows)], t


def case_one_digit(rows, rng):
    """keys that share every radix digit but one (byte 13 of the canonical value): 31 passes are skipped"""
    base = int.from_bytes(rng.bytes(32), "little") % (1 << 250) & ~(0xFF << 104)
    t = [base | (i % 256) << 104 for i in range(rows)]
    return [t[int(i)] for i in rng.integers(0, rows, size=rows)], t


CASES = {"range_zero_tail": case_range_zero_tail, "all_equal": case_all_equal, "shuffle": case_shuffle, "duplicated_table": case_duplicated_table,
         "montgomery_order": case_montgomery_order, "straddling_run": case_straddling_run, "one_digit": case_one_digit}
SIZES = [1, 2, 63, 64, 65, 257, 4099, 65539]


def with_missing(inputs, table, row):
    """the inputs with a value the table lacks at `row`"""
    have = set(table)
    absent = next(v for v in range(2, len(table) + 3) if v not in have)
    out = list(inputs)
    out[row] = absent
    return out
