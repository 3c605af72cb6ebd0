"""tests/guard_common.py catches what it exists for: fake kernels written in numpy run against a host arena, and each faulty one must be reported with the right view
name and element offset, under the poison that can show it.  The correct versions pass.  The placement rule and the guard rule hold for random carve sequences."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import guard_common as gc
from tests.guard_common import Arena, GuardViolation, OracleMismatch

R = gc.R_MOD
MASK = (1 << 256) - 1


def words(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(raw):
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, 32)
    return [int.from_bytes(r.tobytes(), "little") for r in raw]


def rand_words(seed, n):
    rng = np.random.default_rng(seed)
    return words([int.from_bytes(rng.bytes(31), "little") for _ in range(n)])       # below 2^248 < r


class Mem:
    """the fake kernels' window on the arena: word-granular loads and stores at any arena byte address"""

    def __init__(self, arena):
        self.a = arena

    def load(self, addr, n):
        return ints(self.a.mem[addr:addr + 32 * n])

    def store(self, addr, vals):
        raw = words(vals).view(np.uint8).reshape(-1)
        self.a.mem[addr:addr + raw.size] = raw


def vec_add(mem, dst, a, b, n, stored=None):
    """dst = a + b mod r; a faulty launch stores `stored` > n words (the lanes past n add what they read there)"""
    m = n if stored is None else stored
    x, y = mem.load(a, m), mem.load(b, m)
    mem.store(dst, [(p + q) % R if p < R and q < R else (p + q) & MASK for p, q in zip(x, y)])


def kate_division(mem, dst, poly, n, z, stored=None):
    a = mem.load(poly, n)
    q, acc = [0] * n, 0
    for i in range(n - 1, 0, -1):
        acc = (a[i] + z * acc) % R
        q[i - 1] = acc
    mem.store(dst, q[:n - 1 if stored is None else stored])


def prefix_sum(mem, dst, src, n, extra_read=0):
    """dst[i] = sum_{j<i} src[j]; the faulty form folds `extra_read` words past n into a carry that reaches the last element"""
    a = mem.load(src, n + extra_read)
    out, acc = [], 0
    for i in range(n):
        out.append(acc); acc = (acc + a[i]) % R
    if extra_read:
        out[n - 1] = (out[n - 1] + sum(a[n:])) % R
    mem.store(dst, out)


def make(poison, specs):
    ar = Arena("host", Arena.bytes_for(specs), poison)
    return ar, Mem(ar)


@pytest.mark.parametrize("poison", ["A", "B"])
def test_correct_kernels_pass(poison):
    n = 2047
    a, b = rand_words(1, n), rand_words(2, n)
    ar, mem = make(poison, [(n, 32)] * 3)
    A, B, D = ar.view(n, 32, fill=a, name="a"), ar.view(n, 32, fill=b, name="b"), ar.view(n, 32, name="dst")
    want = words([(p + q) % R for p, q in zip(ints(a), ints(b))])
    ar.run(lambda: vec_add(mem, D.data_ptr(), A.data_ptr(), B.data_ptr(), n), writes=[(D, 0, n)], expect=[(D, 0, want)])
    assert (D.download() == want).all() and (A.download() == a).all()
    z = 12345
    ar.run(lambda: kate_division(mem, D.data_ptr(), A.data_ptr(), n, z), writes=[(D, 0, n - 1)])
    q = ints(D.download()[:n - 1])
    ai = ints(a)
    assert all((q[i - 1] - z * (q[i] if i < n - 1 else 0) - ai[i]) % R == 0 for i in range(1, n))
    ar.run(lambda: kate_division(mem, A.at(1), A.data_ptr(), n, z), writes=[(A, 1, n - 1)], expect=[(A, 1, words(q))])     # dst == poly + 1 element
    A.upload(a)
    acc, ps = 0, []
    for v in ai:
        ps.append(acc); acc = (acc + v) % R
    ar.run(lambda: prefix_sum(mem, D.data_ptr(), A.data_ptr(), n), writes=[(D, 0, n)], expect=[(D, 0, words(ps))])
    ar.run(lambda: prefix_sum(mem, A.data_ptr(), A.data_ptr(), n), writes=[(A, 0, n)], expect=[(A, 0, words(ps))])        # in place
    ar.check_layout()


@pytest.mark.parametrize("poison", ["A", "B"])
def test_vector_add_that_stores_one_word_too_many(poison):
    n = 257
    ar, mem = make(poison, [(n, 32)] * 3)
    A, B, D = ar.view(n, 32, fill=rand_words(1, n), name="a"), ar.view(n, 32, fill=rand_words(2, n), name="b"), ar.view(n, 32, name="dst")
    with pytest.raises(GuardViolation) as e:
        ar.run(lambda: vec_add(mem, D.data_ptr(), A.data_ptr(), B.data_ptr(), n, stored=n + 1), writes=[(D, 0, n)])
    assert (e.value.view, e.value.anchor, e.value.offset) == ("dst", "end", 0)


@pytest.mark.parametrize("poison", ["A", "B"])
def test_whole_tile_stored_at_a_ragged_size(poison):
    n = 2047
    ar, mem = make(poison, [(n, 32)] * 3)
    A, B, D = ar.view(n, 32, fill=rand_words(1, n), name="a"), ar.view(n, 32, name="dst"), ar.view(n, 32, fill=rand_words(2, n), name="b")
    with pytest.raises(GuardViolation) as e:
        ar.run(lambda: vec_add(mem, B.data_ptr(), A.data_ptr(), D.data_ptr(), n, stored=2048), writes=[(B, 0, n)])
    assert (e.value.view, e.value.anchor, e.value.offset, e.value.count <= 32) == ("dst", "end", 0, True)


@pytest.mark.parametrize("poison", ["A", "B"])
def test_kate_division_that_writes_n_words(poison):
    n = 100
    ar, mem = make(poison, [(n, 32)] * 2)
    A, D = ar.view(n, 32, fill=rand_words(3, n), name="poly"), ar.view(n, 32, name="quotient")
    with pytest.raises(GuardViolation) as e:
        ar.run(lambda: kate_division(mem, D.data_ptr(), A.data_ptr(), n, 7, stored=n), writes=[(D, 0, n - 1)])
    assert (e.value.view, e.value.anchor, e.value.offset) == ("quotient", "start", n - 1)      # inside the view: the word the contract leaves alone
    with pytest.raises(GuardViolation) as e:                                                # the in-place form: n words at poly + 1 spill one behind poly
        ar.run(lambda: kate_division(mem, A.at(1), A.data_ptr(), n, 7, stored=n), writes=[(A, 1, n - 1)])
    assert (e.value.view, e.value.anchor, e.value.offset) == ("poly", "end", 0)


def test_prefix_sum_that_reads_word_n_is_caught_by_the_oracle_under_a_or_b():
    n = 2049
    a = rand_words(4, n)
    acc, ps = 0, []
    for v in ints(a):
        ps.append(acc); acc = (acc + v) % R
    caught = []
    for poison in ("A", "B"):
        ar, mem = make(poison, [(n, 32)] * 2)
        A, D = ar.view(n, 32, fill=a, name="src"), ar.view(n, 32, name="dst")
        try:
            ar.run(lambda: prefix_sum(mem, D.data_ptr(), A.data_ptr(), n, extra_read=1), writes=[(D, 0, n)], expect=[(D, 0, words(ps))])
        except OracleMismatch as e:
            assert "'dst'" in str(e) and "element %d " % (n - 1) in str(e)
            caught.append(poison)
    assert caught == ["A", "B"]
    # a read that a ZERO behind the operand would hide: a buffer that happens to be followed by zeros passes, both poisons do not
    ar, mem = make("A", [(n, 32)] * 2)
    A, D = ar.view(n, 32, fill=a, name="src"), ar.view(n, 32, name="dst")
    ar.mem[A.byte_range[1]:A.byte_range[1] + 32] = 0
    ar.run(lambda: prefix_sum(mem, D.data_ptr(), A.data_ptr(), n, extra_read=1), writes=[(D, 0, n)], expect=[(D, 0, words(ps))])


@pytest.mark.parametrize("poison", ["A", "B"])
def test_op_that_modifies_a_read_only_operand(poison):
    n = 65
    ar, mem = make(poison, [(n, 32)] * 3)
    A, B, D = ar.view(n, 32, fill=rand_words(1, n), name="a"), ar.view(n, 32, fill=rand_words(2, n), name="b"), ar.view(n, 32, name="dst")

    def call():
        vec_add(mem, D.data_ptr(), A.data_ptr(), B.data_ptr(), n)
        mem.store(B.at(17), [5])                                                              # "normalises" an input on the way
    with pytest.raises(GuardViolation) as e:
        ar.run(call, writes=[(D, 0, n)])
    assert (e.value.view, e.value.anchor, e.value.offset) == ("b", "start", 17)


@pytest.mark.parametrize("poison", ["A", "B"])
def test_store_that_jumps_the_guard_into_the_next_view(poison):
    n = 4096
    ar, mem = make(poison, [(n, 32)] * 2)
    D, B = ar.view(n, 32, name="dst"), ar.view(n, 32, fill=rand_words(2, n), name="bystander")
    far = D.byte_range[1] + (70 << 10)
    assert B.byte_range[0] <= far < B.byte_range[1]
    with pytest.raises(GuardViolation) as e:
        ar.run(lambda: mem.store(far, [1]), writes=[(D, 0, n)])
    assert (e.value.view, e.value.anchor, e.value.offset) == ("bystander", "start", (far - B.byte_range[0]) // 32)
    # and a store one word BEFORE a view
    with pytest.raises(GuardViolation) as e:
        ar.run(lambda: mem.store(B.at(-1), [1]), writes=[(D, 0, n)])
    assert (e.value.view, e.value.anchor, e.value.offset) == ("bystander", "start", -1)
    # the last word of the arena's tail guard
    with pytest.raises(GuardViolation) as e:
        ar.run(lambda: mem.store(ar.nbytes - 32, [1]), writes=[(D, 0, n)])
    assert (e.value.view, e.value.anchor) == ("bystander", "end")


def test_a_wrong_result_inside_the_declared_range_is_an_oracle_mismatch():
    n = 33
    a, b = rand_words(1, n), rand_words(2, n)
    ar, mem = make("A", [(n, 32)] * 3)
    A, B, D = ar.view(n, 32, fill=a, name="a"), ar.view(n, 32, fill=b, name="b"), ar.view(n, 32, name="dst")
    want = words([(p + q) % R for p, q in zip(ints(a), ints(b))])
    want[20, 0] ^= np.uint64(1)
    with pytest.raises(OracleMismatch) as e:
        ar.run(lambda: vec_add(mem, D.data_ptr(), A.data_ptr(), B.data_ptr(), n), writes=[(D, 0, n)], expect=[(D, 0, want)])
    assert "element 20 " in str(e.value)


def test_poison_b_is_a_valid_operand_in_phase_with_its_view():
    assert int.from_bytes(gc.FR_B, "little") == (R - 1) * (1 << 256) % R
    x, y = (int.from_bytes(gc.G1_AFFINE_B[i:i + 32], "little") * pow(1 << 256, -1, gc.P_MOD) % gc.P_MOD for i in (0, 32))
    assert (y * y - x * x * x - 3) % gc.P_MOD == 0
    assert gc.G1_JACOBIAN_B[64:] == gc.G1_AFFINE_B[:32]                                      # z = the Montgomery word of one = x
    specs = [(5, 32), (7, 64), (3, 96), (4, 128), (9, 32)]
    ar = Arena("host", Arena.bytes_for(specs), "B")
    S = ar.view(5, 32, name="scalars")
    P = ar.view(7, 64, name="points", poison_b=gc.G1_AFFINE_B)
    J = ar.view(3, 96, name="jacobian", poison_b=gc.G1_JACOBIAN_B)
    Q = ar.view(4, 128, name="g2", poison_b=gc.G2_AFFINE_B)
    T = ar.view(9, 32, name="tail")
    for v, pat in ((S, gc.FR_B), (P, gc.G1_AFFINE_B), (J, gc.G1_JACOBIAN_B), (Q, gc.G2_AFFINE_B), (T, gc.FR_B)):
        lo, hi = v.byte_range
        e = len(pat)
        assert ar.mem[hi:hi + 4 * e].tobytes() == pat * 4, v.name                            # element n, n + 1, .. of the view: whole valid elements
        assert ar.mem[lo - 4 * e:lo].tobytes() == pat * 4, v.name                            # element -1, -2, ..
        assert ar.mem[lo:hi].tobytes() == (pat * (v.nbytes // e + 1))[:v.nbytes], v.name     # an unfilled view holds poison too
    assert ar.mem[ar.nbytes - 32:].tobytes() == gc.FR_B
    arA = Arena("host", Arena.bytes_for(specs), "A")
    arA.view(7, 64, poison_b=gc.G1_AFFINE_B)
    assert (arA.mem == gc.POISON_A).all()


def test_placement_and_guard_rules_over_random_carve_sequences():
    rng = np.random.default_rng(20240607)
    for trial in range(300):
        specs = [(int(rng.integers(0, 5000)), int(rng.choice([32, 64, 96, 128]))) for _ in range(int(rng.integers(1, 7)))]
        ar = Arena("host", Arena.bytes_for(specs), "AB"[trial % 2])
        prev_end = 0
        for i, (c, e) in enumerate(specs):
            v = ar.view(c, e, align=16 if e == 32 else 1, poison_b=gc.G1_AFFINE_B if e == 64 else None)
            lo, hi = v.byte_range
            assert (v.data_ptr() - ar.base) % (2 * e) == e and lo % 16 == 0
            assert lo - prev_end >= gc.GUARD and lo - prev_end < gc.GUARD + 2 * e + 1          # at least one tile of poison, and no more slack than the rule needs
            assert hi - lo == c * e
            prev_end = hi
        assert ar.nbytes - prev_end >= gc.TAIL_GUARD
        ar.check_layout()
        ar.run(lambda: None)                                                                  # nothing ran: nothing changed
