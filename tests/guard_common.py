"""an arena of guarded views (TEST INFRASTRUCTURE): what a kernel writes NEXT TO the buffer it was given, and whether a result depends on memory past the end of an operand.

One contiguous block -- a halo2.DeviceBuffer (a library block, as the Rust shim would hold it) or, for the self-test of the checker, a numpy byte array -- is filled with a
poison; operands are carved out of it as views at odd element offsets with at least GUARD bytes of poison around each.  Arena.run snapshots the whole block, runs one call,
downloads the block again and holds every byte outside the declared write ranges to the snapshot: that one rule covers the guards, the tail of a ragged output and every
read-only operand.  The declared output is compared with an oracle that never saw the poison, under two poisons, so a result that moves with the poison is a read past the end.

Poison A is the byte 0xA5 everywhere: a word above r, coordinates above p, no curve point.  Poison B is a VALID operand repeated -- the Montgomery word of r - 1 for Fr
vectors, a curve point for point arrays (the poison_b argument of Arena.view) -- so that a validity check cannot hide a stray read.  Poison B is laid in phase with the view it surrounds: the word
at element offset n of a view of n elements is a whole poison element.
"""
import numpy as np

GUARD = 64 << 10                # one 2048-word scan tile, the largest unit any kernel here stores per workgroup
TAIL_GUARD = 1 << 20
POISON_A = 0xA5
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def _mont(v, m):
    return (v % m * (1 << 256) % m).to_bytes(32, "little")


FR_B = _mont(R_MOD - 1, R_MOD)                                             # r - 1: valid, non-zero, changes every sum and product it enters
G1_AFFINE_B = _mont(1, P_MOD) + _mont(2, P_MOD)                            # the generator (1, 2)
G1_JACOBIAN_B = G1_AFFINE_B + _mont(1, P_MOD)
G1_COMPRESSED_B = (1).to_bytes(32, "little")                               # x = 1, y = 2 is even: the generator's 32-byte word
G2_AFFINE_B = b"".join(_mont(c, P_MOD) for c in (
    0x1800DEEF121F1E76426A00665E5C4479674322D4F75EDADD46DEBD5CD992F6ED, 0x198E9393920D483A7260BFB731FB5D25F1AA493335A9E71297E485B7AEF312C2,
    0x12C85EA5DB8C6DEB4AAB71808DCB408FE3D1E7690C43D37B4CE6CC0166FA7DAA, 0x090689D0585FF075EC9E99AD690C3395BC4B313370B38EF355ACDADCD122975B))


class GuardViolation(AssertionError):
    """a byte outside the declared writes changed.  view: the nearest view's name; anchor: "start" or "end"; offset: signed ELEMENT offset from it (a byte inside the view
    counts from its start; before it: negative from the start; behind it: >= 0 from the end)"""

    def __init__(self, view, anchor, offset, byte_offset, count):
        super().__init__("%d byte(s) changed outside the declared writes; the first at arena byte %d = view %r, %s %+d elements" % (count, byte_offset, view, anchor, offset))
        self.view, self.anchor, self.offset, self.byte_offset, self.count = view, anchor, offset, byte_offset, count


class OracleMismatch(AssertionError):
    pass


def _tile(pattern: bytes, nbytes: int, phase: int = 0) -> np.ndarray:
    """nbytes of the repeating pattern, starting `phase` bytes into it"""
    p = np.frombuffer(pattern, dtype=np.uint8)
    phase %= len(p)
    reps = (nbytes + phase + len(p) - 1) // len(p)
    return np.tile(p, reps)[phase:phase + nbytes]


class View:
    """`count` elements of `elem_bytes` inside an arena.  Quacks like a device tensor for the halo2 wrappers (data_ptr / numel / element_size / is_cuda)."""
    is_cuda = True

    def __init__(self, arena, name, offset, count, elem_bytes):
        self.arena, self.name, self.offset, self.count, self.elem_bytes = arena, name, offset, count, elem_bytes
        self.nbytes = count * elem_bytes

    @property
    def byte_range(self):
        return self.offset, self.offset + self.nbytes

    def data_ptr(self) -> int:
        return self.arena.base + self.offset

    def at(self, elem: int) -> int:
        """the address of element `elem` (a pointer INTO the view, for aliased forms such as dst == poly + 1 element)"""
        return self.arena.base + self.offset + elem * self.elem_bytes

    def numel(self) -> int:
        return self.nbytes

    def element_size(self) -> int:
        return 1

    def upload(self, arr, first_elem: int = 0) -> None:
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert first_elem * self.elem_bytes + raw.size <= self.nbytes, "upload leaves the view %r" % self.name
        self.arena._write(self.offset + first_elem * self.elem_bytes, raw)

    def download(self, dtype=np.uint64) -> np.ndarray:
        return self.arena._read(self.offset, self.nbytes).view(dtype).reshape(self.count, -1)


class Arena:
    """backend "device": one halo2.DeviceBuffer (h2 = the halo2 module, sync = mi355_synchronize); backend "host": a numpy byte array.  poison: "A" or "B"."""

    def __init__(self, backend, nbytes, poison="A", h2=None, sync=None):
        assert backend in ("device", "host") and poison in ("A", "B")
        self.backend, self.nbytes, self.poison, self.views, self._sync = backend, (int(nbytes) + 63) // 64 * 64, poison, [], sync
        self._pattern = bytes([POISON_A]) if poison == "A" else FR_B
        fill = _tile(self._pattern, self.nbytes)
        if backend == "device":
            self.buf = h2.DeviceBuffer(self.nbytes)
            self.base = self.buf.data_ptr()
            assert self.base % 256 == 0
            self.buf.upload(fill)
        else:
            self.mem = fill.copy()
            self.base = 0
        self._cursor, self._own_poison_behind = 0, False

    @staticmethod
    def bytes_for(specs):
        """an arena size that holds views of (count, elem_bytes) carved in this order"""
        return sum(GUARD + 3 * e + c * e for c, e in specs) + TAIL_GUARD + 64

    # ---- the two backends
    def _write(self, off, raw):
        assert 0 <= off and off + raw.size <= self.nbytes
        if self.backend == "device":
            if raw.size:
                self.buf.upload(raw, offset=off)
        else:
            self.mem[off:off + raw.size] = raw

    def _read(self, off, n):
        assert 0 <= off and off + n <= self.nbytes
        if self.backend == "device":
            return self.buf.download(n, offset=off).view(np.uint8) if n % 8 == 0 else self.buf.download((n + 7) // 8 * 8, offset=off).view(np.uint8)[:n]
        return self.mem[off:off + n].copy()

    def free(self):
        if self.backend == "device":
            self.buf.free()

    # ---- carving
    def view(self, count, elem_bytes, fill=None, name=None, poison_b=None, align=1):
        """the next view: `count` elements at base + odd * elem_bytes (and a multiple of `align`, where the header states one), GUARD bytes or more behind the previous
        view.  fill: the initial contents (an array of count * elem_bytes bytes); without it the view holds poison like its surroundings.  poison_b: under poison B, the
        valid element (bytes whose length divides elem_bytes or is a multiple of 32) repeated around THIS view in place of the Fr word: half of the gap before it, and
        everything behind it up to the next view's half."""
        e = int(elem_bytes)
        start = self._cursor + GUARD
        start += (e - start % (2 * e)) % (2 * e)                     # start = e (mod 2 e): an odd multiple of the element size
        assert start % (2 * e) == e and start % align == 0, "element size %d cannot honour alignment %d at an odd offset" % (e, align)
        v = View(self, name or "view%d" % len(self.views), start, int(count), e)
        end = start + v.nbytes
        assert end + TAIL_GUARD <= self.nbytes, "arena too small for view %r" % v.name
        if self.poison == "B" and poison_b is not None:
            half = self._cursor + (start - self._cursor) // 2 if self.views else 0
            self._write(half, _tile(poison_b, start - half, phase=-(start - half)))
            self._write(start, _tile(poison_b, self.nbytes - start))   # the view itself and all that follows: a later view re-lays its own half
            self._own_poison_behind = True
        elif self._own_poison_behind:
            half = self._cursor + (start - self._cursor) // 2          # back to the arena's own word behind a view that brought its own
            self._write(half, _tile(self._pattern, self.nbytes - half, phase=half))
            self._own_poison_behind = False
        self.views.append(v)
        self._cursor = end
        if fill is not None:
            raw = np.ascontiguousarray(fill).view(np.uint8).reshape(-1)
            assert raw.size == v.nbytes, "fill of view %r: %d bytes for %d" % (v.name, raw.size, v.nbytes)
            self._write(start, raw)
        return v

    # ---- the check
    def locate(self, byte_offset):
        """(view name, anchor, signed element offset) of an arena byte"""
        best = None
        for v in self.views:
            lo, hi = v.byte_range
            if lo <= byte_offset < hi:
                return v.name, "start", (byte_offset - lo) // v.elem_bytes
            if byte_offset < lo:
                d, where = lo - byte_offset, (v.name, "start", -((lo - byte_offset + v.elem_bytes - 1) // v.elem_bytes))
            else:
                d, where = byte_offset - hi + 1, (v.name, "end", (byte_offset - hi) // v.elem_bytes)
            if best is None or d < best[0]:
                best = (d, where)
        assert best is not None, "an arena without views"
        return best[1]

    def run(self, call, writes=(), expect=()):
        """snapshot the whole arena, run call() and synchronise, download the arena, hold every byte outside `writes` = [(view, first_elem, n_elems), ...] to the snapshot
        (GuardViolation), then hold `expect` = [(view, first_elem, array), ...] to the bytes now in the arena (OracleMismatch).  Returns (call's result, the arena's bytes)."""
        assert self.views and self._cursor + TAIL_GUARD <= self.nbytes
        before = self._read(0, self.nbytes)
        result = call()
        if self._sync is not None:
            self._sync()
        after = self._read(0, self.nbytes)
        changed = before != after
        for v, first, n in writes:
            assert v.arena is self and 0 <= first and first + n <= v.count, "a declared write leaves view %r" % v.name
            changed[v.offset + first * v.elem_bytes:v.offset + (first + n) * v.elem_bytes] = False
        bad = np.flatnonzero(changed)
        if bad.size:
            raise GuardViolation(*self.locate(int(bad[0])), int(bad[0]), int(bad.size))
        for v, first, want in expect:
            raw = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
            lo = v.offset + first * v.elem_bytes
            assert lo + raw.size <= v.offset + v.nbytes
            diff = np.flatnonzero(after[lo:lo + raw.size] != raw)
            if diff.size:
                i = int(diff[0]) // v.elem_bytes
                raise OracleMismatch("view %r: element %d of the declared output differs from the oracle under poison %s (%d elements differ): got %s, want %s" % (
                    v.name, first + i, self.poison, np.unique(diff // v.elem_bytes).size,
                    after[lo + i * v.elem_bytes:lo + (i + 1) * v.elem_bytes].tobytes().hex(), raw[i * v.elem_bytes:(i + 1) * v.elem_bytes].tobytes().hex()))
        return result, after

    def check_layout(self):
        """the placement rule and the guard rule of every view carved so far"""
        prev_end = None
        for v in self.views:
            lo, hi = v.byte_range
            assert lo % (2 * v.elem_bytes) == v.elem_bytes, (v.name, lo)
            assert lo - (prev_end or 0) >= GUARD, (v.name, lo, prev_end)
            prev_end = hi
        assert self.nbytes - prev_end >= TAIL_GUARD
