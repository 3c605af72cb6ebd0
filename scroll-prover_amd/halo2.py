"""
halo2.py -- host-side mirror of the halo2_proofs operator surface that scroll-prover reaches through
`gen_halo2_chunk_proof` / `gen_batch_proof` / `gen_bundle_proof` [REF integration/src/prove.rs:37,67,96], implemented
on libmi355zk.so.  Names, argument meaning and error behaviour follow halo2_proofs@e5ddf67 [EXT-recalled]:

  best_multiexp(coeffs, bases)          src/arithmetic.rs   panics (here: AssertionError) on length mismatch
  best_fft(a, omega, log_n)             src/arithmetic.rs   in place, natural -> natural
  EvaluationDomain(j, k)                src/poly/domain.rs  lagrange_to_coeff, coeff_to_lagrange, coeff_to_extended,
                                                            extended_to_coeff, constants omega/omega_inv/extended_omega/g_coset
  ParamsKZG                             src/poly/kzg/commitment.rs  setup, commit, commit_lagrange, downsize, n, k

Host arrays are numpy uint64: [n, 4] field elements (Montgomery LE limbs), [n, 8] G1Affine, [12] G1 (Jacobian).
Device-resident operands are torch.uint8/uint64 CUDA tensors; they are passed by address (torch is plumbing only).
The constants (omega, n^-1, ...) are computed with Python integers -- host set-up, exactly as EvaluationDomain::new does.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import Mi355Error, check, lib, ptr

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
FR_S = 28
FR_ROOT_OF_UNITY = pow(7, (R_MOD - 1) >> FR_S, R_MOD)
FR_ZETA = 0x30644E72E131A029048B6E193FD84104CC37A73FEC2BC5E9B8CA0B2D36636F23  # halo2curves bn256::Fr::ZETA [EXT-recalled]
_M64 = (1 << 64) - 1


def fr(x: int) -> np.ndarray:
    """canonical integer -> 4 x u64 Montgomery limbs (the in-memory form of halo2curves Fr)."""
    v = (x % R_MOD) * (1 << 256) % R_MOD
    return np.array([(v >> (64 * i)) & _M64 for i in range(4)], dtype=np.uint64)


def fr_to_int(limbs) -> int:
    v = sum(int(l) << (64 * i) for i, l in enumerate(limbs))
    return v * pow(1 << 256, -1, R_MOD) % R_MOD


def _is_device(x) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


# ------------------------------------------------------------------------------------------ arithmetic.rs
def best_multiexp(coeffs, bases) -> np.ndarray:
    """sum_i coeffs[i] * bases[i] -> G1 (12 u64: normalised Jacobian).  bases: host [n,8] array or a ParamsKZG basis handle slice."""
    n = int(coeffs.shape[0])
    out = np.zeros(12, dtype=np.uint64)
    if isinstance(bases, SrsSlice):
        assert n == bases.n, "best_multiexp: coeffs.len() != bases.len()"
        fn = lib().mi355_msm_g1_dev if _is_device(coeffs) else lib().mi355_msm_g1_host
        check(fn(bases.handle, bases.offset, ptr(coeffs), n, ptr(out)))
        return out
    assert n == int(bases.shape[0]), "best_multiexp: coeffs.len() != bases.len()"
    check(lib().mi355_msm_g1_adhoc_host(ptr(np.ascontiguousarray(bases)), ptr(np.ascontiguousarray(coeffs)), n, ptr(out)))
    return out


def best_fft(a, omega: np.ndarray, log_n: int) -> None:
    """in place; a is a host [2^log_n, 4] uint64 array or a device tensor of 2^log_n * 32 bytes (G = Fr), or -- the G = G1
    instantiation used by g_to_lagrange -- a host [2^log_n, 12] array / device tensor of 2^log_n * 96 bytes of Jacobian points."""
    if _is_device(a):
        nbytes = a.numel() * a.element_size()
        if nbytes == 96 << log_n:
            check(lib().mi355_g1_fft_dev(ptr(a), log_n, ptr(omega)))
            return
        assert nbytes == 32 << log_n
        check(lib().mi355_ntt_fr_dev(ptr(a), log_n, ptr(omega)))
    elif a.ndim == 2 and a.shape[1] == 12:
        assert a.shape == (1 << log_n, 12) and a.dtype == np.uint64
        check(lib().mi355_g1_fft_host(ptr(a), log_n, ptr(omega)))
    else:
        assert a.shape == (1 << log_n, 4) and a.dtype == np.uint64
        check(lib().mi355_ntt_fr_host(ptr(a), log_n, ptr(omega)))


def best_fft_many(polys, omega: np.ndarray, log_n: int, divisor=None) -> None:
    """`for a in polys: best_fft(a, omega, log_n)` (divisor: ... followed by a *= divisor, i.e. EvaluationDomain::ifft) as ONE call:
    mi355_ntt_fr_batch_host / _dev deal the independent transforms over the bound devices (host arrays round-robin; device buffers on the
    device that owns them).  In place; all host arrays or all device buffers."""
    if len(polys) == 0:
        return
    dev = _is_device(polys[0])
    assert all(_is_device(q) == dev for q in polys), "best_fft_many: mix of host and device polynomials"
    if dev:
        arr = (C.c_void_p * len(polys))(*[q.data_ptr() for q in polys])
        check(lib().mi355_ntt_fr_batch_dev(arr, len(polys), log_n, ptr(omega), ptr(divisor)))
    else:
        for q in polys:
            assert q.shape == (1 << log_n, 4) and q.dtype == np.uint64 and q.flags["C_CONTIGUOUS"]
        arr = (C.c_void_p * len(polys))(*[q.ctypes.data for q in polys])
        check(lib().mi355_ntt_fr_batch_host(arr, len(polys), log_n, ptr(omega), ptr(divisor)))


def compact_nonzero(col: np.ndarray, threads: int = 8):
    """(indices, values) of the non-zero cells of a [n, 4] u64 column, in index order (mi355_host_compact_nonzero: host threads, no device)"""
    col = np.ascontiguousarray(col, dtype=np.uint64)
    n = col.shape[0]
    idx = np.empty(n, dtype=np.uint32); vals = np.empty((n, 4), dtype=np.uint64); cnt = C.c_uint64()
    check(lib().mi355_host_compact_nonzero(ptr(col), n, ptr(idx), ptr(vals), C.byref(cnt), threads))
    return idx[: cnt.value].copy(), vals[: cnt.value].copy()


class DeviceBuffer:
    """One mi355_buf_alloc block: the Python twin of the Rust shim's DevicePoly (rust_shim/mi355zk.rs).  Quacks like a device tensor for
    the wrappers of this module (data_ptr / numel / element_size); `slot` picks the device of an mi355_init_multi process."""

    def __init__(self, nbytes: int, slot: int = 0):
        p = C.c_void_p()
        check(lib().mi355_buf_alloc(nbytes, slot, C.byref(p)))
        self._ptr, self.nbytes, self.slot = p.value, nbytes, slot

    @classmethod
    def from_host(cls, arr: np.ndarray, slot: int = 0) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes, slot)
        b.upload(arr)
        return b

    @classmethod
    def from_packed(cls, values: np.ndarray, slot: int = 0) -> "DeviceBuffer":
        """a column whose cells are known to fit 1 / 2 / 4 / 8 bytes (values: uint8 / 16 / 32 / 64, CANONICAL integers): that many bytes per cell cross PCIe, the device
        expands to Montgomery words (mi355_buf_upload_packed)"""
        values = np.ascontiguousarray(values)
        assert values.dtype in (np.uint8, np.uint16, np.uint32, np.uint64) and values.ndim == 1
        b = cls(32 * values.shape[0], slot)
        check(lib().mi355_buf_upload_packed(C.c_void_p(b._ptr), ptr(values), values.shape[0], values.dtype.itemsize))
        return b

    @classmethod
    def from_sparse(cls, col: np.ndarray, slot: int = 0, threads: int = 8) -> "DeviceBuffer":
        """a mostly-zero column ([n, 4] u64 Montgomery words): only its non-zero cells cross PCIe (mi355_host_compact_nonzero + mi355_buf_upload_sparse)"""
        idx, vals = compact_nonzero(col, threads)
        b = cls(col.nbytes, slot)
        check(lib().mi355_buf_upload_sparse(C.c_void_p(b._ptr), col.shape[0], ptr(idx), ptr(vals), idx.shape[0]))
        return b

    def data_ptr(self) -> int:
        return self._ptr

    def numel(self) -> int:
        return self.nbytes

    def element_size(self) -> int:
        return 1

    is_cuda = True

    def upload(self, arr: np.ndarray, offset: int = 0) -> None:
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        check(lib().mi355_buf_upload(C.c_void_p(self._ptr + offset), ptr(arr), arr.nbytes))

    def download(self, nbytes: int | None = None, offset: int = 0) -> np.ndarray:
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(nbytes // 8, dtype=np.uint64)
        check(lib().mi355_buf_download(ptr(out), C.c_void_p(self._ptr + offset), nbytes))
        return out

    def fr(self) -> np.ndarray:
        return self.download().reshape(-1, 4)

    def free(self) -> None:
        if self._ptr:
            check(lib().mi355_buf_free(C.c_void_p(self._ptr)))
            self._ptr = 0


def g_to_lagrange(g_dev, k: int):
    """g_to_lagrange(g_projective, k) [EXT-recalled halo2_proofs src/arithmetic.rs]: g_lagrange = n^-1 * best_fft(g, omega^-1, k), as a new
    device tensor of 2^k affine points; g_dev: device tensor (or raw device address) holding at least 2^k affine points."""
    import torch
    n = 1 << k
    w_inv = pow(pow(FR_ROOT_OF_UNITY, 1 << (FR_S - k), R_MOD), R_MOD - 2, R_MOD)
    out = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    src = C.c_void_p(g_dev) if isinstance(g_dev, int) else ptr(g_dev)
    check(lib().mi355_g_to_lagrange_dev(src, ptr(out), k, ptr(fr(w_inv)), ptr(fr(pow(n, R_MOD - 2, R_MOD)))))
    return out


def eval_polynomial(poly, point: np.ndarray) -> np.ndarray:
    """halo2_proofs::arithmetic::eval_polynomial: sum_i poly[i] * point^i -> Fr (4 x u64 Montgomery limbs)."""
    out = np.zeros(4, dtype=np.uint64)
    if _is_device(poly):
        n = poly.numel() * poly.element_size() // 32
        check(lib().mi355_eval_polynomial_dev(ptr(poly), n, ptr(point), ptr(out)))
    else:
        poly = np.ascontiguousarray(poly, dtype=np.uint64)
        check(lib().mi355_eval_polynomial_host(ptr(poly), poly.shape[0], ptr(point), ptr(out)))
    return out


def eval_polynomial_many(polys, points) -> np.ndarray:
    """[eval_polynomial(p, x) for p, x in zip(polys, points)] on device-resident coefficient vectors of equal length with ONE synchronisation
    (mi355_eval_polynomial_batch_dev): step 9 of create_proof evaluates every queried (polynomial, rotation) pair.  -> [len(polys), 4] u64."""
    m = len(polys)
    out = np.zeros((m, 4), dtype=np.uint64)
    if m == 0:
        return out
    n = polys[0].numel() * polys[0].element_size() // 32
    assert all(q.numel() * q.element_size() // 32 == n for q in polys), "eval_polynomial_many: polynomials of equal length"
    pts = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.uint64) for x in points]))
    arr = (C.c_void_p * m)(*[q.data_ptr() for q in polys])
    check(lib().mi355_eval_polynomial_batch_dev(arr, m, n, ptr(pts), ptr(out)))
    return out


def interleave(parts, out=None):
    """the extended-domain vector from its Q coset parts (scroll fork: part q = the evaluations at zeta * extended_omega^(q + Q i)):
    out[i * Q + q] = parts[q][i] (mi355_fr_interleave_dev); what extended_to_coeff inverts."""
    import torch
    q = len(parts)
    n = parts[0].numel() * parts[0].element_size() // 32
    if out is None:
        out = torch.empty((q * n, 4), dtype=torch.int64, device=parts[0].device)
    arr = (C.c_void_p * q)(*[p_.data_ptr() for p_ in parts])
    check(lib().mi355_fr_interleave_dev(ptr(out), arr, q, n))
    return out


def mem_info(slot: int = 0) -> dict:
    """HBM accounting of one bound device (mi355_mem_info): what HIP reports free / in total and what the library holds, in bytes."""
    v = [C.c_uint64() for _ in range(5)]
    check(lib().mi355_mem_info(slot, *[C.byref(x) for x in v]))
    return dict(zip(("free", "total", "live_buffers", "pooled", "workspace"), (x.value for x in v)))


MEM_CLASSES = ("buffers", "workspace", "ntt_required", "ntt_optional", "srs", "window_tables", "fixed_tables")


def mem_set_limit(bytes_: int, slot: int = 0) -> None:
    """A limit on the device memory the library holds on one device slot (mi355_mem_set_limit; 0 lifts it).  An allocation that would pass it is decided on the host, before
    any HIP call: the pool and the free slabs go back first, then the optional NTT tables, then the call raises Mi355Error(EOOM) naming the limit."""
    check(lib().mi355_mem_set_limit(slot, int(bytes_)))


def mem_usage(slot: int = 0) -> dict:
    """What the library's ledger holds on one device slot (mi355_mem_usage), in bytes: held (the sum of the classes), limit (0: none), high_water since mem_reset_peak,
    classes {name: bytes} in the order of MEM_CLASSES, reclaims, refused."""
    held, limit, peak, reclaims, refused = (C.c_uint64() for _ in range(5))
    cls = (C.c_uint64 * len(MEM_CLASSES))()
    check(lib().mi355_mem_usage(slot, C.byref(held), C.byref(limit), C.byref(peak), cls, len(MEM_CLASSES), C.byref(reclaims), C.byref(refused)))
    return {"held": held.value, "limit": limit.value, "high_water": peak.value, "classes": dict(zip(MEM_CLASSES, (int(x) for x in cls))), "reclaims": reclaims.value, "refused": refused.value}


def mem_reset_peak(slot: int = 0) -> None:
    check(lib().mi355_mem_reset_peak(slot))


def fr_vec_op(op: str, dst, a, b):
    """element-wise add / sub / mul of device-resident Fr vectors (pointwise steps of the quotient construction)."""
    n = a.numel() * a.element_size() // 32
    check(lib().mi355_fr_vec_op_dev({"add": 0, "sub": 1, "mul": 2}[op], ptr(dst), ptr(a), ptr(b), n))
    return dst


def fr_vec_axpy(dst, a, b, scalar: np.ndarray):
    """dst = a + scalar * b on device-resident Fr vectors (a = None: dst = scalar * b)."""
    n = b.numel() * b.element_size() // 32
    check(lib().mi355_fr_vec_axpy_dev(ptr(dst), ptr(a) if a is not None else None, ptr(b), ptr(scalar), n))
    return dst


def gate_eval(dst, polys, terms, n: int, accumulate: bool = False):
    """dst[i] (+)= sum_j c_j * prod_k polys[p][(i + rot) mod n] in ONE launch (mi355_fr_gate_eval_dev): the operand shape of halo2's
    evaluate_h (rotated columns, sums of products).  terms: list of (c_j: [4] u64 Montgomery, [(poly index, rotation in elements), ...])."""
    coeffs = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.uint64) for c, _ in terms])) if terms else np.zeros((0, 4), dtype=np.uint64)
    term_len = (C.c_uint32 * max(1, len(terms)))(*[len(f) for _, f in terms])
    flat = [pr for _, f in terms for pr in f]
    fp = (C.c_uint32 * max(1, len(flat)))(*[p for p, _ in flat])
    fr_ = (C.c_int32 * max(1, len(flat)))(*[r for _, r in flat])
    arr = (C.c_void_p * max(1, len(polys)))(*[q.data_ptr() for q in polys])
    check(lib().mi355_fr_gate_eval_dev(ptr(dst), arr, len(polys), ptr(coeffs), term_len, len(terms), fp, fr_, n, 1 if accumulate else 0))
    return dst


def kate_division(poly, z: np.ndarray, dst=None):
    """halo2_proofs::arithmetic::kate_division: (poly(X) - poly(z)) / (X - z) on a device-resident coefficient vector -> n - 1 coefficients."""
    import torch
    n = poly.numel() * poly.element_size() // 32
    if dst is None:
        dst = torch.empty((max(n - 1, 0), 4), dtype=torch.int64, device=poly.device)
    check(lib().mi355_fr_kate_division_dev(ptr(dst) if n > 1 else None, ptr(poly), n, ptr(z)))
    return dst


def batch_invert(a):
    """ff::BatchInvert on a device-resident Fr vector, in place: a[i] = a[i]^-1, zeros stay zero."""
    check(lib().mi355_fr_batch_invert_dev(ptr(a), a.numel() * a.element_size() // 32))
    return a


def prefix_product(src, dst=None, want_total: bool = False):
    """the grand-product column of the permutation / lookup arguments: dst[0] = 1, dst[i] = prod_{j<i} src[j] (device tensors; dst
    defaults to a new tensor).  want_total: also return prod_{j<n} src[j] (the value that must be one for a valid argument)."""
    import torch
    if dst is None:
        dst = torch.empty_like(src)
    total = np.zeros(4, dtype=np.uint64) if want_total else None
    check(lib().mi355_fr_prefix_product_dev(ptr(dst), ptr(src), src.numel() * src.element_size() // 32, ptr(total) if want_total else None))
    return (dst, total) if want_total else dst


def prefix_sum(src, dst=None, want_total: bool = False):
    """the running sum phi of the log-derivative (mv-lookup) argument: dst[0] = 0, dst[i] = sum_{j<i} src[j] (device buffers; dst defaults to a
    new tensor).  want_total: also return sum_{j<n} src[j] (zero for a valid argument)."""
    import torch
    if dst is None:
        dst = torch.empty_like(src)
    total = np.zeros(4, dtype=np.uint64) if want_total else None
    check(lib().mi355_fr_prefix_sum_dev(ptr(dst), ptr(src), src.numel() * src.element_size() // 32, ptr(total) if want_total else None))
    return (dst, total) if want_total else dst


def lookup_multiplicities(table, inputs, table_rows: int, input_rows: int, last: bool = False):
    """the multiplicity column m of the mv-lookup argument (mi355_fr_lookup_multiplicities_dev) on device tensors: `table` holds n words (rows < table_rows
    are the table), `inputs` is one tensor or a list of them (rows < input_rows read).  m[r] = how many input cells equal the value of table row r, where r is
    the first row holding that value (last=True: the last); rows >= table_rows are zero.  Returns m as a new tensor like `table`.  A value missing from the
    table raises Mi355Error (EBADARG) whose `.column` / `.row` name the smallest such (input, row)."""
    import torch
    if not isinstance(inputs, (list, tuple)):
        inputs = [inputs]
    n = table.numel() * table.element_size() // 32
    for t in inputs:
        assert t.numel() * t.element_size() >= 32 * input_rows, "an input column is shorter than input_rows"
    m = torch.empty_like(table)
    arr = (C.c_void_p * max(1, len(inputs)))(*[t.data_ptr() for t in inputs])
    missing = C.c_uint64(0)
    rc = lib().mi355_fr_lookup_multiplicities_dev(ptr(m), n, ptr(table), table_rows, arr, len(inputs), input_rows, 1 if last else 0, C.byref(missing))
    if rc != 0:
        err = Mi355Error(rc, lib().mi355_last_error().decode())
        err.column, err.row = (missing.value >> 40, missing.value & ((1 << 40) - 1)) if rc == 1 and missing.value != (1 << 64) - 1 else (None, None)
        raise err
    return m


def lookup_permute(input, table, rows: int, perm_input=None, perm_table=None):
    """the permuted columns (A', S') of the classic halo2 lookup argument (mi355_fr_lookup_permute_dev) on device tensors: rows < `rows` of `input` and `table`
    are the theta-compressed columns.  A' is the input sorted ascending by canonical value; S' holds the run's value where a run of A' starts and the table's
    leftover copies, ascending, from the last other row backwards.  Returns (perm_input, perm_table): new tensors like `input` unless given; rows >= `rows` are
    not written.  A value missing from the table raises Mi355Error (EBADARG) whose `.row` is the smallest such row of `input`."""
    import torch
    for t in (input, table):
        assert t.numel() * t.element_size() >= 32 * rows, "a column is shorter than rows"
    if perm_input is None:
        perm_input = torch.empty_like(input)
    if perm_table is None:
        perm_table = torch.empty_like(input)
    missing = C.c_uint64(0)
    rc = lib().mi355_fr_lookup_permute_dev(ptr(perm_input), ptr(perm_table), ptr(input), ptr(table), rows, C.byref(missing))
    if rc != 0:
        err = Mi355Error(rc, lib().mi355_last_error().decode())
        err.row = missing.value if rc == 1 and missing.value != (1 << 64) - 1 else None
        raise err
    return perm_input, perm_table


class PermutationAssembly:
    """the copy-constraint bookkeeping of permutation::keygen::Assembly [EXT-recalled halo2_proofs src/plonk/permutation/keygen.rs]; the twin of
    halo2::PermutationAssembly in include/mi355zk_halo2.hpp.  A cell is the integer column * n + row.  `mapping[cell]` is the cell's image, `aux[cell]` the
    cell that names its cycle, `sizes[cell]` the length of the cycle a naming cell names.  copy() joins two cycles the way halo2 does -- the smaller one is
    relabelled into the larger, then the two cells' mapping entries are swapped -- and does nothing inside one cycle, so the cycle order is halo2's."""

    def __init__(self, n_cols: int, n: int):
        self.n_cols, self.n = int(n_cols), int(n)
        self.mapping = np.arange(self.n_cols * self.n, dtype=np.uint64)
        self.aux = self.mapping.copy()
        self.sizes = np.ones(self.n_cols * self.n, dtype=np.uint64)

    def copy(self, col_a: int, row_a: int, col_b: int, row_b: int) -> None:
        assert 0 <= col_a < self.n_cols and 0 <= col_b < self.n_cols and 0 <= row_a < self.n and 0 <= row_b < self.n, "PermutationAssembly.copy: cell outside the permutation"
        mapping, aux, sizes = self.mapping, self.aux, self.sizes
        a, b = col_a * self.n + row_a, col_b * self.n + row_b
        keep, fold = int(aux[a]), int(aux[b])
        if keep == fold:
            return
        if sizes[keep] < sizes[fold]:
            keep, fold = fold, keep
        sizes[keep] += sizes[fold]
        c = fold
        while True:
            aux[c] = keep
            c = int(mapping[c])
            if c == fold:
                break
        mapping[a], mapping[b] = mapping[b], mapping[a]

    def overrides(self):
        """(cells, images): exactly the cells with mapping != identity, in cell order -- the two lists permutation_sigma takes"""
        cells = np.nonzero(self.mapping != np.arange(self.mapping.size, dtype=np.uint64))[0].astype(np.uint64)
        return cells, self.mapping[cells].copy()


def permutation_sigma(n_cols: int, log_n: int, delta: np.ndarray, omega: np.ndarray, cells=(), images=(), device=None, trusted: bool = False, out=None):
    """the sigma columns of the permutation argument (mi355_fr_permutation_sigma_dev) as device tensors: sigma[j][r] = delta^j omega^r, then
    sigma[cells[t]] = delta^j' omega^r' for (j', r') = images[t] (cell = column * n + row; PermutationAssembly.overrides() gives the lists).  Returns a list of
    n_cols tensors of [2^log_n, 4] int64 (`out`: write into these instead).  A list that is no permutation of its cells raises Mi355Error (EBADARG) naming the
    first offending index, before anything reaches the device; trusted=True keeps the range check only."""
    cells = np.ascontiguousarray(cells, dtype=np.uint64).reshape(-1)
    images = np.ascontiguousarray(images, dtype=np.uint64).reshape(-1)
    assert cells.size == images.size, "permutation_sigma: cells and images differ in length"
    if out is None:
        import torch
        out = [torch.empty((1 << log_n, 4), dtype=torch.int64, device=device) for _ in range(n_cols)]
    assert len(out) == n_cols
    for t in out:
        assert t.numel() * t.element_size() == 32 << log_n, "permutation_sigma: a column is not 2^log_n words"
    arr = (C.c_void_p * max(1, n_cols))(*[t.data_ptr() for t in out])
    u64p = C.POINTER(C.c_uint64)
    check(lib().mi355_fr_permutation_sigma_dev(arr, n_cols, log_n, ptr(delta), ptr(omega), cells.ctypes.data_as(u64p), images.ctypes.data_as(u64p), cells.size, 1 if trusted else 0))
    return out


def nonzero_rows(vecs, cap: int = 16):
    """MockProver::verify's gate check on device tensors (mi355_fr_nonzero_rows_dev): `vecs` is one tensor or a list of tensors of n 32-byte words each (a gate
    evaluated on the Lagrange domain).  Returns (counts, rows): counts[v] = the rows of vector v whose word is not all-zero, rows[v] = the smallest `cap` of them,
    ascending, unused slots 2^64 - 1 (numpy uint64, shapes [batch] and [batch, cap]).  A failing witness is not an error.  cap = 0: counts only."""
    if not isinstance(vecs, (list, tuple)):
        vecs = [vecs]
    n = vecs[0].numel() * vecs[0].element_size() // 32 if vecs else 0
    for t in vecs:
        assert t.numel() * t.element_size() == 32 * n, "nonzero_rows: the vectors differ in length"
    arr = (C.c_void_p * max(1, len(vecs)))(*[t.data_ptr() for t in vecs])
    counts = np.zeros(len(vecs), dtype=np.uint64)
    rows = np.full((len(vecs), cap), (1 << 64) - 1, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    check(lib().mi355_fr_nonzero_rows_dev(arr, len(vecs), n, cap, counts.ctypes.data_as(u64p), rows.ctypes.data_as(u64p) if cap else None))
    return counts, rows


def copy_check(cols, cells, images, cap: int = 16):
    """MockProver::verify's permutation check on device tensors (mi355_fr_copy_check_dev): `cols` are the columns in permutation position order, 2^log_n words each;
    (cells, images) is what PermutationAssembly.overrides() returns (cell = column * n + row).  Pair t fails when the two cells hold different words.  Returns
    (n_failed, failed_t): the number of failing pairs and the smallest `cap` failing t, ascending, unused slots 2^64 - 1.  A list with a cell outside the columns raises
    Mi355Error (EBADARG) naming the pair, before anything reaches the device."""
    cells = np.ascontiguousarray(cells, dtype=np.uint64).reshape(-1)
    images = np.ascontiguousarray(images, dtype=np.uint64).reshape(-1)
    assert cells.size == images.size, "copy_check: cells and images differ in length"
    n = cols[0].numel() * cols[0].element_size() // 32 if len(cols) else 1
    log_n = max(0, n.bit_length() - 1)
    for t in cols:
        assert t.numel() * t.element_size() == 32 << log_n, "copy_check: a column is not 2^log_n words"
    arr = (C.c_void_p * max(1, len(cols)))(*[t.data_ptr() for t in cols])
    n_failed = C.c_uint64(0)
    failed = np.full(cap, (1 << 64) - 1, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    check(lib().mi355_fr_copy_check_dev(arr, len(cols), log_n, cells.ctypes.data_as(u64p), images.ctypes.data_as(u64p), cells.size, cap, C.byref(n_failed),
                                        failed.ctypes.data_as(u64p) if cap else None))
    return int(n_failed.value), failed


def _key_buf(key: bytes):
    assert isinstance(key, (bytes, bytearray)) and len(key) == 32, "a ChaCha20 key is 32 bytes"
    return (C.c_uint8 * 32).from_buffer_copy(bytes(key))


def fr_random(dst, key: bytes, stream: int, counter0: int = 0, n: int | None = None):
    """uniform field elements drawn on the device (mi355_fr_random_dev): word i of the device tensor `dst` (n words; default: all of it) = from_u512 of the ChaCha20
    block (key, stream, counter0 + i).  A pure function of its arguments: the same words whatever the grid, the device, or how a vector is cut into calls.
    Asynchronous on the library stream.  A draw that would wrap the 64-bit block counter raises Mi355Error (EBADARG)."""
    if n is None:
        n = dst.numel() * dst.element_size() // 32
    assert n * 32 <= dst.numel() * dst.element_size(), "fr_random: more words than the tensor holds"
    check(lib().mi355_fr_random_dev(ptr(dst), n, _key_buf(key), stream, counter0))
    return dst


def fr_random_rows(cols, row0: int, rows: int, key: bytes, stream: int, counter0: int = 0):
    """rows [row0, row0 + rows) of every device tensor of `cols` in one launch (mi355_fr_random_rows_dev): column c, row row0 + j = element counter0 + c * rows + j
    of the stream.  The other rows are not touched (the blinding rows of a batch of witness columns)."""
    cols = list(cols)
    for t in cols:
        assert (row0 + rows) * 32 <= t.numel() * t.element_size(), "fr_random_rows: the rows leave a column"
    arr = (C.c_void_p * max(1, len(cols)))(*[t.data_ptr() for t in cols])
    check(lib().mi355_fr_random_rows_dev(arr, len(cols), row0, rows, _key_buf(key), stream, counter0))
    return cols


def fr_from_u512(src, dst=None):
    """halo2curves' Fr::from_uniform_bytes over an array on the device (mi355_fr_from_u512_dev): `src` is a device tensor of n 64-byte little-endian integers;
    returns (or fills `dst` with) their residues mod r as n Montgomery words [n, 4] int64."""
    n = src.numel() * src.element_size() // 64
    assert n * 64 == src.numel() * src.element_size(), "fr_from_u512: the input is not a whole number of 64-byte words"
    if dst is None:
        import torch
        dst = torch.empty((n, 4), dtype=torch.int64, device=src.device)
    assert dst.numel() * dst.element_size() == 32 * n, "fr_from_u512: the output is not n words"
    check(lib().mi355_fr_from_u512_dev(ptr(dst), ptr(src), n))
    return dst


# halo2curves bn256 G2 generator (x.c0, x.c1, y.c0, y.c1) [EXT-recalled src/bn256/curve.rs]; the same four words are the first pairing
# input of the released verifier [REF release-v0.13.1/evm_verifier.yul:1230-1233] (tests/test_oracle_golden.py)
G2_GENERATOR = (0x1800DEEF121F1E76426A00665E5C4479674322D4F75EDADD46DEBD5CD992F6ED, 0x198E9393920D483A7260BFB731FB5D25F1AA493335A9E71297E485B7AEF312C2,
                0x12C85EA5DB8C6DEB4AAB71808DCB408FE3D1E7690C43D37B4CE6CC0166FA7DAA, 0x090689D0585FF075EC9E99AD690C3395BC4B313370B38EF355ACDADCD122975B)


def fq(x: int) -> np.ndarray:
    v = (x % P_MOD) * (1 << 256) % P_MOD
    return np.array([(v >> (64 * i)) & _M64 for i in range(4)], dtype=np.uint64)


def g2_generator() -> np.ndarray:
    """G2Affine (16 u64: x.c0 | x.c1 | y.c0 | y.c1, Montgomery) of the generator: the `g2` field of every ParamsKZG."""
    return np.concatenate([fq(c) for c in G2_GENERATOR])


def g2_mul(point: np.ndarray, scalar: np.ndarray) -> np.ndarray:
    """scalar * point on the twist (mi355_g2_mul_host): ParamsKZG::setup's s_g2 = tau * G2."""
    out = np.zeros(16, dtype=np.uint64)
    check(lib().mi355_g2_mul_host(ptr(np.ascontiguousarray(point, dtype=np.uint64)), ptr(scalar), ptr(out)))
    return out


def g2_msm(bases: np.ndarray, scalars: np.ndarray) -> np.ndarray:
    """sum_i scalars[i] * bases[i] on the twist (mi355_msm_g2_adhoc_host): bases [n,16] u64 G2Affine, scalars [n,4] u64 Fr (Montgomery)
    -> normalised G2Affine (16 u64, identity = zeros).  Every base must lie on the twist (Mi355Error EBADARG names the first that does not)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 16)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    n = int(scalars.shape[0])
    assert n == int(bases.shape[0]), "g2_msm: scalars.len() != bases.len()"
    out = np.zeros(16, dtype=np.uint64)
    check(lib().mi355_msm_g2_adhoc_host(ptr(bases), ptr(scalars), n, ptr(out)))
    return out


def g2_msm_dev(bases, scalars, n: int) -> np.ndarray:
    """mi355_msm_g2_dev: bases (n x 128 B) and scalars (n x 32 B) in device memory (DeviceBuffer, torch tensor or address) -> G2Affine."""
    out = np.zeros(16, dtype=np.uint64)
    check(lib().mi355_msm_g2_dev(ptr(bases), ptr(scalars), n, ptr(out)))
    return out


def g2_msm_batch_dev(bases, scalars_list, n: int) -> np.ndarray:
    """mi355_msm_g2_batch_dev: len(scalars_list) scalar vectors over one device basis -> [batch, 16] u64."""
    m = len(scalars_list)
    arr = (C.c_void_p * max(m, 1))(*[ptr(s).value for s in scalars_list])
    out = np.zeros((max(m, 1), 16), dtype=np.uint64)
    check(lib().mi355_msm_g2_batch_dev(ptr(bases), arr, m, n, ptr(out)))
    return out[:m]


def pairing_products(P, Q, groups: int, pairs_per_group: int, want_gt: bool = True, want_is_one: bool = True):
    """mi355_pairing_products_host: out[g] = prod_j e(P[g * ppg + j], Q[g * ppg + j]) on the device.  P: [groups * ppg, 8] u64 G1Affine, Q: [groups * ppg, 16] u64
    G2Affine (Montgomery, identity = zeros: such a pair contributes 1) -> (gt [groups, 48] u64 in halo2curves' Fq12 layout, is_one [groups] u32: 1 where the product
    is 1, the answer of the EVM precompile at address 8).  want_gt / want_is_one = False leaves that output out (None in its place).  Every point must lie on its
    curve (Mi355Error EBADARG names the first pair that does not); Q is not checked for membership of the subgroup of order r."""
    n = int(groups) * int(pairs_per_group)
    P = np.ascontiguousarray(P, dtype=np.uint64).reshape(-1, 8)
    Q = np.ascontiguousarray(Q, dtype=np.uint64).reshape(-1, 16)
    assert P.shape[0] == n and Q.shape[0] == n, "pairing_products: groups * pairs_per_group points on each side"
    gt = np.zeros((groups, 48), dtype=np.uint64) if want_gt else None
    one = np.zeros(groups, dtype=np.uint32) if want_is_one else None
    check(lib().mi355_pairing_products_host(ptr(P), ptr(Q), groups, pairs_per_group, ptr(gt), None if one is None else one.ctypes.data_as(C.POINTER(C.c_uint32))))
    return gt, one


def verify_proof(protocol, instances, proof: bytes, transcript: str | None = None, vk_bytes: bytes | None = None, preprocessed=None, initial_state: int | None = None,
                 g2=None, s_g2=None, neg_s_g2=None, check_accumulator: bool = True, accumulator: bool | None = None, host_only: bool = False, timeout: int = 600) -> dict:
    """plonk::verify_proof (include/mi355zk_plonk_verify.hpp) through its compiled driver tests/cpp/test_verify_proof.cpp, run as a process the way replay.py runs the prover.
    protocol: a path to a PlonkProtocol JSON or the dict itself; instances: integers; key: vk_bytes (.vkey) | preprocessed ([n, 8] u64 G1Affine) | the protocol file's own;
    g2 + (s_g2 | neg_s_g2): 128-byte G2Affine values (bytes or 16 u64; default g2: the generator) -- s_g2 is negated on the host.  host_only=True stops after the
    (scalars, points) list and needs no device.  Returns the driver's record: ok, error (the name of the first failed check), challenges, numerator_at_x, msm {scalars,
    points, result, w_prime}, pairing (per-group flags); field elements and coordinates as integers."""
    import json, subprocess, tempfile
    from . import build
    exe = build.build_cpp("test_verify_proof")
    as_g2 = lambda q: q if isinstance(q, (bytes, bytearray)) else np.ascontiguousarray(q, dtype=np.uint64).tobytes()
    with tempfile.TemporaryDirectory(prefix="mi355_verify_") as d:
        def put(name, data):
            path = os.path.join(d, name)
            with open(path, "wb") as f:
                f.write(data)
            return path
        if isinstance(protocol, dict):
            path = os.path.join(d, "protocol.json")
            with open(path, "w") as f:
                json.dump(protocol, f, separators=(",", ":"))
            protocol = path
        args = [exe, "--protocol", protocol, "--proof", put("proof.bin", bytes(proof)), "--instances", put("instances.bin", b"".join(int(v).to_bytes(32, "big") for v in instances))]
        if transcript:
            args += ["--transcript", transcript]
        if vk_bytes is not None:
            args += ["--vk", put("vk.bin", bytes(vk_bytes))]
        if preprocessed is not None:
            args += ["--preprocessed", put("pre.bin", np.ascontiguousarray(preprocessed, dtype=np.uint64).tobytes())]
        if initial_state is not None:
            args += ["--initial-state", "%x" % initial_state]
        if not host_only:
            args += ["--g2", put("g2.bin", as_g2(g2 if g2 is not None else g2_generator()))]
            assert (s_g2 is None) != (neg_s_g2 is None), "verify_proof: give s_g2 or neg_s_g2"
            args += ["--s-g2", put("sg2.bin", as_g2(s_g2))] if s_g2 is not None else ["--neg-s-g2", put("nsg2.bin", as_g2(neg_s_g2))]
        if not check_accumulator:
            args.append("--no-accumulator")
        if accumulator:
            args.append("--accumulator")
        if host_only:
            args.append("--host-only")
        out = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
    if out.returncode != 0 or line is None:
        raise Mi355Error(_capi.EBADARG, "verify_proof driver failed: " + (out.stdout + out.stderr)[-800:])
    return _verify_record(json.loads(line))


def _verify_record(rec: dict) -> dict:
    """a driver's VerifyResult line: hexadecimal field elements and coordinates -> integers"""
    h = lambda s: int(s, 16)
    rec["challenges"] = {k: h(v) for k, v in rec["challenges"].items()}
    rec["numerator_at_x"] = h(rec["numerator_at_x"])
    m = rec["msm"]
    m["scalars"] = [h(v) for v in m["scalars"]]
    for key in ("result", "w_prime"):
        m[key] = (h(m[key][0]), h(m[key][1]))
    m["points"] = [(h(a), h(b)) for a, b in m["points"]]
    return rec


def _run_verify_proofs(cases, mode, g2, s_g2, neg_s_g2, host_only, need_srs, timeout, extra=(), driver="test_verify_proofs", raw=False):
    """tests/cpp/<driver> over a manifest written from `cases` -> (per-proof records, the closing summary line); raw: the records as the driver printed them"""
    import json, subprocess, tempfile
    from . import build
    exe = build.build_cpp(driver)
    as_g2 = lambda q: q if isinstance(q, (bytes, bytearray)) else np.ascontiguousarray(q, dtype=np.uint64).tobytes()
    with tempfile.TemporaryDirectory(prefix="mi355_verify_") as d:
        def put(name, data):
            path = os.path.join(d, name)
            with open(path, "wb") as f:
                f.write(data)
            return path
        man = {"proofs": []}
        protocols = {}
        for i, c in enumerate(cases):
            c = dict(c)
            protocol = c.pop("protocol")
            if isinstance(protocol, dict):                       # one file per distinct dict: the driver parses each protocol file once
                key = id(protocol)
                if key not in protocols:
                    protocols[key] = os.path.join(d, "protocol%d.json" % len(protocols))
                    with open(protocols[key], "w") as f:
                        json.dump(protocol, f, separators=(",", ":"))
                protocol = protocols[key]
            e = {"protocol": protocol, "proof": put("proof%d.bin" % i, bytes(c.pop("proof"))),
                 "instances": put("instances%d.bin" % i, b"".join(int(v).to_bytes(32, "big") for v in c.pop("instances")))}
            if c.get("transcript"):
                e["transcript"] = c["transcript"]
            if c.get("vk_bytes") is not None:
                e["vk"] = put("vk%d.bin" % i, bytes(c["vk_bytes"]))
            if c.get("preprocessed") is not None:
                e["preprocessed"] = put("pre%d.bin" % i, np.ascontiguousarray(c["preprocessed"], dtype=np.uint64).tobytes())
            if c.get("initial_state") is not None:
                e["initial_state"] = "%x" % c["initial_state"]
            if not c.get("check_accumulator", True):
                e["no_accumulator"] = True
            if c.get("accumulator"):
                e["accumulator"] = True
            unknown = set(c) - {"transcript", "vk_bytes", "preprocessed", "initial_state", "check_accumulator", "accumulator"}
            assert not unknown, "verify_proofs: unknown keys %s in case %d" % (sorted(unknown), i)
            man["proofs"].append(e)
        if need_srs:
            man["g2"] = put("g2.bin", as_g2(g2 if g2 is not None else g2_generator()))
            assert (s_g2 is None) != (neg_s_g2 is None), "give s_g2 or neg_s_g2"
            if s_g2 is not None:
                man["s_g2"] = put("sg2.bin", as_g2(s_g2))
            else:
                man["neg_s_g2"] = put("nsg2.bin", as_g2(neg_s_g2))
        path = os.path.join(d, "manifest.json")
        with open(path, "w") as f:
            json.dump(man, f)
        args = [exe, "--manifest", path] + list(mode) + (["--host-only"] if host_only else []) + list(extra)
        out = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        raise Mi355Error(_capi.EBADARG, "verify_proofs driver failed: " + (out.stdout + out.stderr)[-800:])
    return lines[:-1] if raw else [_verify_record(r) for r in lines[:-1]], lines[-1]


def verify_proofs(cases, g2=None, s_g2=None, neg_s_g2=None, host_only: bool = False, one_by_one: bool = False, timeout: int = 600, device_transcript: bool = False,
                  tile: int = 0, device_scalars: bool = False, host_only_at=()) -> list:
    """plonk::verify_proofs (include/mi355zk_plonk_verify.hpp) through its compiled driver tests/cpp/test_verify_proofs.cpp: N proofs, ONE point decompression, ONE segmented
    MSM, ONE pairing call.  cases: dictionaries with protocol (path or dict), instances, proof and verify_proof's per-proof keywords (transcript, vk_bytes, preprocessed,
    initial_state, check_accumulator, accumulator); protocols and transcripts may differ.  g2 / s_g2 / neg_s_g2 / host_only as in verify_proof.  Returns verify_proof's record
    per proof, each equal to what verify_proof gives for that proof alone; the last one carries "device_calls" (how many device calls the batch made).
    one_by_one=True runs the unchanged verify_proof in a loop inside the same process instead.  device_transcript=True (VerifyOptions::device_transcript, through
    tests/cpp/test_device_transcripts.cpp): the Poseidon transcripts of the batch are hashed by ONE mi355_poseidon_transcripts_host call -- one device call more, the same
    records; it needs the device, so it excludes host_only and one_by_one.  tile=N: the driver repeats the cases cyclically up to N proofs (--tile).
    device_scalars=True (VerifyOptions::device_scalars, through tests/cpp/test_device_scalars.cpp): the scalar sides of the batch run on the device, ONE mi355_fr_program_host
    call per distinct protocol -- that many device calls more, the same records; composes with device_transcript.  host_only_at: indices of proofs that get
    VerifyOptions::host_only inside that batch (they take the host path; their records say host_only)."""
    extra = ["--tile", str(int(tile))] if tile else []
    if device_scalars:
        assert not host_only and not one_by_one, "verify_proofs: device_scalars needs the device and the batched call"
        extra += (["--device-transcript"] if device_transcript else []) + (["--host-only-at", ",".join(str(int(i)) for i in host_only_at)] if len(host_only_at) else [])
        recs, summary = _run_verify_proofs(cases, [], g2, s_g2, neg_s_g2, False, True, timeout, extra=extra, driver="test_device_scalars")
    elif device_transcript:
        assert not host_only and not one_by_one, "verify_proofs: device_transcript needs the device and the batched call"
        recs, summary = _run_verify_proofs(cases, [], g2, s_g2, neg_s_g2, False, True, timeout, extra=extra, driver="test_device_transcripts")
    else:
        recs, summary = _run_verify_proofs(cases, ["--one-by-one"] if one_by_one else [], g2, s_g2, neg_s_g2, host_only, not host_only, timeout, extra=extra)
    assert len(recs) == (tile or len(cases))
    for r in recs:
        r["device_calls"] = summary["device_calls"]
    return recs


def aggregate(cases, g2=None, s_g2=None, neg_s_g2=None, pairing: bool = True, host_only: bool = False, timeout: int = 600, device_transcript: bool = False,
              device_scalars: bool = False) -> dict:
    """plonk::aggregate through the same driver (--aggregate): the KZG accumulators of the proofs -- (msm_result, W') of each, its carried accumulator after it -- folded with the
    powers of a Poseidon transcript challenge into the accumulator the next layer's first twelve instances carry.  Returns ok, error, detail, proofs (records), accumulators
    [((x, y), (x, y)), ...], r, lhs, rhs, limbs (12 integers below 2^88), pairing, device_calls.  pairing=False: fold only, no SRS.  host_only=True: no device; the lists'
    sums come from the oracle and the result stops after r (lhs, rhs and limbs are zero).  device_transcript=True: the proofs' Poseidon transcripts are hashed on the device
    (as in verify_proofs; the aggregation's own transcript, one sponge, stays on the host).  device_scalars=True: the proofs' scalar sides run on the device (as in
    verify_proofs: one more device call per distinct protocol)."""
    assert not ((device_transcript or device_scalars) and host_only), "aggregate: device_transcript and device_scalars need the device"
    extra = ([] if pairing or host_only else ["--no-pairing"]) + (["--device-transcript"] if device_scalars and device_transcript else [])
    recs, a = _run_verify_proofs(cases, ["--aggregate"], g2, s_g2, neg_s_g2, host_only, pairing and not host_only, timeout, extra=extra,
                                 driver="test_device_scalars" if device_scalars else "test_device_transcripts" if device_transcript else "test_verify_proofs")
    h = lambda s: int(s, 16)
    pt = lambda p: (h(p[0]), h(p[1]))
    a["proofs"] = recs
    a["accumulators"] = [(pt(l), pt(r)) for l, r in a["accumulators"]]
    a["r"] = h(a["r"]); a["lhs"] = pt(a["lhs"]); a["rhs"] = pt(a["rhs"]); a["limbs"] = [h(v) for v in a["limbs"]]
    return a


def record_transcripts(cases, timeout: int = 600) -> list:
    """the recording pass of VerifyOptions::device_transcript alone (tests/cpp/test_device_transcripts --host-only; no device): per proof {"job", "error", "detail", "words",
    "squeeze_at", "challenges"} -- the words its Poseidon transcript absorbs (integers), the word count at each squeeze and, from the host sponge, the challenges.
    job is False, and the lists empty, for a proof that records none: another transcript (error ""), or a named failure of the transcript section (error = its name)."""
    recs, summary = _run_verify_proofs(cases, [], None, None, None, True, False, timeout, driver="test_device_transcripts", raw=True)
    assert len(recs) == len(cases) and summary["jobs"] == sum(r["job"] for r in recs)
    for r in recs:
        r["words"] = [int(v, 16) for v in r["words"]]; r["challenges"] = [int(v, 16) for v in r["challenges"]]
    return recs


def scalar_programs(cases, timeout: int = 600) -> list:
    """what VerifyOptions::device_scalars compiles for the cases (tests/cpp/test_device_scalars --program-info; no device): per distinct (protocol, number of instances) one
    dictionary with layer, k, instances, usable, instructions, registers, constants, inputs, outputs, inversions."""
    recs, summary = _run_verify_proofs(cases, ["--program-info"], None, None, None, False, False, timeout, driver="test_device_scalars", raw=True)
    assert summary["programs"] == len(recs)
    return recs


def fr_program(code, n_regs: int, consts, inputs, out_regs):
    """mi355_fr_program_host: ONE straight-line program over Fr for MANY jobs in one launch, a lane per job.  code [n, 4] u32 (op, dst, a, b): 0 ADD, 1 SUB, 2 MUL, 3 SQRN
    (dst = a^(2^b), b an immediate <= 64), 4 INV (zero gives zero and sets bit 0 of the job's flag word), 5 NZ (sets flag bit b in 1 .. 31 when a == 0).  Registers
    [0, len(consts)) hold consts [c, 4] u64, the next n_inputs the job's row of inputs [jobs, n_inputs, 4] u64 (Fr, Montgomery, below r), the rest are temporaries.
    -> (outputs [jobs, len(out_regs), 4] u64, flags [jobs] u32)."""
    code = np.ascontiguousarray(code, dtype=np.uint32).reshape(-1, 4)
    consts = np.ascontiguousarray(consts, dtype=np.uint64).reshape(-1, 4)
    inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
    assert inputs.ndim == 3 and inputs.shape[2] == 4, "fr_program: inputs is [jobs, n_inputs, 4]"
    out_regs = np.ascontiguousarray(out_regs, dtype=np.uint32).reshape(-1)
    jobs, n_inputs = inputs.shape[0], inputs.shape[1]
    out = np.zeros((jobs, out_regs.shape[0], 4), dtype=np.uint64)
    flags = np.zeros(jobs, dtype=np.uint32)
    check(lib().mi355_fr_program_host(ptr(code), code.shape[0], n_regs, ptr(consts), consts.shape[0], ptr(inputs), n_inputs, jobs, ptr(out_regs), out_regs.shape[0], ptr(out), ptr(flags)))
    return out, flags


def msm_g1_segmented(bases, scalars, offsets) -> np.ndarray:
    """mi355_msm_g1_segmented_host: out[s] = sum over [offsets[s], offsets[s + 1]) of scalars[i] * bases[i] -- MANY SHORT multi-scalar multiplications in one launch (a wavefront
    per segment; the final MSMs of a batch of verifiers).  bases [n, 8] u64 G1Affine, scalars [n, 4] u64 Fr (Montgomery), offsets [segments + 1] (first 0, non-decreasing, last n)
    -> [segments, 8] u64 G1Affine, identity = zeros.  A long segment is correct and slow: best_multiexp is the tool for those."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    assert offsets.shape[0] >= 1, "msm_g1_segmented: offsets holds segments + 1 values"
    bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    assert bases.shape[0] == scalars.shape[0] == int(offsets[-1]), "msm_g1_segmented: offsets[-1] != scalars.len() or bases.len()"
    segments = offsets.shape[0] - 1
    out = np.zeros((segments, 8), dtype=np.uint64)
    check(lib().mi355_msm_g1_segmented_host(ptr(bases), ptr(scalars), ptr(offsets), segments, ptr(out)))
    return out


def poseidon_transcripts(words, word_offsets, squeeze_at, squeeze_offsets) -> np.ndarray:
    """mi355_poseidon_transcripts_host: MANY Poseidon sponges (T = 5, RATE = 4, R_F = 8, R_P = 60: the transcript of snark-verifier's native loader) in one launch, a lane per
    job.  words [n, 4] u64 Fr (Montgomery, below r); job j hashes words[word_offsets[j]:word_offsets[j + 1]] and squeezes at the positions
    squeeze_at[squeeze_offsets[j]:squeeze_offsets[j + 1]] (non-decreasing, relative to the job's first word, at most its length) -> [squeezes, 4] u64 challenges in the order of
    squeeze_at.  Challenge k of a job = Sponge.squeeze() after update(the words up to squeeze_at[k] not yet absorbed)."""
    word_offsets = np.ascontiguousarray(word_offsets, dtype=np.uint64).reshape(-1)
    squeeze_offsets = np.ascontiguousarray(squeeze_offsets, dtype=np.uint64).reshape(-1)
    squeeze_at = np.ascontiguousarray(squeeze_at, dtype=np.uint32).reshape(-1)
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    assert word_offsets.shape[0] >= 1 and word_offsets.shape == squeeze_offsets.shape, "poseidon_transcripts: both offset arrays hold jobs + 1 values"
    assert int(word_offsets[-1]) == words.shape[0] and int(squeeze_offsets[-1]) == squeeze_at.shape[0], "poseidon_transcripts: the offsets must end at len(words) and len(squeeze_at)"
    out = np.zeros((squeeze_at.shape[0], 4), dtype=np.uint64)
    check(lib().mi355_poseidon_transcripts_host(ptr(words), ptr(word_offsets), ptr(squeeze_at), ptr(squeeze_offsets), word_offsets.shape[0] - 1, ptr(out)))
    return out


def g1_sum(points: np.ndarray) -> np.ndarray:
    """fold of per-GPU partial results: results.iter().fold(identity, |a, b| a + b)."""
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(12, dtype=np.uint64)
    check(lib().mi355_g1_sum_host(ptr(points), points.shape[0], ptr(out)))
    return out


def batch_normalize(points, out=None):
    """group::Curve::batch_normalize: n Jacobian G1 (any representative, [n,12] u64) -> n affine points ([n,8] u64, identity = (0, 0)).
    Host arrays go through mi355_g1_batch_normalize_host; device tensors (96 n bytes in, 64 n bytes out, `out` required) stay in HBM."""
    if _is_device(points):
        n = points.numel() * points.element_size() // 96
        assert out is not None and out.numel() * out.element_size() == 64 * n, "batch_normalize: device output tensor of 64 n bytes required"
        check(lib().mi355_g1_batch_normalize_dev(ptr(points), ptr(out), n))
        return out
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    res = np.zeros((points.shape[0], 8), dtype=np.uint64)
    check(lib().mi355_g1_batch_normalize_host(ptr(points), ptr(res), points.shape[0]))
    return res


# ------------------------------------------------------------------------------------------ poly/domain.rs
class EvaluationDomain:
    """EvaluationDomain::new(j, k): n = 2^k, quotient_poly_degree = j - 1, extended_k minimal with 2^extended_k >= n * (j - 1)."""

    def __init__(self, j: int, k: int):
        self.k, self.n = k, 1 << k
        self.quotient_poly_degree = j - 1
        ext = k
        while (1 << ext) < self.n * self.quotient_poly_degree:
            ext += 1
        assert ext <= FR_S, "extended_k exceeds the two-adicity of Fr"
        self.extended_k = ext
        ew = pow(FR_ROOT_OF_UNITY, 1 << (FR_S - ext), R_MOD)
        w = pow(ew, 1 << (ext - k), R_MOD)
        self._omega, self._extended_omega = w, ew
        self.omega, self.omega_inv = fr(w), fr(pow(w, -1, R_MOD))
        self.extended_omega, self.extended_omega_inv = fr(ew), fr(pow(ew, -1, R_MOD))
        self.g_coset, self.g_coset_inv = fr(FR_ZETA), fr(FR_ZETA * FR_ZETA % R_MOD)
        # t_evaluations: (zeta * extended_omega^i)^n - 1 for i < 2^(extended_k - k) (it is periodic), stored inverted as halo2 does
        q = 1 << (ext - k)
        self.t_evaluations_inv = np.stack([fr(pow((pow(FR_ZETA, self.n, R_MOD) * pow(ew, i * self.n, R_MOD) - 1) % R_MOD, -1, R_MOD)) for i in range(q)])
        self.ifft_divisor = fr(pow(self.n, -1, R_MOD))
        self.extended_ifft_divisor = fr(pow(1 << ext, -1, R_MOD))

    def extended_len(self) -> int:
        return 1 << self.extended_k

    def coeff_to_lagrange(self, a):
        best_fft(a, self.omega, self.k)
        return a

    def lagrange_to_coeff(self, a):
        """ifft: best_fft(a, omega_inv, k) then a[i] *= n^-1."""
        if _is_device(a):
            check(lib().mi355_intt_fr_dev(ptr(a), self.k, ptr(self.omega_inv), ptr(self.ifft_divisor)))
        else:
            check(lib().mi355_intt_fr_host(ptr(a), self.k, ptr(self.omega_inv), ptr(self.ifft_divisor)))
        return a

    def coeff_to_extended(self, a, out=None):
        """zero-pad to the extended domain, move into the coset g_coset * H, transform.  Returns a new array (host) or fills `out` (device)."""
        if _is_device(a):
            assert out is not None and _is_device(out)
            check(lib().mi355_coeff_to_extended_dev(ptr(out), ptr(a), self.k, self.extended_k, ptr(self.g_coset), ptr(self.g_coset_inv), ptr(self.extended_omega)))
            return out
        dst = np.zeros((self.extended_len(), 4), dtype=np.uint64)
        check(lib().mi355_coeff_to_extended_host(ptr(dst), ptr(np.ascontiguousarray(a)), self.k, self.extended_k, ptr(self.g_coset), ptr(self.g_coset_inv), ptr(self.extended_omega)))
        return dst

    def coeff_to_extended_part(self, a, part: int, out):
        """scroll-fork style: evaluations of the 2^k coefficients on the coset (g_coset * extended_omega^part) * H  (device tensors)."""
        assert _is_device(a) and _is_device(out)
        factor = fr(FR_ZETA * pow(self._extended_omega, part, R_MOD) % R_MOD)
        check(lib().mi355_coset_ntt_fr_dev(ptr(out), ptr(a), self.k, ptr(factor), ptr(self.omega)))
        return out

    def divide_by_vanishing_poly(self, a):
        """EvaluationDomain::divide_by_vanishing_poly on extended-coset evaluations (device tensor, in place): a[i] *= t_evaluations[i % len]^-1."""
        assert _is_device(a)
        n = a.numel() * a.element_size() // 32
        check(lib().mi355_fr_vec_mul_periodic_dev(ptr(a), n, ptr(self.t_evaluations_inv), self.t_evaluations_inv.shape[0]))
        return a

    def extended_to_coeff(self, a):
        """inverse of coeff_to_extended, truncated to n * quotient_poly_degree coefficients (host) / in place (device, caller truncates)."""
        if _is_device(a):
            check(lib().mi355_extended_to_coeff_dev(ptr(a), self.extended_k, ptr(self.g_coset), ptr(self.g_coset_inv), ptr(self.extended_omega_inv), ptr(self.extended_ifft_divisor)))
            return a
        a = np.array(a, dtype=np.uint64, copy=True, order="C")
        check(lib().mi355_extended_to_coeff_host(ptr(a), self.extended_k, ptr(self.g_coset), ptr(self.g_coset_inv), ptr(self.extended_omega_inv), ptr(self.extended_ifft_divisor)))
        return a[: self.n * self.quotient_poly_degree]


# ------------------------------------------------------------------------------------------ poly/kzg/commitment.rs
class SrsSlice:
    """&params.g[..n] / &params.g_lagrange[..n]: a registered, HBM-resident basis plus (offset, n)."""

    def __init__(self, handle: int, offset: int, n: int):
        self.handle, self.offset, self.n = handle, offset, n


class ParamsKZG:
    """ParamsKZG<Bn256> { k, n, g, g_lagrange } with both bases resident in HBM for the life of the object
    (the reference keeps them in the process-wide params_map [REF bin/src/trace_prover.rs:35-43])."""

    def __init__(self, k: int, g_handle: int, gl_handle: int, owner=None):
        self.k, self.n = k, 1 << k
        self._g, self._gl, self._owner = g_handle, gl_handle, owner
        self.g2, self.s_g2 = bytes(128), bytes(128)   # G2Affine bytes as in the params file; setup() / params_from_file() fill them

    @classmethod
    def from_host(cls, k: int, g: np.ndarray, g_lagrange: np.ndarray) -> "ParamsKZG":
        """what `Prover::load_params_map` hands down, registered once."""
        hs = []
        for arr in (g, g_lagrange):
            arr = np.ascontiguousarray(arr, dtype=np.uint64)
            assert arr.shape == (1 << k, 8)
            h = C.c_uint64()
            check(lib().mi355_srs_register_host(ptr(arr), 1 << k, C.byref(h)))
            hs.append(h.value)
        return cls(k, hs[0], hs[1])

    @classmethod
    def setup(cls, k: int, tau: int) -> "ParamsKZG":
        """ParamsKZG::setup(k, rng) with the toxic scalar given explicitly: g[i] = tau^i G, g_lagrange[i] = L_i(tau) G, built on the device."""
        import torch
        n = 1 << k
        g = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        gl = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
        w = pow(FR_ROOT_OF_UNITY, 1 << (FR_S - k), R_MOD)
        check(lib().mi355_srs_setup_dev(ptr(g), ptr(gl), k, ptr(fr(tau)), ptr(fr(w))))
        hs = []
        for t in (g, gl):
            h = C.c_uint64()
            check(lib().mi355_srs_register_dev(ptr(t), n, 0, C.byref(h)))
            hs.append(h.value)
        p = cls(k, hs[0], hs[1], owner=(g, gl))
        p.g2 = g2_generator().tobytes()                               # g2 = G2 generator, s_g2 = tau * g2 [EXT-recalled ParamsKZG::setup]
        p.s_g2 = g2_mul(g2_generator(), fr(tau)).tobytes()
        return p

    def clone_downsized(self, k: int) -> "ParamsKZG":
        """`let mut p = params.clone(); p.downsize(k)` of load_params_map [REF integration/tests/integration.rs:12-22]: the clone's g is a
        PREFIX VIEW of this object's registration (mi355_srs_register_prefix: same device memory, same window tables), its g_lagrange is
        rebuilt on the device.  Either object may be released first."""
        assert k <= self.k
        h = C.c_uint64()
        check(lib().mi355_srs_register_prefix(self._g, 1 << k, C.byref(h)))
        w_inv = pow(pow(FR_ROOT_OF_UNITY, 1 << (FR_S - k), R_MOD), R_MOD - 2, R_MOD)
        hl = C.c_uint64()
        check(lib().mi355_srs_downsize(h.value, k, ptr(fr(w_inv)), ptr(fr(pow(1 << k, R_MOD - 2, R_MOD))), C.byref(hl)))
        p = ParamsKZG(k, h.value, hl.value, owner=self._owner)
        p.g2, p.s_g2 = getattr(self, "g2", bytes(128)), getattr(self, "s_g2", bytes(128))
        return p

    def commit(self, poly_coeff) -> np.ndarray:
        """commit(&self, poly: &Polynomial<_, Coeff>, _: Blind) = best_multiexp(poly, &self.g[..poly.len()])"""
        n = poly_coeff.shape[0] if not _is_device(poly_coeff) else poly_coeff.numel() * poly_coeff.element_size() // 32
        return best_multiexp(_as_scalars(poly_coeff, n), SrsSlice(self._g, 0, n))

    def commit_lagrange(self, poly_lagrange) -> np.ndarray:
        """commit_lagrange = best_multiexp(poly, &self.g_lagrange[..poly.len()])"""
        n = poly_lagrange.shape[0] if not _is_device(poly_lagrange) else poly_lagrange.numel() * poly_lagrange.element_size() // 32
        assert n == self.n, "commit_lagrange: polynomial must have exactly n evaluations"
        return best_multiexp(_as_scalars(poly_lagrange, n), SrsSlice(self._gl, 0, n))

    def precompute(self, n_hint: int = 0, c: int = 0, lagrange: bool = True, coeff: bool = True) -> None:
        """registration-time window tables 2^(c w) * P for the two bases (mi355_srs_precompute): W x the HBM, fewer windows, no Horner tail."""
        if coeff:
            check(lib().mi355_srs_precompute(self._g, n_hint, c))
        if lagrange:
            check(lib().mi355_srs_precompute(self._gl, n_hint, c))

    def commit_many(self, polys, lagrange: bool = False) -> np.ndarray:
        """commit / commit_lagrange for a list of polynomials of equal length (all device tensors or all host arrays) in ONE pass
        (mi355_msm_g1_batch_dev / _host): [M, 12].  create_proof commits the advice columns of a phase one after the other
        [EXT halo2_proofs src/plonk/prover.rs, SURVEY 3.2 step 2]; this is that loop as one call."""
        out = np.zeros((len(polys), 12), dtype=np.uint64)
        if len(polys) == 0:
            return out
        dev = _is_device(polys[0])
        assert all(_is_device(p) == dev for p in polys), "commit_many: mix of host and device polynomials"
        if dev:
            n = polys[0].numel() * polys[0].element_size() // 32
            assert all(p.numel() * p.element_size() // 32 == n for p in polys), "commit_many: polynomials must have equal length"
            arr = (C.c_void_p * len(polys))(*[p.data_ptr() for p in polys])
            fn = lib().mi355_msm_g1_batch_dev
        else:
            polys = [np.ascontiguousarray(p, dtype=np.uint64) for p in polys]
            n = polys[0].shape[0]
            assert all(p.shape == (n, 4) for p in polys), "commit_many: polynomials must have equal length"
            arr = (C.c_void_p * len(polys))(*[p.ctypes.data for p in polys])
            fn = lib().mi355_msm_g1_batch_host
        assert n <= self.n and (not lagrange or n == self.n)
        check(fn(self._gl if lagrange else self._g, 0, arr, len(polys), n, ptr(out)))
        return out

    def downsize(self, k: int) -> None:
        """ParamsKZG::downsize(k) [REF integration/tests/integration.rs:17-22]: keep g[..2^k], rebuild g_lagrange = g_to_lagrange(g, k)
        (a size-2^k inverse DFT over G1 points, on the device).  The coefficient basis keeps its registration (and window tables)."""
        assert k <= self.k, "downsize: k must not exceed the current degree"
        if k == self.k:
            return
        w_inv = pow(pow(FR_ROOT_OF_UNITY, 1 << (FR_S - k), R_MOD), R_MOD - 2, R_MOD)
        h = C.c_uint64()
        check(lib().mi355_srs_downsize(self._g, k, ptr(fr(w_inv)), ptr(fr(pow(1 << k, R_MOD - 2, R_MOD))), C.byref(h)))
        check(lib().mi355_srs_release(self._gl))
        self._gl = h.value
        self.k, self.n = k, 1 << k

    def check_g2(self) -> bool:
        """e(g[0], s_g2) * e(-g[1], g2) == 1: the file's (or setup's) s_g2 is [tau] g2 for the tau of the G1 basis, with G2 ordered and signed as the pairing
        reads it.  One pairing call over two points read back from the device; nothing calls it by default."""
        assert self.n >= 2, "check_g2 needs g[0] and g[1]"
        g01 = np.zeros((2, 8), dtype=np.uint64)
        check(lib().mi355_srs_read_host(self._g, 0, 2, ptr(g01)))
        y = sum(int(v) << (64 * i) for i, v in enumerate(g01[1, 4:]))
        if g01[1].any():
            y = (P_MOD - y) % P_MOD
            g01[1, 4:] = [(y >> (64 * i)) & _M64 for i in range(4)]
        Q = np.stack([np.frombuffer(self.s_g2, dtype=np.uint64), np.frombuffer(self.g2, dtype=np.uint64)])
        _, one = pairing_products(g01, Q, 1, 2, want_gt=False)
        return bool(one[0])

    def read_g(self, lagrange: bool = False) -> np.ndarray:
        """the first n points of g (or g_lagrange) back on the host: [n, 8] (what ParamsKZG::write serialises)."""
        out = np.zeros((self.n, 8), dtype=np.uint64)
        check(lib().mi355_srs_read_host(self._gl if lagrange else self._g, 0, self.n, ptr(out)))
        return out

    def g_slice(self, offset: int, n: int) -> SrsSlice:
        return SrsSlice(self._g, offset, n)

    def g_lagrange_slice(self, offset: int, n: int) -> SrsSlice:
        return SrsSlice(self._gl, offset, n)

    def write(self, path: str, format: str = "raw") -> None:
        """ParamsKZG::write (SerdeFormat::RawBytes): a file prover::load_params / params_from_file accepts.  format="processed" is
        ParamsKZG::write_custom(.., SerdeFormat::Processed): both bases are compressed on the device (mi355_srs_dev_ptr + mi355_g1_compress_dev, shard by
        shard when the basis is spread over several devices) and only the 32-byte words cross to the host; g2 / s_g2 are compressed on the host."""
        if format == "raw":
            write_params(path, self.k, self.read_g(), self.read_g(lagrange=True), self.g2, self.s_g2)
            return
        assert format == "processed", "format must be 'raw' or 'processed'"
        with open(path, "wb") as f:
            f.write(int(self.k).to_bytes(4, "little"))
            for h in (self._g, self._gl):
                f.write(_srs_compressed(h, self.n).tobytes())
            f.write(g2_to_bytes(self.g2)); f.write(g2_to_bytes(self.s_g2))

    def release(self) -> None:
        for h in (self._g, self._gl):
            check(lib().mi355_srs_release(h))
        self._owner = None


# ------------------------------------------------------------------------------------------ wire codec of G1 (proof / .vkey bytes)
def g1_to_bytes(g1) -> bytes:
    """compressed encoding written to transcripts and .vkey files [EXT-recalled halo2curves derive/curve.rs; pinned by fixture KAT A4]:
    32 bytes little-endian x, bit 254 = parity of canonical y, identity = 32 zero bytes.  Accepts G1Affine (8 limbs) or a normalised
    G1 (12 limbs) as returned by best_multiexp.  Host-side (the transcript lives on the host, as in the reference)."""
    v = [int(t) for t in g1]
    if len(v) == 12:
        assert v[8:] == [0, 0, 0, 0] or sum(l << (64 * i) for i, l in enumerate(v[8:])) == (1 << 256) % P_MOD, "normalise first"
        if v[8:] == [0, 0, 0, 0]:
            return bytes(32)
    rinv = pow(1 << 256, -1, P_MOD)
    x = sum(l << (64 * i) for i, l in enumerate(v[0:4])) * rinv % P_MOD
    y = sum(l << (64 * i) for i, l in enumerate(v[4:8])) * rinv % P_MOD
    if x == 0 and y == 0:
        return bytes(32)
    return (x | ((y & 1) << 254)).to_bytes(32, "little")


def g1_from_bytes(b: bytes) -> np.ndarray:
    """inverse of g1_to_bytes -> G1Affine limbs (Montgomery); raises ValueError for x not on the curve (y^2 = x^3 + 3, p = 3 mod 4)."""
    v = int.from_bytes(b, "little")
    sign, x = (v >> 254) & 1, v & ((1 << 254) - 1)
    if x == 0 and sign == 0:
        return np.zeros(8, dtype=np.uint64)
    if x >= P_MOD:
        raise ValueError("x out of range")
    y2 = (x * x * x + 3) % P_MOD
    y = pow(y2, (P_MOD + 1) // 4, P_MOD)
    if y * y % P_MOD != y2:
        raise ValueError("not on the curve")
    if (y & 1) != sign:
        y = P_MOD - y
    m = lambda t: [((t << 256) % P_MOD >> (64 * i)) & _M64 for i in range(4)]
    return np.array(m(x) + m(y), dtype=np.uint64)


def g1_decompress(words) -> np.ndarray:
    """G1Affine::from_bytes over an array, on the device (mi355_g1_decompress_host / _dev): words = [n, 32] uint8 (or n * 32 bytes) on the host -> [n, 8] uint64
    points; a device tensor of n * 32 bytes -> a device tensor of n * 64 bytes.  Raises Mi355Error (EBADARG, `.index` = the smallest rejected index) for a word
    that is no curve point."""
    bad = C.c_uint64()
    if _is_device(words):
        import torch
        n = words.numel() * words.element_size() // 32
        out = torch.empty(n * 64, dtype=torch.uint8, device=words.device)
        rc = lib().mi355_g1_decompress_dev(ptr(words), ptr(out), n, C.byref(bad))
    else:
        w = np.ascontiguousarray(np.frombuffer(words, dtype=np.uint8) if isinstance(words, (bytes, bytearray)) else words, dtype=np.uint8).reshape(-1, 32)
        n = w.shape[0]
        out = np.zeros((n, 8), dtype=np.uint64)
        rc = lib().mi355_g1_decompress_host(ptr(w), ptr(out), n, C.byref(bad))
    if rc != _capi.OK:
        e = Mi355Error(rc, lib().mi355_last_error().decode())
        e.index = bad.value if bad.value != (1 << 64) - 1 else None
        raise e
    return out


def g1_compress(points):
    """G1Affine::to_bytes over an array, on the device: [n, 8] uint64 host points -> [n, 32] uint8 words; a device tensor of n * 64 bytes -> a device tensor of
    n * 32 bytes (queued on the library stream)."""
    if _is_device(points):
        import torch
        n = points.numel() * points.element_size() // 64
        out = torch.empty(n * 32, dtype=torch.uint8, device=points.device)
        check(lib().mi355_g1_compress_dev(ptr(points), ptr(out), n))
        return out
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((p.shape[0], 32), dtype=np.uint8)
    check(lib().mi355_g1_compress_host(ptr(p), ptr(out), p.shape[0]))
    return out


def _srs_compressed(handle: int, n: int) -> np.ndarray:
    """the first n points of a registered basis as [n, 32] compressed words: compressed on the device that holds them; only the words are downloaded.  A basis
    sharded over several devices exposes its primary shard through mi355_srs_dev_ptr only: the other shards go through mi355_srs_read_host + the host form."""
    dp = C.c_void_p()
    check(lib().mi355_srs_dev_ptr(handle, C.byref(dp)))
    out = np.zeros((n, 32), dtype=np.uint8)
    if _single_device():
        chunk = min(n, 1 << 24)
        buf = DeviceBuffer(chunk * 32)
        try:
            for lo in range(0, n, chunk):
                m = min(chunk, n - lo)
                check(lib().mi355_g1_compress_dev(C.c_void_p(dp.value + lo * 64), C.c_void_p(buf.data_ptr()), m))
                check(lib().mi355_buf_download(ptr(out[lo:lo + m]), C.c_void_p(buf.data_ptr()), m * 32))
        finally:
            buf.free()
        return out
    chunk = min(n, 1 << 22)
    pts = np.zeros((chunk, 8), dtype=np.uint64)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        check(lib().mi355_srs_read_host(handle, lo, m, ptr(pts)))
        check(lib().mi355_g1_compress_host(ptr(pts), ptr(out[lo:lo + m]), m))
    return out


def _single_device() -> bool:
    """whether a registered basis sits whole on the primary device (one bound device): slot 1 does not exist then"""
    return lib().mi355_mem_info(1, None, None, None, None, None) != _capi.OK


def g2_to_bytes(g2affine: bytes) -> bytes:
    """the 64-byte compressed form of a G2Affine (128 B, Montgomery) in a SerdeFormat::Processed params file: x.c0 then x.c1 as canonical little-endian words,
    bit 6 of byte 63 = parity of canonical y.c0, identity = 64 zero bytes [EXT-recalled halo2curves; no fixture of the reference pins this layout]."""
    assert len(g2affine) == 128
    if not any(g2affine):
        return bytes(64)
    rinv = pow(1 << 256, -1, P_MOD)
    c = [int.from_bytes(g2affine[32 * i:32 * i + 32], "little") * rinv % P_MOD for i in range(3)]
    out = bytearray(c[0].to_bytes(32, "little") + c[1].to_bytes(32, "little"))
    out[63] |= (c[2] & 1) << 6
    return bytes(out)


# ------------------------------------------------------------------------------------------ params files (SerdeFormat::RawBytes / Processed)
def params_file_size(k: int, format: str = "raw") -> int:
    """`u32 LE k | g[2^k] x 64 B | g_lagrange[2^k] x 64 B | g2 128 B | s_g2 128 B` [EXT-recalled ParamsKZG::write_custom, RawBytes];
    params26 = 8 589 934 852 bytes.  `prover::load_params` rejects any other length.  format="processed": 32-byte G1 words and 64-byte G2 words."""
    assert format in ("raw", "processed")
    return 4 + 2 * (1 << k) * 64 + 256 if format == "raw" else 4 + 2 * (1 << k) * 32 + 128


def write_params(path: str, k: int, g: np.ndarray, g_lagrange: np.ndarray, g2: bytes = bytes(128), s_g2: bytes = bytes(128)) -> None:
    g = np.ascontiguousarray(g, dtype=np.uint64); g_lagrange = np.ascontiguousarray(g_lagrange, dtype=np.uint64)
    assert g.shape == (1 << k, 8) and g_lagrange.shape == (1 << k, 8) and len(g2) == 128 and len(s_g2) == 128
    with open(path, "wb") as f:
        f.write(int(k).to_bytes(4, "little")); f.write(g.tobytes()); f.write(g_lagrange.tobytes()); f.write(g2); f.write(s_g2)


def read_params(path: str):
    """-> (k, g [n,8], g_lagrange [n,8], g2 bytes, s_g2 bytes); memory-mapped so a params26 file is not copied twice."""
    import os
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        k = int.from_bytes(f.read(4), "little")
    if not (0 < k <= FR_S) or size != params_file_size(k):
        raise ValueError(f"{path}: not a RawBytes params file (k={k}, {size} bytes, expected {params_file_size(k) if 0 < k <= FR_S else 'n/a'})")
    n = 1 << k
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    g = mm[4: 4 + n * 64].view(np.uint64).reshape(n, 8)
    gl = mm[4 + n * 64: 4 + 2 * n * 64].view(np.uint64).reshape(n, 8)
    tail = bytes(mm[4 + 2 * n * 64:])
    return k, g, gl, tail[:128], tail[128:]


def params_from_file(path: str, validate: bool = False, downsize_to: int = 0, format: str = "raw") -> "ParamsKZG":
    """Prover::load_params(dir, degree) [REF bin/src/trace_prover.rs:35-36] for one degree: the file is streamed into HBM by the library
    (mi355_srs_load_params_file: pinned double-buffered reads, exact-length rule, optional on-device point validation) and both bases
    are registered; downsize_to < k reproduces load_params on a larger file (g truncated, g_lagrange rebuilt on the device).
    format="processed": the file is SerdeFormat::Processed (32-byte compressed points, decompressed on the device while the next chunk is copied)."""
    assert format in ("raw", "processed"), "format must be 'raw' or 'processed'"
    k, hg, hl = C.c_uint32(), C.c_uint64(), C.c_uint64()
    g2 = (C.c_uint8 * 128)(); s_g2 = (C.c_uint8 * 128)()
    flags = (1 if validate else 0) | (2 if format == "processed" else 0)
    check(lib().mi355_srs_load_params_file(path.encode(), flags, C.byref(k), C.byref(hg), C.byref(hl), g2, s_g2))
    p = ParamsKZG(k.value, hg.value, hl.value)
    p.g2, p.s_g2 = bytes(g2), bytes(s_g2)
    if downsize_to and downsize_to < p.k:
        p.downsize(downsize_to)
    return p


class _Scalars:
    """adapter giving device tensors the `.shape[0]` best_multiexp expects"""

    def __init__(self, t, n):
        self._t, self.shape = t, (n,)
        self.is_cuda = True

    def data_ptr(self):
        return self._t.data_ptr()


def _as_scalars(x, n):
    return _Scalars(x, n) if _is_device(x) else np.ascontiguousarray(x, dtype=np.uint64)
