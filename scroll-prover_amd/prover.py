"""
prover.py -- the prover and the verifier IN PROCESS: plonk::keygen / create_proof / check_witness / verify_proofs / aggregate through the mi355_plonk_* entry points of
libmi355zk.so (include/mi355zk.h; csrc/lib_plonk.cpp), over ctypes.  replay.py and halo2.verify_proof(s) / halo2.aggregate run the same C++ as child processes of compiled
test programs; here a proving key stays resident between proofs and a call pays neither process start nor mi355_init, SRS set-up and keygen.

    pr = Protocol.from_json(protocols.layer_protocol(2, 7))        # or .from_file(path)
    c = Circuit.synthetic(pr, seed=1)                               # or Circuit(pr) + c.set("advice", i, column) ...
    params = halo2.ParamsKZG.setup(pr.info("k"), tau)               # the SRS handles are halo2.ParamsKZG's: same library, same context
    pk = keygen(pr, c, params)
    proof, record = create_proof(params, pk, c)                     # bytes, dict
    verify_proofs([{"protocol": pr, "vk_bytes": pk.vk, "instances": c.instances(), "proof": proof}], params=params)

Objects free their handle on close() or __del__; a circuit and a key keep their protocol alive inside the library.  An object is used by one thread at a time.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _capi
from ._capi import check, lib, Mi355Error  # noqa: F401
from .halo2 import R_MOD, fr, fr_to_int

CIRCUIT_PARTS = ("preprocessed", "advice", "m", "m_counts", "m_blind", "z_blind", "phi_blind", "random_poly", "instances", "copies",
                 "perm_blind", "lz_blind")   # the last two: protocols with the classic (permuted) lookup argument, which have no m, m_counts, m_blind, phi_blind
MODE_BATCHED, MODE_ONE_BY_ONE, MODE_AGGREGATE, MODE_FOLD_ONLY = 0, 1, 2, 3


class _Handle:
    """one uint64 handle of the library; freed once, by close() or at collection"""
    kind = "object"

    def __init__(self, handle: int):
        self.handle = int(handle)

    def close(self) -> None:
        h, self.handle = getattr(self, "handle", 0), 0
        if h:
            check(lib().mi355_plonk_free(h))

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __int__(self):
        return self.handle


def _bytes_out(call) -> bytes:
    """the (out, cap, bytes_out) convention: ask for the size, then fetch"""
    n = C.c_uint64()
    check(call(None, 0, C.byref(n)))
    buf = (C.c_uint8 * max(1, n.value))()
    check(call(C.cast(buf, C.c_void_p), n.value, C.byref(n)))
    return bytes(buf[: n.value])


def _record(handle: int):
    """a record handle -> the parsed JSON; the handle is freed"""
    if not handle:
        return None
    try:
        return json.loads(_bytes_out(lambda out, cap, n: lib().mi355_plonk_record_json(handle, out, cap, n)).decode())
    finally:
        lib().mi355_plonk_free(handle)


class Protocol(_Handle):
    kind = "protocol"
    FIELDS = ("k", "n", "layer", "num_preprocessed", "num_instance", "num_advice", "num_lookups", "num_perm_columns", "num_perm_chunks", "num_gates", "num_witness", "num_commitments",
              "blind", "usable", "quotient_pieces", "extended_k", "num_evaluations", "num_queries", "lookup_bits", "proof_bytes_poseidon", "proof_bytes_evm", "has_initial_state",
              "has_accumulator", "lookup_permuted")

    @classmethod
    def from_json(cls, protocol) -> "Protocol":
        """protocol: the PlonkProtocol as a dict (protocols.layer_protocol), str or bytes"""
        text = protocol if isinstance(protocol, (bytes, bytearray)) else (protocol if isinstance(protocol, str) else json.dumps(protocol, separators=(",", ":"))).encode()
        h = C.c_uint64()
        check(lib().mi355_plonk_protocol_from_json(bytes(text), len(text), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_file(cls, path: str) -> "Protocol":
        h = C.c_uint64()
        check(lib().mi355_plonk_protocol_from_file(str(path).encode(), C.byref(h)))
        return cls(h.value)

    def info(self, field: str | None = None):
        """one figure by name, or all of them as a dict; layer is -1 when the file names none"""
        if field is None:
            return {f: self.info(f) for f in self.FIELDS}
        v = C.c_uint64()
        check(lib().mi355_plonk_protocol_info(self.handle, field.encode(), C.byref(v)))
        return -1 if field == "layer" and v.value == 2**64 - 1 else v.value


class Circuit(_Handle):
    kind = "circuit"

    def __init__(self, protocol, handle: int | None = None):
        """Circuit(protocol): every column present and zero, no copies, no instance values"""
        if handle is None:
            h = C.c_uint64()
            check(lib().mi355_plonk_circuit_new(int(protocol), C.byref(h)))
            handle = h.value
        super().__init__(handle)
        self.protocol = protocol

    @classmethod
    def synthetic(cls, protocol, seed: int = 1, blind_seed: int = 0, fill: float = 0.9, assign_density: float = 1.0, pinned: bool = False, zero_blinding: bool = False) -> "Circuit":
        """plonk::build_circuit, as tests/cpp/test_plonk_replay.cpp calls it: a satisfying instance for the protocol; the same arguments give the same instance"""
        h = C.c_uint64()
        check(lib().mi355_plonk_circuit_synthetic(int(protocol), seed, blind_seed, fill, assign_density, (1 if pinned else 0) | (2 if zero_blinding else 0), C.byref(h)))
        return cls(protocol, h.value)

    def set(self, what: str, index: int, data) -> None:
        """data: bytes or a C-contiguous numpy array (uint64 limbs; uint32 for m_counts; [pairs, 4] uint64 for copies)"""
        raw = bytes(data) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).tobytes()
        check(lib().mi355_plonk_circuit_set(self.handle, what.encode(), index, C.cast(C.c_char_p(raw), C.c_void_p), len(raw)))

    def get_bytes(self, what: str, index: int = 0) -> bytes:
        return _bytes_out(lambda out, cap, n: lib().mi355_plonk_circuit_get(self.handle, what.encode(), index, out, cap, n))

    def get(self, what: str, index: int = 0) -> np.ndarray:
        """the part as an array: [rows, 4] uint64 limbs (Montgomery), uint32 counts for m_counts, [pairs, 4] uint64 for copies"""
        raw = self.get_bytes(what, index)
        if what == "m_counts":
            return np.frombuffer(raw, dtype=np.uint32).copy()
        return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()

    def instances(self) -> list:
        """the instance values as integers (what the verifier takes)"""
        return [fr_to_int(v) for v in self.get("instances")]


class ProvingKey(_Handle):
    kind = "proving key"

    def __init__(self, handle: int, protocol):
        super().__init__(handle)
        self.protocol = protocol
        self._vk = None

    @property
    def vk(self) -> bytes:
        """the .vkey bytes"""
        if self._vk is None:
            self._vk = _bytes_out(lambda out, cap, n: lib().mi355_plonk_pk_vk(self.handle, out, cap, n))
        return self._vk


class Options(_Handle):
    """the fields of ProofOptions, VerifyOptions and CheckOptions by name: Options(device_multiplicities=True, transcript="poseidon", rng_key=bytes(32))"""
    kind = "options"

    def __init__(self, **fields):
        h = C.c_uint64()
        check(lib().mi355_plonk_options_new(C.byref(h)))
        super().__init__(h.value)
        for k, v in fields.items():
            self.set(k, v)

    def set(self, name: str, value) -> "Options":
        if isinstance(value, bool):
            value = "1" if value else "0"
        elif isinstance(value, (bytes, bytearray)):
            value = bytes(value).hex()
        elif name == "initial_state" and isinstance(value, int):
            value = "%064x" % value
        check(lib().mi355_plonk_options_set(self.handle, name.encode(), str(value).encode()))
        return self


def _opts(options):
    """None | Options | dict -> (handle, temporary to close)"""
    if options is None:
        return 0, None
    if isinstance(options, Options):
        return options.handle, None
    tmp = Options(**options)
    return tmp.handle, tmp


def keygen(protocol: Protocol, circuit: Circuit, params, resident_cosets: bool = True, device_sigma: bool = False, devices: int = 1) -> ProvingKey:
    """plonk::keygen on params' Lagrange basis (a halo2.ParamsKZG, or the handle itself); the key stays in HBM until it is closed"""
    gl = params if isinstance(params, int) else params._gl
    h = C.c_uint64()
    check(lib().mi355_plonk_keygen(protocol.handle, circuit.handle, gl, (1 if resident_cosets else 0) | (2 if device_sigma else 0), devices, C.byref(h)))
    return ProvingKey(h.value, protocol)


def _srs(params):
    return params if isinstance(params, tuple) else (params._g, params._gl)


def create_proof(params, pk: ProvingKey, circuit: Circuit, options=None):
    """plonk::create_proof -> (proof bytes, record dict).  With check_witness set and a failing witness: Mi355Error (code EBADARG) carrying the record as `.record`"""
    g, gl = _srs(params)
    oh, tmp = _opts(options)
    try:
        cap = pk.protocol.info("proof_bytes_evm")   # the longest layout: whichever transcript the options or the layer pick fits
        buf = (C.c_uint8 * cap)()
        n, rec = C.c_uint64(), C.c_uint64()
        rc = lib().mi355_plonk_create_proof(g, gl, pk.handle, circuit.handle, oh, C.cast(buf, C.c_void_p), cap, C.byref(n), C.byref(rec))
        if rc != _capi.OK:
            err = Mi355Error(rc, lib().mi355_last_error().decode())
            err.record = _record(rec.value)
            raise err
        return bytes(buf[: n.value]), _record(rec.value)
    finally:
        if tmp is not None:
            tmp.close()


def check_witness(pk: ProvingKey, circuit: Circuit, options=None) -> dict:
    """plonk::check_witness (MockProver::verify on the device) -> {"n_failures", "failures": [{kind, index, row, count, col_a, col_b, row_b, message}]}"""
    oh, tmp = _opts(options)
    try:
        n, rec = C.c_uint64(), C.c_uint64()
        check(lib().mi355_plonk_check_witness(pk.handle, circuit.handle, oh, C.byref(n), C.byref(rec)))
        out = _record(rec.value)
        assert out["n_failures"] == n.value
        return out
    finally:
        if tmp is not None:
            tmp.close()


def _verify_call(cases, mode: int, params, g2, s_g2, neg_s_g2, options):
    n = len(cases)
    as_g2 = lambda q: q if isinstance(q, (bytes, bytearray)) else np.ascontiguousarray(q, dtype=np.uint64).tobytes()
    if params is not None:
        g2, s_g2 = params.g2, params.s_g2
    if g2 is None and (s_g2 is not None or neg_s_g2 is not None):
        from .halo2 import g2_generator
        g2 = g2_generator()                                            # as halo2.verify_proof: the default g2 is the generator
    keep = []   # every buffer the pointer arrays name, alive for the call

    def buf(raw: bytes):
        b = C.create_string_buffer(bytes(raw), max(1, len(raw)))
        keep.append(b)
        return C.cast(b, C.c_void_p)

    protos = (C.c_uint64 * max(1, n))(*[int(c["protocol"]) for c in cases])
    vks, vkl = (C.c_void_p * max(1, n))(), (C.c_uint64 * max(1, n))()
    ins, nin = (C.c_void_p * max(1, n))(), (C.c_uint64 * max(1, n))()
    prs, prl = (C.c_void_p * max(1, n))(), (C.c_uint64 * max(1, n))()
    for i, c in enumerate(cases):
        unknown = set(c) - {"protocol", "vk_bytes", "instances", "proof"}
        assert not unknown, "verify_proofs: unknown keys %s in case %d (per-proof options go into `options`)" % (sorted(unknown), i)
        if c.get("vk_bytes") is not None:
            vks[i], vkl[i] = buf(c["vk_bytes"]), len(c["vk_bytes"])
        words = np.stack([fr(int(v) % R_MOD) for v in c["instances"]]).tobytes() if len(c["instances"]) else b""
        ins[i], nin[i] = buf(words), len(c["instances"])
        prs[i], prl[i] = buf(c["proof"]), len(c["proof"])
    negated = neg_s_g2 is not None
    q = neg_s_g2 if negated else s_g2
    ok = (C.c_uint8 * max(1, n))()
    rec = C.c_uint64()
    oh, tmp = _opts(options)
    try:
        check(lib().mi355_plonk_verify_proofs(n, protos, vks, vkl, ins, nin, prs, prl, buf(as_g2(g2)) if g2 is not None else None, buf(as_g2(q)) if q is not None else None,
                                              1 if negated else 0, oh, mode, ok, C.byref(rec)))
    finally:
        if tmp is not None:
            tmp.close()
    return [bool(ok[i]) for i in range(n)], _record(rec.value)


def _ints(rec: dict) -> dict:
    """a per-proof record: hexadecimal field elements and coordinates -> integers (what halo2._verify_record does to a driver's line)"""
    from .halo2 import _verify_record
    return _verify_record(rec)


def verify_proofs(cases, params=None, g2=None, s_g2=None, neg_s_g2=None, options=None, one_by_one: bool = False) -> list:
    """plonk::verify_proofs (or verify_proof in a loop) over cases = [{"protocol": Protocol, "instances": integers, "proof": bytes, "vk_bytes": bytes | None}, ...].
    The SRS side: params (a halo2.ParamsKZG) or g2 + s_g2 | neg_s_g2 (128-byte G2Affine); not needed with host_only.  options: Options or a dict (transcript, host_only,
    check_accumulator, accumulator, initial_state, device_transcript, device_scalars), applied to every proof.  Returns the records halo2.verify_proofs returns, one per proof; a rejected
    proof is a record with ok False and the named failure in "error"."""
    ok, rec = _verify_call(cases, MODE_ONE_BY_ONE if one_by_one else MODE_BATCHED, params, g2, s_g2, neg_s_g2, options)
    out = [_ints(r) for r in rec["proofs"]]
    assert [r["ok"] for r in out] == ok
    for r in out:
        r["device_calls"] = rec["device_calls"]
    return out


def aggregate(cases, params=None, g2=None, s_g2=None, neg_s_g2=None, options=None, pairing: bool = True) -> dict:
    """plonk::aggregate: the dict halo2.aggregate returns (ok, error, detail, proofs, accumulators, r, lhs, rhs, limbs, pairing, device_calls)"""
    ok, rec = _verify_call(cases, MODE_AGGREGATE if pairing else MODE_FOLD_ONLY, params, g2, s_g2, neg_s_g2, options)
    h = lambda s: int(s, 16)
    pt = lambda p: (h(p[0]), h(p[1]))
    a = dict(rec["aggregate"])
    a["aggregate"] = True
    a["proofs"] = [_ints(r) for r in rec["proofs"]]
    a["accumulators"] = [(pt(l), pt(r)) for l, r in a["accumulators"]]
    a["r"] = h(a["r"]); a["lhs"] = pt(a["lhs"]); a["rhs"] = pt(a["rhs"]); a["limbs"] = [h(v) for v in a["limbs"]]
    a["device_calls"] = rec["device_calls"]
    a["accepted"] = ok
    return a
