"""CPU-only: the surface of the device transcripts.  mi355_poseidon_transcripts_host is declared in include/mi355zk.h (six arguments, citing the call site it serves), sits in
the ctypes table, is exported by the library and bound in the Rust shim; halo2.poseidon_transcripts / halo2::poseidon_transcripts exist; the driver test_device_transcripts is
one of the compiled programs.  Without a device the entry point fails with MI355_ENODEVICE -- after its argument checks, which read host memory only and therefore answer
MI355_EBADARG here as well, each case with its own message.  The recording pass of VerifyOptions::device_transcript (the driver's --host-only) over the ten released proofs:
what it puts on the tape, fed to oracle.poseidon.Sponge, gives the eight challenges oracle.plonk.verify squeezes for that proof."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk, poseidon, pyref

import aggregate_common as ac
from verify_common import ALL_TEN, case, layout, oracle_verify, product_protocol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_poseidon_transcripts_host"
R = pyref.R_MOD


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_declared_bound_exported_and_in_the_rust_block(zk):
    hdr = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m and len(m.group(1).split(",")) == 6
    for arg in ("const void *words_host", "const uint64_t *word_offsets_host", "const uint32_t *squeeze_at_host", "const uint64_t *squeeze_offsets_host", "uint32_t jobs", "void *challenges_out_host"):
        assert arg in " ".join(m.group(1).split()), arg
    comment = hdr[:m.start()].rsplit("/*", 1)[1]
    assert "[REF integration/src/prove.rs:67]" in comment and "gen_batch_proof" in comment and "PoseidonTranscript<NativeLoader>" in comment
    ret, args = zk._capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(args) == 6 and args[4] is C.c_uint32
    assert hasattr(zk._capi.lib(), NAME)
    rs = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rs, flags=re.S).group(1)
    assert re.search(r"fn\s+%s\s*\(" % NAME, block)


def test_python_and_cpp_surfaces_exist(zk):
    import inspect
    for f in ("poseidon_transcripts", "record_transcripts"):
        assert callable(getattr(zk.halo2, f))
    for f in ("verify_proofs", "aggregate"):
        assert inspect.signature(getattr(zk.halo2, f)).parameters["device_transcript"].default is False
    h2 = open(os.path.join(ROOT, "include", "mi355zk_halo2.hpp")).read()
    assert "poseidon_transcripts(" in h2 and NAME in h2
    pv = open(os.path.join(ROOT, "include", "mi355zk_plonk_verify.hpp")).read()
    assert "bool device_transcript = false;" in pv
    assert "test_device_transcripts" in ge.CPP_PROGRAMS and "test_device_transcripts" in ge._build_module().CPP_PROGRAMS
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_device_transcripts.cpp"))
    assert os.path.exists(os.path.join(ROOT, "scroll-prover_amd", "csrc", "poseidon.hpp"))
    assert '#include "poseidon.hpp"' in open(os.path.join(ROOT, "scroll-prover_amd", "csrc", "lib_aux.hip")).read()


def _args():
    """two jobs: three words squeezed at 1 and 3, two words squeezed at 2"""
    words = np.zeros((5, 4), dtype=np.uint64); words[:, 0] = np.arange(5)
    return words, np.array([0, 3, 5], dtype=np.uint64), np.array([1, 3, 2], dtype=np.uint32), np.array([0, 2, 3], dtype=np.uint64), np.full((3, 4), 7, dtype=np.uint64)


def test_no_device_is_a_loud_failure(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for a machine without a GPU")
    capi, ptr, lib = zk._capi, zk._capi.ptr, zk._capi.lib()
    w, woff, sq, soff, out = _args()
    assert lib.mi355_poseidon_transcripts_host(ptr(w), ptr(woff), ptr(sq), ptr(soff), 2, ptr(out)) == capi.ENODEVICE
    assert (out == 7).all()
    assert lib.mi355_poseidon_transcripts_host(None, None, None, None, 0, None) == capi.ENODEVICE      # jobs == 0 launches nothing, but it is still a compute entry point
    with pytest.raises(zk.Mi355Error):
        zk.halo2.poseidon_transcripts(w, woff, sq, soff)


def test_bad_arguments_are_named_before_the_device_is_asked_for(zk):
    """every EBADARG case of the entry point, each with its message; the output stays untouched"""
    capi, ptr, lib = zk._capi, zk._capi.ptr, zk._capi.lib()
    w, woff, sq, soff, out = _args()
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    u32 = lambda *v: np.array(v, dtype=np.uint32)

    def refused(needle, words=w, word_off=woff, squeeze_at=sq, squeeze_off=soff, jobs=2, res=out):
        rc = lib.mi355_poseidon_transcripts_host(ptr(words), ptr(word_off), ptr(squeeze_at), ptr(squeeze_off), jobs, ptr(res))
        msg = lib.mi355_last_error()
        assert rc == capi.EBADARG and msg.startswith(b"poseidon_transcripts: ") and needle in msg, (rc, msg)

    for missing in ("words", "word_off", "squeeze_at", "squeeze_off", "res"):
        refused(b"null pointer", **{missing: None})
    refused(b"word_offsets[0] must be 0", word_off=u64(1, 3, 5))
    refused(b"squeeze_offsets[0] must be 0", squeeze_off=u64(1, 2, 3))
    refused(b"word_offsets decrease at job 1", word_off=u64(0, 3, 2))
    refused(b"squeeze_offsets decrease at job 1", squeeze_off=u64(0, 3, 2))
    refused(b"squeeze positions decrease in job 0", squeeze_at=u32(2, 1, 2))
    refused(b"squeeze position 3 exceeds the 2 words of job 1", squeeze_at=u32(1, 3, 3))
    refused(b"more than 2^20 jobs", jobs=(1 << 20) + 1)                                             # refused before a single offset is read
    refused(b"more than 2^24 words", word_off=u64(0, 3, (1 << 24) + 1))
    refused(b"more than 2^24 squeezes", squeeze_off=u64(0, 2, (1 << 24) + 1))
    bad = w.copy(); bad[3] = np.array(pyref.to_limbs(R), dtype=np.uint64)                              # the word r itself; word 4 is worse and comes later
    bad[4] = 0xFFFFFFFFFFFFFFFF
    refused(b"word 3 is not below r", words=bad)
    assert (out == 7).all()


# ---- the recording pass over the released proofs

class _Listening(plonk.TRANSCRIPTS["poseidon"]):
    """the oracle's own Poseidon transcript, writing down what it squeezes"""
    heard = None

    def squeeze(self):
        c = super().squeeze()
        _Listening.heard.append(c)
        return c


def oracle_squeezes(name, monkeypatch):
    """the eight challenges oracle.plonk.verify squeezes for a released proof, in order: theta, beta, gamma, y, x, and SHPLONK's y, v, u"""
    layer, inst, proof, okw, _ = case(name)
    _Listening.heard = []
    monkeypatch.setitem(plonk.TRANSCRIPTS, "poseidon", _Listening)
    got = oracle_verify(layer, inst, proof, okw)
    monkeypatch.undo()
    assert got["ok"], (name, got)
    ch = got["challenges"]
    assert _Listening.heard[:5] == [ch["theta"], ch["beta"], ch["gamma"], ch["y"], ch["x"]] and len(_Listening.heard) == 8
    assert _Listening.heard[7] == got["msm"]["scalars"][-1]                                          # u is the scalar of W' in the list
    return list(_Listening.heard)


@pytest.fixture(scope="module")
def recorded(zk):
    return zk.halo2.record_transcripts([ac.product_case(n) for n in ALL_TEN])


def through_the_oracle_sponge(rec):
    sp = poseidon.Sponge(); prev = 0; out = []
    for p in rec["squeeze_at"]:
        sp.update(rec["words"][prev:p]); prev = p
        out.append(sp.squeeze())
    return out


def test_recorded_jobs_give_the_oracles_challenges(recorded, monkeypatch):
    assert len(recorded) == 10
    for name, rec in zip(ALL_TEN[:9], recorded):
        assert rec["job"] and rec["error"] == "", (name, rec["error"], rec["detail"])
        assert len(rec["squeeze_at"]) == 8 and rec["squeeze_at"] == sorted(rec["squeeze_at"]) and rec["squeeze_at"][-1] <= len(rec["words"])
        assert all(0 <= v < R for v in rec["words"])
        want = oracle_squeezes(name, monkeypatch)
        assert through_the_oracle_sponge(rec) == want, name
        assert rec["challenges"] == want, name                                                       # and the host sponge of the product agrees
    # 26 permutations for a chunk proof, 25 for a batch proof: the count the design rests on
    perms = lambda rec: sum((p - q) // 4 + 1 for p, q in zip(rec["squeeze_at"], [0] + rec["squeeze_at"][:-1]))
    assert perms(recorded[0]) == 26 and perms(recorded[7]) == 25


def test_the_bundle_proof_records_no_job(recorded):
    rec = recorded[ALL_TEN.index("bundle_proof")]                                                    # the EVM transcript: nothing for the device
    assert not rec["job"] and rec["error"] == "" and rec["words"] == [] and rec["squeeze_at"] == [] and rec["challenges"] == []


def not_a_point_word(word: bytes) -> bytes:
    for d in range(1, 64):
        w = bytearray(word); w[0] = (w[0] + d) & 0xFF
        try:
            if pyref.g1_decompress(bytes(w)) is None:
                return bytes(w)
        except AssertionError:
            return bytes(w)
    raise AssertionError("no rejected word nearby")


def test_an_invalid_point_records_no_job_and_leaves_the_others_unchanged(zk, recorded):
    name = ALL_TEN[3]
    layer, inst, proof, okw, pkw = case(name)
    coms, _, _, _ = layout(layer, okw["transcript"])
    bad = bytearray(proof); bad[coms[2]:coms[2] + 32] = not_a_point_word(proof[coms[2]:coms[2] + 32])
    cases = [ac.product_case(n) for n in ALL_TEN]
    cases[3] = ac.product_case(name, proof=bytes(bad))
    got = zk.halo2.record_transcripts(cases)
    alone = zk.halo2.verify_proof(product_protocol(layer), inst, bytes(bad), host_only=True, **pkw)
    assert not got[3]["job"] and got[3]["words"] == [] and got[3]["squeeze_at"] == []
    assert got[3]["error"] == alone["error"] == "invalid_point" and got[3]["detail"] == alone["detail"]
    for i in range(10):
        if i != 3:
            assert got[i] == recorded[i], i
