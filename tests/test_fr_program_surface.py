"""CPU-only: the surface of the device scalar sides.  mi355_fr_program_host is declared in include/mi355zk.h (twelve arguments, citing the call site it serves), sits in the
ctypes table, is exported by the library and bound in the Rust shim; halo2.fr_program / halo2::fr_program exist; VerifyOptions::device_scalars is a field, a name of the C ABI's
option table and a keyword of halo2.verify_proofs / halo2.aggregate; the driver test_device_scalars is one of the compiled programs and does not link the oracle's library.
Without a device the entry point fails with MI355_ENODEVICE -- after its argument checks, which read host memory only and therefore answer MI355_EBADARG here as well, each case
with its own message.  The programs compiled for the released proofs' three protocols: one inverse each, a few hundred registers."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import pyref

import aggregate_common as ac
from verify_common import ALL_TEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_fr_program_host"
ARGS = ("const uint32_t *code_host", "uint32_t n_instr", "uint32_t n_regs", "const void *consts_host", "uint32_t n_consts", "const void *inputs_host", "uint32_t n_inputs",
        "uint32_t jobs", "const uint32_t *out_regs_host", "uint32_t n_outputs", "void *outputs_host", "uint32_t *flags_out_host")


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def test_declared_bound_exported_and_in_the_rust_block(zk):
    hdr = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m and len(m.group(1).split(",")) == 12
    for arg in ARGS:
        assert arg in " ".join(m.group(1).split()), arg
        assert not arg.endswith("_dev")
    comment = hdr[:m.start()].rsplit("/*", 1)[1]
    assert "[REF integration/src/prove.rs:67]" in comment and "gen_batch_proof" in comment and "device_scalars" in comment and '"fr_program"' in comment
    ret, args = zk._capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(args) == 12 and args[7] is C.c_uint32
    assert hasattr(zk._capi.lib(), NAME)
    rs = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rs, flags=re.S).group(1)
    assert re.search(r"fn\s+%s\s*\(" % NAME, block)


def test_the_option_and_the_other_surfaces_exist(zk):
    assert callable(zk.halo2.fr_program) and callable(zk.halo2.scalar_programs)
    for f in ("verify_proofs", "aggregate"):
        assert inspect.signature(getattr(zk.halo2, f)).parameters["device_scalars"].default is False
    assert "fr_program(" in open(os.path.join(ROOT, "include", "mi355zk_halo2.hpp")).read()
    pv = open(os.path.join(ROOT, "include", "mi355zk_plonk_verify.hpp")).read()
    assert "bool device_scalars = false;" in pv and "scalar_call" in pv and '#include "mi355zk_plonk_scalar.hpp"' in pv
    capi = open(os.path.join(ROOT, "scroll-prover_amd", "csrc", "plonk_capi.hpp")).read()
    assert '{"device_scalars", OptType::Bool, 0, 1, "VerifyOptions"}' in capi
    hdr = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    assert "device_scalars" in hdr[hdr.index("Names: devices"):hdr.index("int mi355_plonk_options_new")]
    pvm = zk.prover
    with pvm.Options() as o:
        o.set("device_scalars", True); o.set("device_scalars", 0)
    assert "test_device_scalars" in ge.CPP_PROGRAMS and "test_device_scalars" in ge._build_module().CPP_PROGRAMS
    assert '#include "frprog.hpp"' in open(os.path.join(ROOT, "scroll-prover_amd", "csrc", "lib_aux.hip")).read()
    exe = ge.build_cpp("test_device_scalars")
    assert b"oracle_bn254" not in open(exe, "rb").read()                                              # neither NEEDED nor on its run path


def _args():
    """two jobs of r3 = (in0 + c0) * in1 with one constant and two inputs"""
    code = np.array([[0, 3, 1, 0], [2, 3, 3, 2]], dtype=np.uint32)
    consts = np.zeros((1, 4), dtype=np.uint64); inputs = np.zeros((4, 4), dtype=np.uint64); inputs[:, 0] = np.arange(4)
    return code, consts, inputs, np.array([3], dtype=np.uint32), np.full((2, 4), 7, dtype=np.uint64), np.full(2, 7, dtype=np.uint32)


def _call(zk, code, consts, inputs, outs, res, flags, n_instr=2, n_regs=4, n_consts=1, n_inputs=2, jobs=2, n_outputs=1):
    ptr = zk._capi.ptr
    return zk._capi.lib().mi355_fr_program_host(ptr(code), n_instr, n_regs, ptr(consts), n_consts, ptr(inputs), n_inputs, jobs, ptr(outs), n_outputs, ptr(res), ptr(flags))


def test_no_device_is_a_loud_failure(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for a machine without a GPU")
    a = _args()
    assert _call(zk, *a) == zk._capi.ENODEVICE
    assert (a[4] == 7).all() and (a[5] == 7).all()
    assert _call(zk, None, None, None, None, None, None, n_instr=0, n_regs=0, n_consts=0, n_inputs=0, jobs=0, n_outputs=0) == zk._capi.ENODEVICE   # nothing to launch, still a compute entry point
    with pytest.raises(zk.Mi355Error):
        zk.halo2.fr_program(a[0], 4, a[1], a[2].reshape(2, 2, 4), a[3])


def test_bad_arguments_are_named_before_the_device_is_asked_for(zk):
    """every EBADARG case of the entry point, each with its message and the offending index; the outputs stay untouched"""
    capi, lib = zk._capi, zk._capi.lib()
    code, consts, inputs, outs, res, flags = _args()
    names = ("code", "consts", "inputs", "outs", "res", "flags")

    def refused(needle, **over):
        a = dict(zip(names, (code, consts, inputs, outs, res, flags)))
        sizes = {k: over.pop(k) for k in list(over) if k not in names}
        a.update(over)
        rc = _call(zk, *[a[n] for n in names], **sizes)
        msg = lib.mi355_last_error()
        assert rc == capi.EBADARG and msg.startswith(b"fr_program: ") and needle in msg, (rc, msg)

    for missing in names:
        refused(b"null pointer", **{missing: None})
    refused(b"more than 2^16 registers", n_regs=(1 << 16) + 1)
    refused(b"more than 2^20 instructions", n_instr=(1 << 20) + 1)                              # refused before a single instruction is read
    refused(b"more than 2^20 jobs", jobs=(1 << 20) + 1)
    refused(b"n_consts + n_inputs = 3 exceeds n_regs = 2", n_regs=2)
    u32 = lambda rows: np.array(rows, dtype=np.uint32)
    refused(b"instruction 1: unknown op 6", code=u32([[0, 3, 1, 0], [6, 3, 3, 2]]))
    refused(b"instruction 0: operand register 4 is not below n_regs = 4", code=u32([[0, 3, 4, 0], [2, 3, 3, 2]]))
    refused(b"instruction 1: operand register 5 is not below n_regs = 4", code=u32([[0, 3, 1, 0], [2, 3, 3, 5]]))
    refused(b"instruction 1: destination register 4 is not below n_regs = 4", code=u32([[0, 3, 1, 0], [2, 4, 3, 2]]))
    refused(b"instruction 0: destination register 2 is a constant or an input (the first temporary is 3)", code=u32([[0, 2, 1, 0], [2, 3, 3, 2]]))
    refused(b"instruction 0: SQRN by 65", code=u32([[3, 3, 1, 65], [2, 3, 3, 2]]))
    refused(b"instruction 1: NZ names flag bit 0", code=u32([[0, 3, 1, 0], [5, 0, 3, 0]]))
    refused(b"instruction 1: NZ names flag bit 32", code=u32([[0, 3, 1, 0], [5, 0, 3, 32]]))
    refused(b"output 0 names register 4", outs=u32([4]))
    r_word = np.array([pyref.to_limbs(pyref.R_MOD)], dtype=np.uint64)
    refused(b"constant 0 is not below r", consts=r_word)
    bad = inputs.copy(); bad[3] = r_word[0]
    refused(b"input 1 of job 1 is not below r", inputs=bad)
    assert (res == 7).all() and (flags == 7).all()


def test_the_programs_of_the_released_proofs(zk):
    recs = zk.halo2.scalar_programs([ac.product_case(n) for n in ALL_TEN])
    assert len(recs) == 3 and {25, 26} <= {r["k"] for r in recs}                               # the chunk proofs' protocol, the batch proofs', the bundle proof's
    for r in recs:
        assert r["usable"] and r["inversions"] == 1 and 0 < r["registers"] <= 1 << 16 and 0 < r["instructions"] <= 1 << 20, r
        assert r["inputs"] > 8 + r["instances"] and r["outputs"] >= 4, r                          # the eight challenges, the evaluations, the instances; the numerator and the list
