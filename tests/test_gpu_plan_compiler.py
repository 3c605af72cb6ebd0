"""The device runs the plans plonk::Compiler (include/mi355zk_plonk.hpp) makes of the gate families of tests/plan_common.py: 16-term and 24-polynomial launches of
mi355_fr_gate_eval_dev, accumulating launches into temporaries, relocated temporaries reused in stream order, the pooled part buffers of coset_group_polys and the lean key.
In process through scroll-prover_amd/prover.py, as tests/test_gpu_plonk_capi.py; tests/test_plan_compiler_on_host.py holds the same plans to the numerator on the CPU.

  proof bytes     A, D, E, F, G: verifying key and proof equal oracle/plonk.py's restatement on the instance read back through circuit_get; the verifier accepts; the
                  record's plan counts show the family's path
  whatever plan   E, F: the same bytes under MI355_PLAN_PREFIX_MIN unset / 0 / 2 (the compiler reads it at every compile), a key made under one value and a proof under
                  another, coset_group_polys = 24 (E's 24-polynomial launch fills a group exactly), a lean key (resident_cosets = False), and the last two together
  witness check   B, C, F, G: no failure on the builder's instance; with three advice cells off (one read at rotation -1, at row 0; one read at rotation 2, at row n - 1;
                  a gate's target on the last usable row) exactly the failures of tests/witness_check_common.py's Reference
  refusal         H: keygen fails with MI355_EBADARG naming the 32-temporary limit and leaves no device memory behind

k = 6: the smallest domain with the builder's blocks, the 6 blinding rows and the omega^-7 link.  Measured on the CPU: the restatement's proof of one case takes 0.3 - 0.4 s
at advice = 60 (E), its verifier 0.6 s; nothing here had to shrink."""
import pytest

import __graft_entry__ as ge
from oracle import plonk

import plan_common as pc
import witness_check_common as wc
from plonk_capi_common import proof_inputs, tau_of

pytestmark = pytest.mark.gpu
K = 6
TAU = tau_of(0)
PREFIX_ENV = "MI355_PLAN_PREFIX_MIN"
WITNESS_SEED = 4      # the builder's instance of the witness check: one on which C's long monomials are nonzero on rows 0 and 1 (its lookup-input cells are zero now and then), so that
                      # all three wrong cells show in many gates; the test asserts that they do


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


class Case:
    """one family at k = 6: protocol, SRS, the builder's circuit; keys are made by the tests.  close() frees everything"""

    def __init__(self, zk, family, seed=1):
        self.zk, self.family, self.seed = zk, family, seed
        self.d = pc.family_protocol(family, K)
        self.protocol = zk.prover.Protocol.from_json(self.d)
        self.info = self.protocol.info()
        self.params = zk.halo2.ParamsKZG.setup(K, TAU)
        self.circuit = zk.prover.Circuit.synthetic(self.protocol, seed=seed)
        self.constraints = len(self.d["quotient"]["numerator"]["DistributePowers"][0])

    def keygen(self, **kw):
        return self.zk.prover.keygen(self.protocol, self.circuit, self.params, **kw)

    def restated(self, circuit=None):
        inp = proof_inputs(circuit or self.circuit, self.d, TAU, self.info)
        vk = plonk.keygen_vk(inp.pr, inp.pre, inp.tau)
        return vk, plonk.prove(inp, vk, transcript="poseidon"), inp

    def close(self):
        for x in (self.circuit, self.protocol):
            x.close()
        self.params.release()


@pytest.fixture(scope="module")
def cases(zk):
    """the provable families with the CPU restatement's key and proof, computed once and never modified"""
    made = {}
    for fam in pc.PROVABLE:
        c = Case(zk, fam)
        c.want_vk, c.want_proof, c.inputs = c.restated()
        made[fam] = c
    yield made
    for c in made.values():
        c.close()


def first_difference(got, want):
    return next((i // 32 for i in range(0, min(len(got), len(want)), 32) if got[i:i + 32] != want[i:i + 32]), None)


def prove(zk, case, pk, options=None):
    proof, rec = zk.prover.create_proof(case.params, pk, case.circuit, options)
    assert proof == case.want_proof, f"family {case.family}: proof bytes differ from the CPU restatement from word {first_difference(proof, case.want_proof)} on; plan " \
        f"{ {k: rec[k] for k in ('plan_launches', 'plan_terms', 'plan_tmps', 'plan_constraints', 'plan_prefix_groups')} }"
    assert rec["plan_constraints"] == case.constraints and rec["plan_terms"] <= 16 * rec["plan_launches"]
    return rec


# ------------------------------------------------------------------------------------------------ proof bytes
@pytest.mark.parametrize("family", pc.PROVABLE)
def test_key_and_proof_bytes_equal_the_cpu_restatement(zk, cases, family, monkeypatch):
    monkeypatch.delenv(PREFIX_ENV, raising=False)
    c = cases[family]
    with c.keygen() as pk:
        assert pk.vk == c.want_vk, "verifying key differs"
        rec = prove(zk, c, pk)
    print(family, {k: rec[k] for k in ("plan_launches", "plan_terms", "plan_tmps", "plan_constraints", "plan_prefix_groups", "gate_launches")})
    assert plonk.verify(c.inputs.pr, c.want_vk, c.inputs.instances, c.want_proof, c.inputs.tau, transcript="poseidon")["ok"]
    # the path conditions of tests/test_plan_compiler_on_host.py on what the record holds
    assert rec["plan_prefix_groups"] == 1                                   # every family has >= 16 gates under the one selector: one G_p by default
    assert rec["plan_tmps"] >= rec["plan_prefix_groups"] + 1
    if family in ("A", "E"):
        # one launch per temporary and the fewest launches of 16 terms that hold the quotient's terms are not enough: a sum was cut at a launch limit and continued by an
        # accumulating launch, or a temporary was written again
        assert rec["plan_launches"] > rec["plan_tmps"] + -(-rec["plan_terms"] // 16)
    if family == "F":
        assert rec["plan_tmps"] - rec["plan_prefix_groups"] > 12            # local temporaries beyond TMP_GROUP: one constraint needed them all
    if family == "G":
        assert rec["plan_tmps"] - rec["plan_prefix_groups"] >= 12


# ------------------------------------------------------------------------------------------------ same bytes whatever the plan
def set_prefix(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(PREFIX_ENV, raising=False)
    else:
        monkeypatch.setenv(PREFIX_ENV, value)


def check_prefix_record(rec, value):
    if value == "0":
        assert rec["plan_prefix_groups"] == 0
    if value == "2":
        assert rec["plan_prefix_groups"] >= 2 and rec["plan_tmps"] >= rec["plan_prefix_groups"] + 1


@pytest.mark.parametrize("key_prefix,proof_prefix", [(None, None), ("0", "0"), ("2", "2"), ("0", "2"), ("2", None)])
@pytest.mark.parametrize("family", ["E", "F"])
def test_the_prefix_threshold_changes_the_plan_and_not_the_bytes(zk, cases, family, key_prefix, proof_prefix, monkeypatch):
    c = cases[family]
    set_prefix(monkeypatch, key_prefix)
    with c.keygen() as pk:
        assert pk.vk == c.want_vk
        set_prefix(monkeypatch, proof_prefix)
        check_prefix_record(prove(zk, c, pk), proof_prefix)


@pytest.mark.parametrize("lean,group", [(False, 24), (True, 0), (True, 24)], ids=["group24", "lean", "lean_group24"])
@pytest.mark.parametrize("family", ["E", "F"])
def test_coset_groups_and_a_lean_key_give_the_same_bytes(zk, cases, family, lean, group, monkeypatch):
    monkeypatch.delenv(PREFIX_ENV, raising=False)
    c = cases[family]
    with c.keygen(resident_cosets=not lean) as pk:
        assert pk.vk == c.want_vk
        rec = prove(zk, c, pk, dict(coset_group_polys=group) if group else None)
    if group:
        assert rec["coset_groups"] >= 2                                     # either family reads more than 24 polynomials in all
    else:
        assert rec["coset_groups"] == 0


# ------------------------------------------------------------------------------------------------ witness check
def bump(circuit, column, row):
    col = circuit.get("advice", column)
    col[row] = plonk.ints_to_mont([plonk.mont_to_ints(col[row:row + 1])[0] + 1])[0]
    circuit.set("advice", column, col)


def strip(failures):
    return [{k: v for k, v in f.items() if k != "message"} for f in failures]


@pytest.mark.parametrize("family", ["B", "C", "F", "G"])
def test_check_witness_reports_the_references_failures(zk, family, monkeypatch):
    monkeypatch.delenv(PREFIX_ENV, raising=False)
    pv = zk.prover
    c = Case(zk, family, seed=WITNESS_SEED)
    try:
        n, u, A = c.info["n"], c.info["usable"], c.info["num_advice"]
        with c.keygen() as pk:
            assert pv.check_witness(pk, c.circuit) == {"kind": "check", "n_failures": 0, "failures": []}
            with pv.Circuit.synthetic(c.protocol, seed=c.seed) as bad:
                cells = [(pc.reads_at(c.d, -1), 0), (pc.reads_at(c.d, 2), n - 1), (A - 1, u - 1)]
                for column, row in cells:
                    bump(bad, column, row)
                ref = wc.Reference.from_inputs(proof_inputs(bad, c.d, TAU, c.info))
                want = wc.expected_failures(ref, 16)
                failing = ref.gates()
                last_gate = A - 1 - c.d["synthetic"]["n_free"]              # the gates lead the numerator's list, one per dependent column
                assert len(failing) >= 3 and u - 1 in failing[last_gate], sorted(failing)
                assert any(1 in rows for rows in failing.values())          # rotation -1 reads row 0 from row 1
                chk = pv.check_witness(pk, bad)
                got = strip(chk["failures"])
                assert [f for f in got if f["kind"] != "lookup"] == want, "gates / copies differ from the definition"
                assert {f["index"]: (f["col_a"], f["row"], f["count"]) for f in got if f["kind"] == "lookup"} == {l: (0, row, 1) for l, row in ref.lookups().items()}
                assert chk["n_failures"] == len(chk["failures"])
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ refusal
def test_more_than_32_temporaries_are_refused_and_nothing_stays_behind(zk, cases, monkeypatch):
    monkeypatch.delenv(PREFIX_ENV, raising=False)
    lib, check = zk._capi.lib(), zk._capi.check
    cases["A"].keygen().close()                                             # a key of this size has come and gone: what is measured below is the refused call alone
    h = Case(zk, "H")                                                       # Protocol.from_json succeeds: the recogniser accepts any selector * (P - target)
    try:
        check(lib.mi355_synchronize()); check(lib.mi355_buf_trim())
        before = zk.halo2.mem_usage()["held"]
        with pytest.raises(zk.Mi355Error) as e:
            h.keygen()
        assert e.value.code == zk._capi.EBADARG and pc.LIMIT_TEXT in str(e.value) and pc.LIMIT_TEXT in lib.mi355_last_error().decode()
        check(lib.mi355_synchronize()); check(lib.mi355_buf_trim())
        assert zk.halo2.mem_usage()["held"] == before
    finally:
        h.close()
