"""-m gpu: proofs of protocols with upstream halo2's classic lookup argument, made by the in-process prover (mi355_plonk_*) and once by tests/cpp/test_plonk_replay.
No CPU prover of this argument exists (the reference is mv-lookup throughout), so the proofs are pinned from two sides: the oracle's tree-walking verifier -- itself
pinned by the reference's released proofs -- accepts them through a subclass that overrides `_recognise` only (tests/classic_lookup_common.py), and the three
argument columns of every lookup (A', S', z) are recomputed on Python integers from the circuit read back through circuit_get and the challenges that verifier
re-derives, checked against all five constraints on every row, and their commitments under the trapdoor held equal to the ones the proof carries: the device's
columns bit for bit.  Shapes: layer 2 (one in-place lookup) and layer 3 (8 lookups) at k = 8 and 10, the layer-0 stand-in (three-column compressed lookups) at k = 9."""
import pytest

import __graft_entry__ as ge
from oracle import plonk, pyref
from tests import classic_lookup_common as cl
from tests.plonk_capi_common import SMALL0, tau_of

pytestmark = pytest.mark.gpu
CASES = [(2, 8), (2, 10), (3, 8), (3, 10), (0, 9)]
R = plonk.R


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


@pytest.fixture(scope="module")
def pv(zk):
    return zk.prover


class Layer:
    def __init__(self, zk, layer, k, lookup_argument="permuted"):
        self.zk, self.layer, self.k = zk, layer, k
        self.d = zk.protocols.layer_protocol(layer, k, lookup_argument=lookup_argument, **(SMALL0 if layer == 0 else {}))
        self.pr = cl.ClassicProtocol(self.d)
        self.protocol = zk.prover.Protocol.from_json(self.d)
        self.info = self.protocol.info()
        self.params = zk.halo2.ParamsKZG.setup(k, tau_of(layer))
        self.circuit = zk.prover.Circuit.synthetic(self.protocol)
        self.pk = zk.prover.keygen(self.protocol, self.circuit, self.params)

    def case(self, proof=None):
        return {"protocol": self.protocol, "vk_bytes": self.pk.vk, "instances": self.circuit.instances(), "proof": self.proof if proof is None else proof}

    def oracle_verdict(self, proof=None):
        try:
            return plonk.verify(self.pr, self.pk.vk, self.circuit.instances(), self.proof if proof is None else proof, tau_of(self.layer), transcript="poseidon")
        except AssertionError as e:                                     # a word that is no point / no canonical scalar
            return {"ok": False, "error": str(e)}

    def close(self):
        for x in (self.pk, self.circuit, self.protocol):
            x.close()
        self.params.release()


@pytest.fixture(scope="module")
def layers(zk):
    """the five cases, proven once; before the first and after the last permuted proof one mv-lookup proof of layer 2 at k = 8 (check 8)"""
    mv = Layer(zk, 2, 8, "mv")
    mv.proof, _ = zk.prover.create_proof(mv.params, mv.pk, mv.circuit)
    made = {"mv": mv}
    for layer, k in CASES:
        L = Layer(zk, layer, k)
        L.proof, L.record = zk.prover.create_proof(L.params, L.pk, L.circuit)
        L.verdict = L.oracle_verdict()
        made[(layer, k)] = L
    mv.proof_after, _ = zk.prover.create_proof(mv.params, mv.pk, mv.circuit)
    yield made
    for L in made.values():
        L.close()


# ------------------------------------------------------------------------------------------------ 1, 2, 3: the verifiers accept
@pytest.mark.parametrize("layer,k", CASES)
def test_the_oracle_verifier_and_the_library_accept(pv, layers, layer, k):
    L = layers[(layer, k)]
    assert L.info["lookup_permuted"] == 1 and len(L.proof) == L.info["proof_bytes_poseidon"] and L.record["transcript"] == "poseidon"
    assert L.verdict["ok"], L.verdict
    (one,) = pv.verify_proofs([L.case()], params=L.params, one_by_one=True)                        # plonk::verify_proof
    assert one["ok"] and one["error"] == "" and one["pairing"] == [1], (one["error"], one["detail"])
    (host,) = pv.verify_proofs([L.case()], options=dict(host_only=True), one_by_one=True)
    assert host["ok"] and host["host_only"] and host["pairing"] == []
    want = L.verdict
    assert one["numerator_at_x"] == want["numerator_at_x"] and one["challenges"]["theta"] == want["challenges"]["theta"] and one["challenges"]["x"] == want["challenges"]["x"]
    assert one["msm"]["scalars"] == [s % R for s in want["msm"]["scalars"]] and one["msm"]["result"] == tuple(want["msm"]["result"])
    for opts in (dict(device_scalars=True), dict(device_transcript=True), dict(device_scalars=True, device_transcript=True)):
        many = pv.verify_proofs([L.case(), L.case()], params=L.params, options=opts)             # plonk::verify_proofs, scalar side / transcripts on the device
        for r in many:
            assert {key: r[key] for key in one if key != "device_calls"} == {key: one[key] for key in one if key != "device_calls"}, opts


# ------------------------------------------------------------------------------------------------ 4: one byte off is a rejection
@pytest.mark.parametrize("layer,k", [(2, 8), (3, 8), (0, 9)])
def test_a_flipped_byte_in_the_arguments_words_is_rejected_by_both_verifiers(pv, layers, layer, k):
    L = layers[(layer, k)]; pr = L.pr
    lk = pr.lookups[-1]
    ev0 = 32 * (sum(pr.num_witness) + pr.Q)
    spots = {"A' commitment": 32 * (lk["perm_input"] - pr.wit0) + 3, "S' evaluation": ev0 + 32 * pr.evaluations.index((lk["perm_table"], 0)) + 5,
             "z evaluation": ev0 + 32 * pr.evaluations.index((lk["z"], 0)) + 7}
    for what, at in spots.items():
        bad = bytearray(L.proof); bad[at] ^= 1
        assert not L.oracle_verdict(bytes(bad))["ok"], what
        (rec,) = pv.verify_proofs([L.case(bytes(bad))], params=L.params, one_by_one=True)
        assert not rec["ok"] and rec["error"], what
        (rec,) = pv.verify_proofs([L.case(bytes(bad)), L.case()], params=L.params, options=dict(device_scalars=True, device_transcript=True))[:1]
        assert not rec["ok"], what


# ------------------------------------------------------------------------------------------------ 5: the device's columns, bit for bit
@pytest.mark.parametrize("layer,k", CASES)
def test_the_argument_columns_recomputed_in_python_are_the_committed_ones(layers, layer, k):
    L = layers[(layer, k)]; pr = L.pr; c = L.circuit
    col = lambda what, i: plonk.mont_to_ints(c.get(what, i))
    columns = {p: col("preprocessed", p) for p in range(pr.num_pre)}
    inst = col("instances", 0)
    columns[pr.inst0] = inst + [0] * (pr.n - len(inst))
    columns.update({pr.phase0[0] + a: col("advice", a) for a in range(pr.num_witness[0])})
    ch = L.verdict["challenges"]
    basis = cl.lagrange_basis_at(pr, tau_of(layer))
    in_proof = lambda p: pyref.g1_decompress(L.proof[32 * (p - pr.wit0):32 * (p - pr.wit0) + 32])
    for l, lk in enumerate(pr.lookups):
        a, s, z, a_in, s_in = cl.argument_columns(pr, lk, columns, ch["theta"], ch["beta"], ch["gamma"], col("perm_blind", l), col("lz_blind", l))
        cl.check_five_constraints(pr, a, s, z, a_in, s_in, ch["beta"], ch["gamma"])
        for name, column, p in (("A'", a, lk["perm_input"]), ("S'", s, lk["perm_table"]), ("z", z, lk["z"])):
            assert cl.commitment(basis, column) == in_proof(p), "lookup %d: the commitment of %s differs from the proof's" % (l, name)
    with pytest.raises(L.zk.Mi355Error):
        c.get("m", 0)                                                   # a permuted protocol's circuit carries no m


# ------------------------------------------------------------------------------------------------ 6: check_witness and a value outside the table
def test_check_witness_names_the_lookup_and_the_row_and_create_proof_refuses(zk, pv, layers):
    L = layers[(3, 8)]; pr = L.pr
    assert pv.check_witness(L.pk, L.circuit) == {"kind": "check", "n_failures": 0, "failures": []}
    target = 3
    a = pr.lookups[target]["input"]["DistributePowers"][0][0]["Polynomial"]["poly"] - pr.phase0[0]      # the lookup-advice column of lookup 3
    with pv.Circuit.synthetic(L.protocol) as c:
        column = c.get("advice", a)
        column[41] = plonk.ints_to_mont([(1 << 200) + 5])[0]            # no range table holds it
        c.set("advice", a, column)
        chk = pv.check_witness(L.pk, c)
        found = [(f["index"], f["row"]) for f in chk["failures"] if f["kind"] == "lookup"]
        assert found == [(target, 41)], chk["failures"]
        with pytest.raises(zk.Mi355Error) as e:
            pv.create_proof(L.params, L.pk, c)
        assert e.value.code == zk._capi.EBADARG and "lookup 3: input row 41 is not in the table" in str(e.value)
    again, _ = pv.create_proof(L.params, L.pk, L.circuit)                # the refusal left nothing behind
    assert again == L.proof


# ------------------------------------------------------------------------------------------------ 7: options
def test_device_randomness_is_refused_by_name_and_the_other_options_change_nothing(zk, pv, layers):
    L = layers[(2, 8)]
    with pytest.raises(zk.Mi355Error) as e:
        pv.create_proof(L.params, L.pk, L.circuit, dict(device_randomness=True, rng_key=bytes(range(32))))
    assert "device_randomness is not available for a protocol with the classic (permuted) lookup argument" in str(e.value)
    for options in (dict(device_multiplicities=True), dict(coset_group_polys=24), dict(sparse_uploads=True), dict(threads=2, upload_threads=2, early_intt=1, commit_batch=2)):
        proof, _ = pv.create_proof(L.params, L.pk, L.circuit, options)
        assert proof == L.proof, options
    with pv.Circuit.synthetic(L.protocol, blind_seed=5) as c:            # other blinding values: another proof, accepted as well
        proof, _ = pv.create_proof(L.params, L.pk, c)
        assert proof != L.proof and plonk.verify(L.pr, L.pk.vk, c.instances(), proof, tau_of(2), transcript="poseidon")["ok"]


def test_the_replay_program_makes_the_same_proof(zk, layers, tmp_path):
    rec = zk.replay.run(2, 8, out_dir=str(tmp_path), args=["--proofs", "1"], lookup_argument="permuted")
    assert rec.get("ok"), rec.get("error")
    L = layers[(2, 8)]
    assert rec["proof"] == L.proof and rec["vk"] == L.pk.vk
    assert rec["protocol"]["num_witness"] == [1, 2, 3] and rec["protocol"]["lookups"] == 1


# ------------------------------------------------------------------------------------------------ 8: no state leaks between the kinds
def test_an_mv_lookup_proof_is_the_same_before_and_after_the_permuted_ones(layers):
    mv = layers["mv"]
    assert mv.proof == mv.proof_after and len(mv.proof) == 896
    assert plonk.verify(plonk.Protocol(mv.d), mv.pk.vk, mv.circuit.instances(), mv.proof, tau_of(2), transcript="poseidon")["ok"]
