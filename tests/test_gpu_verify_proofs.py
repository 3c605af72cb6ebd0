"""plonk::verify_proofs on the device (halo2.verify_proofs -> tests/cpp/test_verify_proofs): N proofs through ONE decompression, ONE segmented MSM and ONE pairing call.  The ten
released proofs (layers 2, 4, 6) in one batch under the released -[s]G2; one changed bit rejects exactly its proof; a negated accumulator fails its own group alone; a batch
that fails on the host makes no device call; our own proofs verify under ParamsKZG's own g2 / s_g2.  Every accept or reject is the oracle's first (oracle/plonk.py, on the CPU),
and every record is held to what the unchanged single verify_proof returns."""
import json

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk, pyref

import aggregate_common as ac
from verify_common import ALL_TEN, NEG_S_G2_WORDS, P, case, layout, oracle_verify, product_protocol, same_as_oracle

pytestmark = pytest.mark.gpu
TAU0 = 0x5343524F4C4C0001


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


@pytest.fixture(scope="module")
def seven(zk):
    """the seven chunk proofs, untouched, in one batch: what the other six of a tampered batch must still equal"""
    return zk.halo2.verify_proofs([ac.product_case(n) for n in ac.SEVEN], neg_s_g2=NEG_S_G2_WORDS)


def strip(rec):
    return {k: v for k, v in rec.items() if k != "device_calls"}


def test_all_ten_released_proofs_in_one_call(zk):
    for name in ALL_TEN:
        assert ac.oracle_verdict(name)["ok"], name                            # the oracle accepts: what follows is the product's
    got = zk.halo2.verify_proofs([ac.product_case(n) for n in ALL_TEN], neg_s_g2=NEG_S_G2_WORDS)
    assert got[0]["device_calls"] == 3                                         # one decompression (nine compressed proofs), one segmented MSM, one pairing call
    for name, rec in zip(ALL_TEN, got):
        want = ac.oracle_verdict(name)
        assert rec["ok"] and rec["error"] == "" and rec["has_accumulator"] and rec["pairing"] == [1, 1], (name, rec)
        same_as_oracle(rec, want)
        assert rec["msm"]["result"] == tuple(want["msm"]["result"]), name
    loop = zk.halo2.verify_proofs([ac.product_case(n) for n in ALL_TEN], neg_s_g2=NEG_S_G2_WORDS, one_by_one=True)   # the unchanged verify_proof, proof by proof
    assert [strip(r) for r in loop] == [strip(r) for r in got]
    layer, inst, proof, _, pkw = case("batch_proof")                           # and through verify_proof's own driver
    assert strip(got[ALL_TEN.index("batch_proof")]) == zk.halo2.verify_proof(product_protocol(layer), inst, proof, neg_s_g2=NEG_S_G2_WORDS, **pkw)


@pytest.mark.parametrize("where", ["evaluation", "shplonk_w", "instance_12"])
def test_one_flipped_bit_rejects_exactly_its_proof(zk, seven, where):
    name = ac.SEVEN[3]
    layer, inst, proof, okw, pkw = case(name)
    _, evs, shp, _ = layout(layer, okw["transcript"])
    inst, proof = list(inst), bytearray(proof)
    if where == "instance_12":
        inst[12] ^= 1
    elif where == "evaluation":
        proof[evs[5] + 2] ^= 1
    else:                                                                      # the first bit of W' (from byte 2 on) whose flip is still the word of a curve point: the
        w0 = shp[1]                                                            # proof then passes the host part and it is the pairing that rejects it
        for k in range(2, 32):
            word = bytearray(proof[w0:w0 + 32]); word[k] ^= 1
            try:
                if pyref.g1_decompress(bytes(word)) is not None:
                    proof[w0 + k] ^= 1
                    break
            except AssertionError:
                pass
        else:
            raise AssertionError("no flipped bit of W' is a point")
    assert not oracle_verify(layer, inst, bytes(proof), okw)["ok"]
    cases = [ac.product_case(n) for n in ac.SEVEN]
    cases[3] = ac.product_case(name, inst=inst, proof=bytes(proof))
    got = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS)
    assert [r["ok"] for r in got] == [True, True, True, False, True, True, True]
    assert got[3]["error"] == "pairing" and got[3]["pairing"] == [0, 1], got[3]
    assert strip(got[3]) == zk.halo2.verify_proof(product_protocol(layer), inst, bytes(proof), neg_s_g2=NEG_S_G2_WORDS, **pkw)
    for i in (0, 1, 2, 4, 5, 6):
        assert strip(got[i]) == strip(seven[i]), i


def test_negated_accumulator_fails_its_own_group_alone(zk, seven):
    name = ac.SEVEN[3]
    layer, inst, proof, okw, pkw = case(name)
    y = inst[9] + (inst[10] << 88) + (inst[11] << 176)
    ny = (P - y) % P
    bad = list(inst); bad[9:12] = [ny & ((1 << 88) - 1), (ny >> 88) & ((1 << 88) - 1), ny >> 176]
    assert pyref.g1_is_on_curve(ac.carried(bad)[1])
    want = oracle_verify(layer, bad, proof, okw)
    assert not want["ok"]
    cases = [ac.product_case(n) for n in ac.SEVEN]
    cases[3] = ac.product_case(name, inst=bad)
    got = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS)
    assert [r["ok"] for r in got] == [True, True, True, False, True, True, True]
    # the carried accumulator's group is 0.  The instances are absorbed by the transcript, so the changed limbs move the challenges as well: the proof's own group is whatever
    # the oracle's pairing says on the same input, and the first failed check gives the name
    own = int(bool(want.get("pairing")))
    assert got[3]["pairing"] == [own, 0] and got[3]["error"] == ("accumulator_pairing" if own else "pairing"), got[3]
    assert strip(got[3]) == zk.halo2.verify_proof(product_protocol(layer), bad, proof, neg_s_g2=NEG_S_G2_WORDS, **pkw)
    for i in (0, 1, 2, 4, 5, 6):
        assert strip(got[i]) == strip(seven[i]), i


def test_the_groups_of_one_proof_do_not_shift_the_next(zk):
    """the same proof twice, once with its accumulator check off (one group) and once on (two): the flags are dealt out by each proof's own group count"""
    name = ac.SEVEN[0]
    got = zk.halo2.verify_proofs([ac.product_case(name, check_accumulator=False), ac.product_case(name)], neg_s_g2=NEG_S_G2_WORDS)
    assert got[0]["ok"] and got[0]["pairing"] == [1] and not got[0]["has_accumulator"]
    assert got[1]["ok"] and got[1]["pairing"] == [1, 1] and got[1]["has_accumulator"]


def test_a_batch_that_fails_on_the_host_makes_no_device_call_after_decoding(zk):
    cut = [ac.product_case(n, proof=case(n)[2][:-32]) for n in ac.SEVEN[:3]]
    got = zk.halo2.verify_proofs(cut, neg_s_g2=NEG_S_G2_WORDS)
    assert all(not r["ok"] and r["error"] == "proof_length" for r in got)
    assert got[0]["device_calls"] == 0


@pytest.fixture(scope="module")
def own_proofs(zk, tmp_path_factory):
    out = {}
    for layer in (2, 4):
        rec = zk.replay.run(layer, k=8, out_dir=str(tmp_path_factory.mktemp("own%d" % layer)))
        assert rec.get("ok"), rec.get("error")
        out[layer] = rec
    return out


def test_our_own_proofs_of_two_layers_in_one_batch(zk, own_proofs):
    """our own layer-2 and layer-4 proofs at k = 8 in ONE batch -- two protocols, two keys.  replay.run derives the trapdoor of its synthetic SRS from the layer (TAU0 + layer),
    so no single [s]G2 fits both: under layer 2's ParamsKZG the batch accepts the layer-2 proof and rejects the other with `pairing`, under layer 4's the reverse, and with
    s_g2 = g2 both are rejected.  It is the pairing that decides, proof by proof, and every record equals single verify_proof's under the same points."""
    cases, srs = [], {}
    for layer in (2, 4):
        rec = own_proofs[layer]
        pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
        inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
        assert plonk.verify(pr, rec["vk"], inst, rec["proof"], TAU0 + layer, transcript=rec["transcript"])["ok"]
        assert not plonk.verify(pr, rec["vk"], inst, rec["proof"], TAU0 + 6 - layer, transcript=rec["transcript"])["ok"]      # and not under the other layer's trapdoor
        cases.append(dict(protocol=rec["protocol_path"], instances=inst, proof=rec["proof"], transcript=rec["transcript"], vk_bytes=rec["vk"]))
        params = zk.halo2.ParamsKZG.setup(8, TAU0 + layer)
        try:
            assert params.check_g2()
            srs[layer] = (params.g2, params.s_g2)
        finally:
            params.release()
    single = lambda c, g2, s_g2: zk.halo2.verify_proof(c["protocol"], c["instances"], c["proof"], transcript=c["transcript"], vk_bytes=c["vk_bytes"], g2=g2, s_g2=s_g2)
    for layer, verdicts in ((2, [True, False]), (4, [False, True])):
        g2, s_g2 = srs[layer]
        got = zk.halo2.verify_proofs(cases, g2=g2, s_g2=s_g2)
        assert [r["ok"] for r in got] == verdicts and [r["pairing"] for r in got] == [[int(v)] for v in verdicts], got
        assert [r["error"] for r in got] == ["" if v else "pairing" for v in verdicts] and not any(r["has_accumulator"] for r in got)
        assert [strip(r) for r in got] == [single(c, g2, s_g2) for c in cases]
    g2 = srs[2][0]
    got = zk.halo2.verify_proofs(cases, g2=g2, s_g2=g2)                      # the wrong [s]G2 for both
    assert all(not r["ok"] and r["error"] == "pairing" and r["pairing"] == [0] for r in got), got
