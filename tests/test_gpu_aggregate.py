"""plonk::aggregate on the device (halo2.aggregate -> tests/cpp/test_verify_proofs --aggregate): the KZG accumulators of N proofs folded with the powers of a transcript challenge
into the accumulator the next layer's first twelve instances carry.  No fixture pins the challenge r (the reference stores no layer-1 or layer-3 proof): what is verified here is
the algebra -- the fold equals an independent restatement with Python integers (tests/aggregate_common.py), satisfies the pairing under the released -[s]G2, and its limbs are
accepted back as a carried accumulator."""
import json

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk, pyref

import aggregate_common as ac
from verify_common import ALL_TEN, NEG_S_G2_WORDS, P, case, g1_abi, layout, oracle_verify

pytestmark = pytest.mark.gpu
TAU0 = 0x5343524F4C4C0001


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


@pytest.mark.parametrize("names", [ac.SEVEN, ALL_TEN], ids=["seven_chunk_proofs", "all_ten"])
def test_fold_of_released_proofs(zk, names):
    names = list(names)
    for n in names:
        assert ac.oracle_verdict(n)["ok"], n
    accs, r = ac.restated(names)
    lhs, rhs = ac.fold(accs, r)
    got = zk.halo2.aggregate([ac.product_case(n) for n in names], neg_s_g2=NEG_S_G2_WORDS)
    assert got["ok"] and got["error"] == "" and got["pairing"] == 1, got["error"] + ": " + got["detail"]
    assert got["accumulators"] == accs and got["r"] == r
    assert (got["lhs"], got["rhs"]) == (lhs, rhs)
    assert got["device_calls"] == 4                                            # decompression, the lists' segmented MSM, the fold's, the pairing
    for n, rec in zip(names, got["proofs"]):
        assert rec["ok"] and rec["msm"]["result"] == tuple(ac.oracle_verdict(n)["msm"]["result"]) and rec["pairing"] == []
    # the limbs: below 2^88, the restatement's, and they decode back to the points
    assert all(0 <= v < (1 << 88) for v in got["limbs"]) and got["limbs"] == ac.limbs(lhs, rhs)
    assert ac.carried(got["limbs"]) == (lhs, rhs)
    # ... and are accepted as a carried accumulator: the pairing on the decoded pair
    back = ac.carried(got["limbs"])
    Ps = g1_abi([back[0], back[1]])
    Qs = np.stack([zk.halo2.g2_generator(), NEG_S_G2_WORDS])
    assert zk.halo2.pairing_products(Ps, Qs, 1, 2, want_gt=False)[1].tolist() == [1]


def test_a_single_proof_without_an_accumulator_is_its_own_fold(zk, tmp_path):
    """our own k = 8 layer-2 proof with accumulator=0: one accumulator, r^0 = 1, so the result is that proof's (msm result, W') -- judged under the proof's own SRS"""
    rec = zk.replay.run(2, k=8, out_dir=str(tmp_path / "own"))
    assert rec.get("ok"), rec.get("error")
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
    want = plonk.verify(pr, rec["vk"], inst, rec["proof"], TAU0 + 2, transcript=rec["transcript"])
    assert want["ok"]
    c = dict(protocol=rec["protocol_path"], instances=inst, proof=rec["proof"], transcript=rec["transcript"], vk_bytes=rec["vk"], check_accumulator=False)
    params = zk.halo2.ParamsKZG.setup(8, TAU0 + 2)
    try:
        g2, s_g2 = params.g2, params.s_g2
    finally:
        params.release()
    got = zk.halo2.aggregate([c], g2=g2, s_g2=s_g2)
    assert got["ok"] and got["pairing"] == 1, got["error"] + ": " + got["detail"]
    own = (tuple(want["msm"]["result"]), tuple(want["msm"]["w_prime"]))
    assert got["accumulators"] == [own] and (got["lhs"], got["rhs"]) == own
    assert got["r"] == ac.challenge([own]) and ac.carried(got["limbs"]) == own
    got = zk.halo2.aggregate([c], g2=g2, s_g2=g2)                             # the wrong [s]G2
    assert not got["ok"] and got["error"] == "aggregate_pairing" and got["pairing"] == 0


def test_one_flipped_bit_fails_the_aggregate_pairing_and_the_fold_is_still_returned(zk):
    name = ac.SEVEN[2]
    layer, inst, proof, okw, _ = case(name)
    _, evs, _, _ = layout(layer, okw["transcript"])
    bad = bytearray(proof); bad[evs[5] + 2] ^= 1
    want = oracle_verify(layer, inst, bytes(bad), okw)
    assert not want["ok"] and "msm" in want                                    # rejected by the pairing, not on the host
    cases = [ac.product_case(n) for n in ac.SEVEN]
    cases[2] = ac.product_case(name, proof=bytes(bad))
    got = zk.halo2.aggregate(cases, neg_s_g2=NEG_S_G2_WORDS)
    assert not got["ok"] and got["error"] == "aggregate_pairing" and got["pairing"] == 0, got
    # the independent restatement on the same (wrong) accumulators
    verdicts = [want if n == name else ac.oracle_verdict(n) for n in ac.SEVEN]
    accs = ac.accumulators(verdicts, [case(n)[1] for n in ac.SEVEN], [True] * 7)
    r = ac.challenge(accs)
    assert got["accumulators"] == accs and got["r"] == r and (got["lhs"], got["rhs"]) == ac.fold(accs, r)
    fold_only = zk.halo2.aggregate(cases, pairing=False)                       # srs = nullptr: the fold, no verdict
    assert fold_only["ok"] and fold_only["pairing"] == 0 and (fold_only["lhs"], fold_only["rhs"], fold_only["limbs"]) == (got["lhs"], got["rhs"], got["limbs"])
    assert fold_only["device_calls"] == 3


def test_a_proof_cut_short_fails_the_aggregation_with_its_index(zk):
    cases = [ac.product_case(n) for n in ac.SEVEN[:4]]
    cases[2] = ac.product_case(ac.SEVEN[2], proof=case(ac.SEVEN[2])[2][:-32])
    got = zk.halo2.aggregate(cases, neg_s_g2=NEG_S_G2_WORDS)
    assert not got["ok"] and got["error"] == "proof_length" and got["detail"].startswith("proof 2:"), got
    assert got["accumulators"] == [] and got["device_calls"] == 1              # the one decompression of the other three proofs' words; no MSM, no pairing
