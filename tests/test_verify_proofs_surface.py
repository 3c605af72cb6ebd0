"""CPU-only: the host side of plonk::verify_proofs and plonk::aggregate (halo2.verify_proofs / halo2.aggregate with host_only=True -> tests/cpp/test_verify_proofs).  A batch of
all ten released proofs -- layers 2, 4 and 6, two transcripts -- gives, proof by proof, the record verify_proof gives alone and the oracle's values; a proof that fails on the
host keeps its named failure and leaves the others unchanged; the accumulator list and the challenge r of the aggregation equal tests/aggregate_common.py's restatement."""
import json
import os

import pytest

import __graft_entry__ as ge
from oracle import pyref

import aggregate_common as ac
from verify_common import ALL_TEN, GOLD, case, layout, product_protocol, same_as_oracle

R = pyref.R_MOD


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def batch_of_ten(zk):
    return zk.halo2.verify_proofs([ac.product_case(n) for n in ALL_TEN], host_only=True)


@pytest.fixture(scope="module")
def batch_of_seven(zk):
    return zk.halo2.verify_proofs([ac.product_case(n) for n in ac.SEVEN], host_only=True)


def strip(rec):
    return {k: v for k, v in rec.items() if k != "device_calls"}


def test_every_record_of_the_batch_equals_the_oracle(batch_of_ten):
    assert len(batch_of_ten) == 10
    for name, got in zip(ALL_TEN, batch_of_ten):
        want = ac.oracle_verdict(name)
        assert want["ok"], (name, want)
        assert got["ok"] and got["error"] == "" and got["host_only"] and got["has_accumulator"] and got["pairing"] == [], (name, got)
        same_as_oracle(got, want)
    assert batch_of_ten[0]["device_calls"] == 0


@pytest.mark.parametrize("name", ["chunk_proof", "more_chunk_proofs:3", "batch_proof", "bundle_proof"])
def test_records_equal_single_verify_proof(zk, batch_of_ten, name):
    layer, inst, proof, _, pkw = case(name)
    alone = zk.halo2.verify_proof(product_protocol(layer), inst, proof, host_only=True, **pkw)
    assert strip(batch_of_ten[ALL_TEN.index(name)]) == alone


def test_one_by_one_mode_gives_the_same_records(zk, batch_of_seven):
    loop = zk.halo2.verify_proofs([ac.product_case(n) for n in ac.SEVEN], host_only=True, one_by_one=True)
    assert [strip(r) for r in loop] == [strip(r) for r in batch_of_seven]


def test_lists_equal_the_released_kats(batch_of_ten):
    kats = json.load(open(os.path.join(GOLD, "released_kats.json")))
    seen = 0
    for name, got in zip(ALL_TEN, batch_of_ten):
        if name not in kats or "msm" not in kats[name]:
            continue
        kat = kats[name]["msm"]; seen += 1
        assert got["msm"]["scalars"] == [int(s, 16) for s in kat["scalars"]]
        assert got["msm"]["points"] == [(int(p[0], 16), int(p[1], 16)) for p in kat["points"]]
        assert got["msm"]["w_prime"] == (int(kat["w_prime"][0], 16), int(kat["w_prime"][1], 16))
    assert seen >= 3


def not_a_point_word(word: bytes) -> bytes:
    for d in range(1, 64):
        w = bytearray(word); w[0] = (w[0] + d) & 0xFF
        try:
            if pyref.g1_decompress(bytes(w)) is None:
                return bytes(w)
        except AssertionError:
            return bytes(w)
    raise AssertionError("no rejected word nearby")


def broken(how):
    """proof 3 of the seven chunk proofs with one defect"""
    layer, inst, proof, okw, _ = case(ac.SEVEN[3])
    coms, evs, _, _ = layout(layer, okw["transcript"])
    if how == "proof_length":
        return proof[:-32]
    bad = bytearray(proof)
    if how == "non_canonical_scalar":
        bad[evs[3]:evs[3] + 32] = R.to_bytes(32, "little")
    else:
        bad[coms[2]:coms[2] + 32] = not_a_point_word(proof[coms[2]:coms[2] + 32])
    return bytes(bad)


@pytest.mark.parametrize("how", ["proof_length", "non_canonical_scalar", "invalid_point"])
def test_a_host_failure_keeps_its_name_and_leaves_the_others_unchanged(zk, batch_of_seven, how):
    cases = [ac.product_case(n) for n in ac.SEVEN]
    cases[3] = ac.product_case(ac.SEVEN[3], proof=broken(how))
    got = zk.halo2.verify_proofs(cases, host_only=True)
    assert not got[3]["ok"] and got[3]["error"] == how, got[3]
    layer, inst, _, _, pkw = case(ac.SEVEN[3])
    assert strip(got[3]) == zk.halo2.verify_proof(product_protocol(layer), inst, broken(how), host_only=True, **pkw)
    for i in (0, 1, 2, 4, 5, 6):
        assert strip(got[i]) == strip(batch_of_seven[i]), i


@pytest.mark.parametrize("names", [ac.SEVEN, ALL_TEN], ids=["seven_chunk_proofs", "all_ten"])
def test_aggregate_host_side_equals_the_restatement(zk, names):
    """the accumulator list (count and order: each proof's own, then the one it carries) and r; the sums of the lists come from the oracle here, the fold is the device's"""
    accs, r = ac.restated(list(names))
    got = zk.halo2.aggregate([ac.product_case(n) for n in names], host_only=True)
    assert got["ok"] and got["error"] == "" and got["device_calls"] == 0, got["error"] + got["detail"]
    assert len(got["accumulators"]) == 2 * len(names) == len(accs)
    assert got["accumulators"] == accs
    assert got["r"] == r


def test_aggregate_names_the_proof_that_fails(zk):
    cases = [ac.product_case(n) for n in ac.SEVEN[:3]]
    cases[1] = ac.product_case(ac.SEVEN[1], proof=case(ac.SEVEN[1])[2][:-32])
    got = zk.halo2.aggregate(cases, host_only=True)
    assert not got["ok"] and got["error"] == "proof_length" and got["detail"].startswith("proof 1:"), got
