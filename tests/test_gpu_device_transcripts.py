"""plonk::verify_proofs / plonk::aggregate with VerifyOptions::device_transcript (halo2.verify_proofs / halo2.aggregate with device_transcript=True ->
tests/cpp/test_device_transcripts): the Poseidon transcripts of a batch recorded on the host, hashed by ONE mi355_poseidon_transcripts_host call, replayed.  Every record
must equal, field for field, the record with the option off (the route of tests/cpp/test_verify_proofs, which tests/test_gpu_verify_proofs.py holds to the oracle); the
call count grows by exactly one; named failures of the transcript section stay what they were; a batch without a Poseidon proof makes no transcript call."""
import pytest

import __graft_entry__ as ge
from oracle import pyref

import aggregate_common as ac
from verify_common import ALL_TEN, NEG_S_G2_WORDS, case, layout

pytestmark = pytest.mark.gpu
NINE = ALL_TEN[:9]


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def strip(rec):
    return {k: v for k, v in rec.items() if k != "device_calls"}


def both(zk, cases, **kw):
    off = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS, **kw)
    on = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS, device_transcript=True, **kw)
    return off, on


@pytest.fixture(scope="module")
def ten(zk):
    return both(zk, [ac.product_case(n) for n in ALL_TEN])


def test_the_ten_released_proofs_equal_the_host_route_and_are_accepted(ten):
    off, on = ten
    assert len(on) == 10
    for name, a, b in zip(ALL_TEN, off, on):
        assert strip(b) == strip(a), name
        assert b["ok"] and b["error"] == "" and b["pairing"] == [1, 1], (name, b["error"], b["detail"])
    assert off[0]["device_calls"] == 3 and on[0]["device_calls"] == 4                 # decompression, segmented MSM, pairing -- and the transcripts


def test_one_flipped_bit_in_an_evaluation_is_rejected_under_the_same_name(zk, ten):
    name = ALL_TEN[3]
    layer, inst, proof, okw, _ = case(name)
    _, evs, _, _ = layout(layer, okw["transcript"])
    bad = bytearray(proof); bad[evs[5] + 2] ^= 1
    cases = [ac.product_case(n) for n in ALL_TEN]
    cases[3] = ac.product_case(name, proof=bytes(bad))
    off, on = both(zk, cases)
    assert not on[3]["ok"] and on[3]["error"] == off[3]["error"] == "pairing" and strip(on[3]) == strip(off[3])
    for i in range(10):
        if i != 3:
            assert strip(on[i]) == strip(ten[1][i]) and on[i]["ok"], i


def not_a_point_word(word: bytes) -> bytes:
    for d in range(1, 64):
        w = bytearray(word); w[0] = (w[0] + d) & 0xFF
        try:
            if pyref.g1_decompress(bytes(w)) is None:
                return bytes(w)
        except AssertionError:
            return bytes(w)
    raise AssertionError("no rejected word nearby")


def test_an_invalid_point_keeps_its_name_and_the_batch_goes_on(zk, ten):
    name = ALL_TEN[3]
    layer, inst, proof, okw, _ = case(name)
    coms, _, _, _ = layout(layer, okw["transcript"])
    bad = bytearray(proof); bad[coms[2]:coms[2] + 32] = not_a_point_word(proof[coms[2]:coms[2] + 32])
    cases = [ac.product_case(n) for n in ALL_TEN]
    cases[3] = ac.product_case(name, proof=bytes(bad))
    off, on = both(zk, cases)
    assert not on[3]["ok"] and on[3]["error"] == "invalid_point" and strip(on[3]) == strip(off[3])
    assert on[0]["device_calls"] == off[0]["device_calls"] + 1
    for i in range(10):
        if i != 3:
            assert strip(on[i]) == strip(ten[1][i]) and on[i]["ok"], i


def test_a_batch_of_the_bundle_proof_alone_makes_no_transcript_call(zk, ten):
    off, on = both(zk, [ac.product_case("bundle_proof")])
    assert on[0]["ok"] and strip(on[0]) == strip(off[0]) == strip(ten[0][9])
    assert on[0]["device_calls"] == off[0]["device_calls"] == 2                      # uncompressed points: the segmented MSM and the pairing, nothing else


def test_the_seven_chunk_proofs_tiled_to_130(zk, ten):
    got = zk.halo2.verify_proofs([ac.product_case(n) for n in ac.SEVEN], neg_s_g2=NEG_S_G2_WORDS, device_transcript=True, tile=130)
    assert len(got) == 130 and got[0]["device_calls"] == 4
    for i, rec in enumerate(got):
        assert rec["ok"], (i, rec["error"], rec["detail"])
        assert strip(rec) == strip(ten[1][i % 7]), i


def test_aggregate_over_the_nine_poseidon_proofs(zk):
    cases = [ac.product_case(n) for n in NINE]
    off = zk.halo2.aggregate(cases, neg_s_g2=NEG_S_G2_WORDS)
    on = zk.halo2.aggregate(cases, neg_s_g2=NEG_S_G2_WORDS, device_transcript=True)
    assert off["ok"] and on["ok"] and on["pairing"] == 1, on["error"] + on["detail"]
    for key in ("r", "lhs", "rhs", "limbs", "accumulators"):
        assert on[key] == off[key], key
    assert len(on["limbs"]) == 12 and [strip(r) for r in on["proofs"]] == [strip(r) for r in off["proofs"]]
    assert on["device_calls"] == off["device_calls"] + 1
