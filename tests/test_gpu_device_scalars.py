"""plonk::verify_proofs / plonk::aggregate with VerifyOptions::device_scalars (halo2.verify_proofs / halo2.aggregate with device_scalars=True -> tests/cpp/test_device_scalars):
the scalar side of every proof runs on the device, ONE mi355_fr_program_host call per distinct protocol of the batch.  Every record must equal, field for field, the record with
the option off (the route of tests/cpp/test_verify_proofs, which tests/test_gpu_verify_proofs.py holds to the oracle), failures included, with the transcripts on the host and
on the device; the call count grows by exactly the number of distinct protocols."""
import pytest

import __graft_entry__ as ge
from oracle import pyref

import aggregate_common as ac
from verify_common import ALL_TEN, NEG_S_G2_WORDS, case, layout

pytestmark = pytest.mark.gpu
ORDER = [4, 9, 0, 7, 2, 8, 6, 1, 5, 3]                      # the ten released proofs, shuffled: the three protocols interleave
NAMES = [ALL_TEN[i] for i in ORDER]
PROTOCOLS = 3                                               # chunk proofs (layer 2), batch proofs (layer 4), the bundle proof (layer 6)


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def strip(rec):
    return {k: v for k, v in rec.items() if k != "device_calls"}


def both(zk, cases, **kw):
    off = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS, **kw)
    on = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS, device_scalars=True, **kw)
    return off, on


@pytest.fixture(scope="module")
def ten(zk):
    return both(zk, [ac.product_case(n) for n in NAMES])


def test_the_ten_released_proofs_equal_the_host_route_and_are_accepted(ten):
    off, on = ten
    assert len(on) == 10
    for name, a, b in zip(NAMES, off, on):
        assert strip(b) == strip(a), name
        assert b["ok"] and b["error"] == "" and b["pairing"] == [1, 1], (name, b["error"], b["detail"])
    assert off[0]["device_calls"] == 3 and on[0]["device_calls"] == 3 + PROTOCOLS        # decompression, segmented MSM, pairing -- and one program call per protocol


def test_with_the_transcripts_on_the_device_as_well(zk, ten):
    on = zk.halo2.verify_proofs([ac.product_case(n) for n in NAMES], neg_s_g2=NEG_S_G2_WORDS, device_scalars=True, device_transcript=True)
    for name, a, b in zip(NAMES, ten[0], on):
        assert strip(b) == strip(a) and b["ok"], name
    assert on[0]["device_calls"] == 4 + PROTOCOLS


def with_changed_evaluations(names, which):
    cases = [ac.product_case(n) for n in names]
    for i in which:
        layer, inst, proof, okw, _ = case(names[i])
        _, evs, _, _ = layout(layer, okw["transcript"])
        bad = bytearray(proof); bad[evs[3 + i % 4] + 2] ^= 1
        cases[i] = ac.product_case(names[i], proof=bytes(bad))
    return cases


@pytest.mark.parametrize("device_transcript", [False, True])
def test_a_changed_evaluation_word_in_three_proofs_fails_their_pairing_alone(zk, ten, device_transcript):
    which = (0, 3, 6)                                                                      # a chunk proof, a batch proof, another chunk proof
    off, on = both(zk, with_changed_evaluations(NAMES, which), device_transcript=device_transcript)
    for i in range(10):
        assert strip(on[i]) == strip(off[i]), i
        if i in which:
            assert not on[i]["ok"] and on[i]["error"] == "pairing" and on[i]["pairing"][0] == 0, (i, on[i]["error"])
        else:
            assert on[i]["ok"] and strip(on[i]) == strip(ten[1][i]), i
    assert on[0]["device_calls"] == off[0]["device_calls"] + PROTOCOLS


def test_a_non_canonical_scalar_keeps_its_name_and_never_reaches_the_program(zk, ten):
    name = NAMES[2]
    layer, inst, proof, okw, _ = case(name)
    _, evs, _, _ = layout(layer, okw["transcript"])
    bad = bytearray(proof); bad[evs[5]:evs[5] + 32] = pyref.R_MOD.to_bytes(32, "little")             # the word r itself
    cases = [ac.product_case(n) for n in NAMES]
    cases[2] = ac.product_case(name, proof=bytes(bad))
    off, on = both(zk, cases)
    assert not on[2]["ok"] and on[2]["error"] == "non_canonical_scalar" and strip(on[2]) == strip(off[2])
    for i in range(10):
        if i != 2:
            assert strip(on[i]) == strip(ten[1][i]) and on[i]["ok"], i
    alone_off, alone_on = both(zk, [cases[2]])
    assert strip(alone_on[0]) == strip(alone_off[0]) and alone_on[0]["device_calls"] == alone_off[0]["device_calls"] == 1     # the decompression; no program call, no MSM


def test_a_host_only_proof_inside_the_batch(zk, ten):
    cases = [ac.product_case(n) for n in NAMES]
    on = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS, device_scalars=True, host_only_at=[4])
    alone = zk.halo2.verify_proofs([cases[4]], host_only=True)[0]
    assert on[4]["host_only"] and on[4]["ok"] and on[4]["pairing"] == [] and strip(on[4]) == strip(alone)
    for key in ("challenges", "numerator_at_x"):
        assert on[4][key] == ten[0][4][key]
    assert on[4]["msm"]["scalars"] == ten[0][4]["msm"]["scalars"] and on[4]["msm"]["points"] == ten[0][4]["msm"]["points"]
    for i in range(10):
        if i != 4:
            assert strip(on[i]) == strip(ten[1][i]), i
    assert on[0]["device_calls"] == 3 + PROTOCOLS                                          # the chunk proofs' group lost one member, not its call


def test_aggregate_over_the_nine_poseidon_proofs(zk):
    cases = [ac.product_case(n) for n in NAMES if n != "bundle_proof"]
    off = zk.halo2.aggregate(cases, neg_s_g2=NEG_S_G2_WORDS)
    on = zk.halo2.aggregate(cases, neg_s_g2=NEG_S_G2_WORDS, device_scalars=True)
    assert off["ok"] and on["ok"] and on["pairing"] == 1, on["error"] + on["detail"]
    for key in ("r", "lhs", "rhs", "limbs", "accumulators"):
        assert on[key] == off[key], key
    assert len(on["limbs"]) == 12 and [strip(r) for r in on["proofs"]] == [strip(r) for r in off["proofs"]]
    assert on["device_calls"] == off["device_calls"] + 2                                   # two protocols among the nine


def test_the_seven_chunk_proofs_tiled_to_130(zk):
    cases = [ac.product_case(n) for n in ac.SEVEN]
    off = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS, tile=130)
    on = zk.halo2.verify_proofs(cases, neg_s_g2=NEG_S_G2_WORDS, device_scalars=True, tile=130)
    assert len(on) == 130 and on[0]["device_calls"] == off[0]["device_calls"] + 1 == 4     # two wavefronts and a ragged tail in ONE program call
    for i, (a, b) in enumerate(zip(off, on)):
        assert b["ok"], (i, b["error"], b["detail"])
        assert strip(b) == strip(a), i
