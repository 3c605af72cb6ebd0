"""plonk::verify_proof on the device (halo2.verify_proof -> tests/cpp/test_verify_proof): the ten released proofs of tests/golden/kat.json are accepted under the released
-[s]G2 with the carried accumulator checked, and rejected with one bit changed; our own proofs verify under ParamsKZG's own g2 / s_g2 -- the pairing, not the trapdoor.
Every accept or reject is one oracle/plonk.py verify() reaches on the same input: each test asserts that first, on the CPU."""
import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk, pyref

from verify_common import ALL_TEN, NEG_S_G2_WORDS, P, case, layout, oracle_verify, product_protocol, same_as_oracle

pytestmark = pytest.mark.gpu
TAU0 = 0x5343524F4C4C0001


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


def product_verify(zk, layer, inst, proof, pkw, **over):
    return zk.halo2.verify_proof(product_protocol(layer), inst, proof, neg_s_g2=NEG_S_G2_WORDS, **dict(pkw, **over))


@pytest.mark.parametrize("name", ALL_TEN)
def test_released_proofs_are_accepted(zk, name):
    layer, inst, proof, okw, pkw = case(name)
    want = oracle_verify(layer, inst, proof, okw)
    assert want["ok"], want
    got = product_verify(zk, layer, inst, proof, pkw)
    assert got["ok"] and got["error"] == "" and got["has_accumulator"] and got["pairing"] == [1, 1], got
    same_as_oracle(got, want)
    assert got["msm"]["result"] == tuple(want["msm"]["result"])


TAMPER = ["commitment", "last_commitment", "first_evaluation", "last_evaluation", "shplonk_h", "shplonk_w", "instance_0", "instance_12", "instance_last", "wrong_transcript"]


@pytest.mark.parametrize("how", TAMPER)
@pytest.mark.parametrize("name", ["chunk_proof", "batch_proof", "bundle_proof"])
def test_tampered_released_proofs_are_rejected(zk, name, how):
    layer, inst, proof, okw, pkw = case(name)
    coms, evs, shp, nb = layout(layer, okw["transcript"])
    inst, proof, okw, pkw = list(inst), bytearray(proof), dict(okw), dict(pkw)
    at = {"commitment": coms[1], "last_commitment": coms[-1], "first_evaluation": evs[0], "last_evaluation": evs[-1], "shplonk_h": shp[0], "shplonk_w": shp[1]}
    if how in at:
        proof[at[how] + 2] ^= 1
    elif how.startswith("instance"):
        i = {"instance_0": 0, "instance_12": 12, "instance_last": len(inst) - 1}[how]
        inst[i] ^= 1
    else:
        okw["transcript"] = pkw["transcript"] = "blake2b" if okw["transcript"] == "poseidon" else "poseidon"
    assert not oracle_verify(layer, inst, bytes(proof), okw)["ok"]
    got = product_verify(zk, layer, inst, bytes(proof), pkw)
    assert not got["ok"] and got["error"] != "", got


def test_negated_accumulator_fails_its_own_group(zk):
    layer, inst, proof, okw, pkw = case("chunk_proof")
    y = inst[9] + (inst[10] << 88) + (inst[11] << 176)
    ny = (P - y) % P
    bad = list(inst); bad[9:12] = [ny & ((1 << 88) - 1), (ny >> 88) & ((1 << 88) - 1), ny >> 176]
    c = [bad[3 * i] + (bad[3 * i + 1] << 88) + (bad[3 * i + 2] << 176) for i in range(4)]
    assert pyref.g1_is_on_curve((c[2], c[3]))
    want = oracle_verify(layer, bad, proof, okw)
    assert not want["ok"]
    got = product_verify(zk, layer, bad, proof, pkw)
    assert not got["ok"] and got["has_accumulator"] and len(got["pairing"]) == 2 and got["pairing"][1] == 0, got
    # the accumulator alone, untouched by the transcript: the original holds, the negated one does not
    g1 = lambda pt: np.array(pyref.mont_limbs(pt[0], P) + pyref.mont_limbs(pt[1], P), dtype=np.uint64)
    o = [inst[3 * i] + (inst[3 * i + 1] << 88) + (inst[3 * i + 2] << 176) for i in range(4)]
    Ps = np.stack([g1((o[0], o[1])), g1((o[2], o[3])), g1((c[0], c[1])), g1((c[2], c[3]))])
    Qs = np.stack([zk.halo2.g2_generator(), NEG_S_G2_WORDS] * 2)
    assert zk.halo2.pairing_products(Ps, Qs, 2, 2, want_gt=False)[1].tolist() == [1, 0]
    # with the accumulator check off the verdict is whatever the changed instances give: the oracle's
    got = product_verify(zk, layer, bad, proof, pkw, check_accumulator=False)
    assert got["ok"] == want["ok"] and not got["has_accumulator"] and len(got["pairing"]) == 1, got
    same_as_oracle(got, want)


@pytest.mark.parametrize("layer", [2, 4])
def test_our_own_proofs_verify_by_the_pairing(zk, tmp_path, layer):
    rec = zk.replay.run(layer, k=8, out_dir=str(tmp_path / "good"))
    assert rec.get("ok"), rec.get("error")
    import json
    pr = plonk.Protocol(json.load(open(rec["protocol_path"])))
    inst = plonk.mont_to_ints(np.frombuffer(rec["instances"], dtype=np.uint64).reshape(-1, 4))
    tau = TAU0 + layer
    assert plonk.verify(pr, rec["vk"], inst, rec["proof"], tau, transcript=rec["transcript"])["ok"]
    params = zk.halo2.ParamsKZG.setup(8, tau)
    try:
        assert params.check_g2()
        got = zk.halo2.verify_proof(rec["protocol_path"], inst, rec["proof"], transcript=rec["transcript"], vk_bytes=rec["vk"], g2=params.g2, s_g2=params.s_g2)
        assert got["ok"] and got["pairing"] == [1] and not got["has_accumulator"], got
        got = zk.halo2.verify_proof(rec["protocol_path"], inst, rec["proof"], transcript=rec["transcript"], vk_bytes=rec["vk"], g2=params.g2, s_g2=params.g2)   # the wrong [s]G2
        assert not got["ok"] and got["error"] == "pairing"
        bad = zk.replay.run(layer, k=8, out_dir=str(tmp_path / "bad"), args=["--corrupt-witness"])
        assert "proof" in bad, bad.get("error")
        binst = plonk.mont_to_ints(np.frombuffer(bad["instances"], dtype=np.uint64).reshape(-1, 4))
        assert not plonk.verify(pr, bad["vk"], binst, bad["proof"], tau, transcript=bad["transcript"])["ok"]
        got = zk.halo2.verify_proof(bad["protocol_path"], binst, bad["proof"], transcript=bad["transcript"], vk_bytes=bad["vk"], g2=params.g2, s_g2=params.s_g2)
        assert not got["ok"] and got["error"] == "pairing", got
        keep = params.s_g2; params.s_g2 = params.g2
        assert not params.check_g2()
        params.s_g2 = keep
    finally:
        params.release()


def test_compiled_check_g2(zk, tmp_path):
    """the C++ twin ParamsKZG::check_g2 through the driver, on a params file written from a synthetic SRS: holds, and fails once s_g2 is replaced by g2"""
    import json, subprocess
    params = zk.halo2.ParamsKZG.setup(8, TAU0)
    try:
        path = str(tmp_path / "params8")
        params.write(path)
    finally:
        params.release()
    exe = ge.build_cpp("test_verify_proof")
    for extra, want in (([], True), (["--swap-g2"], False)):
        out = subprocess.run([exe, "--check-g2", path] + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert json.loads(out.stdout.strip().splitlines()[-1]) == {"check_g2": want, "k": 8}
