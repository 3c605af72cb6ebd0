"""The BN254 pairing on the device (mi355_pairing_products_host) against oracle/pairing.py.  Expected GT values are taken cheaply as E^s with E = e(G1, G2) computed once
and s = sum a_i b_i mod r for pairs (a_i G1, b_i G2) made with the C oracle; the shapes are the wave and workgroup edges of the lane mapping and of the product tree."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import cref, pairing, pyref

import gpu_common as gc

pytestmark = pytest.mark.gpu

R, P = pyref.R_MOD, pyref.P_MOD
RINV_P = pow(pyref.MONT_R, -1, P)
F12 = pairing.F12
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 64), (1, 65), (63, 2), (64, 2), (65, 2), (3, 257)]


@pytest.fixture(scope="module")
def zk():
    pkg = ge.load_package()
    pkg.init(0)
    return pkg


@pytest.fixture(scope="module")
def E():
    return pairing.pairing(pyref.G2_GEN, pyref.G1_GEN)


def gt_words(x):
    """oracle F12 -> 48 u64 in the ABI's layout (the inverse of the basis map: a1 = c[k + 6], a0 = c[k] + 9 a1 at k = 2 i + j)"""
    out = []
    for m in range(6):
        j, i = divmod(m, 3)
        a1 = x.c[2 * i + j + 6]
        out += pyref.mont_limbs((x.c[2 * i + j] + 9 * a1) % P, P) + pyref.mont_limbs(a1, P)
    return np.array(out, dtype=np.uint64)


def make_pairs(a, b):
    """(a_i G1, b_i G2) as ABI arrays; a zero scalar gives the identity"""
    g1 = cref.g1_mul_generator_vec(np.stack([cref.fr_mont(int(x)) for x in a]))
    gen2 = cref.g2_generator()
    memo = {}
    q = []
    for x in b:
        x = int(x) % R
        if x not in memo:
            memo[x] = cref.g2_mul(gen2, cref.fr_mont(x)) if x else np.zeros(16, dtype=np.uint64)
        q.append(memo[x])
    return np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 8), np.stack(q).astype(np.uint64)


def shape_case(groups, ppg, seed):
    """scalars for a shape: group `one` multiplies to 1 by the choice of its last scalar, group `near` differs from it in that single scalar"""
    rng = np.random.default_rng(seed)
    n = groups * ppg
    a = [int(rng.integers(1, 2**62)) ** 4 % R for _ in range(n)]
    few = [int(rng.integers(1, 2**62)) ** 4 % R for _ in range(5)]          # few distinct G2 multiples: they take the Python time
    b = [few[int(rng.integers(0, 5))] for _ in range(n)]
    one = groups - 1 if groups > 1 else 0
    if ppg > 1:
        lo = one * ppg
        s = sum(a[lo + j] * b[lo + j] for j in range(ppg - 1)) % R
        a[lo + ppg - 1] = (-s) * pow(b[lo + ppg - 1], -1, R) % R
        if groups > 1:
            near = (one + groups // 2) % groups if groups > 2 else 0
            for j in range(ppg):
                a[near * ppg + j], b[near * ppg + j] = a[lo + j], b[lo + j]
            a[near * ppg + ppg - 1] = (a[lo + ppg - 1] + 1) % R
    sums = [sum(a[g * ppg + j] * b[g * ppg + j] for j in range(ppg)) % R for g in range(groups)]
    return a, b, sums


@pytest.mark.parametrize("groups,ppg", SHAPES)
def test_pairing_products_match_oracle(zk, E, groups, ppg):
    a, b, sums = shape_case(groups, ppg, 9000 + 1000 * groups + ppg)
    Pa, Qa = make_pairs(a, b)
    want_one = np.array([1 if s == 0 else 0 for s in sums], dtype=np.uint32)
    if ppg > 1:
        assert want_one.sum() == 1
    gt, one = zk.halo2.pairing_products(Pa, Qa, groups, ppg)
    assert (one == want_one).all()
    check = sorted({0, groups - 1} | {g for g in (63, 64, 65) if g < groups})
    for g in check:
        assert (gt[g] == gt_words(E ** sums[g])).all(), g
    for g in np.nonzero(want_one)[0]:
        assert (gt[g] == gt_words(F12.one())).all()
    gt2, none = zk.halo2.pairing_products(Pa, Qa, groups, ppg, want_is_one=False)      # only the GT output
    assert none is None and (gt2 == gt).all()
    none, one2 = zk.halo2.pairing_products(Pa, Qa, groups, ppg, want_gt=False)         # only the flags
    assert none is None and (one2 == want_one).all()
    gt3, one3 = zk.halo2.pairing_products(Pa, Qa, groups, ppg)                         # two identical calls agree
    assert (gt3 == gt).all() and (one3 == one).all()
    if ppg == 1:                                                                       # one pair per group: the only scalar that gives 1 is zero
        Pz = Pa.copy(); Pz[groups - 1] = 0
        assert zk.halo2.pairing_products(Pz, Qa, groups, ppg)[1].tolist() == [0] * (groups - 1) + [1]


def test_identities_contribute_one(zk, E):
    a, b = [3, 5, 7, 11, 13, 17], [19, 23, 29, 31, 37, 41]
    Pa, Qa = make_pairs(a, b)
    Pa[1] = 0                                                                # identity in P
    Qa[2] = 0                                                                # identity in Q
    Pa[4] = 0; Qa[4] = 0; Pa[5] = 0; Qa[5] = 0                               # a group of identities only
    gt, one = zk.halo2.pairing_products(Pa, Qa, 3, 2)
    assert (gt[0] == gt_words(E ** (3 * 19))).all() and (gt[1] == gt_words(E ** (11 * 31))).all() and (gt[2] == gt_words(F12.one())).all()
    assert one.tolist() == [0, 0, 1]
    gt, one = zk.halo2.pairing_products(Pa[4:5], Qa[4:5], 1, 1)
    assert one.tolist() == [1] and (gt[0] == gt_words(F12.one())).all()


def g1_words(pt):
    return np.array(pyref.mont_limbs(pt[0], P) + pyref.mont_limbs(pt[1], P), dtype=np.uint64)


def test_released_msm_results_satisfy_the_pairing_equation(zk, kat):
    """the three released (result, W') pairs against G2 and the released -[s]G2: e(result, G2) e(W', -[s]G2) == 1, and not with result + G"""
    kats = {k: v for k, v in json.load(open(os.path.join(GOLD, "released_kats.json"))).items() if not k.startswith("_")}
    assert sorted(kats) == ["batch_proof", "bundle_proof", "chunk_proof"]
    neg = pyref.g2_from_evm_words([int(w, 16) for w in kat["yul"]["s_g2_words"]])
    g2, ns = np.array(pyref.g2_to_limbs(pyref.G2_GEN), dtype=np.uint64), np.array(pyref.g2_to_limbs(neg), dtype=np.uint64)
    Ps, Qs = [], []
    for name in sorted(kats):
        m = kats[name]["msm"]
        res = (int(m["result"][0], 16), int(m["result"][1], 16)); wp = (int(m["w_prime"][0], 16), int(m["w_prime"][1], 16))
        Ps += [g1_words(res), g1_words(wp), g1_words(pyref.g1_add(res, pyref.G1_GEN)), g1_words(wp)]
        Qs += [g2, ns, g2, ns]
    _, one = zk.halo2.pairing_products(np.stack(Ps), np.stack(Qs), 6, 2, want_gt=False)
    assert one.tolist() == [1, 0, 1, 0, 1, 0]


def test_adversarial_g1_points_match_the_oracles_full_pairing(zk):
    """8 pool points (an adversarial coordinate word each) against random G2 multiples: not known multiples of the generator, so the oracle's full pairing"""
    abi, _, _ = gc.adversarial_g1_points("mont")
    pts, _, _ = gc.adversarial_g1_info("mont")
    idx = [int(i) for i in np.linspace(0, len(pts) - 1, 8)]
    rng = np.random.default_rng(9100)
    bs = [int(rng.integers(1, 2**62)) ** 4 % R for _ in idx]
    Qpy = [pyref.g2_mul(pyref.G2_GEN, x) for x in bs]
    Qa = np.array([pyref.g2_to_limbs(q) for q in Qpy], dtype=np.uint64)
    gt, one = zk.halo2.pairing_products(abi[idx], Qa, 8, 1)
    assert not one.any()
    for n, i in enumerate(idx):
        assert (gt[n] == gt_words(pairing.pairing(Qpy[n], pts[i]))).all(), i


def test_points_off_their_curves_are_rejected_and_named(zk, E):
    Pa, Qa = make_pairs([2, 3, 5, 7, 11, 13], [3, 3, 3, 3, 3, 3])
    for side, where in (("P", 3), ("Q", 4), ("P", 0), ("Q", 5)):
        Pb, Qb = Pa.copy(), Qa.copy()
        (Pb if side == "P" else Qb)[where, 1] ^= np.uint64(4)
        with pytest.raises(zk.Mi355Error) as ei:
            zk.halo2.pairing_products(Pb, Qb, 3, 2)
        assert ei.value.code == zk._capi.EBADARG
        msg = str(ei.value)
        assert "pair %d " % where in msg and "(group %d, pair %d of it)" % (where // 2, where % 2) in msg
        assert ("P is not on the curve" in msg) == (side == "P") and ("Q is not on the twist" in msg) == (side == "Q")
        gt, one = zk.halo2.pairing_products(Pa, Qa, 3, 2)                     # a valid call follows and is right
        assert not one.any() and (gt[0] == gt_words(E ** 15)).all() and (gt[2] == gt_words(E ** 72)).all()
    Pb, Qb = Pa.copy(), Qa.copy()                                            # both sides bad: the first bad pair is named
    Pb[5, 0] ^= np.uint64(1); Qb[2, 9] ^= np.uint64(1)
    with pytest.raises(zk.Mi355Error) as ei:
        zk.halo2.pairing_products(Pb, Qb, 3, 2)
    assert "pair 2 " in str(ei.value) and "Q is not on the twist" in str(ei.value)


def test_argument_errors(zk):
    lib, capi = zk._capi.lib(), zk._capi
    Pa, Qa = make_pairs([2, 3], [5, 7])
    gt, one = np.zeros(48, dtype=np.uint64), (C.c_uint32 * 1)()
    assert lib.mi355_pairing_products_host(capi.ptr(Pa), capi.ptr(Qa), 0, 2, None, None) == capi.OK              # groups == 0: a no-op
    assert lib.mi355_pairing_products_host(None, None, 0, 0, None, None) == capi.OK
    assert lib.mi355_pairing_products_host(capi.ptr(Pa), capi.ptr(Qa), 1, 0, capi.ptr(gt), one) == capi.EBADARG
    assert lib.mi355_pairing_products_host(capi.ptr(Pa), capi.ptr(Qa), 1, 2, None, None) == capi.EBADARG
    assert lib.mi355_pairing_products_host(None, capi.ptr(Qa), 1, 2, capi.ptr(gt), one) == capi.EBADARG
    assert lib.mi355_pairing_products_host(capi.ptr(Pa), capi.ptr(Qa), 1 << 11, 1 << 10, capi.ptr(gt), one) == capi.EBADARG
    assert lib.mi355_pairing_products_host(capi.ptr(Pa), capi.ptr(Qa), 1, 2, capi.ptr(gt), one) == capi.OK
    assert one[0] == 0 and gt.any()


def test_off_subgroup_twist_points_return(zk):
    """a Q on the twist but outside the subgroup of order r: unspecified value, but the call returns and the next one is right"""
    limbs, _, _ = gc.adversarial_g2_points()
    Pa, _ = make_pairs([2, 3, 5, 7], [1, 1, 1, 1])
    zk.halo2.pairing_products(Pa, limbs[:4].copy(), 2, 2)
    Pa, Qa = make_pairs([2, R - 2], [5, 5])
    assert zk.halo2.pairing_products(Pa, Qa, 1, 2)[1].tolist() == [1]


def test_workspace_returns_to_the_pool(zk):
    lib = zk._capi.lib()
    zk._capi.check(lib.mi355_buf_trim())
    before = zk.halo2.mem_info()
    Pa, Qa = make_pairs([2, 3, 5, 7, 9, 11], [4, 4, 4, 4, 4, 4])
    zk.halo2.pairing_products(Pa, Qa, 2, 3)
    mid = zk.halo2.mem_info()
    assert mid["live_buffers"] == before["live_buffers"]                      # nothing stays allocated to the caller
    assert mid["pooled"] > before["pooled"]                                   # the block sits in the pool ...
    zk._capi.check(lib.mi355_buf_trim())
    after = zk.halo2.mem_info()
    assert after["pooled"] == before["pooled"]                                # ... and goes back to HIP under mi355_buf_trim


def test_kernels_report_under_pairing_names(zk):
    lib = zk._capi.lib()
    zk._capi.check(lib.mi355_profile_enable(1))
    try:
        zk._capi.check(lib.mi355_profile_reset())
        Pa, Qa = make_pairs([2, 3, 5], [4, 4, 4])
        zk.halo2.pairing_products(Pa, Qa, 1, 3)
        for name, launches in (("pairing_validate", 1), ("pairing_miller", 1), ("pairing_reduce", 2), ("pairing_final_exp", 1)):
            ms, cnt = C.c_double(), C.c_uint64()
            zk._capi.check(lib.mi355_profile_get(name.encode(), C.byref(ms), C.byref(cnt)))
            assert cnt.value == launches and ms.value > 0, name
    finally:
        zk._capi.check(lib.mi355_profile_enable(0))


def test_params_check_g2(zk):
    """ParamsKZG.check_g2: e(g[0], s_g2) e(-g[1], g2) == 1 for a synthetic SRS -- the pairing, not the trapdoor -- and not once s_g2 is replaced"""
    params = zk.halo2.ParamsKZG.setup(8, 0x5eed1234abcdef)
    try:
        assert params.check_g2()
        keep = params.s_g2
        params.s_g2 = params.g2
        assert not params.check_g2()
        neg = np.frombuffer(keep, dtype=np.uint64).copy()                    # -[s]G2: (x, -y)
        for o in (8, 12):
            y = sum(int(v) << (64 * i) for i, v in enumerate(neg[o:o + 4]))
            neg[o:o + 4] = pyref.to_limbs((P - y) % P)
        params.s_g2 = neg.tobytes()
        assert not params.check_g2()
        params.s_g2 = keep
        assert params.check_g2()
    finally:
        params.release()
