"""CPU-only: protocols with upstream halo2's classic lookup argument (permuted columns A', S' and a grand product z per lookup; protocols.py
lookup_argument="permuted") load in Protocol::load -- through mi355_plonk_protocol_from_json and _info, which need no device -- and in the test-side subclass of the
oracle's Protocol; their polynomial, query and evaluation counts are the argument's; malformed ones are refused with the reason; and the generator's default output
is what it was before the parameter existed."""
import copy
import json

import pytest

import __graft_entry__ as ge
from oracle import plonk
from tests.classic_lookup_common import ClassicProtocol
from tests.plonk_capi_common import SMALL0

SHAPES = [("layer2", 2, 8, {}), ("layer3", 3, 8, {}), ("layer0_stand_in", 0, 9, SMALL0)]


@pytest.fixture(scope="module")
def zk():
    ge.build()
    return ge.load_package()


def generated(zk, layer, k, shape, **kw):
    return zk.protocols.layer_protocol(layer, k, **shape, **kw)


@pytest.mark.parametrize("name,layer,k,shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_permuted_protocols_load_with_the_arguments_counts(zk, name, layer, k, shape):
    mv, d = generated(zk, layer, k, shape), generated(zk, layer, k, shape, lookup_argument="permuted")
    L = mv["num_witness"][1]                                           # one m per lookup
    Z = mv["num_witness"][2] - L - 1
    assert L == {2: 1, 3: 8, 0: 3}[layer]
    assert d["num_witness"] == [mv["num_witness"][0], 2 * L, Z + L + 1] and d["num_challenge"] == [1, 2, 1] and d["lookup_argument"] == "permuted"
    assert len(d["queries"]) == len(mv["queries"]) + 2 * L and len(d["evaluations"]) == len(mv["evaluations"]) + 2 * L      # (z,0) (z,1) (A',0) (A',-1) (S',0) for (phi,0) (phi,1) (m,0)
    n_cons = lambda p: len(p["quotient"]["numerator"]["DistributePowers"][0])
    assert n_cons(d) == n_cons(mv) + 2 * L                             # five constraints per lookup for three
    # the library's recogniser
    with zk.prover.Protocol.from_json(d) as p:
        info = p.info()
    assert info["lookup_permuted"] == 1 and info["num_lookups"] == L and info["num_perm_chunks"] == Z and info["num_advice"] == d["num_witness"][0]
    assert info["num_witness"] == sum(d["num_witness"]) and info["num_evaluations"] == len(d["evaluations"]) and info["num_queries"] == len(d["queries"])
    assert info["num_commitments"] == sum(d["num_witness"]) + info["quotient_pieces"] + 2
    with zk.prover.Protocol.from_json(mv) as p:
        assert p.info("lookup_permuted") == 0 and p.info("num_lookups") == L
    # the oracle's, through the subclass
    pr = ClassicProtocol(d)
    assert len(pr.lookups) == L and len(pr.perm) == Z and pr.blind == 6 and pr.usable == (1 << k) - 7
    ph1, ph2 = pr.phase0[1], pr.phase0[2]
    for l, lk in enumerate(pr.lookups):
        assert (lk["perm_input"], lk["perm_table"], lk["z"]) == (ph1 + 2 * l, ph1 + 2 * l + 1, ph2 + Z + l)
        opened = [(lk["z"], 0), (lk["z"], 1), (lk["perm_input"], 0), (lk["perm_input"], -1), (lk["perm_table"], 0)]
        at = pr.evaluations.index(opened[0])
        assert pr.evaluations[at:at + 5] == opened and all(q in pr.queries for q in opened)
    if layer == 0:
        assert all(len(lk["input"]["DistributePowers"][0]) == 3 and len(lk["table"]["DistributePowers"][0]) == 3 for lk in pr.lookups)     # three-column compressed lookups
    assert len(ClassicProtocol(mv).lookups) == L and "m" in ClassicProtocol(mv).lookups[0]                # an mv protocol goes the base class's way
    with pytest.raises((AssertionError, KeyError)):
        plonk.Protocol(d)                                              # the oracle's own recogniser knows the mv-lookup only


def _constraints(d):
    return d["quotient"]["numerator"]["DistributePowers"][0]


def _refused(zk, d):
    with pytest.raises(zk.Mi355Error) as e:
        zk.prover.Protocol.from_json(d)
    assert e.value.code == zk._capi.EBADARG
    return str(e.value)


def test_malformed_protocols_are_refused_with_the_reason(zk):
    good = generated(zk, 3, 8, {}, lookup_argument="permuted")
    ph1 = ClassicProtocol(good).phase0[1]
    is5 = lambda c: "Product" in c["Product"][1]                       # l_active (A' - S')(A' - A'(w^-1 X)): the only constraints whose second factor is a product
    fives = [i for i, c in enumerate(_constraints(good)) if is5(c)]
    assert len(fives) == 8
    # constraint 5 of lookup 2 names lookup 3's A' in its rotated factor
    d = copy.deepcopy(good)
    d["quotient"]["numerator"]["DistributePowers"][0][fives[2]]["Product"][1]["Product"][1]["Sum"][1]["Negated"]["Polynomial"]["poly"] = ph1 + 6
    msg = _refused(zk, d)
    assert "permuted lookup 2" in msg and "(A' - S')(A' - A'(w^-1 X))" in msg and "names other columns" in msg
    with pytest.raises(AssertionError, match="constraint 5"):
        ClassicProtocol(d)
    # ... or has rotation +1 where -1 belongs
    d = copy.deepcopy(good)
    d["quotient"]["numerator"]["DistributePowers"][0][fives[0]]["Product"][1]["Product"][1]["Sum"][1]["Negated"]["Polynomial"]["rotation"] = 1
    assert "permuted lookup 0" in _refused(zk, d)
    # constraint 4 missing: constraint 5 stands where l_0 (A' - S') is due
    d = copy.deepcopy(good)
    del d["quotient"]["numerator"]["DistributePowers"][0][fives[0] - 1]
    assert "l_0 (A' - S') does not follow" in _refused(zk, d)
    # a protocol that mixes the two kinds: the last lookup of the permuted protocol replaced by an mv-lookup's three constraints over the same polynomials
    mv = generated(zk, 3, 8, {})
    d = copy.deepcopy(good)
    d["quotient"]["numerator"]["DistributePowers"][0][fives[7] - 4:fives[7] + 1] = copy.deepcopy(_constraints(mv)[-3:])
    msg = _refused(zk, d)
    assert "mv-lookups and permuted lookups in one protocol" in msg and "1 and 7" in msg
    # a wrong phase-1 count
    d = copy.deepcopy(good)
    d["num_witness"][1] -= 1
    msg = _refused(zk, d)
    assert "num_witness[1] = 15" in msg and "8 permuted lookups" in msg
    # the rejections that exist keep their words
    d = copy.deepcopy(mv)
    d["num_witness"][1] += 1
    assert "num_witness does not match the recognised arguments" in _refused(zk, d)
    d = copy.deepcopy(mv)
    d["quotient"]["numerator"]["DistributePowers"][0][-1]["Product"][1]["Sum"][0]["Product"][1] = {"Challenge": 1}
    assert "unrecognised lookup constraint" in _refused(zk, d)


def test_the_default_is_the_mv_lookup_byte_for_byte(zk):
    text = lambda p: json.dumps(p, separators=(",", ":"))
    for layer in range(7):
        shape = SMALL0 if layer == 0 else {}
        k = 9 if layer == 0 else 8
        assert text(zk.protocols.layer_protocol(layer, k, **shape)) == text(zk.protocols.layer_protocol(layer, k, lookup_argument="mv", **shape))
        assert "lookup_argument" not in zk.protocols.layer_protocol(layer, k, **shape)
    # ... and equal to the committed fixtures of the reference's own constraint systems, which predate the parameter
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for layer in (2, 4):
        fx = json.load(open(os.path.join(gold, f"protocol_layer{layer}.json")))
        fx = fx.get("protocol", fx)
        ours = zk.protocols.layer_protocol(layer)
        assert ours["quotient"]["numerator"] == fx["quotient"]["numerator"] and ours["num_witness"] == fx["num_witness"]
        assert ours["queries"] == fx["queries"] and ours["evaluations"] == fx["evaluations"]
    with pytest.raises(AssertionError):
        zk.protocols.layer_protocol(2, 8, lookup_argument="classic")
