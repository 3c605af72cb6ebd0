"""CPU-only: plonk::Compiler (include/mi355zk_plonk.hpp), the code that decides what the quotient kernels are asked to compute, on the gate families of tests/plan_common.py.
tests/hostcheck/plan_interp_main.cpp, built under -fsanitize=address,undefined, compiles a protocol's numerator with the challenges (2, 3, 5, 7) and interprets the launch
list on the Lagrange domain over random columns; every row it prints must equal oracle.plonk.evaluate of the whole numerator in Python integers over the same columns
(poly(i, rot) = column i at row r + rot mod n, lagrange(i) = [r == i mod n], identity() = omega^r).  n = 16 (k = 4): the rotation wrap and every Lagrange index lie inside
the data.  Each family runs under MI355_PLAN_PREFIX_MIN unset, 0 and 2 and is held to the printed fact that shows its path was reached; family H must be refused by name.
Also: protocols.synthetic_inner_protocol without `gate_body` returns what it returned before the argument existed (SHA-256 of the sorted JSON)."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import plonk

import plan_common as pc
from plonk_capi_common import SMALL0

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = plonk.R
K = 4
CHALLENGES = (2, 3, 5, 7)
PREFIX = (None, "0", "2")
FAMILIES = ("A", "B", "C", "D", "D_dpow", "E", "F", "G", "stock")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("planinterp") / "plan_interp_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           "-o", path, os.path.join(HERE, "hostcheck", "plan_interp_main.cpp")])
    return path


def protocol_of(family):
    if family == "stock":
        return ge.load_package().protocols.layer_protocol(0, K, **SMALL0)
    return pc.family_protocol(family, K)


def run(exe, directory, family, prefix):
    """(facts, rows, refusal, columns) of one run of the program on the family's protocol over random columns"""
    d = protocol_of(family)
    pr = plonk.Protocol(d)
    rng = np.random.default_rng(sum(map(ord, family)))               # the same columns under every prefix setting
    cols = [[int.from_bytes(rng.bytes(40), "little") % R for _ in range(pr.n)] for _ in range(pr.quotient_poly)]
    proto, data = os.path.join(directory, f"{family}.json"), os.path.join(directory, f"{family}.bin")
    with open(proto, "w") as f:
        json.dump(d, f, separators=(",", ":"))
    with open(data, "wb") as f:
        f.write(plonk.ints_to_mont([v for c in cols for v in c]).tobytes())
    env = {k: v for k, v in os.environ.items() if k != "MI355_PLAN_PREFIX_MIN"}
    if prefix is not None:
        env["MI355_PLAN_PREFIX_MIN"] = prefix
    out = subprocess.run([exe, proto, data], capture_output=True, text=True, timeout=300, env=env)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr and "LeakSanitizer" not in out.stderr, out.stderr
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    facts, rows, refusal = {}, {}, None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "fact":
            facts[w[1]] = int(w[2])
        elif w[0] == "row":
            rows[int(w[1])] = int(w[2], 16)
        elif w[0] == "refused":
            refusal = line[len("refused "):]
    return facts, rows, refusal, (pr, cols)


def numerator_rows(pr, cols):
    """the whole numerator on all n rows in Python integers"""
    n = pr.n
    arr = [np.array(c, dtype=object) for c in cols]
    ident = np.array([pow(pr.omega, r, R) for r in range(n)], dtype=object)

    def lagrange(i):
        v = np.zeros(n, dtype=object)
        v[i % n] = 1
        return v
    v = plonk.evaluate(pr.numerator, lambda i, rot: np.roll(arr[i], -rot), lambda i: CHALLENGES[i], lambda: ident, lagrange)
    return [int(x) % R for x in v]


@pytest.fixture(scope="module")
def results(exe, tmp_path_factory):
    """every (family, prefix setting), run once; the Python-integer numerator once per family"""
    tmp = str(tmp_path_factory.mktemp("planruns"))
    out = {}
    for fam in FAMILIES:
        want = None
        for prefix in PREFIX:
            facts, rows, refusal, (pr, cols) = run(exe, tmp, fam, prefix)
            if want is None:
                want = numerator_rows(pr, cols)
            out[(fam, prefix)] = (facts, rows, refusal, want)
    return out


@pytest.mark.parametrize("prefix", PREFIX, ids=["prefix_default", "prefix_0", "prefix_2"])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_plan_computes_the_numerator_on_every_row(results, family, prefix):
    facts, rows, refusal, want = results[(family, prefix)]
    assert refusal is None, refusal
    assert sorted(rows) == list(range(1 << K))
    bad = [r for r in range(1 << K) if rows[r] != want[r]]
    assert not bad, f"family {family}, MI355_PLAN_PREFIX_MIN={prefix}: rows {bad} differ from the Python-integer numerator; plan {facts}"
    assert any(want), "the numerator vanishes on random columns: the comparison would hold nothing"


@pytest.mark.parametrize("prefix", PREFIX, ids=["prefix_default", "prefix_0", "prefix_2"])
@pytest.mark.parametrize("family", FAMILIES)
def test_each_family_reaches_its_path(results, family, prefix):
    facts = results[(family, prefix)][0]
    print(family, prefix, facts)
    assert facts["max_terms"] <= 16 and facts["max_factors"] <= 48 and facts["max_polys"] <= 24 and facts["max_term_len"] <= 16
    if family in ("A", "E"):
        assert facts["accumulate_into_tmp"] >= 1           # a temporary written by two launches, the second accumulating
    if family == "E":
        assert facts["max_polys"] == 24 and facts["max_terms"] == 16
    if family == "C":
        assert facts["max_term_len"] <= 16 and facts["tmps_used"] >= 1     # the source holds a 20-cell monomial: it was cut through temporaries
    if family == "F":
        assert facts["constraint_tmps_max"] > 12           # more than TMP_GROUP in one constraint
    if family in ("B", "G"):
        assert facts["constraint_tmps_max"] >= 2
    if family in ("B", "F", "G"):
        assert facts["tmps_used"] >= 13
    if prefix is None:
        # what tests/test_gpu_plan_compiler.py asks of the proof record (plan_launches, plan_terms, plan_tmps, plan_prefix_groups): the plan does not depend on k
        assert facts["prefix_groups"] == 1 and facts["tmps_used"] >= 2 and facts["terms"] <= 16 * facts["launches"]
        if family in ("A", "E"):
            assert facts["launches"] > facts["tmps_used"] + -(-facts["terms"] // 16)
        if family == "F":
            assert facts["tmps_used"] - facts["prefix_groups"] > 12
        if family == "G":
            assert facts["tmps_used"] - facts["prefix_groups"] >= 12
    if prefix == "2":
        assert facts["prefix_groups"] >= 2 and facts["tmp_max"] > 32
    if prefix == "0":
        assert facts["prefix_groups"] == 0


def test_more_than_32_temporaries_in_one_constraint_are_refused_by_name(exe, tmp_path):
    for prefix in PREFIX:
        facts, rows, refusal, _ = run(exe, str(tmp_path), "H", prefix)
        assert refusal is not None and pc.LIMIT_TEXT in refusal, (prefix, refusal, facts)
        assert not rows and not facts


def test_the_generator_without_gate_body_is_unchanged():
    """digests of json.dumps(..., sort_keys=True) taken before synthetic_inner_protocol had the argument"""
    P = ge.load_package().protocols
    digest = lambda d: hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()
    assert digest(P.synthetic_inner_protocol(k=7, **SMALL0)) == "57e9e88746376fa57914d92c7165eb185329700f78376389f5d062910fe84d28"
    assert digest(P.synthetic_inner_protocol()) == "5647440b91f4f4e224c5849419b3168f7c886860cb1cbb7bc44e864f389de1b0"
    assert digest(P.synthetic_inner_protocol(k=7, gate_body=lambda i, adv, consts: None, **SMALL0)) == "57e9e88746376fa57914d92c7165eb185329700f78376389f5d062910fe84d28"
