"""gate families that drive plonk::Compiler (include/mi355zk_plonk.hpp) down the paths the stock circuits never reach (TEST INFRASTRUCTURE, not a test): PlonkProtocol dicts
from protocols.synthetic_inner_protocol with the body P of chosen assigned gates  s (P - a_i)  replaced through its `gate_body` argument.  Shared by
tests/test_plan_compiler_on_host.py (the launch lists interpreted on the CPU) and tests/test_gpu_plan_compiler.py (the same plans run by the device).

Every P reads advice columns with a smaller index than its target only, at rotations in {0, 1, -1, 2}: the circuit builder's rule (build_circuit assigns the dependent
columns in index order).  Sums and products are folded to the left, so the builder's row evaluator needs a stack of a few entries whatever their length.

  family  body P                                                                    reaches                                                              degree of P
  A       (sum of 20 cells) (sum of 20 cells), every third dependent column         materialised sums of > 16 terms: a temporary written by two launches       2
  B       N(0), N(d) = N(d+1) N'(d+1) + cell, N(4) a two-cell sum                   many small temporaries                                                    16
  C       one monomial of 17 .. 20 cells                                            maxlen(A) + maxlen(B) > 16 forces materialising                      17 .. 20
  D       ((5 + x0) - 5) + Scaled((x1 + 0) (x2 x3 + (3 - 3)), s), s = 0 every       cancelling constants, a zero constant, Scaled by zero and by nonzero       3
          fifth gate; D-dpow adds DistributePowers([x4, x5, 2], 3) (host only: the builder's row evaluator refuses that node)
  E       a sum of 30 two-cell products over distinct columns (advice = 60)         the 24-polynomial and the 16-term limit in one sum                         2
  F       (sum_{j<4} S8 S8) (sum_{j<4} S8 S8), S8 a sum of 8 cells; degree = 5      more than TMP_GROUP = 12 temporaries in one constraint                     4
  G       as B with depth 3 and six-cell leaf sums; degree = 9                      nested temporaries within the degree-9 bound                               8
  H       as B with depth 6, on one gate only                                       more than 32 temporaries: the compiler must refuse                         -
B and C exceed the quotient's degree bound (degree of P <= degree - 1): host and check_witness only.  A, D, E, F, G satisfy it and are proven."""
import __graft_entry__ as ge

ROTS = (0, 1, -1, 2)
LIMIT_TEXT = "more than 32 temporaries"      # what the compiler's refusal of H must say
N_PLAIN, N_FREE = 4, 10                      # every shape below: 4 plain free columns, then lookups = 2 tuples of 3 lookup-input columns; the dependent columns follow


def _protocols():
    return ge.load_package().protocols


class _Cells:
    """an endless stream of distinct-as-far-as-possible cells of the columns below dependent column i: column index descending from i - 1, the rotation stepping through ROTS"""

    def __init__(self, i, adv, start=0):
        self.i, self.adv, self.j = i, adv, start

    def __call__(self):
        P = _protocols()
        j = self.j
        self.j += 1
        return P.Poly(self.adv[(self.i - 1 - j) % self.i], ROTS[(self.i + j) % 4])


def _sum(xs):
    P = _protocols()
    return P._fold(P.Sum, xs)


def _prod(xs):
    P = _protocols()
    return P._fold(P.Prod, xs)


def _nest(cell, depth, leaf_cells, d=0):
    """N(d) = N(d + 1) N'(d + 1) + cell,  N(depth) = a sum of `leaf_cells` cells; N and N' differ in the cells they draw"""
    P = _protocols()
    if d == depth:
        return _sum([cell() for _ in range(leaf_cells)])
    return P.Sum(P.Prod(_nest(cell, depth, leaf_cells, d + 1), _nest(cell, depth, leaf_cells, d + 1)), cell())


def body_A(i, adv, consts):
    if i % 3:
        return None
    c = _Cells(i, adv)
    return _protocols().Prod(_sum([c() for _ in range(20)]), _sum([c() for _ in range(20)]))


def body_B(i, adv, consts):
    return _nest(_Cells(i, adv), 4, 2)


def body_C(i, adv, consts):
    """the cells are those of the lookup-input columns (table tuples: rarely zero), so that the monomial is not zero on nearly every row as a product of witness-like
    cells (60 % zeros) would be, and a wrong cell shows"""
    P = _protocols()
    lookup_inputs = range(N_PLAIN, N_FREE)
    cells = [P.Poly(adv[c], rot) for rot in ROTS for c in lookup_inputs]
    return _prod([cells[(i + j) % len(cells)] for j in range(17 + i % 4)])


def _body_D(i, adv, consts, dpow):
    P = _protocols()
    c = _Cells(i, adv)
    x0, x1, x2, x3 = c(), c(), c(), c()
    s = 0 if i % 5 == 0 else 11 + i
    inner = P.Sum(P.Prod(x2, x3), P.Sum(P.Const(3), P.Neg(P.Const(3))))
    body = P.Sum(P.Sum(P.Sum(P.Const(5), x0), P.Neg(P.Const(5))), P.Scaled(P.Prod(P.Sum(x1, P.Const(0)), inner), s))
    if dpow:
        body = P.Sum(body, P.DP([c(), c(), P.Const(2)], P.Const(3)))
    return body


def body_D(i, adv, consts):
    return _body_D(i, adv, consts, False)


def body_D_dpow(i, adv, consts):
    return _body_D(i, adv, consts, True)


def body_E(i, adv, consts):
    if i < 48:
        return None
    c = _Cells(i, adv)
    return _sum([_protocols().Prod(c(), c()) for _ in range(30)])


def body_F(i, adv, consts):
    if i % 4:
        return None
    P = _protocols()
    c = _Cells(i, adv)
    s8 = lambda: _sum([c() for _ in range(8)])
    half = lambda: _sum([P.Prod(s8(), s8()) for _ in range(4)])
    return P.Prod(half(), half())


def body_G(i, adv, consts):
    if i % 2:
        return None
    return _nest(_Cells(i, adv), 3, 6)


def body_H(i, adv, consts):
    if i != 30:
        return None
    return _nest(_Cells(i, adv), 6, 2)


# family -> (gate_body, generator shape).  lookups = 2 gives n_free = 4 + 3 * 2 = 10 free columns; advice <= 60
BASE = dict(fixed=8, lookups=2, perm_columns=12, degree=5)
FAMILIES = {
    "A": (body_A, dict(BASE, advice=40)),
    "B": (body_B, dict(BASE, advice=32)),
    "C": (body_C, dict(BASE, advice=40)),
    "D": (body_D, dict(BASE, advice=40)),
    "D_dpow": (body_D_dpow, dict(BASE, advice=40)),
    "E": (body_E, dict(BASE, advice=60)),
    "F": (body_F, dict(BASE, advice=40)),
    "G": (body_G, dict(BASE, advice=32, degree=9)),
    "H": (body_H, dict(BASE, advice=40)),
}
PROVABLE = ("A", "D", "E", "F", "G")         # the degree of P is at most degree - 1
WITNESS_ONLY = ("B", "C")                    # beyond the degree bound: the plan and check_witness, no proof


def family_protocol(name, k):
    """the PlonkProtocol dict of one family at domain size 2^k (layer 0: the Poseidon transcript)"""
    body, shape = FAMILIES[name]
    d = _protocols().layer_protocol(0, k, gate_body=body, **shape)
    assert d["synthetic"]["n_free"] == N_FREE
    return d


def reads_at(protocol_dict, rotation):
    """(advice index, rotation) of the first advice cell some gate's P reads at `rotation`, scanning the gates in order"""
    d = protocol_dict
    adv0 = d["num_preprocessed"] + 1
    A = d["num_witness"][0]
    found = []

    def walk(e):
        if isinstance(e, dict):
            for k, v in e.items():
                if k == "Polynomial":
                    if adv0 <= v["poly"] < adv0 + A and v["rotation"] == rotation:
                        found.append(v["poly"] - adv0)
                else:
                    walk(v)
        elif isinstance(e, list):
            for v in e:
                walk(v)
    for c in d["quotient"]["numerator"]["DistributePowers"][0]:
        a, b = c["Product"]
        if "Polynomial" in a and a["Polynomial"]["poly"] < d["num_preprocessed"]:      # selector * (P - target)
            walk(b["Sum"][0])
            if found:
                return found[0]
    raise AssertionError(f"no gate reads an advice cell at rotation {rotation}")
