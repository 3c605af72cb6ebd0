"""the classic halo2 lookup argument on the test side (TEST INFRASTRUCTURE): a subclass of oracle.plonk.Protocol that overrides `_recognise` only, so that the
oracle's tree-walking verifier -- pinned by the reference's released proofs -- reads protocols whose lookups are the permuted kind; and the argument's three
columns (A', S', z) restated on Python integers from a circuit, the challenges and the blinding values, with the five constraints checked row by row and the
commitment of a column computed under the trapdoor.  Nothing here looks at the C++."""
from oracle import plonk
from tests import lookup_permute_common as pc

R = plonk.R


def _poly(i, rot=0):
    return {"Polynomial": {"poly": i, "rotation": rot}}


class ClassicProtocol(plonk.Protocol):
    """oracle.plonk.Protocol for protocols with permuted lookups: self.lookups holds {"z", "perm_input", "perm_table", "input", "table"} per lookup.  mv-lookup
    protocols are recognised as the base class does."""

    def _recognise(self):
        cons = self.numerator["DistributePowers"][0]
        assert self.numerator["DistributePowers"][1] == {"Challenge": sum(self.num_challenge) - 1}
        if not any(self._is_permuted_head(c) for c in cons):
            return super()._recognise()
        self.gates, self.perm, self.lookups = [], [], []
        i = 0
        while i < len(cons):
            c = cons[i]; i += 1
            a, b = c["Product"]
            if plonk._is_lagrange(a) is not None:
                continue
            if not plonk._is_common_linear(a):
                self.gates.append(c)
                continue
            s0, s1 = b["Sum"]
            l0, l1 = s0["Product"]
            z = l0["Polynomial"]["poly"]
            assert l0 == _poly(z, 1)
            r0, r1 = s1["Negated"]["Product"]
            assert r0 == _poly(z)
            if self._is_permuted_head(c):
                (ab, sb), (ib, tb) = l1["Product"], r1["Product"]
                ap, sp = ab["Sum"][0]["Polynomial"]["poly"], sb["Sum"][0]["Polynomial"]["poly"]
                assert ab == {"Sum": [_poly(ap), {"Challenge": 1}]} and sb == {"Sum": [_poly(sp), {"Challenge": 2}]}
                assert ib["Sum"][1] == {"Challenge": 1} and tb["Sum"][1] == {"Challenge": 2}
                diff = {"Sum": [_poly(ap), {"Negated": _poly(sp)}]}
                c4, c5 = cons[i], cons[i + 1]; i += 2
                assert c4 == {"Product": [{"CommonPolynomial": {"Lagrange": 0}}, diff]}, "constraint 4 of a permuted lookup"
                assert c5 == {"Product": [a, {"Product": [diff, {"Sum": [_poly(ap), {"Negated": _poly(ap, -1)}]}]}]}, "constraint 5 of a permuted lookup"
                self.lookups.append({"z": z, "perm_input": ap, "perm_table": sp, "input": ib["Sum"][0], "table": tb["Sum"][0]})
            else:
                cols = []
                for fs, fi in zip(plonk._flatten_product(l1), plonk._flatten_product(r1)):
                    (cs, bs), g = fs["Sum"][0]["Sum"], fs["Sum"][1]
                    (ci, bi), g2 = fi["Sum"][0]["Sum"], fi["Sum"][1]
                    assert cs == ci and g == g2 == {"Challenge": 2} and bs["Product"][0] == {"Challenge": 1} and bi["Product"][1] == {"CommonPolynomial": "Identity"}
                    cols.append((cs["Polynomial"]["poly"], bs["Product"][1]["Polynomial"]["poly"], plonk.limbs_mont_to_int(bi["Product"][0]["Product"][1]["Constant"])))
                self.perm.append({"z": z, "columns": cols})
        L, Z = len(self.lookups), len(self.perm)
        assert self.num_witness[1] == 2 * L and self.num_witness[2] == Z + L + 1
        for l, lk in enumerate(self.lookups):
            assert (lk["perm_input"], lk["perm_table"], lk["z"]) == (self.phase0[1] + 2 * l, self.phase0[1] + 2 * l + 1, self.phase0[2] + Z + l)

    @staticmethod
    def _is_permuted_head(c):
        """l_active (z(wX) (A' + beta)(S' + gamma) - ...): the factor behind z(wX) starts with a polynomial plus beta (a permutation factor starts with a sum)"""
        try:
            a, b = c["Product"]
            if plonk._is_lagrange(a) is not None or not plonk._is_common_linear(a):
                return False
            first = b["Sum"][0]["Product"][1]["Product"][0]["Sum"]
            return "Polynomial" in first[0] and first[1] == {"Challenge": 1}
        except (KeyError, TypeError, IndexError):
            return False


def compressed(pr, expr, columns, theta, rows):
    """the theta-compressed expression on rows 0 .. rows - 1; columns: polynomial index -> list of n integers (Lagrange values)"""
    n = pr.n
    return [plonk.evaluate(expr, poly=lambda p, r: columns[p][(i + r) % n], challenge=lambda j: {0: theta}[j], identity=None, lagrange=None) for i in range(rows)]


def argument_columns(pr, lookup, columns, theta, beta, gamma, perm_blind, lz_blind):
    """(A', S', z) of one permuted lookup as lists of n integers: the rule of tests/lookup_permute_common.py over the usable rows, the blinding values behind
    (perm_blind: blind + 1 values of A' then of S', from the l_last row on; lz_blind: blind values of z, behind the l_last row)"""
    n, u, t = pr.n, pr.usable, pr.blind + 1
    a_in, s_in = compressed(pr, lookup["input"], columns, theta, u), compressed(pr, lookup["table"], columns, theta, u)
    a, s, miss = pc.permute(a_in, s_in)
    assert miss is None, miss
    assert len(perm_blind) == 2 * t and len(lz_blind) == pr.blind
    a, s = a + list(perm_blind[:t]), s + list(perm_blind[t:])
    z = [1]
    for i in range(u):
        z.append(z[i] * (a_in[i] + beta) % R * (s_in[i] + gamma) % R * plonk.inv((a[i] + beta) * (s[i] + gamma)) % R)
    z += list(lz_blind)
    assert len(a) == len(s) == len(z) == n
    return a, s, z, a_in, s_in


def check_five_constraints(pr, a, s, z, a_in, s_in, beta, gamma):
    """every constraint of the argument on every row of the domain (l_0 is row 0, l_last row u, l_active rows < u)"""
    n, u = pr.n, pr.usable
    assert z[0] == 1, "l_0 (1 - z)"
    assert (z[u] * z[u] - z[u]) % R == 0 and z[u] == 1, "l_last (z^2 - z)"
    assert a[0] == s[0], "l_0 (A' - S')"
    for i in range(u):
        assert (z[(i + 1) % n] * (a[i] + beta) % R * (s[i] + gamma) - z[i] * (a_in[i] + beta) % R * (s_in[i] + gamma)) % R == 0, ("constraint 3", i)
        assert (a[i] - s[i]) * (a[i] - a[(i - 1) % n]) % R == 0, ("constraint 5", i)


def lagrange_basis_at(pr, tau):
    """L_i(tau) for every row i"""
    n = pr.n
    zn = (pow(tau, n, R) - 1) * plonk.inv(n) % R
    out, w = [], 1
    for _ in range(n):
        out.append(w * zn % R * plonk.inv(tau - w) % R)
        w = w * pr.omega % R
    return out


def commitment(basis, column):
    """the commitment of a column of Lagrange values under the trapdoor SRS: (sum_i column[i] L_i(tau)) G"""
    return plonk.g1_of_scalar(sum(c * b for c, b in zip(column, basis)) % R)
