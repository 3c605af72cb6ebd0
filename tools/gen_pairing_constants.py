#!/usr/bin/env python3
"""gen_pairing_constants.py -- derives the constants of the BN254 pairing used by scroll-prover_amd/csrc/fq12.hpp and pairing.hpp and writes them into fq12.hpp.

  gamma[i][k] = xi^(k (p^i - 1) / 6) in Fq2,  xi = 9 + u,  i = 1, 2, 3,  k = 1 .. 5 : the Frobenius map p^i sends the tower coefficient a at w^k (w^6 = xi,
  k = 2 (power of v) + (power of w)) to  conj^i(a) * gamma[i][k]; the same table gives pi(Q) and pi^2(Q) on the twist (k = 2 for x, k = 3 for y).
  The hard part of the final exponentiation: (p^4 - p^2 + 1) / r = p^3 + l2 p^2 + l1 p + l0 with l2 = 6 t^2 + 1, l1 = -36 t^3 - 18 t^2 - 12 t + 1,
  l0 = -36 t^3 - 30 t^2 - 18 t - 2 (Scott, Benger, Charlemagne, Dominguez Perez, Kachisa: "On the final exponentiation for calculating pairings on ordinary
  elliptic curves", Pairing 2009) -- checked below as an identity of integers, together with the multi-exponentiation chain pairing.hpp walks.
Everything is computed from p, r and t with Python integers.  Without arguments the table is printed; --write replaces the block between the GENERATED markers of
fq12.hpp; tests/test_pairing_on_host.py recomputes the powers with pow-style exponentiation and compares them with what the compiled code holds."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyref

P, R = pyref.P_MOD, pyref.R_MOD
T = 4965661367192848881
HEADER = os.path.join(ROOT, "scroll-prover_amd", "csrc", "fq12.hpp")
BEGIN, END = "// ---- BEGIN GENERATED (tools/gen_pairing_constants.py --write)", "// ---- END GENERATED"


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_pow(a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = f2_mul(out, a)
        a = f2_mul(a, a)
        e >>= 1
    return out


def derive():
    assert P == 36 * T**4 + 36 * T**3 + 24 * T**2 + 6 * T + 1 and R == 36 * T**4 + 36 * T**3 + 18 * T**2 + 6 * T + 1
    assert 6 * T + 2 == 29793968203157093288
    gamma = {}
    for i in (1, 2, 3):
        assert (P**i - 1) % 6 == 0
        for k in range(1, 6):
            gamma[(i, k)] = f2_pow((9, 1), k * (P**i - 1) // 6)
    return gamma


def hard_part_chain():
    """the exponent the chain of pairing.hpp (final_exp_hard) computes, as an integer: y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 by the steps written there"""
    x = T
    y0, y1, y2, y3, y4, y5, y6 = P + P**2 + P**3, -1, x * x * P**2, -x * P, -(x + x * x * P), -x * x, -(x**3 + x**3 * P)
    t0 = 2 * y6; t0 += y4; t0 += y5
    t1 = y3 + y5; t1 += t0
    t0 += y2
    t1 *= 2; t1 += t0; t1 *= 2
    t0 = t1 + y1
    t1 += y0
    t0 *= 2; t0 += t1
    return t0


def check_exponent():
    l2, l1, l0 = 6 * T * T + 1, -36 * T**3 - 18 * T * T - 12 * T + 1, -36 * T**3 - 30 * T * T - 18 * T - 2
    assert (P**4 - P**2 + 1) % R == 0
    hard = (P**4 - P**2 + 1) // R
    assert P**3 + l2 * P**2 + l1 * P + l0 == hard, "lambda decomposition is not the exact hard exponent"
    assert hard_part_chain() == hard, "the chain does not compute the exact hard exponent"
    assert (P**6 - 1) * (P**2 + 1) * hard == (P**12 - 1) // R


def limbs32(x):
    return ", ".join("0x%08xu" % ((x >> (32 * i)) & 0xffffffff) for i in range(8))


def block(gamma):
    mont = lambda a: a * (1 << 256) % P
    lines = [BEGIN,
             "// FROB_GAMMA[i - 1][k - 1] = xi^(k (p^i - 1) / 6) as {c0, c1}, 8 x 32-bit Montgomery limbs each",
             "#define ZK_FQ12_FROB_GAMMA { \\"]
    for i in (1, 2, 3):
        lines.append("  { \\")
        for k in range(1, 6):
            c0, c1 = gamma[(i, k)]
            lines.append("    {%s, %s}%s \\" % (limbs32(mont(c0)), limbs32(mont(c1)), "," if k < 5 else ""))
        lines.append("  }%s \\" % ("," if i < 3 else ""))
    lines.append("}")
    lines.append(END)
    return "\n".join(lines)


if __name__ == "__main__":
    check_exponent()
    text = block(derive())
    if "--write" in sys.argv:
        with open(HEADER) as f:
            src = f.read()
        a, b = src.index(BEGIN), src.index(END) + len(END)
        with open(HEADER, "w") as f:
            f.write(src[:a] + text + src[b:])
        print("wrote", os.path.relpath(HEADER, ROOT))
    else:
        print(text)
