// pairing_selftest.cpp -- TEST INFRASTRUCTURE: compiles the __host__ __device__ tower and pairing code that the pairing kernels run (fq12.hpp, pairing.hpp) for
// the CPU with plain g++, so that it can be checked against oracle/pairing.py without a GPU (tests/test_pairing_on_host.py loads it as a shared object).
// Every function takes `ps`: 1 = the product-scanning multiplier (Fq2ps, what the kernels instantiate), 0 = the plain CIOS multiplier.
// With -DPAIRING_SELFTEST_MAIN the file is a program of its own (bilinearity and tower identities on the generators) for a run under
// -fsanitize=address,undefined.  Never shipped, never linked into libmi355zk.so.
#include "../../scroll-prover_amd/csrc/pairing.hpp"
#include <stdio.h>
#include <string.h>
using namespace zk;

#define BOTH(ps, expr) ((ps) ? [&] { using F12 = Fq12ps; using F6 = Fq6T<Fq2ps>; using PR = PairingPs; (void)sizeof(F6); (void)sizeof(PR); return expr; }() \
                             : [&] { using F12 = Fq12; using F6 = Fq6T<Fq2>; using PR = Pairing; (void)sizeof(F6); (void)sizeof(PR); return expr; }())

static const fe12_t &E12(const void *p) { return *(const fe12_t *)p; }
static const fe6_t &E6(const void *p) { return *(const fe6_t *)p; }
static const fe2_t &E2(const void *p) { return *(const fe2_t *)p; }

extern "C" {
void pst_fq6_mul(int ps, void *o, const void *a, const void *b) { *(fe6_t *)o = BOTH(ps, F6::mul(E6(a), E6(b))); }
void pst_fq6_inv(int ps, void *o, const void *a) { *(fe6_t *)o = BOTH(ps, F6::inv(E6(a))); }
void pst_fq12_add(int ps, void *o, const void *a, const void *b) { *(fe12_t *)o = BOTH(ps, F12::add(E12(a), E12(b))); }
void pst_fq12_sub(int ps, void *o, const void *a, const void *b) { *(fe12_t *)o = BOTH(ps, F12::sub(E12(a), E12(b))); }
void pst_fq12_neg(int ps, void *o, const void *a) { *(fe12_t *)o = BOTH(ps, F12::neg(E12(a))); }
void pst_fq12_mul(int ps, void *o, const void *a, const void *b) { *(fe12_t *)o = BOTH(ps, F12::mul(E12(a), E12(b))); }
void pst_fq12_sqr(int ps, void *o, const void *a) { *(fe12_t *)o = BOTH(ps, F12::sqr(E12(a))); }
void pst_fq12_inv(int ps, void *o, const void *a) { *(fe12_t *)o = BOTH(ps, F12::inv(E12(a))); }
void pst_fq12_conj(int ps, void *o, const void *a) { *(fe12_t *)o = BOTH(ps, F12::conj(E12(a))); }
void pst_fq12_cyclotomic_sqr(int ps, void *o, const void *a) { *(fe12_t *)o = BOTH(ps, F12::cyclotomic_sqr(E12(a))); }
void pst_fq12_frobenius(int ps, int i, void *o, const void *a) {
  *(fe12_t *)o = BOTH(ps, i == 1 ? F12::template frobenius<1>(E12(a)) : i == 2 ? F12::template frobenius<2>(E12(a)) : F12::template frobenius<3>(E12(a)));
}
void pst_fq12_mul_sparse(int ps, void *o, const void *a, const void *l0, const void *l1, const void *l3) { *(fe12_t *)o = BOTH(ps, F12::mul_sparse(E12(a), E2(l0), E2(l1), E2(l3))); }
void pst_fq12_from_sparse(void *o, const void *l0, const void *l1, const void *l3) { *(fe12_t *)o = Fq12::from_sparse(E2(l0), E2(l1), E2(l3)); }
void pst_frob_gamma(int i, int k, void *o) { *(fe2_t *)o = fq12_frob_gamma(i, k); }
void pst_miller(int ps, void *o, const void *p_g1, const void *q_g2) { const fe2_t b3 = g2_twist_3b(); *(fe12_t *)o = BOTH(ps, PR::miller_loop(*(const g1_affine_t *)p_g1, *(const g2_affine_t *)q_g2, b3)); }
void pst_final_exp_easy(int ps, void *o, const void *a) { *(fe12_t *)o = BOTH(ps, PR::final_exp_easy(E12(a))); }
void pst_final_exp(int ps, void *o, const void *a) { *(fe12_t *)o = BOTH(ps, PR::final_exp(E12(a))); }
void pst_pairing(int ps, void *o, const void *p_g1, const void *q_g2) {
  const fe2_t b3 = g2_twist_3b();
  *(fe12_t *)o = BOTH(ps, PR::final_exp(PR::miller_loop(*(const g1_affine_t *)p_g1, *(const g2_affine_t *)q_g2, b3)));
}
int pst_g1_on_curve(const void *p_g1) { return g1_is_on_curve<FqPs>(*(const g1_affine_t *)p_g1) ? 1 : 0; }
}

#ifdef PAIRING_SELFTEST_MAIN
#include "../../scroll-prover_amd/csrc/g1.hpp"
static int fails = 0;
static void expect(bool ok, const char *what) { printf("%s %s\n", ok ? "ok  " : "FAIL", what); if (!ok) fails++; }
int main() {
  g1_affine_t G; fe_t c = Fq::zero(); c.l[0] = 1; G.x = Fq::from_canonical(c); c.l[0] = 2; G.y = Fq::from_canonical(c);
  const g2_affine_t H = {{{{0x02bc2026u, 0x8e83b5d1u, 0x497b0172u, 0xdceb1935u, 0x97811adfu, 0xfbb82647u, 0xaf96503bu, 0x19573841u}},
                          {{0xa84c6140u, 0xafb4737du, 0x5802d8c4u, 0x6043dd5au, 0x52a02f86u, 0x09e950fcu, 0x3aea7b6bu, 0x14fef083u}}},
                         {{{0x886be9f6u, 0x619dfa9du, 0xf59e9b78u, 0xfe7fd297u, 0x231b7dfeu, 0xff9e1a62u, 0xae9e4206u, 0x28fd7eebu}},
                          {{0xc71856eeu, 0x64095b56u, 0x327d3cbbu, 0xdc57f922u, 0x33351076u, 0x55f935beu, 0x93fd6482u, 0x0da4a0e6u}}}};
  expect(g1_is_on_curve(G) && g2_is_on_curve(H), "generators on their curves");
  const g2_affine_t H2 = g2_xyzz_to_affine(g2_xyzz_dbl_affine(H));
  g1_xyzz_t g2x = g1_xyzz_from_affine(G); g1_xyzz_madd(g2x, G); const g1_affine_t G2x = g1_xyzz_to_affine(g2x);
  for (int ps = 0; ps < 2; ps++) {
    fe12_t e, e2a, e2b, en, t, u;
    pst_pairing(ps, &e, &G, &H); pst_pairing(ps, &e2a, &G2x, &H); pst_pairing(ps, &e2b, &G, &H2);
    pst_fq12_sqr(ps, &t, &e);
    expect(!Fq12::is_one(e) && Fq12::eq(t, e2a) && Fq12::eq(t, e2b), "e(2 G1, G2) == e(G1, 2 G2) == e(G1, G2)^2 != 1");
    const g1_affine_t nG = g1_affine_neg(G);
    pst_pairing(ps, &en, &nG, &H); pst_fq12_mul(ps, &t, &e, &en);
    expect(Fq12::is_one(t), "e(G1, G2) e(-G1, G2) == 1");
    pst_fq12_cyclotomic_sqr(ps, &t, &e); pst_fq12_sqr(ps, &u, &e);
    expect(Fq12::eq(t, u), "cyclotomic squaring == squaring on GT");
    pst_miller(ps, &t, &G, &H); pst_fq12_inv(ps, &u, &t); pst_fq12_mul(ps, &u, &u, &t);
    expect(Fq12::is_one(u), "f * f^-1 == 1 on a Miller value");
    fe12_t f1 = t, f2;
    for (int i = 0; i < 12; i++) { pst_fq12_frobenius(ps, 1, &f2, &f1); f1 = f2; }
    expect(Fq12::eq(f1, t), "Frobenius twelve times is the identity");
    const g1_affine_t O1 = {Fq::zero(), Fq::zero()}; g2_affine_t O2; memset(&O2, 0, sizeof O2);
    pst_pairing(ps, &t, &O1, &H); pst_pairing(ps, &u, &G, &O2);
    expect(Fq12::is_one(t) && Fq12::is_one(u), "an identity on either side gives 1");
  }
  printf("%s\n", fails ? "FAILED" : "all passed");
  return fails ? 1 : 0;
}
#endif
