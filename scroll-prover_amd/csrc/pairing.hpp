// pairing.hpp -- the optimal ate pairing of BN254: e(P, Q) for P in G1 (64-byte affine), Q in G2 (128-byte affine on the twist y^2 = x^3 + 3 / xi), value in
// GT inside Fq12 (fq12.hpp).  Specification: oracle/pairing.py -- Miller loop over 6 t + 2 = 29793968203157093288 (t = 4965661367192848881), the two closing lines
// through Q1 = pi(Q) and -Q2 = -pi^2(Q), then f^((p^12 - 1) / r).  What final_exp returns EQUALS the oracle's final_exponentiation of its own Miller value; the
// Miller value itself differs by factors in proper subfields (the lines are scaled by elements of Fq2), which the easy part removes.
//
// Untwist: psi(x, y) = (x w^2, y w^3).  The line through psi(T) with slope lambda' = lambda w (lambda the slope on the twist), at P = (xP, yP):
//     -yP + lambda xP w + (y - lambda x) w^3         (times any non-zero element of Fq2)
// so a line value has three of six Fq2 coefficients: l0 at 1, l1 at w, l3 at w^3 (Fq12T::mul_sparse).
// T is held in homogeneous projective coordinates (x = X / Z, y = Y / Z): no inversion inside the loop.  With b' = 3 / xi:
//   doubling (tangent at T, scaled by 2 Y Z^2 / Z):   l0 = -2 Y Z yP,   l1 = 3 X^2 xP,   l3 = 3 b' Z^2 - Y^2
//     B = Y^2, E = 3 b' Z^2, F = 3 E, H = 2 Y Z:      X3 = 2 X Y (B - F),   Y3 = (B + F)^2 - 12 E^2,   Z3 = 4 B H
//   addition of the affine Q = (x2, y2) (chord, scaled by mu):   theta = Y - y2 Z, mu = X - x2 Z:   l0 = -mu yP,   l1 = theta xP,   l3 = mu y2 - theta x2
//     C = theta^2, D = mu^2, E = mu D, F = Z C, G = X D, H = E + F - 2 G:      X3 = mu H,   Y3 = theta (G - H) - E Y,   Z3 = Z E
// (the formulas of Costello, Lange and Naehrig, "Faster pairing computations on curves with high-degree twists", PKC 2010, for a twist of type D, re-derived
// from the affine chord-and-tangent rule; DESIGN.md section 18 has the derivation).
// Every lane walks the same constant bit string: the only branches are on bits of 6 t + 2 and of t.  An identity on either side runs the loop on zeros -- nothing
// is inverted, so nothing can fault -- and the result is replaced by 1 at the end.  For a Q outside the subgroup of order r the value is unspecified.
//
// Final exponentiation: easy part f^((p^6 - 1)(p^2 + 1)); hard part EXACTLY (p^4 - p^2 + 1) / r = p^3 + l2 p^2 + l1 p + l0 with
//   l2 = 6 t^2 + 1,  l1 = -36 t^3 - 18 t^2 - 12 t + 1,  l0 = -36 t^3 - 30 t^2 - 18 t - 2
// (Scott, Benger, Charlemagne, Dominguez Perez, Kachisa, Pairing 2009): three exponentiations by t, Frobenius maps, and the vectorial addition chain for
// y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36.  tools/gen_pairing_constants.py checks the identity and the chain as integers.
#pragma once
#include "g1.hpp"
#include "fq12.hpp"

namespace zk {

constexpr uint64_t BN_T = 4965661367192848881ull;              // 0x44e992b44a6909f1, 63 bits
constexpr uint64_t BN_ATE_LOW = 0x9d797039be763ba8ull;         // 6 t + 2 = 2^64 + this: the top bit is the starting value T = Q
static_assert(BN_ATE_LOW == 6ull * BN_T + 2ull, "6 t + 2 modulo 2^64");

struct g2_proj_t { fe2_t x, y, z; };

// 3 b' = 9 / (9 + u) (one inversion: formed once on the host and handed to the kernels)
ZK_HD fe2_t g2_twist_3b() { const fe2_t b = g2_twist_b(); return Fq2::add(Fq2::dbl(b), b); }
// y^2 == x^3 + 3, or the identity
template <class F = Fq> ZK_HD bool g1_is_on_curve(const g1_affine_t &p) {
  if (g1_affine_is_identity(p)) return true;
  fe_t three = Fq::one(); three = Fq::add(Fq::dbl(three), three);
  return Fq::eq(F::sqr(p.y), Fq::add(F::mul(F::sqr(p.x), p.x), three));
}

template <class F2> struct PairingT {
  using F6 = Fq6T<F2>;
  using F12 = Fq12T<F2>;

  // T <- 2 T and the tangent at T evaluated at P (xP, nyP = -yP)
  static ZK_HDN void dbl_step(g2_proj_t &T, const fe2_t &b3, const fe_t &xP, const fe_t &nyP, fe2_t &l0, fe2_t &l1, fe2_t &l3) {
    const fe2_t B = F2::sqr(T.y), C = F2::sqr(T.z), E = F2::mul(b3, C), F = F2::add(F2::dbl(E), E);
    const fe2_t H = F2::sub(F2::sub(F2::sqr(F2::add(T.y, T.z)), B), C);
    fe2_t X2 = F2::sqr(T.x); X2 = F2::add(F2::dbl(X2), X2);
    l0 = F6::mul2_fq(H, nyP); l1 = F6::mul2_fq(X2, xP); l3 = F2::sub(E, B);
    const fe2_t XY = F2::mul(T.x, T.y), E2 = F2::sqr(E);
    const fe2_t E2x4 = F2::dbl(F2::dbl(E2)), E2x12 = F2::add(F2::dbl(E2x4), E2x4);
    T.x = F2::mul(F2::dbl(XY), F2::sub(B, F));
    T.y = F2::sub(F2::sqr(F2::add(B, F)), E2x12);
    T.z = F2::dbl(F2::dbl(F2::mul(B, H)));
  }
  // T <- T + Q and the chord through T and Q evaluated at P
  static ZK_HDN void add_step(g2_proj_t &T, const g2_affine_t &Q, const fe_t &xP, const fe_t &nyP, fe2_t &l0, fe2_t &l1, fe2_t &l3) {
    const fe2_t theta = F2::sub(T.y, F2::mul(Q.y, T.z)), mu = F2::sub(T.x, F2::mul(Q.x, T.z));
    l0 = F6::mul2_fq(mu, nyP); l1 = F6::mul2_fq(theta, xP); l3 = F2::sub(F2::mul(mu, Q.y), F2::mul(theta, Q.x));
    const fe2_t C = F2::sqr(theta), D = F2::sqr(mu), E = F2::mul(mu, D), F = F2::mul(T.z, C), G = F2::mul(T.x, D);
    const fe2_t H = F2::sub(F2::add(E, F), F2::dbl(G));
    T.x = F2::mul(mu, H);
    T.y = F2::sub(F2::mul(theta, F2::sub(G, H)), F2::mul(E, T.y));
    T.z = F2::mul(T.z, E);
  }
  // the value before the final exponentiation; 1 when P or Q is the identity
  ZK_HD static fe12_t miller_loop(const g1_affine_t &P, const g2_affine_t &Q, const fe2_t &b3) {
    const fe_t nyP = Fq::neg(P.y);
    g2_proj_t T; T.x = Q.x; T.y = Q.y; T.z = F2::one();
    fe12_t f = F12::one();
    fe2_t l0, l1, l3;
    for (int i = 63; i >= 0; i--) {
      f = F12::sqr(f);
      dbl_step(T, b3, P.x, nyP, l0, l1, l3);
      f = F12::mul_sparse(f, l0, l1, l3);
      if ((BN_ATE_LOW >> i) & 1) {
        add_step(T, Q, P.x, nyP, l0, l1, l3);
        f = F12::mul_sparse(f, l0, l1, l3);
      }
    }
    g2_affine_t Q1, nQ2;   // pi(Q) and -pi^2(Q) on the twist: x at w^2, y at w^3
    Q1.x = F2::mul(F6::conj2(Q.x), fq12_frob_gamma(1, 2)); Q1.y = F2::mul(F6::conj2(Q.y), fq12_frob_gamma(1, 3));
    nQ2.x = F2::mul(Q.x, fq12_frob_gamma(2, 2)); nQ2.y = F2::neg(F2::mul(Q.y, fq12_frob_gamma(2, 3)));
    add_step(T, Q1, P.x, nyP, l0, l1, l3);
    f = F12::mul_sparse(f, l0, l1, l3);
    add_step(T, nQ2, P.x, nyP, l0, l1, l3);
    f = F12::mul_sparse(f, l0, l1, l3);
    if (g1_affine_is_identity(P) || g2_affine_is_identity(Q)) f = F12::one();
    return f;
  }
  // a^t for a in the cyclotomic subgroup
  static ZK_HDN fe12_t exp_by_t(const fe12_t &a) {
    fe12_t r = a;
    for (int i = 61; i >= 0; i--) {
      r = F12::cyclotomic_sqr(r);
      if ((BN_T >> i) & 1) r = F12::mul(r, a);
    }
    return r;
  }
  // f^((p^6 - 1)(p^2 + 1)): lands in the cyclotomic subgroup, where conj is the inverse.  0 -> 0
  ZK_HD static fe12_t final_exp_easy(const fe12_t &f) {
    const fe12_t g = F12::mul(F12::conj(f), F12::inv(f));
    return F12::mul(F12::template frobenius<2>(g), g);
  }
  // f^((p^4 - p^2 + 1) / r), exactly, for f in the cyclotomic subgroup
  ZK_HD static fe12_t final_exp_hard(const fe12_t &f) {
    const fe12_t fx = exp_by_t(f), fx2 = exp_by_t(fx), fx3 = exp_by_t(fx2);
    const fe12_t y0 = F12::mul(F12::mul(F12::template frobenius<1>(f), F12::template frobenius<2>(f)), F12::template frobenius<3>(f));
    const fe12_t y1 = F12::conj(f);
    const fe12_t y2 = F12::template frobenius<2>(fx2);
    const fe12_t y3 = F12::conj(F12::template frobenius<1>(fx));
    const fe12_t y4 = F12::conj(F12::mul(fx, F12::template frobenius<1>(fx2)));
    const fe12_t y5 = F12::conj(fx2);
    const fe12_t y6 = F12::conj(F12::mul(fx3, F12::template frobenius<1>(fx3)));
    fe12_t t0 = F12::cyclotomic_sqr(y6); t0 = F12::mul(t0, y4); t0 = F12::mul(t0, y5);
    fe12_t t1 = F12::mul(y3, y5); t1 = F12::mul(t1, t0);
    t0 = F12::mul(t0, y2);
    t1 = F12::cyclotomic_sqr(t1); t1 = F12::mul(t1, t0); t1 = F12::cyclotomic_sqr(t1);
    t0 = F12::mul(t1, y1);
    t1 = F12::mul(t1, y0);
    t0 = F12::cyclotomic_sqr(t0);
    return F12::mul(t0, t1);
  }
  ZK_HD static fe12_t final_exp(const fe12_t &f) { return final_exp_hard(final_exp_easy(f)); }
};

using Pairing = PairingT<Fq2>;
using PairingPs = PairingT<Fq2ps>;

#if defined(__HIPCC__)
// ---- kernels of mi355_pairing_products_host (lib_pairing.hip).  One lane per pair / per product / per group, workgroups of one wave: the work is latency-bound
// at the sizes a verifier has (2 pairs), and a lane's Fq12 operands live in scratch whatever the workgroup size.
constexpr uint32_t PAIRING_THREADS = 64;
static_assert(sizeof(fe12_t) == 384 && sizeof(g1_affine_t) == 64 && sizeof(g2_affine_t) == 128, "ABI record sizes");

// every P on y^2 = x^3 + 3 and every Q on the twist (or the identity); bad[0] / bad[1] = the first bad P / Q by an atomic minimum (preset 0xffffffff)
__global__ void __launch_bounds__(PAIRING_THREADS) k_pairing_validate(const g1_affine_t *__restrict__ P, const g2_affine_t *__restrict__ Q, uint32_t n, fe2_t b, uint32_t *__restrict__ bad) {
  const uint32_t i = blockIdx.x * PAIRING_THREADS + threadIdx.x;
  if (i >= n) return;
  if (!g1_is_on_curve<FqPs>(P[i])) atomicMin(&bad[0], i);
  if (!g2_is_on_curve_b<Fq2ps>(Q[i], b)) atomicMin(&bad[1], i);
}
// out[i] = the Miller value of (P[i], Q[i]); 1 for a pair with an identity.  All lanes walk the same bit string of 6 t + 2.
__global__ void __launch_bounds__(PAIRING_THREADS) k_pairing_miller(const g1_affine_t *__restrict__ P, const g2_affine_t *__restrict__ Q, uint32_t n, fe2_t b3, fe12_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * PAIRING_THREADS + threadIdx.x;
  if (i >= n) return;
  out[i] = PairingPs::miller_loop(P[i], Q[i], b3);
}
// one level of the product tree inside every group: `groups` runs of len_in values become runs of ceil(len_in / 2); an odd tail is copied.
// in and out are different buffers (a lane reads what another lane's slot would overwrite)
__global__ void __launch_bounds__(PAIRING_THREADS) k_pairing_reduce(const fe12_t *__restrict__ in, fe12_t *__restrict__ out, uint32_t groups, uint32_t len_in) {
  const uint32_t len_out = (len_in + 1) / 2, t = blockIdx.x * PAIRING_THREADS + threadIdx.x;
  if (t >= groups * len_out) return;
  const uint32_t grp = t / len_out, j = t - grp * len_out;
  const fe12_t *src = in + (size_t)grp * len_in + 2 * j;
  fe12_t a = src[0];
  if (2 * j + 1 < len_in) a = Fq12ps::mul(a, src[1]);
  out[(size_t)grp * len_out + j] = a;
}
// gt[grp] = prod[grp]^((p^12 - 1) / r), is_one[grp] = (gt[grp] == 1); either output may be null
__global__ void __launch_bounds__(PAIRING_THREADS) k_pairing_final_exp(const fe12_t *__restrict__ prod, uint32_t groups, fe12_t *__restrict__ gt, uint32_t *__restrict__ is_one) {
  const uint32_t grp = blockIdx.x * PAIRING_THREADS + threadIdx.x;
  if (grp >= groups) return;
  const fe12_t r = PairingPs::final_exp(prod[grp]);
  if (gt) gt[grp] = r;
  if (is_one) is_one[grp] = Fq12ps::is_one(r) ? 1u : 0u;
}
#endif  // __HIPCC__

}  // namespace zk
