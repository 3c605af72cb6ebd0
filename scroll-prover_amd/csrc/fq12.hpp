// fq12.hpp -- the tower above Fq2 for the BN254 pairing: Fq6 = Fq2[v] / (v^3 - xi), xi = 9 + u, and Fq12 = Fq6[w] / (w^2 - v).
// fe12_t = {c0: {c0, c1, c2}, c1: {c0, c1, c2}} = 384 B of Montgomery limbs == halo2curves' bn256::Fq12 (c0.c0.c0 | c0.c0.c1 | c0.c1.c0 | ... | c1.c2.c1), so a
// GT element crosses the C-ABI without conversion.  Both levels take the Fq2 flavour as a template argument, the way the G2 point functions do
// (Fq2 = plain CIOS multiplier, Fq2ps = the product-scanning multiplier; same fully reduced values).
// With w^6 = xi the twelve Fq coordinates are those of Fq[w] / (w^12 - 18 w^6 + 82), the oracle's representation: the coefficient a0 + a1 u at w^j v^i adds
// a0 - 9 a1 at w^(2 i + j) and a1 at w^(2 i + j + 6).  The "w-index" k = 2 i + j orders the six Fq2 coefficients below wherever a loop walks them.
// Inlining: an Fq12 product is 54 field multiplications (~300 instructions each on gfx950).  The Fq2 level is inlined as everywhere else; the products of the two
// levels here are calls on the device (ZK_HDN), so the Miller loop and the final exponentiation stay a few tens of thousands of instructions, not millions; their
// operands then live in scratch (profiles/pairing.md has the figures).
#pragma once
#include "g2.hpp"

#if defined(__HIPCC__)
#define ZK_HDN __host__ __device__ __noinline__
#else
#define ZK_HDN inline
#endif

// ---- BEGIN GENERATED (tools/gen_pairing_constants.py --write)
// FROB_GAMMA[i - 1][k - 1] = xi^(k (p^i - 1) / 6) as {c0, c1}, 8 x 32-bit Montgomery limbs each
#define ZK_FQ12_FROB_GAMMA { \
  { \
    {0x33144907u, 0xaf9ba696u, 0x87afb78au, 0xca6b1d73u, 0xf08a2087u, 0x11bded5eu, 0x1a1f3a7cu, 0x02f34d75u, 0x4c492d72u, 0xa222ae23u, 0x565de15bu, 0xd00f02a4u, 0x53dfc926u, 0xdc2ff3a2u, 0xb3899551u, 0x10a75716u}, \
    {0x4563ab30u, 0xb5773b10u, 0xa9aa6454u, 0x347f91c8u, 0x242e0991u, 0x7a007127u, 0x118214ecu, 0x1956bcd8u, 0xa0aa4757u, 0x6e849f1eu, 0x89f89141u, 0xaa1c7b6du, 0xfae0ca3au, 0xb6e713cdu, 0x4e82ebc3u, 0x26694fbbu}, \
    {0x2936b629u, 0xe4bbdd0cu, 0xe133bacbu, 0xbb30f162u, 0xf9645366u, 0x31a9d1b6u, 0xa500f8ddu, 0x253570beu, 0x5ffe77c7u, 0xa1d77ce4u, 0x7826d1dbu, 0x07affd11u, 0xbb7edc6bu, 0x6d16bd27u, 0x85defeccu, 0x2c872002u}, \
    {0x843abe92u, 0x7361d77fu, 0x273411fbu, 0xa5bb2bd3u, 0x4b3e2399u, 0x9c941f31u, 0xbb9fd3ecu, 0x15df9cddu, 0x4bd8c949u, 0x5dddfd15u, 0xa4445b60u, 0x62cb29a5u, 0x0c7dd2b9u, 0x37bc870au, 0x3171f0fdu, 0x24830a9du}, \
    {0x41690fe7u, 0xc970692fu, 0x27694b0bu, 0xe2403421u, 0x83c459e8u, 0x32bee66bu, 0x0ab08841u, 0x12aabcedu, 0x40aebfa9u, 0x0d485d23u, 0xab2fcc57u, 0x05193418u, 0x8a4910f5u, 0xd3b0a40bu, 0x35d2925au, 0x2f21ebb5u} \
  }, \
  { \
    {0x00fa1bf2u, 0xca8d8005u, 0x68b39769u, 0xf0c5d614u, 0xad0d4418u, 0x0e201271u, 0xbad856e6u, 0x04290f65u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, \
    {0x13e80b9cu, 0x3350c88eu, 0xdb5e56b9u, 0x7dce557cu, 0xb615564au, 0x6001b4b8u, 0x020217e0u, 0x2682e617u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, \
    {0x12edefaau, 0x68c34889u, 0x72aabf4fu, 0x8d087f68u, 0x09081231u, 0x51e1a247u, 0x4729c0fau, 0x2259d6b1u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, \
    {0xd782e155u, 0x71930c11u, 0xffbe3323u, 0xa6bb947cu, 0xd4741444u, 0xaa303344u, 0x26594943u, 0x2c3b3f0du, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}, \
    {0xc494f1abu, 0x08cfc388u, 0x8d1373d4u, 0x19b31514u, 0xcb6c0213u, 0x584e90fdu, 0xdf2f8849u, 0x09e1685bu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u} \
  }, \
  { \
    {0x4e46d97du, 0x36531618u, 0xd4c96d9fu, 0x0af7129eu, 0xca1009b5u, 0x659da72fu, 0x83a20d23u, 0x08116d89u, 0xc39c1939u, 0xb1df4af7u, 0x8a73bf7fu, 0x3d9f0287u, 0x8caf0ae0u, 0x9b222092u, 0xeff054a6u, 0x26684515u}, \
    {0x16ad6badu, 0xc9af22f7u, 0x4aa662b2u, 0xb311782au, 0xe248c7f4u, 0x19eeaf64u, 0xe3439f82u, 0x20273e77u, 0xf7ce93acu, 0xacc02860u, 0x7ba76b4cu, 0x3933d581u, 0x446c8467u, 0x69e6188bu, 0x4417cc55u, 0x0a46036du}, \
    {0xaf46471eu, 0x5764af0au, 0x873e0fc1u, 0xdc50792eu, 0x881d04f6u, 0x86a673ffu, 0x3c30a74cu, 0x0b2eddb4u, 0x787e8580u, 0x9a490f32u, 0xf04af8b1u, 0x8fd16d7fu, 0xc6027bf2u, 0x4b39888eu, 0x5b52a15du, 0x03dd2e70u}, \
    {0x7b6762dfu, 0x448a93a5u, 0x28fdeadfu, 0xbfd62df5u, 0x0e9bd47au, 0xd858f5d0u, 0x3476ec58u, 0x06b03d4du, 0xbcc936d1u, 0x2b19daf4u, 0x56f4299fu, 0xa1a54e7au, 0x5adeaef1u, 0xb533eee0u, 0x84dda0b2u, 0x170c812bu}, \
    {0x75cf559fu, 0xe0bc4b22u, 0xc154e60fu, 0xc238b945u, 0x929a7d5eu, 0x803982a5u, 0xf7e4a37eu, 0x15ce052du, 0xbf3799a7u, 0x2d28efbdu, 0x1ad60773u, 0x9b097e3cu, 0xaf4a535bu, 0x982d4113u, 0xe3056063u, 0x24e18991u} \
  } \
}
// ---- END GENERATED

namespace zk {

struct fe6_t { fe2_t c0, c1, c2; };
struct alignas(16) fe12_t { fe6_t c0, c1; };

// xi^(k (p^i - 1) / 6), i = 1 .. 3, k = 0 .. 5 (k = 0: one)
ZK_HD fe2_t fq12_frob_gamma(int i, int k) {
  constexpr uint32_t tbl[3][5][16] = ZK_FQ12_FROB_GAMMA;
  fe2_t r;
  if (k == 0) { r.c0 = Fq::one(); r.c1 = Fq::zero(); return r; }
  for (int j = 0; j < 8; j++) { r.c0.l[j] = tbl[i - 1][k - 1][j]; r.c1.l[j] = tbl[i - 1][k - 1][8 + j]; }
  return r;
}

template <class F2> struct Fq6T {
  ZK_HD static fe2_t conj2(const fe2_t &a) { fe2_t r; r.c0 = a.c0; r.c1 = Fq::neg(a.c1); return r; }
  // (a0 + a1 u)(9 + u) = 9 a0 - a1 + (a0 + 9 a1) u
  ZK_HD static fe2_t mul_xi(const fe2_t &a) {
    const fe2_t a2 = F2::dbl(a), a4 = F2::dbl(a2), a9 = F2::add(F2::dbl(a4), a);
    fe2_t r; r.c0 = Fq::sub(a9.c0, a.c1); r.c1 = Fq::add(a9.c1, a.c0); return r;
  }
  // a * b for b in Fq (both coordinates by the same word)
  ZK_HD static fe2_t mul2_fq(const fe2_t &a, const fe_t &b) { fe2_t r; r.c0 = F2::fmul(a.c0, b); r.c1 = F2::fmul(a.c1, b); return r; }

  ZK_HD static fe6_t zero() { fe6_t r; r.c0 = F2::zero(); r.c1 = F2::zero(); r.c2 = F2::zero(); return r; }
  ZK_HD static fe6_t one() { fe6_t r; r.c0 = F2::one(); r.c1 = F2::zero(); r.c2 = F2::zero(); return r; }
  ZK_HD static bool is_zero(const fe6_t &a) { return F2::is_zero(a.c0) && F2::is_zero(a.c1) && F2::is_zero(a.c2); }
  ZK_HD static bool eq(const fe6_t &a, const fe6_t &b) { return F2::eq(a.c0, b.c0) && F2::eq(a.c1, b.c1) && F2::eq(a.c2, b.c2); }
  ZK_HD static fe6_t add(const fe6_t &a, const fe6_t &b) { fe6_t r; r.c0 = F2::add(a.c0, b.c0); r.c1 = F2::add(a.c1, b.c1); r.c2 = F2::add(a.c2, b.c2); return r; }
  ZK_HD static fe6_t sub(const fe6_t &a, const fe6_t &b) { fe6_t r; r.c0 = F2::sub(a.c0, b.c0); r.c1 = F2::sub(a.c1, b.c1); r.c2 = F2::sub(a.c2, b.c2); return r; }
  ZK_HD static fe6_t neg(const fe6_t &a) { fe6_t r; r.c0 = F2::neg(a.c0); r.c1 = F2::neg(a.c1); r.c2 = F2::neg(a.c2); return r; }
  ZK_HD static fe6_t dbl(const fe6_t &a) { return add(a, a); }
  // a * v: (a0 + a1 v + a2 v^2) v = xi a2 + a0 v + a1 v^2
  ZK_HD static fe6_t mul_v(const fe6_t &a) { fe6_t r; r.c0 = mul_xi(a.c2); r.c1 = a.c0; r.c2 = a.c1; return r; }
  // Karatsuba over three coefficients: 6 Fq2 products
  static ZK_HDN fe6_t mul(const fe6_t &a, const fe6_t &b) {
    const fe2_t t0 = F2::mul(a.c0, b.c0), t1 = F2::mul(a.c1, b.c1), t2 = F2::mul(a.c2, b.c2);
    const fe2_t m12 = F2::sub(F2::sub(F2::mul(F2::add(a.c1, a.c2), F2::add(b.c1, b.c2)), t1), t2);   // a1 b2 + a2 b1
    const fe2_t m01 = F2::sub(F2::sub(F2::mul(F2::add(a.c0, a.c1), F2::add(b.c0, b.c1)), t0), t1);   // a0 b1 + a1 b0
    const fe2_t m02 = F2::sub(F2::sub(F2::mul(F2::add(a.c0, a.c2), F2::add(b.c0, b.c2)), t0), t2);   // a0 b2 + a2 b0
    fe6_t r; r.c0 = F2::add(t0, mul_xi(m12)); r.c1 = F2::add(m01, mul_xi(t2)); r.c2 = F2::add(m02, t1); return r;
  }
  ZK_HD static fe6_t sqr(const fe6_t &a) { return mul(a, a); }
  // a * (b0 + b1 v): the Fq6 half of a sparse line value
  static ZK_HDN fe6_t mul_01(const fe6_t &a, const fe2_t &b0, const fe2_t &b1) {
    const fe2_t t0 = F2::mul(a.c0, b0), t1 = F2::mul(a.c1, b1);
    const fe2_t m01 = F2::sub(F2::sub(F2::mul(F2::add(a.c0, a.c1), F2::add(b0, b1)), t0), t1);
    fe6_t r; r.c0 = F2::add(t0, mul_xi(F2::mul(a.c2, b1))); r.c1 = m01; r.c2 = F2::add(F2::mul(a.c2, b0), t1); return r;
  }
  static ZK_HDN fe6_t mul_fq2(const fe6_t &a, const fe2_t &b) { fe6_t r; r.c0 = F2::mul(a.c0, b); r.c1 = F2::mul(a.c1, b); r.c2 = F2::mul(a.c2, b); return r; }
  // the cofactors c_i with a (c0 + c1 v + c2 v^2) = N(a) in Fq2, then ONE Fq2 inversion (itself a norm to Fq and one Fq::inv_sgcd); 0 -> 0
  static ZK_HDN fe6_t inv(const fe6_t &a) {
    const fe2_t c0 = F2::sub(F2::sqr(a.c0), mul_xi(F2::mul(a.c1, a.c2)));
    const fe2_t c1 = F2::sub(mul_xi(F2::sqr(a.c2)), F2::mul(a.c0, a.c1));
    const fe2_t c2 = F2::sub(F2::sqr(a.c1), F2::mul(a.c0, a.c2));
    const fe2_t n = F2::add(F2::mul(a.c0, c0), mul_xi(F2::add(F2::mul(a.c2, c1), F2::mul(a.c1, c2))));
    const fe2_t ni = F2::inv(n);
    fe6_t r; r.c0 = F2::mul(c0, ni); r.c1 = F2::mul(c1, ni); r.c2 = F2::mul(c2, ni); return r;
  }
};

template <class F2> struct Fq12T {
  using F6 = Fq6T<F2>;
  ZK_HD static fe12_t zero() { fe12_t r; r.c0 = F6::zero(); r.c1 = F6::zero(); return r; }
  ZK_HD static fe12_t one() { fe12_t r; r.c0 = F6::one(); r.c1 = F6::zero(); return r; }
  ZK_HD static bool is_zero(const fe12_t &a) { return F6::is_zero(a.c0) && F6::is_zero(a.c1); }
  ZK_HD static bool eq(const fe12_t &a, const fe12_t &b) { return F6::eq(a.c0, b.c0) && F6::eq(a.c1, b.c1); }
  ZK_HD static bool is_one(const fe12_t &a) { return eq(a, one()); }
  ZK_HD static fe12_t add(const fe12_t &a, const fe12_t &b) { fe12_t r; r.c0 = F6::add(a.c0, b.c0); r.c1 = F6::add(a.c1, b.c1); return r; }
  ZK_HD static fe12_t sub(const fe12_t &a, const fe12_t &b) { fe12_t r; r.c0 = F6::sub(a.c0, b.c0); r.c1 = F6::sub(a.c1, b.c1); return r; }
  ZK_HD static fe12_t neg(const fe12_t &a) { fe12_t r; r.c0 = F6::neg(a.c0); r.c1 = F6::neg(a.c1); return r; }
  // a^(p^6): w -> -w.  The inverse of an element of the cyclotomic subgroup (norm 1 over Fq6)
  ZK_HD static fe12_t conj(const fe12_t &a) { fe12_t r; r.c0 = a.c0; r.c1 = F6::neg(a.c1); return r; }
  // (a0 + a1 w)(b0 + b1 w) = a0 b0 + a1 b1 v + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) w: 3 Fq6 products
  static ZK_HDN fe12_t mul(const fe12_t &a, const fe12_t &b) {
    const fe6_t t0 = F6::mul(a.c0, b.c0), t1 = F6::mul(a.c1, b.c1);
    fe12_t r;
    r.c1 = F6::sub(F6::sub(F6::mul(F6::add(a.c0, a.c1), F6::add(b.c0, b.c1)), t0), t1);
    r.c0 = F6::add(t0, F6::mul_v(t1));
    return r;
  }
  // (a0 + a1 w)^2 = (a0 + a1)(a0 + a1 v) - t - t v + 2 t w, t = a0 a1: 2 Fq6 products
  static ZK_HDN fe12_t sqr(const fe12_t &a) {
    const fe6_t t = F6::mul(a.c0, a.c1);
    fe12_t r;
    r.c0 = F6::sub(F6::sub(F6::mul(F6::add(a.c0, a.c1), F6::add(a.c0, F6::mul_v(a.c1))), t), F6::mul_v(t));
    r.c1 = F6::dbl(t);
    return r;
  }
  // conj(a) / N(a), N(a) = a0^2 - a1^2 v in Fq6; the norms go down the tower to one Fq::inv_sgcd.  0 -> 0
  static ZK_HDN fe12_t inv(const fe12_t &a) {
    const fe6_t n = F6::sub(F6::sqr(a.c0), F6::mul_v(F6::sqr(a.c1)));
    const fe6_t ni = F6::inv(n);
    fe12_t r; r.c0 = F6::mul(a.c0, ni); r.c1 = F6::neg(F6::mul(a.c1, ni)); return r;
  }
  // a * (l0 + l1 w + l3 w^3), the value of a line of the twist at a point of G1: l0 at w^0 (c0.c0), l1 at w (c1.c0), l3 at w^3 = v w (c1.c1).
  // With L0 = (l0, 0, 0) and L1 = (l1, l3, 0): a0 L0 + a1 L1 v + ((a0 + a1)(L0 + L1) - a0 L0 - a1 L1) w -- 3 + 5 + 5 Fq2 products
  static ZK_HDN fe12_t mul_sparse(const fe12_t &a, const fe2_t &l0, const fe2_t &l1, const fe2_t &l3) {
    const fe6_t t0 = F6::mul_fq2(a.c0, l0), t1 = F6::mul_01(a.c1, l1, l3);
    fe12_t r;
    r.c1 = F6::sub(F6::sub(F6::mul_01(F6::add(a.c0, a.c1), F2::add(l0, l1), l3), t0), t1);
    r.c0 = F6::add(t0, F6::mul_v(t1));
    return r;
  }
  // the same line value as a dense element (tests compare the two products)
  ZK_HD static fe12_t from_sparse(const fe2_t &l0, const fe2_t &l1, const fe2_t &l3) { fe12_t r = zero(); r.c0.c0 = l0; r.c1.c0 = l1; r.c1.c1 = l3; return r; }
  // a^(p^I), I = 1, 2, 3: the coefficient at w-index k goes to conj^I(coefficient) * xi^(k (p^I - 1) / 6)
  template <int I> static ZK_HDN fe12_t frobenius(const fe12_t &a) {
    fe12_t r;
    const fe2_t *s[6] = {&a.c0.c0, &a.c1.c0, &a.c0.c1, &a.c1.c1, &a.c0.c2, &a.c1.c2};
    fe2_t *d[6] = {&r.c0.c0, &r.c1.c0, &r.c0.c1, &r.c1.c1, &r.c0.c2, &r.c1.c2};
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const fe2_t c = (I & 1) ? F6::conj2(*s[k]) : *s[k];
      *d[k] = k == 0 ? c : F2::mul(c, fq12_frob_gamma(I, k));
    }
    return r;
  }
  // a^2 for a in the cyclotomic subgroup (a^(p^6 + 1) = 1 and a^(p^4 - p^2 + 1) = 1, which every value after the easy part of the final exponentiation
  // satisfies): Granger and Scott, "Faster squaring in the cyclotomic subgroup of sixth degree extensions" (PKC 2010).  Fq12 over Fq4 = Fq2[s] / (s^2 - xi)
  // with the pairs (c0.c0, c1.c1), (c1.c0, c0.c2), (c0.c1, c1.c2): three Fq4 squarings, 9 Fq2 products instead of 12.  The result is NOT a^2 outside the subgroup.
  static ZK_HDN fe12_t cyclotomic_sqr(const fe12_t &a) {
    fe2_t t0, t1, t2, t3, t4, t5;
    sqr4(a.c0.c0, a.c1.c1, t0, t1);
    sqr4(a.c1.c0, a.c0.c2, t2, t3);
    sqr4(a.c0.c1, a.c1.c2, t4, t5);
    fe12_t r;
    r.c0.c0 = three_minus_two(t0, a.c0.c0); r.c1.c1 = three_plus_two(t1, a.c1.c1);
    r.c1.c0 = three_plus_two(F6::mul_xi(t5), a.c1.c0); r.c0.c2 = three_minus_two(t4, a.c0.c2);
    r.c0.c1 = three_minus_two(t2, a.c0.c1); r.c1.c2 = three_plus_two(t3, a.c1.c2);
    return r;
  }

 private:
  // (x + y s)^2 = x^2 + xi y^2 + 2 x y s in Fq4
  ZK_HD static void sqr4(const fe2_t &x, const fe2_t &y, fe2_t &o0, fe2_t &o1) {
    const fe2_t t = F2::mul(x, y);
    o0 = F2::sub(F2::sub(F2::mul(F2::add(x, y), F2::add(x, F6::mul_xi(y))), t), F6::mul_xi(t));
    o1 = F2::dbl(t);
  }
  ZK_HD static fe2_t three_minus_two(const fe2_t &t, const fe2_t &z) { const fe2_t d = F2::sub(t, z); return F2::add(F2::dbl(d), t); }   // 3 t - 2 z
  ZK_HD static fe2_t three_plus_two(const fe2_t &t, const fe2_t &z) { const fe2_t s = F2::add(t, z); return F2::add(F2::dbl(s), t); }    // 3 t + 2 z
};

using Fq6 = Fq6T<Fq2>;
using Fq12 = Fq12T<Fq2>;
using Fq12ps = Fq12T<Fq2ps>;

}  // namespace zk
