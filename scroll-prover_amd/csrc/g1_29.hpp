// g1_29.hpp -- XYZZ bucket accumulator on the 9 x 29-bit unsaturated field (fp29.hpp); used by k_msm_accumulate, whose
// time is entirely field multiplications.  Same formulas and exceptional cases as g1.hpp (madd-2008-s / mdbl-2008-s); what
// changes is the bookkeeping of lazy values.  Invariants of an accumulator between additions (p = Fq modulus):
//     x   limbs <= 2^29 + 8, value < 14 p          zz, zzz   tight (mul outputs), value < 1.1 p
//     y   limbs <= 2^30 - 2, value < 6.1 p         identity  <=> all limbs of zz are 0
// Bases arrive in the ABI form (8 x 32, R = 2^256) and are re-sliced on the fly (from_sat: value < 2^259, limbs < 2^29:
// only ever used as a multiplication operand).  Bounds of every intermediate are written next to it.
// The products are the chained multiplier (Fq29::mul_c / sqr_c / mul_sub_c); only the rare doubling branch of the mixed addition, which tightens
// its operands by a multiplication with one, and to_sat use the plain Fq29::mul.  The mixed addition keeps x NEGATED between additions (see
// g1_xyzz29_madd); the full addition and the doubling take and return plain accumulators.
#pragma once
#include "fp29.hpp"
#include "g1.hpp"

namespace zk {

struct g1_xyzz29_t { fe29_t x, y, zz, zzz; };

ZK_HD g1_xyzz29_t g1_xyzz29_identity() { g1_xyzz29_t r; r.x = Fq29::zero(); r.y = Fq29::zero(); r.zz = Fq29::zero(); r.zzz = Fq29::zero(); return r; }
ZK_HD bool g1_xyzz29_is_identity(const g1_xyzz29_t &p) { uint32_t o = 0; for (int i = 0; i < 9; i++) o |= p.zz.l[i]; return o == 0; }

// 64p with limbs >= 2^29 - 1 (top limb 0xc19139c > 2^27): -y for a from_sat() operand (limbs < 2^29, value < 2^259 = 54.4 p)
ZK_HD fe29_t fq29_neg_loaded(const fe29_t &y) {
  constexpr uint32_t c[9] = {0x3f3f51c0u, 0x21182dafu, 0x3ca8d3c1u, 0x3548b437u, 0x21765e04u, 0x36d0302au, 0x29b85044u, 0x37098d00u, 0xc19139bu};
  fe29_t r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = c[i] - y.l[i];
  return r;   // limbs < 2^30, value < 64 p
}

// 2 * (affine point) for tight coordinates xt, yt (< 1.1 p): mdbl-2008-s
ZK_HD g1_xyzz29_t g1_xyzz29_dbl_affine(const fe29_t &xt, const fe29_t &yt) {
  const fe29_t U = Fq29::dbl(yt);                                                   // limbs <= 2^30 - 2, < 2.2 p
  const fe29_t V = Fq29::sqr_c(U), W = Fq29::mul_c(U, V), S = Fq29::mul_c(xt, V);   // tight, < 1.1 p
  const fe29_t xx = Fq29::sqr_c(xt);
  const fe29_t M = Fq29::carry(Fq29::add(Fq29::dbl(xx), xx));                       // 3 x^2, limbs <= 2^29 + 8, < 3.3 p
  g1_xyzz29_t r;
  r.x = Fq29::sub8(Fq29::sqr_c(M), Fq29::dbl(S));                                   // < 1.1 p + 8 p
  const fe29_t t = Fq29::sub16(S, r.x);                                             // < 17.1 p
  r.y = Fq29::sub4(Fq29::mul_c(M, t), Fq29::mul_c(W, yt));                          // < 1.4 p + 4 p
  r.zz = V; r.zzz = W;
  return r;
}

// q is the identity (all-zero words in the ABI).  x alone decides: 3 is not a square in Fq (3^((p-1)/2) = -1), so y^2 = x^3 + 3 has no point with
// x = 0, and Montgomery x = 0 is the all-zero word pattern -- exact for every point of the curve, eight words instead of sixteen per gathered base.
ZK_HD bool g1_affine_is_identity_x(const g1_affine_t &q) { return Fq::is_zero(q.x); }
// plain x (limbs <= 2^29 + 8, value < 9.1 p) -> xn = 16 p - x: limbs <= 2^29 + 8 after the carry, 6.9 p < value <= 16 p; and back (xn < 14 p -> 2 p < x <= 16 p - xn)
ZK_HD fe29_t fq29_negx(const fe29_t &x) { return Fq29::sub16(Fq29::zero(), x); }
// accumulator of the mixed addition (x negated) -> plain accumulator (x limbs <= 2^29 + 8, 2 p < value < 16 p - 2 p: the invariants at the top).  The
// identity stays all-zero.  The only way out of the convention: G1AccOps::store (msm.hpp) calls it on every flushed record.
ZK_HD void g1_xyzz29_negx_to_plain(g1_xyzz29_t &acc) { if (!g1_xyzz29_is_identity(acc)) acc.x = fq29_negx(acc.x); }

// acc += (+-) q, q in the ABI form: the mixed addition of k_msm_accumulate, madd-2008-s.
//
// Convention: between additions acc.x holds xn = -X (limbs <= 2^29 + 8, 0 < value < 14 p) instead of X; y, zz, zzz and the identity are as in the
// invariants at the top.  An accumulator that only ever went through this function (starting from the identity) is in the convention; it
// leaves it through g1_xyzz29_negx_to_plain() before anything else -- g1_xyzz29_add / _dbl / _to_sat -- reads it.  With the sign on that side the two
// differences that involve X need no fat constant and no carry pass (X1 = -xn):
//     Pd  = U2 - X1      = U2 + xn                      limb-wise sum, limbs <= 2^30 + 7: inside what sqr / mul accept (< 2^30.3)
//     Qn  = -Q           = xn PP                        a product (Q = X1 PP)
//     xn3 = -X3          = PPP - RR - 2 Qn + 12 p       the shape of sub4_8, ONE carry
//     T   = Q - X3       = xn3 - Qn + 4 p               sub4_lazy: no carry, the b operand of mul_sub beside Rd (limbs <= 2^29 + 8)
// and Y3 = Rd T - Y1 PPP takes both products under ONE Montgomery reduction (mul_sub_c, signed column accumulator).  8 M + 2 S.
ZK_HD void g1_xyzz29_madd_core(g1_xyzz29_t &acc, const fe29_t &x2, const fe29_t &y2, bool y2_needs_normalise);
ZK_HD void g1_xyzz29_madd(g1_xyzz29_t &acc, const g1_affine_t &q, bool negate) {
  if (g1_affine_is_identity_x(q)) return;
  const fe29_t x2 = Fq29::from_sat(q.x);
  fe29_t y2 = Fq29::from_sat(q.y);
  if (negate) y2 = fq29_neg_loaded(y2);                    // limbs < 2^30, value < 64 p: multiplication operand only
  g1_xyzz29_madd_core(acc, x2, y2, negate);
}
// the same addition for an addend that already sits in 29-bit limbs (x2, y2: limbs < 2^30, value < 64 p, not the identity)
ZK_HD void g1_xyzz29_madd_core(g1_xyzz29_t &acc, const fe29_t &x2, const fe29_t &y2, bool y2_needs_normalise) {
  if (g1_xyzz29_is_identity(acc)) {
    // first point of a bucket: taken by every lane at a different iteration (divergent), so keep it multiplication-free
    acc.x = Fq29::reduce_small(x2); acc.y = Fq29::reduce_small(y2_needs_normalise ? Fq29::normalise(y2) : y2);   // tight, < 2p
    acc.x = Fq29::sub4(Fq29::zero(), acc.x);                                        // xn = 4 p - x: limbs <= 2^29 + 8, 2 p < value <= 4 p
    acc.zz = Fq29::one(); acc.zzz = Fq29::one();
    return;
  }
  const fe29_t U2 = Fq29::mul_c(x2, acc.zz), S2 = Fq29::mul_c(y2, acc.zzz);         // tight, < 1.2 p
  const fe29_t Pd = Fq29::add(U2, acc.x);                                           // limbs <= 2^29 - 1 + 2^29 + 8, top limb < 16 p >> 232; < 15.2 p
  const fe29_t Rd = Fq29::sub8(S2, acc.y);                                          // < 10 p, limbs <= 2^29 + 8
  const fe29_t PP = Fq29::sqr_c(Pd);                                                // < 3 p
  const fe29_t ZZ3 = Fq29::mul_c(acc.zz, PP);                                       // < 1.1 p : zero iff Pd == 0 (acc.zz != 0)
  if (Fq29::is_zero_tight(ZZ3)) {
    // q == +-acc: doubling or annihilation (rare; taken by repeated / opposite points inside one bucket).  The doubling hands back a plain x.
    const fe29_t one = Fq29::one();
    if (Fq29::is_zero_tight(Fq29::mul(Rd, one))) { acc = g1_xyzz29_dbl_affine(Fq29::mul(x2, one), Fq29::mul(y2, one)); acc.x = fq29_negx(acc.x); }
    else acc = g1_xyzz29_identity();
    return;
  }
  const fe29_t PPP = Fq29::mul_c(Pd, PP);                                           // < 1.4 p
  const fe29_t Qn = Fq29::mul_c(acc.x, PP);                                         // < 1.3 p (xn < 14 p)
  // 12 p - 1.6 p - 2.6 p < xn3 < (1.4 + 12) p; the fat 12 p covers RR + 2 Qn limb by limb (<= 3 (2^29 - 1); top limbs 3 * 0x60c89c < 0x244b3a9).
  // One carry: limbs <= 2^29 + 8.
  const fe29_t xn3 = Fq29::sub4_8(PPP, Fq29::sqr_c(Rd), Fq29::dbl(Qn));
  const fe29_t T = Fq29::sub4_lazy(xn3, Qn);                                        // < 17.4 p, NOT carried (limbs < 2^30.6: mul_sub's second operand only, see sub4_lazy)
  const fe29_t Y3 = Fq29::mul_sub_c(Rd, T, acc.y, PPP);                             // (Rd T - Y1 PPP) / R' + p + [0, p) < 3.1 p, limbs <= 2^30 - 2
  acc.x = xn3; acc.y = Y3; acc.zz = ZZ3; acc.zzz = Fq29::mul_c(acc.zzz, PPP);
}

// 2 * acc for an accumulator under the invariants above (dbl-2008-s-1).  Output: x < 9.1 p (limbs <= 2^29 + 8), y < 5.4 p
// (limbs <= 2^29 + 8), zz / zzz tight -- again a valid accumulator.
ZK_HD g1_xyzz29_t g1_xyzz29_dbl(const g1_xyzz29_t &a) {
  if (g1_xyzz29_is_identity(a)) return a;
  const fe29_t xt = Fq29::reduce_small(Fq29::normalise(a.x));                       // tight, < 2 p (x^2 of a 14 p value would leave the < 2 p output range)
  const fe29_t yc = Fq29::carry(a.y);                                               // limbs <= 2^29 + 2, value < 6.1 p
  const fe29_t U = Fq29::dbl(yc);                                                   // limbs <= 2^30 + 4, < 12.2 p   (U^2 = 149 p^2 < 2^261 p = 168 p^2)
  const fe29_t V = Fq29::sqr_c(U), W = Fq29::mul_c(U, V), S = Fq29::mul_c(xt, V);   // tight, < 1.9 p / 1.2 p / 1.1 p
  const fe29_t xx = Fq29::sqr_c(xt);
  const fe29_t M = Fq29::carry(Fq29::add(Fq29::dbl(xx), xx));                       // 3 x^2, limbs <= 2^29 + 8, < 3.3 p
  g1_xyzz29_t r;
  r.x = Fq29::sub8(Fq29::sqr_c(M), Fq29::dbl(S));                                   // < 1.1 p + 8 p
  const fe29_t t = Fq29::sub16(S, r.x);                                             // < 17.1 p
  r.y = Fq29::sub4(Fq29::mul_c(M, t), Fq29::mul_c(W, yc));                          // < 1.4 p + 4 p
  r.zz = Fq29::mul_c(V, a.zz); r.zzz = Fq29::mul_c(W, a.zzz);
  return r;
}

// acc += q, both accumulators under the invariants above (add-2008-s).  The loose coordinates only ever enter multiplications
// (U1 = X1 ZZ2, S1 = Y1 ZZZ2, ...), after which the body is the mixed addition's with (U1, S1) in the place of (X1, Y1): same
// expression shapes, same or tighter bounds.  12 M + 2 S.
ZK_HD void g1_xyzz29_add(g1_xyzz29_t &acc, const g1_xyzz29_t &q) {
  if (g1_xyzz29_is_identity(q)) return;
  if (g1_xyzz29_is_identity(acc)) { acc = q; return; }
  const fe29_t U1 = Fq29::mul_c(acc.x, q.zz), S1 = Fq29::mul_c(acc.y, q.zzz);       // tight, < 1.1 p
  const fe29_t U2 = Fq29::mul_c(q.x, acc.zz), S2 = Fq29::mul_c(q.y, acc.zzz);       // tight, < 1.1 p
  const fe29_t Pd = Fq29::sub4(U2, U1);                                             // < 5.1 p
  const fe29_t Rd = Fq29::sub4(S2, S1);                                             // < 5.1 p
  const fe29_t PP = Fq29::sqr_c(Pd);                                                // < 1.2 p
  const fe29_t ZZt = Fq29::mul_c(acc.zz, PP);                                       // zero iff Pd == 0 (both zz != 0)
  if (Fq29::is_zero_tight(ZZt)) {
    // q == +-acc: doubling or annihilation
    if (Fq29::is_zero_tight(Fq29::mul_c(Rd, Fq29::one()))) acc = g1_xyzz29_dbl(acc);
    else acc = g1_xyzz29_identity();
    return;
  }
  const fe29_t PPP = Fq29::mul_c(Pd, PP);                                           // < 1.1 p
  const fe29_t Q = Fq29::mul_c(U1, PP);                                             // < 1.1 p
  const fe29_t X3 = Fq29::sub4_8(Fq29::sqr_c(Rd), PPP, Fq29::dbl(Q));               // (1.2 + 4 + 8) p = 13.2 p, one carry
  const fe29_t Y3 = Fq29::mul_sub_c(Rd, Fq29::sub16(Q, X3), S1, PPP);               // as in the mixed addition, with the tight S1 for Y1
  acc.x = X3; acc.y = Y3;
  acc.zz = Fq29::mul_c(ZZt, q.zz); acc.zzz = Fq29::mul_c(Fq29::mul_c(acc.zzz, PPP), q.zzz);
}

// accumulator -> the saturated XYZZ record the reduction kernels consume (R = 2^256 Montgomery, fully reduced)
ZK_HD g1_xyzz_t g1_xyzz29_to_sat(const g1_xyzz29_t &a) {
  g1_xyzz_t r;
  if (g1_xyzz29_is_identity(a)) return g1_xyzz_identity();
  r.x = Fq29::to_sat(a.x); r.y = Fq29::to_sat(a.y); r.zz = Fq29::to_sat(a.zz); r.zzz = Fq29::to_sat(a.zzz);
  return r;
}

}  // namespace zk
