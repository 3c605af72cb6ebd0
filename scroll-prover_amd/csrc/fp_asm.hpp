// fp_asm.hpp -- product-scanning (FIPS) Montgomery multiplier tuned for the gfx950 ISA.
//
// Why: hipcc turns the textbook CIOS loop of fp.hpp into mad_u64_u32 + v_lshl_add_u64 + 2 x v_mov per
// limb product (~540 VALU instructions per field multiplication).  CDNA4's v_mad_u64_u32 is a VOP3B
// instruction with a carry-out SGPR, so a column accumulator {acc64, ex32} can absorb one 32x32 product in
// exactly two instructions (v_mad_u64_u32 ; v_addc_co_u32) with no register shuffling: ~300 instructions
// per multiplication.  Squaring uses a pre-doubled operand (a < 2^254 so 2a fits 8 limbs): 36 products
// instead of 64 in the a*a half.
//
// The host build of the same functions (plain C, for tests/hostcheck) uses 128-bit integers in `mac`.
// This file holds the multiplier and the field policy built on it (FqPs / FrPs), no point code.
#pragma once
#include "fp.hpp"
#include "fp_asm_gen.inc"

namespace zk {

// {ex:acc} += a * b      (96-bit column accumulator)
ZK_HD void mac(uint64_t &acc, uint32_t &ex, uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc" : "+v"(acc), "+v"(ex) : "v"(a), "v"(b) : "vcc");
#else
  unsigned __int128 s = (unsigned __int128)acc + (unsigned __int128)a * b; acc = (uint64_t)s; ex += (uint32_t)(s >> 64);
#endif
}
// same, with a wave-uniform second operand held in an SGPR (modulus limbs)
ZK_HD void mac_s(uint64_t &acc, uint32_t &ex, uint32_t a, uint32_t b_uniform) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc" : "+v"(acc), "+v"(ex) : "v"(a), "s"(b_uniform) : "vcc");
#else
  mac(acc, ex, a, b_uniform);
#endif
}
ZK_HD void col_shift(uint64_t &acc, uint32_t &ex) { acc = (acc >> 32) | ((uint64_t)ex << 32); ex = 0; }

// Montgomery reduction columns shared by mul and sqr: P-terms for column k given m[0..]
template <class P> ZK_HD fe_t mont_mul_ps(const fe_t &a, const fe_t &b) {
  uint64_t acc = 0; uint32_t ex = 0; uint32_t m[8]; fe_t r;
#if defined(__HIP_DEVICE_COMPILE__)
  ZK_MONT_MUL_COLUMNS
  return Fp<P>::reduce_once(r);
#else
#pragma unroll
  for (int k = 0; k < 8; k++) {
#pragma unroll
    for (int i = 0; i <= k; i++) mac(acc, ex, a.l[i], b.l[k - i]);
#pragma unroll
    for (int i = 0; i < k; i++) mac_s(acc, ex, m[i], P::mod(k - i));
    m[k] = (uint32_t)acc * P::INV;
    mac_s(acc, ex, m[k], P::mod(0));
    col_shift(acc, ex);
  }
#pragma unroll
  for (int k = 8; k < 15; k++) {
#pragma unroll
    for (int i = k - 7; i < 8; i++) mac(acc, ex, a.l[i], b.l[k - i]);
#pragma unroll
    for (int i = k - 7; i < 8; i++) mac_s(acc, ex, m[i], P::mod(k - i));
    r.l[k - 8] = (uint32_t)acc;
    col_shift(acc, ex);
  }
  r.l[7] = (uint32_t)acc;  // value < 2m < 2^255: nothing above
  return Fp<P>::reduce_once(r);
#endif
}
template <class P> ZK_HD fe_t mont_sqr_ps(const fe_t &a) {
  // 2 * sum_{i<j} a_i a_j 2^(32(i+j)) = sum_i a_i * (2 * (a with limbs <= i cleared)).  Limb j of that doubled
  // upper part is a2[j] = (a_j << 1 | a_{j-1} >> 31) for j > i + 1 and a2lo[j] = a_j << 1 for j == i + 1
  // (the bit shifted in from a_i must not be counted); a < 2^254 so nothing spills into a ninth limb.
  uint32_t a2[8], a2lo[8];
  a2[0] = a2lo[0] = a.l[0] << 1;
#pragma unroll
  for (int i = 1; i < 8; i++) { a2lo[i] = a.l[i] << 1; a2[i] = a2lo[i] | (a.l[i - 1] >> 31); }
  uint64_t acc = 0; uint32_t ex = 0; uint32_t m[8]; fe_t r;
#if defined(__HIP_DEVICE_COMPILE__)
  ZK_MONT_SQR_COLUMNS
  return Fp<P>::reduce_once(r);
#else
#pragma unroll
  for (int k = 0; k < 8; k++) {
#pragma unroll
    for (int i = 0; 2 * i < k; i++) mac(acc, ex, a.l[i], (k - i == i + 1) ? a2lo[k - i] : a2[k - i]);
    if ((k & 1) == 0) mac(acc, ex, a.l[k / 2], a.l[k / 2]);
#pragma unroll
    for (int i = 0; i < k; i++) mac_s(acc, ex, m[i], P::mod(k - i));
    m[k] = (uint32_t)acc * P::INV;
    mac_s(acc, ex, m[k], P::mod(0));
    col_shift(acc, ex);
  }
#pragma unroll
  for (int k = 8; k < 15; k++) {
#pragma unroll
    for (int i = k - 7; 2 * i < k; i++) mac(acc, ex, a.l[i], (k - i == i + 1) ? a2lo[k - i] : a2[k - i]);
    if ((k & 1) == 0) mac(acc, ex, a.l[k / 2], a.l[k / 2]);
#pragma unroll
    for (int i = k - 7; i < 8; i++) mac_s(acc, ex, m[i], P::mod(k - i));
    r.l[k - 8] = (uint32_t)acc;
    col_shift(acc, ex);
  }
  r.l[7] = (uint32_t)acc;
  return Fp<P>::reduce_once(r);
#endif
}

// The field with the product-scanning multiplier as a policy: everything of Fp<P> but mul / sqr.  The point formulas (g1.hpp, g2.hpp) and the
// kernels take the field as a template argument or name it outright, so which multiplier a call site runs is written at that call site.
// The inherited members that multiply inside themselves (pow, pow_u64, inv, inv_sgcd, from_canonical, to_canonical) keep calling the base CIOS
// mul of fp.hpp -- static functions do not dispatch -- which is what those call sites ran before the policy existed; the values are the same.
template <class P> struct FpPs : Fp<P> {
  ZK_HD static fe_t mul(const fe_t &a, const fe_t &b) { return mont_mul_ps<P>(a, b); }
  ZK_HD static fe_t sqr(const fe_t &a) { return mont_sqr_ps<P>(a); }
};
using FqPs = FpPs<FqP>;
using FrPs = FpPs<FrP>;

}  // namespace zk
