// g1codec.hpp -- halo2curves G1Affine::to_bytes / from_bytes for whole arrays of points on the device: the 32-byte compressed word of
// SerdeFormat::Processed params files, proofs and .vkey files [EXT-recalled halo2curves derive/curve.rs; pinned by fixture KAT A4]:
// little-endian canonical x, bit 6 of byte 31 = parity of canonical y, bit 7 ignored, identity = 32 zero bytes.
//
// Decompression is a square root in Fq per point: y = (x^3 + 3)^((q + 1) / 4) (q = 3 mod 4), in the 9 x 29-bit field of fp29.hpp.  The exponent is
// one compile-time constant of 252 bits = 63 nibbles, walked from the top with a table of the ODD powers rhs^1 .. rhs^15 (8 entries, 72 registers):
// a nibble d = odd * 2^s costs 4 - s squarings, one multiplication by the table entry, s squarings; a zero nibble four squarings.  Every lane
// raises to the SAME exponent, so the control flow is uniform across the wavefront (scalar branches, no divergence) and the table entry is picked
// with selects on a scalar condition -- no indexed register access, hence no scratch.  Count per accepted point:
// root 251 S + 63 M (table 1 S + 7 M, walk 250 S + 56 M); x -> Montgomery and x^3 + 3: 1 S + 2 M; the check y^2 == rhs: 1 S + 2 M; the conversions
// out (x, y to the ABI form, y to canonical for its parity): 3 M.  253 S + 70 M = 323 field multiplications.
// No LDS.  g1_decompress_point / g1_compress_point are __host__ __device__: tests/hostcheck/g1codec_selftest.cpp runs this very code on the CPU
// against the oracle.  The host-only tail of the file is the codec of the two G2 points of a Processed params file.
#pragma once
#include "fp29.hpp"
#include "g1.hpp"

namespace zk {

struct G1Codec {
  // (q + 1) / 4, little-endian 32-bit words; bits 252.. are zero
  ZK_HD static constexpr uint32_t exp_word(int i) { constexpr uint32_t e[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu}; return e[i]; }
  static constexpr int NIBBLES = 63;
  ZK_HD static constexpr uint32_t r2_29(int i) { constexpr uint32_t m[9] = {0x59bac10u, 0xd1503a3u, 0x18016b8u, 0x10ab0ca8u, 0x2632639u, 0x2c0169fu, 0x169bfd53u, 0x11869d4cu, 0x2a11a6u}; return m[i]; }      // 2^522 mod q
  ZK_HD static constexpr uint32_t three_29(int i) { constexpr uint32_t m[9] = {0x766463u, 0x1c54760au, 0x8f6927au, 0x3e40c4du, 0x1fea4f2bu, 0x17c6c26au, 0x157fe417u, 0xf8056f9u, 0x2958a2u}; return m[i]; }   // 3 * 2^261 mod q
};

// T[i] when the (wave-uniform) index is i: selects, not an indexed access -- the table stays in registers
ZK_HD fe29_t g1codec_pick(const fe29_t (&T)[8], uint32_t idx) {
  fe29_t r = T[0];
#pragma unroll
  for (int k = 1; k < 8; k++) {
    const bool hit = idx == (uint32_t)k;
#pragma unroll
    for (int j = 0; j < 9; j++) r.l[j] = hit ? T[k].l[j] : r.l[j];
  }
  return r;
}

// a^((q + 1) / 4), a loose (x * 2^261 form), result tight
ZK_HD fe29_t fq29_pow_sqrt_exp(const fe29_t &a) {
  fe29_t T[8];   // a^1, a^3, ..., a^15
  T[0] = a;
  const fe29_t a2 = Fq29::sqr_c(a);
#pragma unroll
  for (int k = 1; k < 8; k++) T[k] = Fq29::mul_c(T[k - 1], a2);
  fe29_t acc = T[0]; bool started = false;
#pragma unroll 1
  for (int w = G1Codec::NIBBLES - 1; w >= 0; w--) {
    const uint32_t d = (G1Codec::exp_word(w >> 3) >> ((w & 7) * 4)) & 15u;
    int s = 0;
    if (d) { while (!((d >> s) & 1u)) s++; }
    const int lead = d ? 4 - s : 4;
    if (started) {
#pragma unroll 1
      for (int j = 0; j < lead; j++) acc = Fq29::sqr_c(acc);
    }
    if (d) {
      const fe29_t t = g1codec_pick(T, d >> (s + 1));
      if (started) acc = Fq29::mul_c(acc, t); else { acc = t; started = true; }
#pragma unroll 1
      for (int j = 0; j < s; j++) acc = Fq29::sqr_c(acc);
    }
  }
  return acc;
}

// 32 bytes (8 little-endian words) -> G1Affine, Montgomery, fully reduced.  false: not an encoding of a point (x >= q, x^3 + 3 a non-residue, or the
// identity's x = 0 with the sign bit set); out is then the identity.  The rule of halo2curves' from_bytes and of oracle orc_g1_decompress.
ZK_HD bool g1_decompress_point(const uint32_t w[8], g1_affine_t &out) {
  out.x = Fq::zero(); out.y = Fq::zero();
  fe_t xc;
#pragma unroll
  for (int i = 0; i < 8; i++) xc.l[i] = w[i];
  const uint32_t sign = (xc.l[7] >> 30) & 1u;
  xc.l[7] &= 0x3fffffffu;
  if (Fq::is_zero(xc)) return sign == 0;
  bool lt = false;
#pragma unroll
  for (int k = 7; k >= 0; k--) { if (xc.l[k] != FqP::mod(k)) { lt = xc.l[k] < FqP::mod(k); break; } }
  if (!lt) return false;
  fe29_t r2, three;
#pragma unroll
  for (int i = 0; i < 9; i++) { r2.l[i] = G1Codec::r2_29(i); three.l[i] = G1Codec::three_29(i); }
  const fe29_t x = Fq29::mul_c(Fq29::from_sat_plain(xc), r2);                          // x * 2^261, tight
  const fe29_t rhs = Fq29::add(Fq29::mul_c(Fq29::sqr_c(x), x), three);                 // x^3 + 3, loose (value < 3q)
  const fe29_t y = fq29_pow_sqrt_exp(rhs);
  if (!Fq::eq(Fq29::to_sat(Fq29::sqr_c(y)), Fq29::to_sat(rhs))) return false;          // a non-residue: y^2 = -rhs
  fe29_t one_plain = Fq29::zero(); one_plain.l[0] = 1;
  const fe29_t yc = Fq29::cond_sub_p(Fq29::normalise(Fq29::mul_c(y, one_plain)));      // canonical y
  fe_t ys = Fq29::to_sat(y);
  if ((yc.l[0] & 1u) != sign) ys = Fq::neg(ys);
  out.x = Fq29::to_sat(x); out.y = ys;
  return true;
}

// G1Affine (reduced Montgomery coordinates, trusted as everywhere in the ABI) -> the 8 words of its compressed form
ZK_HD void g1_compress_point(const g1_affine_t &p, uint32_t w[8]) {
  if (g1_affine_is_identity(p)) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = 0;
    return;
  }
  const fe_t xc = Fq::redc(p.x), yc = Fq::redc(p.y);
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = xc.l[i];
  w[7] |= (yc.l[0] & 1u) << 30;
}

#if defined(__HIPCC__)
constexpr int G1CODEC_THREADS = 256;
// one point per lane, grid-stride; a rejected word leaves the identity in its slot and its index in *first_bad (atomicMin: the smallest rejected
// index whatever the scheduling; the caller presets the word to ~0).  `base` is added to the reported index (a chunk of a larger array).
__global__ void __launch_bounds__(G1CODEC_THREADS) k_g1_decompress(const uint4 *__restrict__ in, uint4 *__restrict__ out, uint64_t n, uint64_t base, unsigned long long *__restrict__ first_bad) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 a = in[2 * i], b = in[2 * i + 1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    g1_affine_t p;
    if (!g1_decompress_point(w, p)) atomicMin(first_bad, (unsigned long long)(base + i));
    uint4 *o = out + 4 * i;
    o[0] = make_uint4(p.x.l[0], p.x.l[1], p.x.l[2], p.x.l[3]); o[1] = make_uint4(p.x.l[4], p.x.l[5], p.x.l[6], p.x.l[7]);
    o[2] = make_uint4(p.y.l[0], p.y.l[1], p.y.l[2], p.y.l[3]); o[3] = make_uint4(p.y.l[4], p.y.l[5], p.y.l[6], p.y.l[7]);
  }
}
__global__ void __launch_bounds__(G1CODEC_THREADS) k_g1_compress(const uint4 *__restrict__ in, uint4 *__restrict__ out, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 a = in[4 * i], b = in[4 * i + 1], c = in[4 * i + 2], d = in[4 * i + 3];
    g1_affine_t p;
    p.x.l[0] = a.x; p.x.l[1] = a.y; p.x.l[2] = a.z; p.x.l[3] = a.w; p.x.l[4] = b.x; p.x.l[5] = b.y; p.x.l[6] = b.z; p.x.l[7] = b.w;
    p.y.l[0] = c.x; p.y.l[1] = c.y; p.y.l[2] = c.z; p.y.l[3] = c.w; p.y.l[4] = d.x; p.y.l[5] = d.y; p.y.l[6] = d.z; p.y.l[7] = d.w;
    uint32_t w[8];
    g1_compress_point(p, w);
    out[2 * i] = make_uint4(w[0], w[1], w[2], w[3]); out[2 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}
#endif

}  // namespace zk

// ---- host only: the two G2 points (g2, s_g2) of a SerdeFormat::Processed params file.  64 bytes: x.c0 then x.c1 as canonical little-endian
// words, bit 6 of byte 63 = parity of canonical y.c0 (bit 7 ignored), identity = 64 zero bytes.  This layout is recalled from halo2curves at the
// pinned commit; NO fixture of the reference pins it (the G1 form is pinned by KAT A4).  Two points per file: plain fp.hpp arithmetic.
#include "g2.hpp"
#include <string.h>
namespace zk {

inline bool fq_sqrt_host(const fe_t &a, fe_t &r) {
  uint32_t e[8]; for (int i = 0; i < 8; i++) e[i] = G1Codec::exp_word(i);
  r = Fq::pow(a, e);
  return Fq::eq(Fq::sqr(r), a);
}
// a square root in Fq2 = Fq[u] / (u^2 + 1) by the norm ("complex") method: for a = a0 + a1 u, s = sqrt(a0^2 + a1^2), x0^2 = (a0 +- s) / 2, x1 = a1 / (2 x0)
inline bool fq2_sqrt_host(const fe2_t &a, fe2_t &r) {
  r = Fq2::zero();
  if (Fq2::is_zero(a)) return true;
  fe_t s;
  if (Fq::is_zero(a.c1)) {   // a in Fq: sqrt(a0), or sqrt(-a0) u (-1 is a non-residue: one of the two exists)
    if (fq_sqrt_host(a.c0, s)) { r.c0 = s; return true; }
    if (fq_sqrt_host(Fq::neg(a.c0), s)) { r.c1 = s; return true; }
    return false;
  }
  if (!fq_sqrt_host(Fq::add(Fq::sqr(a.c0), Fq::sqr(a.c1)), s)) return false;
  const fe_t half = Fq::inv(Fq::dbl(Fq::one()));
  fe_t x0;
  if (!fq_sqrt_host(Fq::mul(Fq::add(a.c0, s), half), x0) && !fq_sqrt_host(Fq::mul(Fq::sub(a.c0, s), half), x0)) return false;
  r.c0 = x0; r.c1 = Fq::mul(a.c1, Fq::inv(Fq::dbl(x0)));
  return Fq2::eq(Fq2::sqr(r), a);
}
inline bool fq_canonical_in_range(const fe_t &c) {
  for (int k = 7; k >= 0; k--) if (c.l[k] != FqP::mod(k)) return c.l[k] < FqP::mod(k);
  return false;
}
// 64 bytes -> G2Affine (128 B, Montgomery).  false: a coordinate >= q, x^3 + b' not a square, the identity's x with the sign bit set, or (never, by
// construction; checked all the same) a result off the twist
inline bool g2_decompress_point(const uint8_t in[64], g2_affine_t &out) {
  uint8_t b[64]; memcpy(b, in, 64);
  const uint32_t sign = (b[63] >> 6) & 1u; b[63] &= 0x3f;
  fe_t c0, c1; memcpy(&c0, b, 32); memcpy(&c1, b + 32, 32);
  out.x = Fq2::zero(); out.y = Fq2::zero();
  if (Fq::is_zero(c0) && Fq::is_zero(c1)) return sign == 0;
  if (!fq_canonical_in_range(c0) || !fq_canonical_in_range(c1)) return false;
  fe2_t x; x.c0 = Fq::from_canonical(c0); x.c1 = Fq::from_canonical(c1);
  fe2_t y;
  if (!fq2_sqrt_host(Fq2::add(Fq2::mul(Fq2::sqr(x), x), g2_twist_b()), y)) return false;
  if ((Fq::to_canonical(y.c0).l[0] & 1u) != sign) y = Fq2::neg(y);
  g2_affine_t p; p.x = x; p.y = y;
  if (!g2_is_on_curve(p)) return false;
  out = p;
  return true;
}
inline void g2_compress_point(const g2_affine_t &p, uint8_t out[64]) {
  memset(out, 0, 64);
  if (g2_affine_is_identity(p)) return;
  const fe_t c0 = Fq::to_canonical(p.x.c0), c1 = Fq::to_canonical(p.x.c1), y0 = Fq::to_canonical(p.y.c0);
  memcpy(out, &c0, 32); memcpy(out + 32, &c1, 32);
  out[63] |= (uint8_t)((y0.l[0] & 1u) << 6);
}

}  // namespace zk
