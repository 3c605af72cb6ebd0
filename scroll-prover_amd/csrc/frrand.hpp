// frrand.hpp -- uniform field elements drawn on the device: one ChaCha20 block (RFC 8439, 20 rounds) per element, reduced from 512 bits to Fr.
// Element i of a draw is a pure function of (key, stream, counter0 + i): the result does not depend on the grid shape, on the device count or on how a
// vector is cut into calls, so a caller (and every test) can recompute any word on the CPU.
//
//   frrand_block        the ChaCha20 block function: constants "expand 32-byte k", key words 4..11, the 64-bit little-endian block counter in state words
//                       12..13 and the 64-bit stream identifier in words 14..15.  With stream = 0 and counter < 2^32 this is RFC 8439 with a zero nonce.
//                       [EXT-recalled rand_chacha ChaCha20Rng: the same state layout (64-bit counter, 64-bit stream); one block is the eight next_u64 words
//                       that halo2curves' Fr::random consumes.]  Plain C++ rotates, sixteen state words in registers, no LDS, no scratch.
//   frrand_from_u512    (d0 + 2^256 d1) mod r in Montgomery form, d0 = words 0..7, d1 = words 8..15, little-endian.  [EXT-recalled halo2curves
//                       Fr::from_u512 / from_uniform_bytes: d0 R^2 + d1 R^3 by two Montgomery products.]  d0 R^2 R^-1 = d0 R and d1 R^3 R^-1 = d1 R^2 = (2^256 d1) R.
//                       BOUND: d0 and d1 are NOT reduced (up to 2^256 - 1 > 5 r).  A Montgomery product returns (a b + m r) / 2^256 with m < 2^256; with ONE
//                       operand below r and the other below 2^256 that is < (r 2^256 + 2^256 r) / 2^256 = 2 r < 2^255: the value fits eight words and one
//                       conditional subtraction reduces it fully.  The product-scanning multiplier (fp_asm.hpp) adds whole columns into a 96-bit
//                       accumulator (at most 16 products below 2^64 per column), so the bound on the final value is all it needs, for either operand order.
//                       The CIOS multiplier of fp.hpp keeps a running value t <- (t + a b_i + m_i r) / 2^32 < t / 2^32 + a + r, which stays below 2 r only when
//                       the operand `a` of the inner loop is the reduced one: the unreduced word must be `b`, whose limbs drive the outer loop.  Both
//                       multipliers are therefore called as mul(constant, word) here, and tests/hostcheck/frrand_selftest.cpp runs both on the extreme words.
//   k_fr_random         element i of a vector = from_u512(block(key, stream, counter0 + i)); the 64-bit add carries into state word 13.
//   k_fr_random_rows    a batch of columns: rows [row0, row0 + rows) of column c get the blocks counter0 + c * rows + j (the blinding rows of a proof's columns).
//   k_fr_from_u512      halo2's Fr::from_uniform_bytes over an array: n 64-byte words in, n 32-byte words out.
// One lane per element, plain 32-byte vector stores (two dwordx4), a grid-stride loop over whole workgroups.  The key travels as a kernel argument (uniform, SGPRs).
#pragma once
#include "fp_asm.hpp"

namespace zk {

struct frrand_key_t { uint32_t w[8]; };   // the 32 key bytes as eight little-endian words

ZK_HD constexpr uint32_t frrand_r3(int i) {   // R^3 mod r (re-derived in tests/test_fr_random_on_host.py)
  constexpr uint32_t m[8] = {0xb4bf0040u, 0x5e94d8e1u, 0x1cfbb6b8u, 0x2a489cbeu, 0xa19fcfedu, 0x893cc664u, 0x7fcc657cu, 0x0cf8594bu};
  return m[i];
}

ZK_HD uint32_t frrand_rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

#define ZK_FRRAND_QR(a, b, c, d) \
  a += b; d = frrand_rotl(d ^ a, 16); c += d; b = frrand_rotl(b ^ c, 12); a += b; d = frrand_rotl(d ^ a, 8); c += d; b = frrand_rotl(b ^ c, 7);

ZK_HD void frrand_block(const frrand_key_t &key, uint64_t stream, uint64_t counter, uint32_t (&out)[16]) {
  const uint32_t i0 = 0x61707865u, i1 = 0x3320646eu, i2 = 0x79622d32u, i3 = 0x6b206574u;
  const uint32_t i12 = (uint32_t)counter, i13 = (uint32_t)(counter >> 32), i14 = (uint32_t)stream, i15 = (uint32_t)(stream >> 32);
  uint32_t x0 = i0, x1 = i1, x2 = i2, x3 = i3, x4 = key.w[0], x5 = key.w[1], x6 = key.w[2], x7 = key.w[3], x8 = key.w[4], x9 = key.w[5], x10 = key.w[6], x11 = key.w[7],
           x12 = i12, x13 = i13, x14 = i14, x15 = i15;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    ZK_FRRAND_QR(x0, x4, x8, x12) ZK_FRRAND_QR(x1, x5, x9, x13) ZK_FRRAND_QR(x2, x6, x10, x14) ZK_FRRAND_QR(x3, x7, x11, x15)
    ZK_FRRAND_QR(x0, x5, x10, x15) ZK_FRRAND_QR(x1, x6, x11, x12) ZK_FRRAND_QR(x2, x7, x8, x13) ZK_FRRAND_QR(x3, x4, x9, x14)
  }
  out[0] = x0 + i0; out[1] = x1 + i1; out[2] = x2 + i2; out[3] = x3 + i3;
  out[4] = x4 + key.w[0]; out[5] = x5 + key.w[1]; out[6] = x6 + key.w[2]; out[7] = x7 + key.w[3];
  out[8] = x8 + key.w[4]; out[9] = x9 + key.w[5]; out[10] = x10 + key.w[6]; out[11] = x11 + key.w[7];
  out[12] = x12 + i12; out[13] = x13 + i13; out[14] = x14 + i14; out[15] = x15 + i15;
}
#undef ZK_FRRAND_QR

// F: Fr (CIOS) or FrPs (product scanning).  The constant is the first operand, the unreduced word the second: see BOUND above.
template <class F> ZK_HD fe_t frrand_from_u512_with(const uint32_t (&w)[16]) {
  fe_t d0, d1, r2, r3;
#pragma unroll
  for (int i = 0; i < 8; i++) { d0.l[i] = w[i]; d1.l[i] = w[8 + i]; r2.l[i] = FrP::r2(i); r3.l[i] = frrand_r3(i); }
  return F::add(F::mul(r2, d0), F::mul(r3, d1));   // both products are fully reduced, so is the sum
}
ZK_HD fe_t frrand_from_u512(const uint32_t (&w)[16]) { return frrand_from_u512_with<FrPs>(w); }

ZK_HD fe_t frrand_element(const frrand_key_t &key, uint64_t stream, uint64_t counter) {
  uint32_t w[16];
  frrand_block(key, stream, counter, w);
  return frrand_from_u512(w);
}

}  // namespace zk

#ifdef __HIPCC__
namespace zk {

constexpr uint32_t FRRAND_THREADS = 256;

__global__ void __launch_bounds__(FRRAND_THREADS) k_fr_random(fe_t *__restrict__ dst, uint64_t n, frrand_key_t key, uint64_t stream, uint64_t counter0) {
  for (uint64_t i = (uint64_t)blockIdx.x * FRRAND_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FRRAND_THREADS)
    g_store(&dst[i], frrand_element(key, stream, counter0 + i));   // counter0 + n does not wrap (checked by the caller)
}

// t = c * rows + j < n_cols * rows: column c, row row0 + j, block counter0 + t
__global__ void __launch_bounds__(FRRAND_THREADS) k_fr_random_rows(fe_t *const *__restrict__ cols, uint32_t n_cols, uint64_t row0, uint32_t rows, frrand_key_t key,
                                                                   uint64_t stream, uint64_t counter0) {
  const uint64_t total = (uint64_t)n_cols * rows;
  for (uint64_t t = (uint64_t)blockIdx.x * FRRAND_THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * FRRAND_THREADS) {
    const uint64_t c = t / rows, j = t - c * rows;
    g_store(&cols[c][row0 + j], frrand_element(key, stream, counter0 + t));
  }
}

__global__ void __launch_bounds__(FRRAND_THREADS) k_fr_from_u512(fe_t *__restrict__ dst, const uint4 *__restrict__ src, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * FRRAND_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FRRAND_THREADS) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 4; q++) { const uint4 v = src[4 * i + q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    g_store(&dst[i], frrand_from_u512(w));
  }
}

}  // namespace zk
#endif  // __HIPCC__
