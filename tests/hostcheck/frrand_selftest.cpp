// frrand_selftest.cpp -- TEST INFRASTRUCTURE: compiles the __host__ __device__ routines of the device randomness (csrc/frrand.hpp: the ChaCha20 block, the
// 512-bit reduction with both multipliers, the element of a draw) for the CPU with plain g++.  tests/test_fr_random_on_host.py loads it as a shared object and checks
// it against tests/frrand_common.py (plain Python, big integers).  With -DFRRAND_MAIN the file is a program of its own (the two published ChaCha20 vectors, the
// counter carry, the extreme words of the reduction against a reduce-first computation) for a run under -fsanitize=address,undefined.
// Never shipped, never linked into libmi355zk.so.
#include "../../scroll-prover_amd/csrc/frrand.hpp"
#include <stdio.h>
#include <string.h>
using namespace zk;

static frrand_key_t key_of(const uint8_t *key32) { frrand_key_t k; memcpy(k.w, key32, 32); return k; }

extern "C" {
void fst_block(const uint8_t *key32, uint64_t stream, uint64_t counter, void *out64) {
  uint32_t w[16]; frrand_block(key_of(key32), stream, counter, w); memcpy(out64, w, 64);
}
// which: 0 = frrand_from_u512 (what the kernels call), 1 = the CIOS multiplier of fp.hpp in the same operand order
void fst_from_u512(const void *src, uint64_t n, void *out, int which) {
  for (uint64_t i = 0; i < n; i++) {
    uint32_t w[16]; memcpy(w, (const uint8_t *)src + 64 * i, 64);
    ((fe_t *)out)[i] = which == 0 ? frrand_from_u512(w) : frrand_from_u512_with<Fr>(w);
  }
}
void fst_elements(const uint8_t *key32, uint64_t stream, uint64_t counter0, uint64_t n, void *out) {
  for (uint64_t i = 0; i < n; i++) ((fe_t *)out)[i] = frrand_element(key_of(key32), stream, counter0 + i);
}
void fst_r3(void *out32) { uint32_t w[8]; for (int i = 0; i < 8; i++) w[i] = frrand_r3(i); memcpy(out32, w, 32); }
}

#ifdef FRRAND_MAIN
static int fails = 0;
static void expect(bool ok, const char *what) { printf("%s %s\n", ok ? "ok  " : "FAIL", what); if (!ok) fails++; }
static bool below_r(const fe_t &a) { uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = FrP::mod(i); return !Fr::w_geq(a.l, m); }
// reduce-first: each half brought below r by subtraction (at most 5 times), then two conversions of REDUCED words and 2^256 = R as a field element
static fe_t reduce_first(const uint32_t (&w)[16]) {
  uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = FrP::mod(i);
  fe_t d0, d1; for (int i = 0; i < 8; i++) { d0.l[i] = w[i]; d1.l[i] = w[8 + i]; }
  while (Fr::w_geq(d0.l, m)) Fr::w_sub(d0.l, m);
  while (Fr::w_geq(d1.l, m)) Fr::w_sub(d1.l, m);
  fe_t r2; for (int i = 0; i < 8; i++) r2.l[i] = FrP::r2(i);   // R^2 as a word = the Montgomery form of R = 2^256
  return Fr::add(Fr::from_canonical(d0), Fr::mul(Fr::from_canonical(d1), r2));
}
static void half(uint32_t *dst, int which) {   // 0, 1, r - 1, r, r + 1, 2r, 5r, 2^256 - 1
  uint64_t c = 0; const uint32_t mul[8] = {0, 0, 1, 1, 1, 2, 5, 0}; const int64_t add[8] = {0, 1, -1, 0, 1, 0, 0, 0};
  if (which == 7) { for (int i = 0; i < 8; i++) dst[i] = 0xffffffffu; return; }
  for (int i = 0; i < 8; i++) { c += (uint64_t)FrP::mod(i) * mul[which]; dst[i] = (uint32_t)c; c >>= 32; }
  if (add[which] == 1) { for (int i = 0; i < 8 && ++dst[i] == 0; i++) {} }
  if (add[which] == -1) { for (int i = 0; i < 8 && dst[i]-- == 0; i++) {} }
}
int main() {
  uint8_t key[32] = {0}, out[64];
  fst_block(key, 0, 0, out);
  const uint8_t z0[16] = {0x76, 0xb8, 0xe0, 0xad, 0xa0, 0xf1, 0x3d, 0x90, 0x40, 0x5d, 0x6a, 0xe5, 0x53, 0x86, 0xbd, 0x28}, z1[8] = {0xc3, 0x87, 0xb6, 0x69, 0xb2, 0xee, 0x65, 0x86};
  expect(!memcmp(out, z0, 16) && !memcmp(out + 56, z1, 8), "zero key, counter 0, stream 0");
  for (int i = 0; i < 32; i++) key[i] = (uint8_t)i;
  fst_block(key, 0x4a000000ull, 1ull | (0x09000000ull << 32), out);
  const uint8_t a0[16] = {0x10, 0xf1, 0xe7, 0xe4, 0xd1, 0x3b, 0x59, 0x15, 0x50, 0x0f, 0xdd, 0x1f, 0xa3, 0x20, 0x71, 0xc4}, a1[8] = {0xcb, 0xd0, 0x83, 0xe8, 0xa2, 0x50, 0x3c, 0x4e};
  expect(!memcmp(out, a0, 16) && !memcmp(out + 56, a1, 8), "RFC 8439 section 2.3.2");
  { uint8_t lo[64], hi[64]; fst_block(key, 0, 0xffffffffull, lo); fst_block(key, 0, 0x100000000ull, hi);
    uint8_t wrong[64]; fst_block(key, 0, 0, wrong);
    expect(memcmp(lo, hi, 64) && memcmp(hi, wrong, 64), "counter 2^32 is not counter 0: the carry reaches word 13"); }
  bool ok = true, agree = true;
  for (int a = 0; a < 8; a++) for (int b = 0; b < 8; b++) {
    uint32_t w[16]; half(w, a); half(w + 8, b);
    const fe_t want = reduce_first(w), ps = frrand_from_u512(w), cios = frrand_from_u512_with<Fr>(w);
    ok = ok && below_r(ps) && Fr::eq(ps, want); agree = agree && Fr::eq(ps, cios);
  }
  expect(ok, "(d0, d1) over {0, 1, r - 1, r, r + 1, 2r, 5r, 2^256 - 1}^2: reduced and equal to the reduce-first value");
  expect(agree, "the product-scanning and the CIOS multiplier agree on them");
  ok = true;
  for (int bit = 0; bit < 512; bit++) { uint32_t w[16] = {0}; w[bit >> 5] = 1u << (bit & 31); const fe_t v = frrand_from_u512(w); ok = ok && below_r(v) && Fr::eq(v, reduce_first(w)) && Fr::eq(v, frrand_from_u512_with<Fr>(w)); }
  expect(ok, "single-bit words");
  ok = true;
  { fe_t e[300]; fst_elements(key, 7, 0xfffffff0ull, 300, e);
    for (int i = 0; i < 300; i++) { uint32_t w[16]; frrand_block(key_of(key), 7, 0xfffffff0ull + i, w); ok = ok && below_r(e[i]) && Fr::eq(e[i], reduce_first(w)); } }
  expect(ok, "300 elements of a draw across the 2^32 counter line");
  printf("%s\n", fails ? "FAILED" : "all passed");
  return fails ? 1 : 0;
}
#endif
