// lookup_hash_main.cpp -- TEST INFRASTRUCTURE: compiles the host-visible part of the multiplicity kernels (csrc/lookup.hpp: lk_hash, lk_eq and the constants of the
// hash set and the wave counter -- the very code the kernels call) for the CPU with plain g++.  tests/test_lookup_hash_on_host.py loads it as a shared object and holds
// the numpy restatement of tests/lookup_common.py equal to it; the GPU tests then place keys in chosen slots with that restatement.  With -DLOOKUP_HASH_MAIN the file is
// a program of its own (hand-derived hashes, the range of the mask, lk_eq on every one-bit difference) for a run under -fsanitize=address,undefined.
// Never shipped, never linked into libmi355zk.so.
#include "../../scroll-prover_amd/csrc/lookup.hpp"
#include <stdio.h>
#include <string.h>
using namespace zk;

static fe_t word_of(const uint64_t *w) { fe_t v; memcpy(v.l, w, 32); return v; }

extern "C" {
// words: n x 4 u64 (32-byte little-endian words, as the ABI holds them)
void lkh_hash(const uint64_t *words, uint64_t n, uint32_t mask, uint32_t *out) {
  for (uint64_t i = 0; i < n; i++) out[i] = lk_hash(word_of(words + 4 * i), mask);
}
int lkh_eq(const uint64_t *a, const uint64_t *b) { return lk_eq(word_of(a), word_of(b)) ? 1 : 0; }
uint32_t lkh_empty() { return LK_EMPTY; }
int lkh_rounds() { return LK_ROUNDS; }
uint32_t lkh_hot_min() { return LK_HOT_MIN; }
}

#ifdef LOOKUP_HASH_MAIN
static int fails = 0;
static void expect(bool ok, const char *what) { printf("%s %s\n", ok ? "ok  " : "FAIL", what); if (!ok) fails++; }
// the finaliser alone, written out again: what the hash of the zero word must be, and of a word with only its top 64 bits set
static uint64_t fin(uint64_t h) { h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull; h = (h ^ (h >> 27)) * 0x94D049BB133111EBull; return h ^ (h >> 31); }
int main() {
  uint64_t z[4] = {0, 0, 0, 0}; uint32_t h = 1;
  lkh_hash(z, 1, 0xffffffffu, &h);
  expect(h == 0 && fin(0) == 0, "the zero word hashes to slot 0 under every mask");
  { uint64_t w[4] = {0, 0, 0, 0x0123456789abcdefull}; lkh_hash(w, 1, 0xffffffffu, &h); expect(h == (uint32_t)fin(w[3]), "a word with only limbs 6, 7 set: the finaliser of those 64 bits"); }
  { uint64_t w[4] = {0, 0, 5, 0}; lkh_hash(w, 1, 0xffffffffu, &h); expect(h == (uint32_t)fin((5 ^ (5ull >> 32)) * 0x94D049BB133111EBull), "a word with only limb 4 set: one multiply, then the finaliser"); }
  bool ok = true, differ = true, eq_ok = true;
  const uint32_t masks[3] = {63u, 4095u, (1u << 27) - 1};
  uint64_t base[4] = {0x9e3779b97f4a7c15ull, 0x0123456789abcdefull, 0xfedcba9876543210ull, 0x0badc0ffee0ddf00ull};
  uint32_t hb; lkh_hash(base, 1, 0xffffffffu, &hb);
  for (int bit = 0; bit < 256; bit++) {
    uint64_t w[4]; memcpy(w, base, 32); w[bit >> 6] ^= 1ull << (bit & 63);
    uint32_t full; lkh_hash(w, 1, 0xffffffffu, &full);
    for (int m = 0; m < 3; m++) { uint32_t hm; lkh_hash(w, 1, masks[m], &hm); ok = ok && hm <= masks[m] && hm == (full & masks[m]); }
    differ = differ && full != hb;
    eq_ok = eq_ok && !lkh_eq(w, base) && !lkh_eq(base, w) && lkh_eq(w, w);
  }
  expect(ok, "masks 63, 4095, 2^27 - 1: the slot is the low bits of the 32-bit hash and never past the mask");
  expect(differ, "every one-bit change of a word changes its 32-bit hash (all 256 bits are mixed in)");
  expect(eq_ok && lkh_eq(base, base), "lk_eq: false at every Hamming distance 1, true on the word itself");
  { uint64_t many[64 * 4]; uint32_t out[64];
    for (int i = 0; i < 64 * 4; i++) many[i] = fin((uint64_t)i + 1);
    lkh_hash(many, 64, 4095u, out);
    bool same = true; for (int i = 0; i < 64; i++) { uint32_t one; lkh_hash(many + 4 * i, 1, 4095u, &one); same = same && one == out[i]; }
    expect(same, "a batch of 64 words equals 64 single calls"); }
  expect(lkh_empty() == 0xffffffffu && lkh_rounds() >= 1 && lkh_hot_min() >= 2 && lkh_hot_min() <= 64, "constants: EMPTY is no row index, at least one round, a hot group fits one block");
  printf("%s\n", fails ? "FAILED" : "all passed");
  return fails ? 1 : 0;
}
#endif
