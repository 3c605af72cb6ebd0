// poseidon_selftest.cpp -- TEST INFRASTRUCTURE: compiles the __host__ __device__ routines of the device transcripts (csrc/poseidon.hpp: the permutation in both schedules,
// the per-job routine -- the very code k_poseidon_transcripts calls, with the jobs as a loop -- and the table generator the library runs) for the CPU with plain g++.
// tests/test_poseidon_on_host.py loads it as a shared object and checks it against oracle/poseidon.py.  With -DPOSEIDON_MAIN the file is a program of its own (the tables'
// self-check, sparse against plain on 64 states, the job set against a sponge written the slow way) for a run under -fsanitize=address,undefined.
// Never shipped, never linked into libmi355zk.so.
#include "../../scroll-prover_amd/csrc/poseidon.hpp"
#include <stdio.h>
#include <string.h>
using namespace zk;

extern "C" {
// the flat table (POS_TABLE_WORDS x 32 bytes, Montgomery); returns its length in field elements and the section offsets in `layout` (rc, mds, prc, row0, what, left, init)
int pst_tables(void *out, int *layout) {
  const std::vector<fe_t> &t = poseidon_tables();
  if (out) memcpy(out, t.data(), t.size() * sizeof(fe_t));
  if (layout) { const int l[7] = {POS_RC, POS_MDS, POS_PRC, POS_ROW0, POS_WHAT, POS_LEFT, POS_INIT}; memcpy(layout, l, sizeof l); }
  return (int)t.size();
}
// n states of five words, permuted in place.  which: 0 = the sparse schedule (what the kernel runs), 1 = the plain one
void pst_permute(void *states, uint64_t n, int which) {
  const fe_t *tab = poseidon_tables().data();
  for (uint64_t i = 0; i < n; i++) {
    fe_t s[POS_T]; memcpy(s, (const fe_t *)states + POS_T * i, sizeof s);
    if (which == 0) poseidon_permute<FrPs>(s, tab); else poseidon_permute_plain<FrPs>(s, tab);
    memcpy((fe_t *)states + POS_T * i, s, sizeof s);
  }
}
// the kernel's contract with the grid as a loop
void pst_jobs(const void *words, const uint64_t *word_off, const uint32_t *sq_at, const uint64_t *sq_off, uint32_t jobs, void *out) {
  const fe_t *tab = poseidon_tables().data();
  for (uint32_t j = 0; j < jobs; j++)
    poseidon_job<FrPs>(tab, (const fe_t *)words + word_off[j], sq_at + sq_off[j], (uint32_t)(sq_off[j + 1] - sq_off[j]), (fe_t *)out + sq_off[j]);
}
}

#ifdef POSEIDON_MAIN
static int fails = 0;
static void expect(bool ok, const char *what) { printf("%s %s\n", ok ? "ok  " : "FAIL", what); if (!ok) fails++; }
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static fe_t random_word() {   // any word below r is a legal element
  uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = FrP::mod(i);
  for (;;) { fe_t a; for (int i = 0; i < 8; i += 2) { const uint64_t v = next64(); a.l[i] = (uint32_t)v; a.l[i + 1] = (uint32_t)(v >> 32); } a.l[7] &= 0x3fffffffu; if (!Fr::w_geq(a.l, m)) return a; }
}
// the sponge the slow way: a buffer, the plain schedule with the CIOS multiplier, update / squeeze as oracle/poseidon.py writes them
struct SlowSponge {
  fe_t st[POS_T]; std::vector<fe_t> buf;
  SlowSponge() { for (auto &w : st) w = Fr::zero(); st[0] = poseidon_tables()[POS_INIT]; }
  void absorb(const fe_t *chunk, size_t len) {
    for (size_t i = 0; i < len; i++) st[1 + i] = Fr::add(st[1 + i], chunk[i]);
    if (len < (size_t)POS_RATE) st[1 + len] = Fr::add(st[1 + len], Fr::one());
    poseidon_permute_plain<Fr>(st, poseidon_tables().data());
  }
  fe_t squeeze() {
    std::vector<fe_t> b; b.swap(buf);
    for (size_t i = 0; i < b.size(); i += POS_RATE) absorb(b.data() + i, std::min<size_t>(POS_RATE, b.size() - i));
    if (b.size() % POS_RATE == 0) absorb(nullptr, 0);
    return st[1];
  }
};
int main() {
  bool ok = true;
  try { (void)poseidon_tables(); } catch (const std::exception &e) { printf("FAIL tables: %s\n", e.what()); return 1; }
  expect(poseidon_tables().size() == (size_t)POS_TABLE_WORDS, "the tables build and pass their own check");
  for (int t = 0; t < 64; t++) {
    fe_t a[POS_T], b[POS_T]; for (int i = 0; i < POS_T; i++) a[i] = b[i] = random_word();
    poseidon_permute<FrPs>(a, poseidon_tables().data()); poseidon_permute_plain<Fr>(b, poseidon_tables().data());
    for (int i = 0; i < POS_T; i++) ok = ok && Fr::eq(a[i], b[i]);
  }
  expect(ok, "sparse schedule (product scanning) = plain schedule (CIOS) on 64 random states");
  // the job set: every length 0..9 x the squeeze patterns; words from the edge pool, then random
  fe_t pool[6]; uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = FrP::mod(i);
  pool[0] = Fr::zero(); pool[1] = Fr::zero(); pool[1].l[0] = 1; for (int i = 0; i < 8; i++) pool[2].l[i] = m[i]; pool[2].l[0] -= 1; pool[3] = Fr::one();
  pool[4] = Fr::zero(); pool[4].l[7] = 1u << 29; pool[5] = Fr::zero(); for (int i = 0; i < 7; i++) pool[5].l[i] = 0xffffffffu; pool[5].l[7] = 0x30644d00u;
  std::vector<fe_t> words; std::vector<uint64_t> woff = {0}, soff = {0}; std::vector<uint32_t> sq;
  size_t draw = 0;
  for (uint32_t L = 0; L <= 9; L++) for (int pat = 0; pat < 6; pat++) {
    for (uint32_t i = 0; i < L; i++, draw++) words.push_back(draw % 3 == 2 ? random_word() : pool[draw % 6]);
    auto c = [&](uint32_t p) { return p < L ? p : L; };
    switch (pat) {
      case 0: sq.push_back(L); break;
      case 1: sq.push_back(0); sq.push_back(L); break;
      case 2: sq.push_back(c(2)); sq.push_back(c(2)); sq.push_back(L); break;
      case 3: sq.push_back(c(3)); sq.push_back(c(4)); sq.push_back(c(5)); break;
      case 4: sq.push_back(2 * L / 3); sq.push_back(L); break;
      default: sq.push_back(L / 2); break;   // the words behind the last squeeze are not hashed
    }
    woff.push_back(words.size()); soff.push_back(sq.size());
  }
  const uint32_t jobs = (uint32_t)woff.size() - 1;
  std::vector<fe_t> got(sq.size() + 1);
  memset(got.data(), 0xa5, got.size() * sizeof(fe_t));
  words.push_back(Fr::zero());   // keeps data() non-null for the empty tail
  pst_jobs(words.data(), woff.data(), sq.data(), soff.data(), jobs, got.data());
  ok = true;
  for (uint32_t j = 0; j < jobs; j++) {
    SlowSponge sp; uint32_t prev = 0;
    for (uint64_t q = soff[j]; q < soff[j + 1]; q++) { for (uint32_t i = prev; i < sq[q]; i++) sp.buf.push_back(words[woff[j] + i]); prev = sq[q]; ok = ok && Fr::eq(sp.squeeze(), got[q]); }
  }
  expect(ok, "60 jobs (lengths 0..9 x six squeeze patterns) = update / squeeze the slow way");
  { const uint8_t *tail = (const uint8_t *)&got[sq.size()]; bool untouched = true; for (size_t i = 0; i < sizeof(fe_t); i++) untouched = untouched && tail[i] == 0xa5; expect(untouched, "nothing is written behind the last challenge"); }
  printf("%s\n", fails ? "FAILED" : "all passed");
  return fails ? 1 : 0;
}
#endif
