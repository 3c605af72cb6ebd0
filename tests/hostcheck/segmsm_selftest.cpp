// segmsm_selftest.cpp -- TEST INFRASTRUCTURE: compiles the __host__ __device__ per-term routine of the segmented MSM kernel (msm_seg.hpp segmsm_term, on the point formulas
// of g1.hpp with the product-scanning multiplier the kernel names) for the CPU with plain g++.  A segment runs here as the kernel runs it: the 64 lanes as a loop, lane l
// walking the terms lo + l, + 64, ...; then the shuffle tree as the same pairwise order over an array (segmsm_tree_takes: at step o lane l < o takes lane l + o's value);
// then lane 0's conversion to affine.  tests/test_msm_segmented_on_host.py loads it as a shared object and checks it against the oracle.
// With -DSEGMSM_MAIN the file is a program of its own (a fixed subset on multiples of the generator) for a run under -fsanitize=address,undefined.
// Never shipped, never linked into libmi355zk.so.
#include "../../scroll-prover_amd/csrc/msm_seg.hpp"
#include <stdio.h>
#include <string.h>
using namespace zk;

static g1_affine_t run_segment(const g1_affine_t *bases, const fe_t *scalars, uint64_t lo, uint64_t hi) {
  g1_xyzz_t lane[SEGMSM_LANES];
  for (uint32_t l = 0; l < SEGMSM_LANES; l++) {
    lane[l] = g1_xyzz_identity();
    for (uint64_t i = lo + l; i < hi; i += SEGMSM_LANES) segmsm_term<FqPs>(lane[l], bases[i], scalars[i]);
  }
  for (uint32_t o = SEGMSM_LANES / 2; o >= 1; o >>= 1)
    for (uint32_t l = 0; l < SEGMSM_LANES; l++) {   // ascending l: lane l + o is read before its own turn changes it (its turn adds the identity anyway)
      const g1_xyzz_t other = segmsm_tree_takes(l, o) ? lane[l + o] : g1_xyzz_identity();
      g1_xyzz_add<FqPs>(lane[l], other);
    }
  return g1_xyzz_to_affine(lane[0]);
}

extern "C" {
// out[s] = sum over [offsets[s], offsets[s + 1]) of scalars[i] * bases[i]: the contract of mi355_msm_g1_segmented_host
void sst_msm_segmented(const void *bases, const void *scalars, const uint64_t *offsets, uint32_t segments, void *out) {
  for (uint32_t s = 0; s < segments; s++) ((g1_affine_t *)out)[s] = run_segment((const g1_affine_t *)bases, (const fe_t *)scalars, offsets[s], offsets[s + 1]);
}
}

#ifdef SEGMSM_MAIN
#include <vector>
static int fails = 0;
static void expect(bool ok, const char *what) { printf("%s %s\n", ok ? "ok  " : "FAIL", what); if (!ok) fails++; }
static fe_t fr_small(uint32_t v) { fe_t c = Fr::zero(); c.l[0] = v; return Fr::from_canonical(c); }
static bool same(const g1_affine_t &a, const g1_affine_t &b) { return Fq::eq(a.x, b.x) && Fq::eq(a.y, b.y); }
static g1_affine_t one_term(const g1_affine_t &P, const fe_t &k) { const uint64_t off[2] = {0, 1}; g1_affine_t o; sst_msm_segmented(&P, &k, off, 1, &o); return o; }
int main() {
  g1_affine_t G; fe_t c = Fq::zero(); c.l[0] = 1; G.x = Fq::from_canonical(c); c.l[0] = 2; G.y = Fq::from_canonical(c);
  const g1_affine_t O = {Fq::zero(), Fq::zero()};
  // n G by repeated mixed addition (the plain multiplier): the values the segments must reproduce
  std::vector<g1_affine_t> mult(261); mult[0] = O;
  { g1_xyzz_t acc = g1_xyzz_identity(); for (int n = 1; n <= 260; n++) { g1_xyzz_madd(acc, G); mult[n] = g1_xyzz_to_affine(acc); } }
  expect(same(one_term(G, fr_small(0)), O) && same(one_term(G, fr_small(1)), G) && same(one_term(G, fr_small(2)), mult[2]) && same(one_term(G, fr_small(77)), mult[77]), "k G for k = 0, 1, 2, 77");
  expect(same(one_term(G, Fr::neg(Fr::one())), g1_affine_neg(G)) && same(one_term(G, Fr::neg(fr_small(2))), g1_affine_neg(mult[2])), "(r - 1) G = -G, (r - 2) G = -2 G");
  expect(same(one_term(O, fr_small(5)), O), "the identity base");
  { fe_t t = Fr::zero(); t.l[7] = 1u << 29; const fe_t k = Fr::from_canonical(t);   // 2^253, the top bit the loop reads
    g1_xyzz_t acc = g1_xyzz_from_affine(G); for (int i = 0; i < 253; i++) acc = g1_xyzz_dbl(acc);
    expect(same(one_term(G, k), g1_xyzz_to_affine(acc)), "2^253 G by 253 doublings"); }
  const uint32_t lens[7] = {0, 1, 2, 63, 64, 65, 130};
  std::vector<g1_affine_t> bs; std::vector<fe_t> sc; std::vector<uint64_t> off = {0};
  for (uint32_t len : lens) { for (uint32_t i = 0; i < len; i++) { bs.push_back(G); sc.push_back(fr_small(1)); } off.push_back(bs.size()); }
  std::vector<g1_affine_t> out(7);
  sst_msm_segmented(bs.data(), sc.data(), off.data(), 7, out.data());
  { bool ok = true; for (int s = 0; s < 7; s++) ok = ok && same(out[s], mult[lens[s]]); expect(ok, "segments of 0, 1, 2, 63, 64, 65, 130 equal terms: every tree step doubles"); }
  { const g1_affine_t two[2] = {G, G}; const fe_t k[2] = {fr_small(130), fr_small(130)}; const uint64_t o2[2] = {0, 2}; g1_affine_t r; sst_msm_segmented(two, k, o2, 1, &r);
    expect(same(r, mult[260]), "the same base twice with equal scalars"); }
  { const g1_affine_t pm[2] = {mult[3], g1_affine_neg(mult[3])}; const fe_t k[2] = {fr_small(41), fr_small(41)}; const uint64_t o2[2] = {0, 2}; g1_affine_t r; sst_msm_segmented(pm, k, o2, 1, &r);
    expect(same(r, O), "P and -P with equal scalars give the identity"); }
  { std::vector<g1_affine_t> b2; std::vector<fe_t> s2; uint32_t want = 0;   // 66 distinct terms: lane 0 and lane 1 walk two terms each
    for (uint32_t i = 0; i < 66; i++) { b2.push_back(mult[1 + i % 3]); s2.push_back(fr_small(i % 2 + 1)); want += (1 + i % 3) * (i % 2 + 1); }
    const uint64_t o2[2] = {0, 66}; g1_affine_t r; sst_msm_segmented(b2.data(), s2.data(), o2, 1, &r);
    expect(want <= 260 && same(r, mult[want]), "66 mixed terms"); }
  printf("%s\n", fails ? "FAILED" : "all passed");
  return fails ? 1 : 0;
}
#endif
