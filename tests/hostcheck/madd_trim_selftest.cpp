// madd_trim_selftest.cpp -- TEST INFRASTRUCTURE: the mixed addition k_msm_accumulate runs (g1_29.hpp, g1_xyzz29_madd: x held
// negated between additions, flushed through g1_xyzz29_negx_to_plain) compiled for the CPU with plain g++.  Never shipped.
#include "../../scroll-prover_amd/csrc/g1.hpp"
#include "../../scroll-prover_amd/csrc/fp29.hpp"
#include "../../scroll-prover_amd/csrc/g1_29.hpp"
using namespace zk;

// the invariants g1_29.hpp documents for an accumulator of the mixed addition (x negated) between additions; returns a bit mask of what is violated
static uint32_t check_acc(const g1_xyzz29_t &a) {
  uint32_t bad = 0;
  if (g1_xyzz29_is_identity(a)) return 0;
  for (int i = 0; i < 8; i++) {
    if (a.x.l[i] > (1u << 29) + 8) bad |= 1;
    if (a.y.l[i] > (1u << 30) - 2) bad |= 2;
    if (a.zz.l[i] >= (1u << 29) || a.zzz.l[i] >= (1u << 29)) bad |= 4;
  }
  if (a.x.l[8] > 0x2a57c4fu /* 14 p >> 232 */) bad |= 8;
  if (a.y.l[8] > 0x12725dfu /* 6.1 p >> 232, rounded up */) bad |= 16;
  if (a.zz.l[8] > 0x60c89cu || a.zzz.l[8] > 0x60c89cu /* 2 p >> 232 */) bad |= 32;
  return bad;
}
static g1_affine_t finish(g1_xyzz29_t acc) {
  g1_xyzz29_negx_to_plain(acc);
  const g1_jac_t j = g1_xyzz_to_jac_normalised(g1_xyzz29_to_sat(acc));
  g1_affine_t r; r.x = j.x; r.y = j.y;
  if (Fq::is_zero(j.z)) { r.x = Fq::zero(); r.y = Fq::zero(); }
  return r;
}
// out[s] = affine sum of sequence s = entries [off[s], off[s+1]) (all-zero words = identity); returns the OR of the invariant masks after every addition
extern "C" uint32_t mt_bucket_sums(void *out_affine, const void *pts, const uint8_t *signs, const uint64_t *off, uint64_t nseq) {
  const g1_affine_t *p = (const g1_affine_t *)pts; g1_affine_t *o = (g1_affine_t *)out_affine; uint32_t bad = 0;
  for (uint64_t s = 0; s < nseq; s++) {
    g1_xyzz29_t acc = g1_xyzz29_identity();
    for (uint64_t i = off[s]; i < off[s + 1]; i++) { g1_xyzz29_madd(acc, p[i], signs[i] & 1); bad |= check_acc(acc); }
    o[s] = finish(acc);
  }
  return bad;
}
// one addition on a raw accumulator (36 words: x, y, zz, zzz as 9 limbs each), so that a test can place lazy coordinates itself
extern "C" uint32_t mt_madd_raw(uint32_t *acc36, const void *pt, int negate) {
  g1_xyzz29_t &acc = *(g1_xyzz29_t *)acc36;
  g1_xyzz29_madd(acc, *(const g1_affine_t *)pt, negate != 0);
  return check_acc(acc);
}
// the same with the addend given as 29-bit limbs (x2, y2 as madd_core takes them): any representative of y2 modulo p with limbs < 2^30
extern "C" uint32_t mt_madd_core_raw(uint32_t *acc36, const uint32_t *x2, const uint32_t *y2, int normalise_y) {
  g1_xyzz29_t &acc = *(g1_xyzz29_t *)acc36; fe29_t x, y;
  for (int i = 0; i < 9; i++) { x.l[i] = x2[i]; y.l[i] = y2[i]; }
  g1_xyzz29_madd_core(acc, x, y, normalise_y != 0);
  return check_acc(acc);
}
extern "C" void mt_from_sat(uint32_t *out9, const void *fe) { const fe29_t r = Fq29::from_sat(*(const fe_t *)fe); for (int i = 0; i < 9; i++) out9[i] = r.l[i]; }
extern "C" void mt_finish(void *out_affine, const uint32_t *acc36) { *(g1_affine_t *)out_affine = finish(*(const g1_xyzz29_t *)acc36); }
