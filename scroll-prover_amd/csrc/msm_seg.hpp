// msm_seg.hpp -- segmented G1 MSM for MANY SHORT segments: out[s] = sum_{offsets[s] <= i < offsets[s+1]} scalars[i] * bases[i].
// The shape is a batch verifier's: one list of 19-24 (scalar, point) terms per proof, hundreds of proofs.  The bucket method of msm.hpp pays its
// digit / sort / accumulate / reduce launches per call and cannot amortise them over 20 points; here ONE wavefront owns a segment:
//   lane l    walks the terms offsets[s] + l, + 64, ...; per term it takes the scalar out of Montgomery form (as k_fixed_base_mul does), runs an MSB-first
//             double-and-add over the affine base (g1_xyzz_dbl / g1_xyzz_madd) and adds the product to its accumulator (g1_xyzz_add)
//   tree      64 -> 1 by shuffles, which EVERY lane reaches (no early return; lanes without terms carry the identity)
//   lane 0    one division-step inversion (g1_xyzz_to_affine) and the 64-byte store
// No LDS, no workspace between kernels, no atomics, no formula of its own: the point arithmetic is g1.hpp's.  A long segment is correct and slow
// (the lanes share it, the double-and-add does not get cheaper); the bucket pipeline is the tool for those.
// segmsm_term is __host__ __device__: tests/hostcheck/segmsm_selftest.cpp runs it on the CPU with the lanes as a loop and segmsm_tree_src as the tree's order.
#pragma once
#include "g1.hpp"
#include "fp_asm.hpp"

namespace zk {

constexpr uint32_t SEGMSM_LANES = 64;
constexpr int SEGMSM_TOP_BIT = 253;   // a canonical Fr scalar is below r < 2^254

// acc += k * P.  k arrives in Montgomery form (the ABI's Fr); P affine, the identity (0, 0) allowed (every madd returns at once, the product stays the identity).
// The exceptional additions -- the first set bit (identity + P), P + P after a lone doubling -- are the formula layer's own cases.
template <class F> ZK_HD void segmsm_term(g1_xyzz_t &acc, const g1_affine_t &P, const fe_t &k_mont) {
  fe_t one_c = Fr::zero(); one_c.l[0] = 1;
  fe_t k = FrPs::mul(k_mont, one_c);
  // the bit under test is always bit 255: the scalar moves left one place per step, so no word of it is indexed by a loop variable (a private array indexed
  // that way would be placed in LDS by the compiler)
  for (int s = 0; s < 255 - SEGMSM_TOP_BIT; s++) { for (int j = 7; j > 0; j--) k.l[j] = (k.l[j] << 1) | (k.l[j - 1] >> 31); k.l[0] <<= 1; }
  g1_xyzz_t m = g1_xyzz_identity();
#pragma unroll 1
  for (int i = SEGMSM_TOP_BIT; i >= 0; i--) {
    m = g1_xyzz_dbl<F>(m);
    if (k.l[7] >> 31) g1_xyzz_madd<F>(m, P);
    for (int j = 7; j > 0; j--) k.l[j] = (k.l[j] << 1) | (k.l[j - 1] >> 31);
    k.l[0] <<= 1;
  }
  g1_xyzz_add<F>(acc, m);
}
// The tree: at step o = 32, 16, ..., 1 lane l < o adds lane l + o's value to its own; the lanes from o on are finished and add the identity.
ZK_HD bool segmsm_tree_takes(uint32_t lane, uint32_t o) { return lane < o; }

#if defined(__HIPCC__)
__device__ __forceinline__ g1_xyzz_t shfl_down_xyzz(const g1_xyzz_t &v, uint32_t o) {
  g1_xyzz_t r;
  const uint32_t *s = reinterpret_cast<const uint32_t *>(&v); uint32_t *d = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
  for (int i = 0; i < 32; i++) d[i] = __shfl_down(s[i], o);
  return r;
}

// grid = segments, one wavefront each.  offsets: segments + 1 values, non-decreasing, offsets[segments] = the length of bases / scalars (checked by the host).
__global__ void __launch_bounds__(64) k_msm_g1_segmented(const g1_affine_t *__restrict__ bases, const fe_t *__restrict__ scalars, const uint64_t *__restrict__ offsets,
                                                         g1_affine_t *__restrict__ out) {
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  const uint64_t lo = offsets[seg], hi = offsets[seg + 1];
  g1_xyzz_t acc = g1_xyzz_identity();
#pragma unroll 1
  for (uint64_t i = lo + lane; i < hi; i += SEGMSM_LANES) segmsm_term<FqPs>(acc, load_affine(&bases[i]), g_load(&scalars[i]));
#pragma unroll 1
  for (uint32_t o = SEGMSM_LANES / 2; o >= 1; o >>= 1) {
    g1_xyzz_t other = shfl_down_xyzz(acc, o);
    if (!segmsm_tree_takes(lane, o)) other = g1_xyzz_identity();
    g1_xyzz_add<FqPs>(acc, other);
  }
  if (lane == 0) { const g1_affine_t r = g1_xyzz_to_affine(acc); g_store(&out[seg].x, r.x); g_store(&out[seg].y, r.y); }
}
#endif  // __HIPCC__

}  // namespace zk
