// msm_g2.hpp -- BN254 G2 multi-scalar multiplication (Pippenger / bucket method over the twist) for gfx950: what is G2-specific.
// Everything else is msm.hpp's, instantiated with the policy below: k_msm_digits and the two-level counting sort (shared = 0, no window
// tables) turn the scalars into a list of (point index | sign << 31) entries grouped by (window, bucket) -- nothing there looks at a point --
// and the segment walk, the segmented fix-up (k_msm_segfix<G2Ops>: a bucket of a million partials, an all-equal scalar column, is a tree,
// never one lane's walk), the running sums, the trees and the Horner kernel (k_msm_bucket_reduce / k_msm_tree_sum / k_msm_final <G2Ops, 1>)
// are the templates G1 uses.
//
//   k_msm_g2_validate     every base on the twist (or the identity); the first bad index by an atomic minimum
//   G2Ops                 256-byte Fq2 XYZZ records, g2_xyzz_add / _dbl<Fq2ps>, one lane per logical thread only, normalised G2Affine out
//   k_msm_g2_accumulate   msm_segment_walk over 128-byte affine bases named by plain index; the sign of the digit negates y
//                         (64 VGPRs of accumulator)
//
// Field: the 8 x 32-bit Montgomery form of fp.hpp with the product-scanning multiplier of fp_asm.hpp (Fq2ps); every value stays fully
// reduced, so the records are plain g2_xyzz_t and the host self-test runs the same functions.
#pragma once
#include "msm.hpp"
#include "g2.hpp"

namespace zk {

#if defined(__HIPCC__)

static_assert(sizeof(g2_affine_t) == 128 && sizeof(g2_xyzz_t) == 256, "G2 record sizes (16-byte vector accesses)");

__device__ __forceinline__ g2_affine_t load_g2_affine(const g2_affine_t *p) {
  g2_affine_t r; uint32_t *w = reinterpret_cast<uint32_t *>(&r); const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
  for (int i = 0; i < 8; i++) { const uint4 a = q[i]; w[4 * i] = a.x; w[4 * i + 1] = a.y; w[4 * i + 2] = a.z; w[4 * i + 3] = a.w; }
  return r;
}
__device__ __forceinline__ g2_xyzz_t load_g2_xyzz(const g2_xyzz_t *p) {
  g2_xyzz_t r; uint32_t *w = reinterpret_cast<uint32_t *>(&r); const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
  for (int i = 0; i < 16; i++) { const uint4 a = q[i]; w[4 * i] = a.x; w[4 * i + 1] = a.y; w[4 * i + 2] = a.z; w[4 * i + 3] = a.w; }
  return r;
}
__device__ __forceinline__ void store_g2_xyzz(g2_xyzz_t *p, const g2_xyzz_t &v) {
  const uint32_t *w = reinterpret_cast<const uint32_t *>(&v); uint4 *q = reinterpret_cast<uint4 *>(p);
#pragma unroll
  for (int i = 0; i < 16; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
__device__ __forceinline__ g2_xyzz_t shfl_down_g2(const g2_xyzz_t &v, uint32_t o) {
  g2_xyzz_t r; const uint32_t *s = reinterpret_cast<const uint32_t *>(&v); uint32_t *d = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
  for (int i = 0; i < 64; i++) d[i] = __shfl_down(s[i], o);
  return r;
}

// ---- 0. validation: y^2 = x^3 + b' for every base (b' formed once on the host); *first_bad starts at 0xffffffff
__global__ void __launch_bounds__(256) k_msm_g2_validate(const g2_affine_t *__restrict__ pts, uint64_t n, fe2_t b, uint32_t *__restrict__ first_bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (!g2_is_on_curve_b<Fq2ps>(load_g2_affine(&pts[i]), b)) atomicMin(first_bad, (uint32_t)i);
}

// ---- the point-operations policy of the twist (see G1Ops in msm.hpp); Q = 1 only
struct G2Ops {
  using rec_t = g2_xyzz_t; using out_t = g2_affine_t;
  static constexpr bool QUAD = false;
  static constexpr const char *ROLE = "msm2.";
  static __device__ __forceinline__ rec_t identity() { return g2_xyzz_identity(); }
  static __device__ __forceinline__ rec_t load(const rec_t *p) { return load_g2_xyzz(p); }
  static __device__ __forceinline__ void store(rec_t *p, const rec_t &v) { store_g2_xyzz(p, v); }
  template <int Q> static __device__ __forceinline__ void add(rec_t &acc, const rec_t &o) { static_assert(Q == 1, "G2 has no quad form"); g2_xyzz_add<Fq2ps>(acc, o); }
  template <int Q> static __device__ __forceinline__ rec_t dbl(const rec_t &a) { static_assert(Q == 1, "G2 has no quad form"); return g2_xyzz_dbl<Fq2ps>(a); }
  static __device__ __forceinline__ rec_t shfl_down(const rec_t &v, uint32_t o) { return shfl_down_g2(v, o); }
  static __device__ __forceinline__ void emit(const rec_t &acc, out_t *out, int) { *out = g2_xyzz_to_affine<Fq2ps>(acc); }   // always normalised; identity: 128 zero bytes
};

// ---- 1. segmented accumulation: the walk of msm.hpp over bases named by plain index
struct G2Bases {
  using base_t = g2_affine_t;
  const g2_affine_t *__restrict__ bases;
  __device__ __forceinline__ g2_affine_t load(uint32_t e) const { return load_g2_affine(&bases[e & 0x7fffffffu]); }
  __device__ __forceinline__ void madd(g2_xyzz_t &acc, g2_affine_t p, bool neg) const {
    if (neg) p.y = Fq2ps::neg(p.y);   // negative digit: -P = (x, -y); the identity stays all zero
    g2_xyzz_madd<Fq2ps>(acc, p);
  }
};
__global__ void __launch_bounds__(256) k_msm_g2_accumulate(const g2_affine_t *__restrict__ bases, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ offsets,
                                                          uint32_t nbuckets, g2_xyzz_t *__restrict__ bucket_sums, g2_xyzz_t *__restrict__ part, int32_t *__restrict__ part_id, uint32_t seg_arg) {
  msm_segment_walk<G2Ops>(G2Bases{bases}, sorted, offsets, nbuckets, bucket_sums, part, part_id, seg_arg, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

#endif  // __HIPCC__

}  // namespace zk
