// msm_g2.hpp -- BN254 G2 multi-scalar multiplication (Pippenger / bucket method over the twist) for gfx950: the point-specific half of
// the schedule.  The scalar half is msm.hpp's, unchanged: k_msm_digits and the two-level counting sort (shared = 0, no window tables)
// turn the scalars into a list of (point index | sign << 31) entries grouped by (window, bucket); nothing there looks at a point.
//
//   0 k_msm_g2_validate     every base on the twist (or the identity); the first bad index by an atomic minimum
//   1 k_msm_g2_accumulate   SEGMENTED bucket accumulation as k_msm_accumulate: thread t owns entries [t*L, (t+1)*L) whatever bucket
//                           boundaries fall inside, keeps an Fq2 XYZZ accumulator in registers (64 VGPRs), gathers 128-byte affine
//                           bases, applies the sign of the digit by negating y, flushes at bucket boundaries (256-byte records)
//   2 k_msm_g2_segfix       buckets that straddle threads: one segmented reduction by key over the partial records (k_msm_segfix's
//                           scheme: doubling steps inside a wavefront, log-many levels), so a bucket of a million partials -- an all-equal
//                           scalar column -- is a tree, never one lane's walk
//   3 k_msm_g2_bucket_reduce / k_msm_g2_tree_sum   sum_b (b+1) B[b] by chunked running sums, then per-window trees
//   4 k_msm_g2_final        Horner over windows, normalisation with Fq2::inv
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

// ---- 1. segmented accumulation (k_msm_accumulate's walk; seg_max / seg_min: the segment bounds, the kernel derives the segment from
// the actual entry count with msm_seg_eff at 100 % fill)
__global__ void __launch_bounds__(256) k_msm_g2_accumulate(const g2_affine_t *__restrict__ bases, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ offsets,
                                                          uint32_t nbuckets, g2_xyzz_t *__restrict__ bucket_sums, g2_xyzz_t *__restrict__ part, int32_t *__restrict__ part_id,
                                                          uint32_t seg_max, uint32_t seg_min) {
  const uint32_t total = offsets[nbuckets];
  const uint32_t seg = msm_seg_eff(total, gridDim.x * blockDim.x, seg_max, seg_min, 100);
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t start64 = (uint64_t)t * seg;
  if (start64 >= total) { part_id[2 * t] = -1; part_id[2 * t + 1] = -1; return; }
  const uint32_t start = (uint32_t)start64, end = (uint32_t)min((uint64_t)total, start64 + seg);
  uint32_t lo = 0, hi = nbuckets;   // offsets[lo] <= start < offsets[hi]
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (offsets[mid] <= start) lo = mid; else hi = mid; }
  uint32_t b = lo, b_start = offsets[b], b_end = offsets[b + 1];
  int32_t id_first = -1, id_last = -1;
  g2_xyzz_t acc = g2_xyzz_identity();
  // software pipeline: the index of entry pos + 1 and its 128-byte base are loaded before the additions of entry pos
  uint32_t ent = sorted[start];
  g2_affine_t p = load_g2_affine(&bases[ent & 0x7fffffffu]);
  for (uint32_t pos = start; pos < end; pos++) {
    uint32_t ent_next = ent; g2_affine_t p_next = p;
    if (pos + 1 < end) { ent_next = sorted[pos + 1]; p_next = load_g2_affine(&bases[ent_next & 0x7fffffffu]); }
    if (pos >= b_end) {
      if (b_start >= start) store_g2_xyzz(&bucket_sums[b], acc);                         // began here too: sole owner
      else { store_g2_xyzz(&part[2 * (uint64_t)t], acc); id_first = (int32_t)b; }       // began in an earlier thread
      acc = g2_xyzz_identity();
      b++; b_start = b_end; b_end = offsets[b + 1];
      if (pos >= b_end) {   // a run of empty buckets: binary search for the bucket that holds `pos`
        uint32_t l2 = b, h2 = nbuckets;
        while (h2 - l2 > 1) { const uint32_t mid = (l2 + h2) >> 1; if (offsets[mid] <= pos) l2 = mid; else h2 = mid; }
        b = l2; b_start = offsets[b]; b_end = offsets[b + 1];
      }
    }
    if (ent >> 31) p.y = Fq2ps::neg(p.y);   // negative digit: -P = (x, -y); the identity stays all zero
    g2_xyzz_madd<Fq2ps>(acc, p);
    ent = ent_next; p = p_next;
  }
  if (b_start >= start && b_end <= end) store_g2_xyzz(&bucket_sums[b], acc);
  else if (b_start < start) { store_g2_xyzz(&part[2 * (uint64_t)t], acc); id_first = (int32_t)b; }   // spans the whole segment or just its head
  else { store_g2_xyzz(&part[2 * (uint64_t)t + 1], acc); id_last = (int32_t)b; }                        // began here, continues in the next thread
  part_id[2 * t] = id_first; part_id[2 * t + 1] = id_last;
}

// ---- 2. fix-up of straddling buckets: k_msm_segfix on 256-byte G2 records.  The 2 * threads partial slots, read in thread order, are
// sorted by bucket; every wavefront fills keys forward over empty slots, forms suffix sums of equal keys by doubling, stores the runs that
// lie strictly inside it and hands its first and last run (two slots) to the next level; last_level: one wavefront stores every run.
__global__ void __launch_bounds__(256) k_msm_g2_segfix(const int32_t *__restrict__ ids, const g2_xyzz_t *__restrict__ recs, uint32_t n, g2_xyzz_t *__restrict__ bucket_sums,
                                                      int32_t *__restrict__ ids_out, g2_xyzz_t *__restrict__ recs_out, int last_level) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63, wave = j >> 6;
  if (wave >= ((n + 63) >> 6)) return;
  const int32_t key0 = j < n ? ids[j] : -1;
  g2_xyzz_t val = key0 >= 0 ? load_g2_xyzz(&recs[j]) : g2_xyzz_identity();
  int32_t key = key0;
  for (uint32_t o = 1; o < 64; o <<= 1) { const int32_t kk = __shfl_up(key, o); if (lane >= o && key < 0) key = kk; }
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const int32_t k2 = __shfl_down(key, o);
    const bool take = lane + o < 64 && key >= 0 && k2 == key;
    if (__ballot(take) == 0) continue;
    const g2_xyzz_t other = shfl_down_g2(val, o);
    if (take) g2_xyzz_add<Fq2ps>(val, other);
  }
  const int32_t kprev = __shfl_up(key, 1);
  const bool head = key >= 0 && (lane == 0 || kprev != key);
  const uint64_t valid = __ballot(key >= 0);
  const uint32_t first_lane = valid ? (uint32_t)__ffsll((unsigned long long)valid) - 1 : 64u;
  const int32_t key_last = __shfl(key, 63), key_first = __shfl(key, first_lane < 64u ? (int)first_lane : 0);
  const bool is_first = head && lane == first_lane, is_last = head && key == key_last;
  if (last_level) { if (head) store_g2_xyzz(&bucket_sums[key], val); return; }
  if (head && !is_first && !is_last) store_g2_xyzz(&bucket_sums[key], val);
  if (is_first) { ids_out[2 * wave] = key; store_g2_xyzz(&recs_out[2 * (uint64_t)wave], val); }
  if (is_last && !is_first) { ids_out[2 * wave + 1] = key; store_g2_xyzz(&recs_out[2 * (uint64_t)wave + 1], val); }
  if (lane == 0) {
    if (first_lane == 64u) { ids_out[2 * wave] = -1; ids_out[2 * wave + 1] = -1; }
    else if (key_first == key_last) ids_out[2 * wave + 1] = -1;
  }
}

// ---- 3a. chunked running sums: logical thread j of bucket set w covers buckets [j K, (j + 1) K) and emits T + (j K) S, S = sum B_i,
// T = sum (i_local + 1) B_i
__global__ void __launch_bounds__(128) k_msm_g2_bucket_reduce(const g2_xyzz_t *__restrict__ bucket_sums, g2_xyzz_t *__restrict__ chunk_out, uint32_t nb, uint32_t sets, uint32_t chunk) {
  const uint32_t chunks_per_set = nb / chunk, gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= chunks_per_set * sets) return;
  const uint32_t w = gi / chunks_per_set, j = gi - w * chunks_per_set;
  const g2_xyzz_t *B = bucket_sums + (uint64_t)w * nb + (uint64_t)j * chunk;
  g2_xyzz_t run = g2_xyzz_identity(), T = g2_xyzz_identity();
  for (uint32_t i = chunk; i-- > 0;) { g2_xyzz_add<Fq2ps>(run, load_g2_xyzz(&B[i])); g2_xyzz_add<Fq2ps>(T, run); }
  if (j != 0) {
    const uint32_t k = j * chunk;
    g2_xyzz_t kS = g2_xyzz_identity();
    for (int bit = 31 - __clz(k); bit >= 0; bit--) { kS = g2_xyzz_dbl<Fq2ps>(kS); if ((k >> bit) & 1) g2_xyzz_add<Fq2ps>(kS, run); }
    g2_xyzz_add<Fq2ps>(T, kS);
  }
  store_g2_xyzz(&chunk_out[gi], T);
}
// ---- 3b. per bucket set: a block of 256 lanes folds up to 256 * TREE_PER_THREAD inputs (wavefront shuffles, LDS across the 4 waves);
// grid = (blocks, sets), launched until one value per set is left
__global__ void __launch_bounds__(256) k_msm_g2_tree_sum(const g2_xyzz_t *__restrict__ in, uint32_t in_per_set, g2_xyzz_t *__restrict__ out, uint32_t out_per_set) {
  __shared__ g2_xyzz_t lds[4];
  const uint32_t w = blockIdx.y, first = blockIdx.x * 256 * TREE_PER_THREAD;
  const g2_xyzz_t *src = in + (uint64_t)w * in_per_set;
  g2_xyzz_t acc = g2_xyzz_identity();
  for (uint32_t k = 0; k < TREE_PER_THREAD; k++) { const uint32_t i = first + k * 256 + threadIdx.x; if (i < in_per_set) g2_xyzz_add<Fq2ps>(acc, load_g2_xyzz(&src[i])); }
  for (uint32_t o = 32; o >= 1; o >>= 1) { const g2_xyzz_t other = shfl_down_g2(acc, o); g2_xyzz_add<Fq2ps>(acc, other); }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) { for (uint32_t k = 1; k < 4; k++) g2_xyzz_add<Fq2ps>(acc, lds[k]); store_g2_xyzz(&out[(uint64_t)w * out_per_set + blockIdx.x], acc); }
}
// ---- 4. Horner over the W window sums of MSM blockIdx.x, then the normalised G2Affine (identity: 128 zero bytes).  One lane.
__global__ void __launch_bounds__(64) k_msm_g2_final(const g2_xyzz_t *__restrict__ window_sums, uint32_t windows, uint32_t c, g2_affine_t *__restrict__ out) {
  if (threadIdx.x != 0) return;
  window_sums += (uint64_t)blockIdx.x * windows;
  g2_xyzz_t acc = g2_xyzz_identity();
  for (uint32_t w = windows; w-- > 0;) {
    for (uint32_t k = 0; k < c; k++) acc = g2_xyzz_dbl<Fq2ps>(acc);
    g2_xyzz_add<Fq2ps>(acc, load_g2_xyzz(&window_sums[w]));
  }
  out[blockIdx.x] = g2_xyzz_to_affine<Fq2ps>(acc);
}

#endif  // __HIPCC__

}  // namespace zk
