// check.hpp -- the two reductions behind MockProver::verify on the device [EXT-recalled halo2_proofs src/dev.rs, MockProver::verify: every gate over every row, every
// copy constraint, every lookup input; the failures it returns name the constraint and the row].  A vector of 2^k words (a gate evaluated on the Lagrange domain) or a
// list of cell pairs (the copy mapping) becomes "how many fail, and the smallest `cap` of them in ascending order" without a column crossing the link.
//
//   check_count / check_write   ONE helper for both kernels: a per-element predicate -> count + the first `cap` indices, ascending.  A workgroup owns CHECK_TILE
//                       consecutive elements (CHECK_ITEMS per thread, strided: lane i of a wave reads word base + i, 32 B each).
//                       PHASE 0 writes the workgroup's count; k_check_scan (one workgroup per vector) turns the counts into exclusive prefixes, carried in from
//                       and out to a running total; PHASE 1 runs again only in workgroups that counted something AND whose prefix is below cap -- a clean
//                       vector is read once -- and ranks its hits by wave ballot: prefix + hits of earlier items + hits of earlier waves + hits of lower lanes.
//   k_fr_nonzero_rows   predicate: the 32-byte word is not all-zero (all eight limbs).  blockIdx.y = vector of the batch.
//   k_fr_copy_check     predicate: the words of cell and image of pair t differ.  A cell is column * n + row (perm.hpp).  The lists arrive in staged pieces; the
//                       running total carries the rank from piece to piece.
// No atomics at all: the output is a pure function of the input (counts, prefixes and ranks are sums of ballots).  LDS: CHECK_ITEMS x 4 wave counts per workgroup
// (the scan: 256 partial sums).  Plain vector stores; no scratch.  Both kernels stream: 32 B per row, or 16 B of list + two 32 B gathers per pair.
#pragma once
#include "fp.hpp"

namespace zk {
#ifdef __HIPCC__

constexpr uint32_t CHECK_THREADS = 256, CHECK_ITEMS = 4, CHECK_TILE = CHECK_THREADS * CHECK_ITEMS, CHECK_MAX_CAP = 65536;
constexpr uint32_t CHECK_PREFIX_SAT = 0xffffffffu;   // a prefix is only compared with cap <= 65536: it saturates here

__device__ __forceinline__ bool check_word_nonzero(const fe_t &a) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) d |= a.l[k];
  return d != 0;
}
__device__ __forceinline__ bool check_words_differ(const fe_t &a, const fe_t &b) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) d |= a.l[k] ^ b.l[k];
  return d != 0;
}

// bit `it` = pred(element base + it * CHECK_THREADS + threadIdx.x).  Every lane evaluates the predicate on an index clamped into [0, count): the loads of the
// CHECK_ITEMS elements are independent and unconditional, the tail is masked afterwards.  count > 0.
template <class Pred> __device__ __forceinline__ uint32_t check_flags(const Pred &pred, uint64_t base, uint64_t count) {
  uint32_t f = 0;
#pragma unroll
  for (uint32_t it = 0; it < CHECK_ITEMS; it++) {
    const uint64_t i = base + it * CHECK_THREADS + threadIdx.x;
    const bool hit = pred(i < count ? i : count - 1);
    f |= (hit && i < count ? 1u : 0u) << it;
  }
  return f;
}

// PHASE 0: block_cnt[blockIdx.x] = hits among the elements [blockIdx.x * CHECK_TILE, + CHECK_TILE) of [0, count)
template <class Pred> __device__ __forceinline__ void check_count(const Pred &pred, uint64_t count, uint32_t *block_cnt) {
  __shared__ uint32_t wave_cnt[CHECK_THREADS / 64];
  const uint32_t f = check_flags(pred, (uint64_t)blockIdx.x * CHECK_TILE, count);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t it = 0; it < CHECK_ITEMS; it++) c += (uint32_t)__popcll(__ballot((f >> it) & 1));
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) { uint32_t s = 0; for (uint32_t w = 0; w < CHECK_THREADS / 64; w++) s += wave_cnt[w]; block_cnt[blockIdx.x] = s; }
}

// PHASE 1: out[rank] = index_base + element for every hit of rank < cap; rank = block_pre[blockIdx.x] + the hits before it in this workgroup, in element order
template <class Pred> __device__ __forceinline__ void check_write(const Pred &pred, uint64_t count, const uint32_t *block_cnt, const uint32_t *block_pre, uint32_t cap,
                                                                  uint64_t index_base, uint64_t *out) {
  __shared__ uint32_t wave_cnt[CHECK_ITEMS][CHECK_THREADS / 64];
  const uint32_t pre = block_pre[blockIdx.x];
  if (block_cnt[blockIdx.x] == 0 || pre >= cap) return;   // uniform over the workgroup
  const uint64_t base = (uint64_t)blockIdx.x * CHECK_TILE;
  const uint32_t f = check_flags(pred, base, count), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t below[CHECK_ITEMS];                              // hits of lower lanes of this wave, per item
#pragma unroll
  for (uint32_t it = 0; it < CHECK_ITEMS; it++) {
    const uint64_t m = __ballot((f >> it) & 1);
    below[it] = (uint32_t)__popcll(m & ((1ull << lane) - 1));
    if (lane == 0) wave_cnt[it][wave] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  uint32_t rank = pre;
#pragma unroll
  for (uint32_t it = 0; it < CHECK_ITEMS; it++) {
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < CHECK_THREADS / 64; w++) { const uint32_t c = wave_cnt[it][w]; all += c; before += w < wave ? c : 0; }
    const uint32_t r = rank + before + below[it];
    if (((f >> it) & 1) && r < cap) out[r] = index_base + base + it * CHECK_THREADS + threadIdx.x;
    rank += all;
  }
}

// one workgroup per vector (blockIdx.x): block_pre[b] = min(total_io + sum_{b' < b} block_cnt[b'], CHECK_PREFIX_SAT), then total_io += sum of all counts.
// A thread sums a contiguous run of counts, the 256 run sums are scanned through LDS, the thread walks its run again.
__global__ void __launch_bounds__(CHECK_THREADS) k_check_scan(const uint32_t *__restrict__ block_cnt, uint32_t *__restrict__ block_pre, uint32_t nblocks, unsigned long long *total_io) {
  __shared__ unsigned long long part[CHECK_THREADS];
  const uint32_t *cnt = block_cnt + (uint64_t)blockIdx.x * nblocks; uint32_t *pre = block_pre + (uint64_t)blockIdx.x * nblocks;
  const uint32_t run = (nblocks + CHECK_THREADS - 1) / CHECK_THREADS;
  const uint64_t lo64 = (uint64_t)threadIdx.x * run;
  const uint32_t lo = lo64 < nblocks ? (uint32_t)lo64 : nblocks, hi = lo64 + run < nblocks ? (uint32_t)(lo64 + run) : nblocks;
  unsigned long long s = 0;
  for (uint32_t b = lo; b < hi; b++) s += cnt[b];
  part[threadIdx.x] = s;
  __syncthreads();
  unsigned long long acc = total_io[blockIdx.x], all = 0;
  for (uint32_t t = 0; t < CHECK_THREADS; t++) { const unsigned long long p = part[t]; all += p; acc += t < threadIdx.x ? p : 0; }
  for (uint32_t b = lo; b < hi; b++) { pre[b] = acc < CHECK_PREFIX_SAT ? (uint32_t)acc : CHECK_PREFIX_SAT; acc += cnt[b]; }
  __syncthreads();   // every thread has read the carried-in total
  if (threadIdx.x == 0) total_io[blockIdx.x] += all;
}

struct NonzeroPred {
  const fe_t *v;
  __device__ __forceinline__ bool operator()(uint64_t i) const { return check_word_nonzero(g_load(&v[i])); }
};
// cells / images: this piece of the lists, every entry < n_cols << log_n (checked on the host before the upload)
struct CopyPred {
  const fe_t *const *cols; const uint64_t *cells, *images; uint32_t log_n;
  __device__ __forceinline__ bool operator()(uint64_t t) const {
    const uint64_t c = cells[t], im = images[t], mask = (1ull << log_n) - 1;
    return check_words_differ(g_load(&cols[c >> log_n][c & mask]), g_load(&cols[im >> log_n][im & mask]));
  }
};

// grid (ceil(n / CHECK_TILE), vectors); block_cnt / block_pre: gridDim.x entries per vector; rows: cap entries per vector, preset to ~0
template <int PHASE> __global__ void __launch_bounds__(CHECK_THREADS) k_fr_nonzero_rows(const fe_t *const *__restrict__ vecs, uint64_t n, uint32_t cap, uint32_t *block_cnt,
                                                                                       const uint32_t *__restrict__ block_pre, uint64_t *rows) {
  const NonzeroPred pred{vecs[blockIdx.y]};
  const uint64_t off = (uint64_t)blockIdx.y * gridDim.x;
  if constexpr (PHASE == 0) check_count(pred, n, block_cnt + off);
  else check_write(pred, n, block_cnt + off, block_pre + off, cap, 0, rows + (uint64_t)blockIdx.y * cap);
}

// grid ceil(len / CHECK_TILE): the piece [t0, t0 + len) of the pair list, staged at cells / images
template <int PHASE> __global__ void __launch_bounds__(CHECK_THREADS) k_fr_copy_check(const fe_t *const *__restrict__ cols, uint32_t log_n, const uint64_t *__restrict__ cells,
                                                                                     const uint64_t *__restrict__ images, uint64_t len, uint64_t t0, uint32_t cap,
                                                                                     uint32_t *block_cnt, const uint32_t *__restrict__ block_pre, uint64_t *failed) {
  const CopyPred pred{cols, cells, images, log_n};
  if constexpr (PHASE == 0) check_count(pred, len, block_cnt);
  else check_write(pred, len, block_cnt, block_pre, cap, t0, failed);
}

#endif  // __HIPCC__
}  // namespace zk
