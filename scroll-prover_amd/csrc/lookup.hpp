// lookup.hpp -- the multiplicity column m of the log-derivative ("mv") lookup argument, computed on the device from the compressed columns
// [EXT-recalled halo2_proofs src/plonk/mv_lookup/prover.rs, `prepare`: a map from each compressed table value to a row of the usable range, then
// m[row] += 1 for every compressed input cell; an input value that is not in the table is Error::ConstraintSystemFailure].
//
//   k_lk_insert   open-addressing hash set in HBM of u32 TABLE ROW INDICES (no key is copied: a slot names a row, and the row's 32-byte word is the key).
//                 Only the row that starts (first-occurrence rule) or ends (last-occurrence rule) a run of equal values inserts, so the zero tail of a
//                 range table is one insert, not 2^k.  A slot is claimed by compare-and-swap; when it already names a row of equal value the inserting
//                 row is folded in by atomicMin (first rule) / atomicMax (last rule), so the slot keeps naming a row of that value and ends on the
//                 smallest / largest such row whatever the order of arrival.
//   k_lk_probe    one wave counts a contiguous range of one input column: hash, probe, and add 1 to the u32 count of the row found.  Equal rows are
//                 combined before any global atomic: the wave keeps one HOT (row, count) pair in registers (the value that dominates real columns --
//                 the all-zero tuple of the rows a selector switches off) and adds it once at the end; up to LK_ROUNDS further groups per 64 rows are
//                 summed by a ballot and added by one lane; whatever is left adds one by one.  A value missing from the table: the wave's first miss is
//                 the smallest row of that column in its range, and only that one goes to the error word by atomicMin of (column << 40 | row).
// The expansion of the counts into Montgomery Fr is k_expand_packed<4> (frscan.hpp).
//
// Equality is equality of the 32-byte words: the ABI holds Fr fully reduced in Montgomery form (include/mi355zk.h, "Data conventions"), so equal
// words are equal field elements and equal elements have equal words.  Integer counts and min / max make the output and the reported error
// independent of scheduling (only which slot a value lands in depends on it, never which row a probe finds).
// Stores are plain C++ stores and vector atomics; no kernel here uses LDS or scratch.
#pragma once
#include "fp.hpp"

namespace zk {
constexpr uint32_t LK_EMPTY = 0xffffffffu;   // a free slot (table rows are < 2^32 - 1)
constexpr int LK_ROUNDS = 4;                 // ballot-combined groups per 64 rows, after the hot row
constexpr uint32_t LK_HOT_MIN = 16;          // the smallest group of one block that may become the hot row

// host code sees the comparison and the hash too (tests/hostcheck/lookup_hash_main.cpp places keys in chosen slots with them)
ZK_HD bool lk_eq(const fe_t &a, const fe_t &b) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) d |= a.l[k] ^ b.l[k];
  return d == 0;
}
// all 256 bits mixed (a range table in Montgomery form differs anywhere in the word), then the splitmix64 finaliser
ZK_HD uint32_t lk_hash(const fe_t &v, uint32_t mask) {
  uint64_t h = ((uint64_t)v.l[1] << 32 | v.l[0]);
  h = (h ^ (h >> 31)) * 0x9E3779B97F4A7C15ull ^ ((uint64_t)v.l[3] << 32 | v.l[2]);
  h = (h ^ (h >> 29)) * 0xBF58476D1CE4E5B9ull ^ ((uint64_t)v.l[5] << 32 | v.l[4]);
  h = (h ^ (h >> 32)) * 0x94D049BB133111EBull ^ ((uint64_t)v.l[7] << 32 | v.l[6]);
  h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull; h = (h ^ (h >> 27)) * 0x94D049BB133111EBull; h ^= h >> 31;
  return (uint32_t)h & mask;
}

#ifdef __HIPCC__

constexpr uint32_t LK_THREADS = 256;

// slots: mask + 1 entries (a power of two >= 2 x rows), LK_EMPTY on entry
template <bool LAST> __global__ void __launch_bounds__(LK_THREADS) k_lk_insert(const fe_t *__restrict__ table, uint64_t rows, uint32_t *slots, uint32_t mask) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * blockDim.x) {
    const fe_t v = g_load(&table[r]);
    if (LAST ? r + 1 < rows : r > 0) { if (lk_eq(g_load(&table[LAST ? r + 1 : r - 1]), v)) continue; }   // inside a run: its first / last row stands for it
    uint32_t h = lk_hash(v, mask);
    for (;;) {
      // a stale read is harmless: a slot only ever goes from EMPTY to a row, then to other rows of the SAME value
      uint32_t cur = __hip_atomic_load(&slots[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == LK_EMPTY) { cur = atomicCAS(&slots[h], LK_EMPTY, (uint32_t)r); if (cur == LK_EMPTY) break; }
      if (lk_eq(g_load(&table[cur]), v)) { if (LAST) atomicMax(&slots[h], (uint32_t)r); else atomicMin(&slots[h], (uint32_t)r); break; }
      h = (h + 1) & mask;
    }
  }
}

// one wave per `wave_rows` (a multiple of 64) consecutive rows of one input column; cnt: u32 per table row; err: (column << 40 | row) of the smallest miss
__global__ void __launch_bounds__(LK_THREADS) k_lk_probe(const fe_t *__restrict__ in, uint64_t rows, uint64_t col, const fe_t *__restrict__ table, const uint32_t *__restrict__ slots,
                                                          uint32_t mask, uint32_t *cnt, unsigned long long *err, uint64_t wave_rows) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t lo = wave * wave_rows, hi = lo + wave_rows < rows ? lo + wave_rows : rows;
  uint32_t hot = LK_EMPTY, hot_cnt = 0;   // wave-uniform
  bool missed = false;                    // wave-uniform
  for (uint64_t base = lo; base < hi; base += 64) {
    const uint64_t r = base + lane;
    uint32_t row = LK_EMPTY; bool miss = false;
    if (r < hi) {
      const fe_t v = g_load(&in[r]);
      uint32_t h = lk_hash(v, mask);
      for (;;) {
        const uint32_t s = slots[h];
        if (s == LK_EMPTY) { miss = true; break; }
        if (lk_eq(g_load(&table[s]), v)) { row = s; break; }
        h = (h + 1) & mask;
      }
    }
    const uint64_t mb = __ballot(miss);
    if (mb && !missed) { missed = true; if (lane == (uint32_t)(__ffsll((unsigned long long)mb) - 1)) atomicMin(err, (unsigned long long)(col << 40 | r)); }
    uint64_t act = __ballot(row != LK_EMPTY);
    if (hot != LK_EMPTY) { const uint64_t m = __ballot(row == hot) & act; hot_cnt += (uint32_t)__popcll(m); act &= ~m; }
    for (int round = 0; round < LK_ROUNDS && act; round++) {
      const int lead = __ffsll((unsigned long long)act) - 1;
      const uint32_t lr = __shfl(row, lead);
      const uint64_t m = __ballot(row == lr) & act;
      const uint32_t c = (uint32_t)__popcll(m);
      if (c >= LK_HOT_MIN && hot_cnt < c) {   // a bigger group than the held one: it becomes the hot row, the old one is added
        if (hot_cnt && lane == (uint32_t)lead) atomicAdd(&cnt[hot], hot_cnt);
        hot = lr; hot_cnt = c;
      } else if (lane == (uint32_t)lead) atomicAdd(&cnt[lr], c);
      act &= ~m;
    }
    if (act >> lane & 1) atomicAdd(&cnt[row], 1u);
  }
  if (hot_cnt && lane == 0) atomicAdd(&cnt[hot], hot_cnt);
}

#endif  // __HIPCC__
}  // namespace zk
