// lookup_permute.hpp -- the permuted columns A' and S' of the classic halo2 lookup argument, built on the device from the compressed input and table
// [EXT-recalled halo2_proofs src/plonk/lookup/prover.rs, `permute_expression_pair`: A' is the input sorted ascending (halo2curves' Ord: the canonical integer,
// to_repr() compared from the most significant byte); the first row of every run of equal values of A' takes that value in S' and uses up one copy of it in the
// table; the copies of the table left over, walked in ascending order, are pop()ed into the other ("repeated") rows from the back, so the j-th leftover lands in the
// j-th LARGEST repeated row; an input value the table lacks is Error::ConstraintSystemFailure].
//
// Only the DISTINCT table values are sorted.  lookup.hpp gives, per distinct value, the smallest table row that holds it (k_lk_insert, first rule) and -- at that
// row -- the number of table rows (k_lk_probe over the table itself) and of input cells (k_lk_probe over the input) with that value.  From there:
//   k_lp_compact   the rows that stand for a value -> a dense list (order of arrival: the sort that follows has distinct keys, so its result does not depend on
//                  it), and the AND / OR of all canonical keys: a radix digit in which AND and OR agree holds ONE value in every key -- its histogram would put
//                  every key in one bucket -- and its pass is skipped (lp_pass_needed; a range table 0 .. 2^bits - 1 costs ceil(bits / 8) passes, not 32)
//   k_lp_gather    one 32-bit word of the canonical key (Montgomery reduction of the table word, lp_canonical) per list entry, once per word that has a pass
//   k_lp_hist / k_lp_scatter   one stable 8-bit LSD pass over (key word, row) pairs: counts per workgroup chunk, a scan (below), ranks by wave ballots
//   k_lp_scan_tile / k_lp_scan_fix   exclusive or inclusive scan of u32 under + or max, 2 048 elements per workgroup, totals scanned recursively
//   k_lp_counts    in sorted order: input cells, leftover copies (lp_leftover_count) and "has a run" per value; their three scans give where each run starts in
//                  A', how many runs precede it and where its leftovers start in the ascending walk
//   k_lp_mark      run i writes i + 1 at its first row / first leftover; an inclusive max-scan then names the run of every row and the owner of every leftover
//   k_lp_expand    row p: A'[p] = the value of its run; S'[p] = the same at a run head, else the value that owns leftover lp_leftover_of_row(p, ...)
// Every quantity is an integer count or a position derived from counts, and every output word is a copy of a table word (fully reduced Montgomery, as the ABI
// holds them): the outputs do not depend on scheduling.  k_lp_hist, k_lp_scatter and k_lp_scan_tile use a few KiB of static LDS; no kernel uses scratch.
#pragma once
#include "lookup.hpp"

namespace zk {
constexpr uint32_t LP_THREADS = 256;
constexpr uint32_t LP_PASSES = 32;                    // 8-bit digits of a 256-bit key, least significant first
constexpr uint32_t LP_CHUNK = 8 * LP_THREADS;         // (key, row) pairs per workgroup of a radix pass: 8 sub-tiles of one pair per thread
constexpr uint32_t LP_SCAN_ITEMS = 8;
constexpr uint32_t LP_SCAN_TILE = LP_SCAN_ITEMS * LP_THREADS;
constexpr uint32_t LP_HEAD = 0xffffffffu;             // lp_leftover_of_row: the row starts its run

// the two header blocks of the workspace: one preset to all-ones, one to zero
struct LpHeadOnes { unsigned long long err, err_table; uint32_t key_and[8]; };
struct LpHeadZero { uint32_t distinct, pad; uint32_t key_or[8]; };

// ---- the per-element bodies, shared with the host check (tests/hostcheck/lookup_permute_main.cpp)
// the integer a Montgomery word stands for: limb 7 is the most significant
ZK_HD fe_t lp_canonical(const fe_t &mont) { return Fr::redc(mont); }
ZK_HD uint32_t lp_key_word(const fe_t &canonical, uint32_t pass) { return canonical.l[pass >> 2]; }
ZK_HD uint32_t lp_digit(uint32_t key_word, uint32_t pass) { return key_word >> ((pass & 3) * 8) & 0xffu; }
// key_and / key_or: AND / OR over the canonical words of every key.  A pass whose digit is the same in all keys moves nothing.
ZK_HD bool lp_pass_needed(const uint32_t key_and[8], const uint32_t key_or[8], uint32_t pass) { return lp_digit(key_and[pass >> 2] ^ key_or[pass >> 2], pass) != 0; }
// copies of a table value that no run head uses up
ZK_HD uint32_t lp_leftover_count(uint32_t table_cells, uint32_t input_cells) { return table_cells - (input_cells ? 1u : 0u); }
// row p of A' lies in a run that starts at row `start` and has `heads_before` runs in front of it; `leftovers`: all leftover copies (= all repeated rows).
// LP_HEAD for the first row of the run; else the index, in the ascending walk of the leftovers, of the copy that lands in row p: p is the
// (p - heads_before - 1)-th repeated row counted from the front, and the walk fills the repeated rows from the back.
ZK_HD uint32_t lp_leftover_of_row(uint32_t p, uint32_t start, uint32_t heads_before, uint32_t leftovers) {
  if (p == start) return LP_HEAD;
  return leftovers - 1u - (p - heads_before - 1u);
}
template <int OP> ZK_HD uint32_t lp_op(uint32_t a, uint32_t b) { return OP ? (a > b ? a : b) : a + b; }   // 0: sum, 1: max; 0 is the identity of both

#ifdef __HIPCC__

// rows that stand for a distinct value (tcnt != 0) -> list[0 .. distinct); AND / OR of their canonical keys
__global__ void __launch_bounds__(LP_THREADS) k_lp_compact(const fe_t *__restrict__ table, uint64_t rows, const uint32_t *__restrict__ tcnt, uint32_t *list, LpHeadOnes *ones, LpHeadZero *zero) {
  uint32_t a[8], o[8];
#pragma unroll
  for (int k = 0; k < 8; k++) { a[k] = 0xffffffffu; o[k] = 0; }
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * blockDim.x) {
    if (!tcnt[r]) continue;
    const uint32_t j = atomicAdd(&zero->distinct, 1u);
    if (j < rows) list[j] = (uint32_t)r;
    const fe_t c = lp_canonical(g_load(&table[r]));
#pragma unroll
    for (int k = 0; k < 8; k++) { a[k] &= c.l[k]; o[k] |= c.l[k]; }
  }
#pragma unroll
  for (int k = 0; k < 8; k++)
    for (int d = 32; d >= 1; d >>= 1) { a[k] &= __shfl_xor(a[k], d); o[k] |= __shfl_xor(o[k], d); }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) { if (a[k] != 0xffffffffu) atomicAnd(&ones->key_and[k], a[k]); if (o[k]) atomicOr(&zero->key_or[k], o[k]); }
  }
}

// key[i] = word `word` of the canonical key of table row list[i]
__global__ void __launch_bounds__(LP_THREADS) k_lp_gather(const fe_t *__restrict__ table, uint64_t rows, const uint32_t *__restrict__ list, uint32_t n, uint32_t word, uint32_t *key) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = list[i];
    if (r >= rows) continue;
    const fe_t c = lp_canonical(g_load(&table[r]));
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) w = (uint32_t)k == word ? c.l[k] : w;
    key[i] = w;
  }
}

// hist[digit * nblk + block]: keys of this workgroup's chunk with that digit
__global__ void __launch_bounds__(LP_THREADS) k_lp_hist(const uint32_t *__restrict__ key, uint32_t n, uint32_t pass, uint32_t *hist, uint32_t nblk) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * LP_CHUNK;
  for (uint32_t t = 0; t < LP_CHUNK / LP_THREADS; t++) {
    const uint64_t e = base + t * LP_THREADS + threadIdx.x;
    if (e < n) atomicAdd(&h[lp_digit(key[e], pass)], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// offs: the exclusive scan of hist.  Stable: within a chunk the pairs keep their order (sub-tile, then wave, then lane).
__global__ void __launch_bounds__(LP_THREADS) k_lp_scatter(const uint32_t *__restrict__ key_in, const uint32_t *__restrict__ val_in, uint32_t *key_out, uint32_t *val_out, uint32_t n,
                                                            uint32_t pass, const uint32_t *__restrict__ offs, uint32_t nblk) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wcnt[LP_THREADS / 64][256];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  base[threadIdx.x] = offs[(uint64_t)threadIdx.x * nblk + blockIdx.x];
  const uint64_t first = (uint64_t)blockIdx.x * LP_CHUNK;
  for (uint32_t t = 0; t < LP_CHUNK / LP_THREADS; t++) {
#pragma unroll
    for (uint32_t w = 0; w < LP_THREADS / 64; w++) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t e = first + t * LP_THREADS + threadIdx.x;
    const bool active = e < n;
    const uint32_t k = active ? key_in[e] : 0, v = active ? val_in[e] : 0, d = lp_digit(k, pass);
    uint64_t same = __ballot(active);   // the active lanes of this wave with the same digit
#pragma unroll
    for (int b = 0; b < 8; b++) { const bool bit = d >> b & 1; const uint64_t bal = __ballot(bit); same &= bit ? bal : ~bal; }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1));
    if (active && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(same);
    __syncthreads();
    if (active) {
      uint32_t pos = base[d] + rank;
      for (uint32_t w = 0; w < wave; w++) pos += wcnt[w][d];
      if (pos < n) { key_out[pos] = k; val_out[pos] = v; }
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (uint32_t w = 0; w < LP_THREADS / 64; w++) add += wcnt[w][threadIdx.x];
    base[threadIdx.x] += add;   // read again only behind the next barrier; wcnt[.][threadIdx.x] is cleared by this thread
  }
}

// one tile of LP_SCAN_TILE elements: out = the scan inside the tile (INCL: inclusive), tile_tot[block] = the tile's total.  in may be out.
template <int OP, bool INCL> __global__ void __launch_bounds__(LP_THREADS) k_lp_scan_tile(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t *tile_tot) {
  __shared__ uint32_t wave_tot[LP_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t e0 = (uint64_t)blockIdx.x * LP_SCAN_TILE + (uint64_t)threadIdx.x * LP_SCAN_ITEMS;
  uint32_t v[LP_SCAN_ITEMS], t = 0;
#pragma unroll
  for (uint32_t k = 0; k < LP_SCAN_ITEMS; k++) { v[k] = e0 + k < n ? in[e0 + k] : 0; t = lp_op<OP>(t, v[k]); }
  uint32_t s = t;   // inclusive over the lanes of the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t x = __shfl_up(s, d); if (lane >= (uint32_t)d) s = lp_op<OP>(s, x); }
  if (lane == 63) wave_tot[wave] = s;
  uint32_t before = __shfl_up(s, 1);
  if (lane == 0) before = 0;
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t w = 0; w < wave; w++) run = lp_op<OP>(run, wave_tot[w]);
  run = lp_op<OP>(run, before);
  if (threadIdx.x == LP_THREADS - 1) tile_tot[blockIdx.x] = lp_op<OP>(run, t);
#pragma unroll
  for (uint32_t k = 0; k < LP_SCAN_ITEMS; k++) {
    const uint32_t incl = lp_op<OP>(run, v[k]);
    if (e0 + k < n) out[e0 + k] = INCL ? incl : run;
    run = incl;
  }
}
// tile_pref: the exclusive scan of the tile totals
template <int OP> __global__ void __launch_bounds__(LP_THREADS) k_lp_scan_fix(uint32_t *out, uint64_t n, const uint32_t *__restrict__ tile_pref) {
  const uint32_t p = tile_pref[blockIdx.x];
  const uint64_t e0 = (uint64_t)blockIdx.x * LP_SCAN_TILE + (uint64_t)threadIdx.x * LP_SCAN_ITEMS;
#pragma unroll
  for (uint32_t k = 0; k < LP_SCAN_ITEMS; k++) if (e0 + k < n) out[e0 + k] = lp_op<OP>(out[e0 + k], p);
}

// sorted[i]: the row that stands for the i-th smallest distinct value.  in_cells / left / heads: its input cells, leftover copies, 1 when it has a run
__global__ void __launch_bounds__(LP_THREADS) k_lp_counts(const uint32_t *__restrict__ sorted, uint32_t n, uint64_t rows, const uint32_t *__restrict__ tcnt, const uint32_t *__restrict__ icnt,
                                                           uint32_t *in_cells, uint32_t *left, uint32_t *heads) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = sorted[i];
    const uint32_t ic = r < rows ? icnt[r] : 0, tc = r < rows ? tcnt[r] : 0;
    in_cells[i] = ic; left[i] = lp_leftover_count(tc, ic); heads[i] = ic ? 1u : 0u;
  }
}
// run_of_row / owner_of_left are zero on entry: value i + 1 at the first row of run i and at its first leftover
__global__ void __launch_bounds__(LP_THREADS) k_lp_mark(uint32_t n, uint64_t rows, const uint32_t *__restrict__ in_cells, const uint32_t *__restrict__ left, const uint32_t *__restrict__ run_start,
                                                         const uint32_t *__restrict__ left_start, uint32_t *run_of_row, uint32_t *owner_of_left) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (in_cells[i] && run_start[i] < rows) run_of_row[run_start[i]] = (uint32_t)i + 1;
    if (left[i] && left_start[i] < rows) owner_of_left[left_start[i]] = (uint32_t)i + 1;
  }
}
// run_of_row / owner_of_left after their inclusive max-scans
__global__ void __launch_bounds__(LP_THREADS) k_lp_expand(const fe_t *__restrict__ table, const uint32_t *__restrict__ sorted, uint64_t rows, uint32_t n, const uint32_t *__restrict__ run_of_row,
                                                           const uint32_t *__restrict__ owner_of_left, const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ heads_before,
                                                           const uint32_t *__restrict__ left_start, const uint32_t *__restrict__ left, fe_t *perm_input, fe_t *perm_table) {
  const uint32_t leftovers = left_start[n - 1] + left[n - 1];
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < rows; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = run_of_row[p] - 1;
    if (i >= n) continue;                                   // cannot happen: row 0 starts a run
    const uint32_t r = sorted[i];
    if (r >= rows) continue;
    const fe_t v = g_load(&table[r]);
    g_store(&perm_input[p], v);
    const uint32_t j = lp_leftover_of_row((uint32_t)p, run_start[i], heads_before[i], leftovers);
    if (j == LP_HEAD) { g_store(&perm_table[p], v); continue; }
    const uint32_t o = j < rows ? owner_of_left[j] - 1 : n;
    if (o >= n || sorted[o] >= rows) continue;              // cannot happen: as many leftovers as repeated rows
    g_store(&perm_table[p], g_load(&table[sorted[o]]));
  }
}

#endif  // __HIPCC__
}  // namespace zk
