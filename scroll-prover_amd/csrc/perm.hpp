// perm.hpp -- the sigma columns of the permutation argument, built on the device from the copy-constraint mapping
// [EXT-recalled halo2_proofs src/plonk/permutation/keygen.rs, Assembly::build_pk / build_vk: permutations[i][j] = delta^i' omega^j' for
// mapping[i][j] = (i', j'), every column and row, from a num_cols x n table of delta^i omega^j built on the CPU].
//
// A cell is the integer column * n + row (column = position in the permutation, n = 2^log_n).  The output is the identity permutation
// sigma[j][r] = delta^j omega^r with the cells of `cells` overridden by the value of their image in `images`: only the constrained cells cross the
// link, 16 bytes each, instead of 32 bytes for every cell of every column.
//
//   perm_check          host: the mapping is a permutation of the listed cells (range, duplicates, image set = cell set) before anything is uploaded or
//                       launched -- a cell >= n_cols * n would be a store outside the columns.  Plain C++, compiled by tests without a device.
//   k_perm_identity     thread = row r: omega^r from two small tables (r split high / low: one multiplication), then a tile of PERM_COL_TILE columns
//                       (blockIdx.y) starting at omega^r delta^j0 with one multiplication by delta per column.  Consecutive lanes store consecutive
//                       32-byte words of one column.  No table of n entries is read: the two tables hold 2^ceil(log_n / 2) and 2^floor(log_n / 2) words.
//   k_perm_override     thread = override t: the same two table reads for the image's row, the product with delta^j' (table of n_cols words), one
//                       32-byte store to the cell.  Reads the tables and the lists only, so it may run behind the identity pass in any order of t.
// Arithmetic: FrPs::mul on Montgomery words (fp_asm.hpp); its output is fully reduced, as the ABI requires of words that are compared as bytes.
// Plain vector stores; no LDS, no atomics.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace zk {

constexpr uint32_t PERM_FLAG_TRUSTED = 1;   // skip the duplicate and bijection checks (the range check always runs)
constexpr uint32_t PERM_MAX_LOG_N = 28;

// 0: accepted.  Otherwise *bad_t = the first offending index t and *why a phrase for the error text.  total = n_cols * n cells.
// The order of the checks per t is: cell range, image range, cell listed twice; then the first t whose image is no listed cell.
inline int perm_check(const uint64_t *cells, const uint64_t *images, uint64_t count, uint64_t total, uint32_t flags, uint64_t *bad_t, std::string *why) {
  for (uint64_t t = 0; t < count; t++) {
    if (cells[t] >= total) { *bad_t = t; *why = "cell " + std::to_string(cells[t]) + " is not below n_cols * n"; return 1; }
    if (images[t] >= total) { *bad_t = t; *why = "image " + std::to_string(images[t]) + " is not below n_cols * n"; return 1; }
  }
  if ((flags & PERM_FLAG_TRUSTED) || count == 0) return 0;
  std::vector<uint64_t> seen((total + 63) / 64, 0);   // one bit per cell: listed as a cell
  for (uint64_t t = 0; t < count; t++) {
    uint64_t &w = seen[cells[t] >> 6]; const uint64_t b = 1ull << (cells[t] & 63);
    if (w & b) { *bad_t = t; *why = "cell " + std::to_string(cells[t]) + " is listed twice"; return 1; }
    w |= b;
  }
  // count images, all of them listed cells and no two equal, are exactly the count cells
  std::vector<uint64_t> hit((total + 63) / 64, 0);
  for (uint64_t t = 0; t < count; t++) {
    const uint64_t i = images[t] >> 6, b = 1ull << (images[t] & 63);
    if (!(seen[i] & b)) { *bad_t = t; *why = "image " + std::to_string(images[t]) + " is not one of the listed cells"; return 1; }
    if (hit[i] & b) { *bad_t = t; *why = "image " + std::to_string(images[t]) + " is the image of two cells"; return 1; }
    hit[i] |= b;
  }
  return 0;
}

// the split of a row index: low = r & (2^lo_bits - 1) indexes omega^i, high = r >> lo_bits indexes omega^(i 2^lo_bits)
inline uint32_t perm_lo_bits(uint32_t log_n) { return (log_n + 1) / 2; }

}  // namespace zk

#ifdef __HIPCC__
#include "fp_asm.hpp"

namespace zk {

constexpr uint32_t PERM_THREADS = 256, PERM_COL_TILE = 16;

// tables: tw_lo[2^lo_bits] = omega^i, tw_hi[2^(log_n - lo_bits)] = omega^(i 2^lo_bits), dpow[n_cols] = delta^j (Montgomery words)
struct PermTables { const fe_t *tw_lo, *tw_hi, *dpow; uint32_t lo_bits; };

__device__ __forceinline__ fe_t perm_omega_pow(const PermTables &T, uint64_t r) {
  return FrPs::mul(g_load(&T.tw_lo[r & ((1ull << T.lo_bits) - 1)]), g_load(&T.tw_hi[r >> T.lo_bits]));
}

__global__ void __launch_bounds__(PERM_THREADS) k_perm_identity(fe_t *const *__restrict__ cols, uint32_t n_cols, uint32_t log_n, PermTables T, fe_t delta) {
  const uint64_t n = 1ull << log_n, r = (uint64_t)blockIdx.x * PERM_THREADS + threadIdx.x;
  if (r >= n) return;
  const uint32_t j0 = blockIdx.y * PERM_COL_TILE, j1 = j0 + PERM_COL_TILE < n_cols ? j0 + PERM_COL_TILE : n_cols;
  fe_t v = perm_omega_pow(T, r);
  if (j0) v = FrPs::mul(v, g_load(&T.dpow[j0]));
  for (uint32_t j = j0; j < j1; j++) {
    g_store(&cols[j][r], v);
    if (j + 1 < j1) v = FrPs::mul(v, delta);
  }
}

__global__ void __launch_bounds__(PERM_THREADS) k_perm_override(fe_t *const *__restrict__ cols, uint32_t log_n, PermTables T, const uint64_t *__restrict__ cells,
                                                                const uint64_t *__restrict__ images, uint64_t count) {
  const uint64_t mask = (1ull << log_n) - 1;
  for (uint64_t t = (uint64_t)blockIdx.x * PERM_THREADS + threadIdx.x; t < count; t += (uint64_t)gridDim.x * PERM_THREADS) {
    const uint64_t c = cells[t], im = images[t];   // both < n_cols * n: perm_check ran on the host before the lists were uploaded
    const fe_t v = FrPs::mul(perm_omega_pow(T, im & mask), g_load(&T.dpow[im >> log_n]));
    g_store(&cols[c >> log_n][c & mask], v);
  }
}

}  // namespace zk
#endif  // __HIPCC__
