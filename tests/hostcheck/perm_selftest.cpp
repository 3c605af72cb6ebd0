// perm_selftest.cpp -- TEST INFRASTRUCTURE: halo2::PermutationAssembly (include/mi355zk_halo2.hpp) compiled with plain g++ and reached through ctypes, so that the
// tests can hold its `mapping` against the Python twin (scroll-prover_amd/halo2.py) and build large mappings quickly.  No device, no library call.  Never shipped.
#include "../../include/mi355zk_halo2.hpp"

// copies: count x 4 u64 (col_a, row_a, col_b, row_b), applied in order.  mapping_out / aux_out / sizes_out: n_cols * n u64 each (any may be null).  1 = done, 0 = a cell outside the permutation
extern "C" int perm_assembly_run(uint32_t n_cols, uint64_t n, const uint64_t *copies, uint64_t count, uint64_t *mapping_out, uint64_t *aux_out, uint64_t *sizes_out) {
  try {
    mi355zk::halo2::PermutationAssembly as(n_cols, n);
    for (uint64_t t = 0; t < count; t++) as.copy((uint32_t)copies[4 * t], copies[4 * t + 1], (uint32_t)copies[4 * t + 2], copies[4 * t + 3]);
    const size_t bytes = as.mapping.size() * 8;
    if (mapping_out) std::memcpy(mapping_out, as.mapping.data(), bytes);
    if (aux_out) std::memcpy(aux_out, as.aux.data(), bytes);
    if (sizes_out) std::memcpy(sizes_out, as.sizes.data(), bytes);
    return 1;
  } catch (const std::exception &) { return 0; }
}
// the override lists of a mapping: cells_out / images_out hold n_cols * n entries in the worst case; returns the count
extern "C" uint64_t perm_assembly_overrides(uint32_t n_cols, uint64_t n, const uint64_t *mapping, uint64_t *cells_out, uint64_t *images_out) {
  mi355zk::halo2::PermutationAssembly as(n_cols, n);
  std::memcpy(as.mapping.data(), mapping, as.mapping.size() * 8);
  std::vector<uint64_t> c, im; as.overrides(c, im);
  std::memcpy(cells_out, c.data(), c.size() * 8); std::memcpy(images_out, im.data(), im.size() * 8);
  return c.size();
}
