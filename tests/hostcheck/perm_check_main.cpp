// perm_check_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around perm_check (scroll-prover_amd/csrc/perm.hpp), the host validation that
// mi355_fr_permutation_sigma_dev runs before anything is uploaded or launched.  tests/test_permutation_check_on_host.py builds it with
// -fsanitize=address,undefined and runs it; every case prints one line "name verdict index" and the exit code is the number of cases that went wrong.  Never shipped.
#include <cstdio>
#include <numeric>

#include "../../scroll-prover_amd/csrc/perm.hpp"

using zk::perm_check;
using List = std::vector<uint64_t>;
static int g_wrong = 0;

// want_bad < 0: must be accepted; otherwise rejected with exactly this first index
static void expect(const char *name, const List &cells, const List &images, uint64_t total, uint32_t flags, long want_bad) {
  uint64_t bad = ~0ull; std::string why;
  const int rc = perm_check(cells.data(), images.data(), cells.size(), total, flags, &bad, &why);
  const bool ok = want_bad < 0 ? rc == 0 : (rc != 0 && bad == (uint64_t)want_bad && !why.empty());
  std::printf("%s %s %ld%s%s\n", name, rc ? "rejected" : "accepted", rc ? (long)bad : -1L, rc ? " " : "", why.c_str());
  if (!ok) { std::printf("  WRONG: wanted %s %ld\n", want_bad < 0 ? "accepted" : "rejected", want_bad); g_wrong++; }
}

int main() {
  const uint64_t n_cols = 3, n = 64, total = n_cols * n;
  for (uint32_t flags : {0u, 1u}) {
    std::printf("flags %u\n", flags);
    expect("empty", {}, {}, total, flags, -1);
    { uint64_t bad; std::string why; if (perm_check(nullptr, nullptr, 0, total, flags, &bad, &why)) { std::printf("  WRONG: null lists of length 0\n"); g_wrong++; } }
    { List c(total), im(total); std::iota(c.begin(), c.end(), 0); for (uint64_t i = 0; i < total; i++) im[i] = (i + 5) % total; expect("dense", c, im, total, flags, -1); }
    expect("two_cycle", {7, 130}, {130, 7}, total, flags, -1);
    { List c, im; for (uint64_t i = 0; i < 17; i++) { c.push_back(11 * i + 3); im.push_back(11 * ((i + 1) % 17) + 3); } expect("seventeen_cycle", c, im, total, flags, -1); }
    // the range check always runs
    expect("cell_equal_to_total", {5, total, 9}, {9, 5, total}, total, flags, 1);
    expect("image_all_ones", {5, 9, 12}, {9, 5, ~0ull}, total, flags, 2);
    // duplicates and the bijection: flags bit 0 waives them
    expect("cell_twice", {5, 9, 5}, {9, 5, 9}, total, flags, flags ? -1 : 2);
    expect("images_not_the_cells", {5, 9, 12}, {9, 5, 13}, total, flags, flags ? -1 : 2);
    expect("image_twice", {5, 9, 12}, {9, 9, 5}, total, flags, flags ? -1 : 1);
    expect("last_cell", {total - 1, 0}, {0, total - 1}, total, flags, -1);
  }
  // one cell, one column of one row: the smallest permutation there is
  expect("single_fixed_point", {0}, {0}, 1, 0, -1);
  expect("single_out_of_range", {1}, {0}, 1, 0, 0);
  std::printf("wrong %d\n", g_wrong);
  return g_wrong;
}
