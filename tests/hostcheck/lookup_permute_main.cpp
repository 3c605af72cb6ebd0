// lookup_permute_main.cpp -- the per-element bodies of csrc/lookup_permute.hpp (lp_canonical, lp_key_word, lp_digit, lp_pass_needed, lp_leftover_count,
// lp_leftover_of_row, lp_op: the very code the kernels call) run on the CPU.  lph_permute walks the device's pipeline with them, one plain loop per kernel:
// counts per distinct table value, the AND / OR of the canonical keys, the stable 8-bit passes that lp_pass_needed keeps, the three scans, the two max-scans
// and the expansion.  tests/test_lookup_permute_on_host.py loads this file as a shared object and holds the result equal to tests/lookup_permute_common.py;
// with -DLOOKUP_PERMUTE_MAIN it is a stand-alone program that checks the same against std::sort + std::map and is built under AddressSanitizer and UBSan.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>
#include <string>
#include <vector>

#include "../../scroll-prover_amd/csrc/lookup_permute.hpp"

using namespace zk;

namespace {

std::string word_key(const fe_t &v) { return std::string((const char *)v.l, 32); }

template <int OP, bool INCL> void scan(const std::vector<uint32_t> &in, std::vector<uint32_t> &out) {
  uint32_t run = 0;
  for (size_t i = 0; i < in.size(); i++) { const uint32_t incl = lp_op<OP>(run, in[i]); out[i] = INCL ? incl : run; run = incl; }
}

// returns 0, or 1 with *missing = the smallest input row whose value the table lacks
int permute(const fe_t *input, const fe_t *table, uint64_t rows, fe_t *perm_input, fe_t *perm_table, uint64_t *missing, uint32_t *passes_out) {
  *missing = ~0ull; *passes_out = 0;
  if (!rows) return 0;
  // lookup.hpp's part: the first row of every distinct table value, and at that row the table rows and the input cells with the value
  std::unordered_map<std::string, uint32_t> rep;
  std::vector<uint32_t> tcnt(rows, 0), icnt(rows, 0), list;
  for (uint64_t r = 0; r < rows; r++) { auto it = rep.emplace(word_key(table[r]), (uint32_t)r).first; tcnt[it->second]++; }
  for (uint64_t r = 0; r < rows; r++) {
    auto it = rep.find(word_key(input[r]));
    if (it == rep.end()) { *missing = r; return 1; }
    icnt[it->second]++;
  }
  // k_lp_compact
  uint32_t key_and[8], key_or[8];
  for (int k = 0; k < 8; k++) { key_and[k] = 0xffffffffu; key_or[k] = 0; }
  for (uint64_t r = 0; r < rows; r++) {
    if (!tcnt[r]) continue;
    list.push_back((uint32_t)r);
    const fe_t c = lp_canonical(table[r]);
    for (int k = 0; k < 8; k++) { key_and[k] &= c.l[k]; key_or[k] |= c.l[k]; }
  }
  const uint32_t n = (uint32_t)list.size();
  // k_lp_gather + k_lp_hist + scan + k_lp_scatter, pass by pass
  std::vector<uint32_t> key(n), other(n);
  for (uint32_t pass = 0; pass < LP_PASSES; pass++) {
    if (!lp_pass_needed(key_and, key_or, pass)) continue;
    for (uint32_t i = 0; i < n; i++) key[i] = lp_key_word(lp_canonical(table[list[i]]), pass);
    std::vector<uint32_t> hist(256, 0), offs(256);
    for (uint32_t i = 0; i < n; i++) hist[lp_digit(key[i], pass)]++;
    scan<0, false>(hist, offs);
    for (uint32_t i = 0; i < n; i++) other[offs[lp_digit(key[i], pass)]++] = list[i];
    list.swap(other);
    ++*passes_out;
  }
  // k_lp_counts and the three scans
  std::vector<uint32_t> in_cells(n), left(n), heads(n), run_start(n), left_start(n), heads_before(n);
  for (uint32_t i = 0; i < n; i++) { in_cells[i] = icnt[list[i]]; left[i] = lp_leftover_count(tcnt[list[i]], in_cells[i]); heads[i] = in_cells[i] ? 1u : 0u; }
  scan<0, false>(in_cells, run_start); scan<0, false>(left, left_start); scan<0, false>(heads, heads_before);
  // k_lp_mark and the two max-scans
  std::vector<uint32_t> run_of_row(rows, 0), owner_of_left(rows, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (in_cells[i]) run_of_row.at(run_start[i]) = i + 1;
    if (left[i]) owner_of_left.at(left_start[i]) = i + 1;
  }
  scan<1, true>(run_of_row, run_of_row); scan<1, true>(owner_of_left, owner_of_left);
  // k_lp_expand
  const uint32_t leftovers = left_start[n - 1] + left[n - 1];
  for (uint64_t p = 0; p < rows; p++) {
    const uint32_t i = run_of_row[p] - 1;
    const fe_t v = table[list.at(i)];
    perm_input[p] = v;
    const uint32_t j = lp_leftover_of_row((uint32_t)p, run_start[i], heads_before[i], leftovers);
    perm_table[p] = j == LP_HEAD ? v : table[list.at(owner_of_left.at(j) - 1)];
  }
  return 0;
}

}  // namespace

extern "C" {
int lph_permute(const void *input, const void *table, uint64_t rows, void *perm_input, void *perm_table, uint64_t *missing, uint32_t *passes) {
  return permute((const fe_t *)input, (const fe_t *)table, rows, (fe_t *)perm_input, (fe_t *)perm_table, missing, passes);
}
void lph_canonical(const void *words, uint64_t n, void *out) { for (uint64_t i = 0; i < n; i++) ((fe_t *)out)[i] = lp_canonical(((const fe_t *)words)[i]); }
int lph_pass_needed(const uint32_t *key_and, const uint32_t *key_or, uint32_t pass) { return lp_pass_needed(key_and, key_or, pass) ? 1 : 0; }
uint32_t lph_digit(uint32_t word, uint32_t pass) { return lp_digit(word, pass); }
uint32_t lph_leftover_of_row(uint32_t p, uint32_t start, uint32_t heads_before, uint32_t leftovers) { return lp_leftover_of_row(p, start, heads_before, leftovers); }
}

#ifdef LOOKUP_PERMUTE_MAIN
namespace {

using Int = std::array<uint32_t, 8>;   // a canonical integer, limb 7 the most significant
struct IntLess { bool operator()(const Int &a, const Int &b) const { for (int k = 7; k >= 0; k--) if (a[k] != b[k]) return a[k] < b[k]; return false; } };

uint64_t g_state = 0x5eed5eed5eedull;
uint64_t next64() { uint64_t z = (g_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
Int small(uint64_t v) { Int x{}; x[0] = (uint32_t)v; x[1] = (uint32_t)(v >> 32); return x; }
Int random_int() { Int x; for (int k = 0; k < 8; k++) x[k] = (uint32_t)next64(); x[7] &= 0x0fffffffu; return x; }   // below 2^252 < r
Int bit(int b) { Int x{}; x[b >> 5] = 1u << (b & 31); return x; }
Int r_minus(uint32_t d) { Int x; for (int k = 0; k < 8; k++) x[k] = FrP::mod(k); x[0] -= d; return x; }
fe_t mont(const Int &x) { fe_t c; for (int k = 0; k < 8; k++) c.l[k] = x[k]; return Fr::from_canonical(c); }
Int canon(const fe_t &w) { const fe_t c = Fr::to_canonical(w); Int x; for (int k = 0; k < 8; k++) x[k] = c.l[k]; return x; }   // by the full product, not by lp_canonical

// the rule restated: std::sort + std::map
bool restate(const std::vector<Int> &in, const std::vector<Int> &tab, std::vector<Int> &a, std::vector<Int> &s, uint64_t &missing) {
  std::map<Int, uint32_t, IntLess> leftover;
  for (const Int &v : tab) leftover[v]++;
  for (size_t r = 0; r < in.size(); r++) if (!leftover.count(in[r])) { missing = r; return false; }
  a = in; std::sort(a.begin(), a.end(), IntLess());
  s.assign(a.size(), Int{});
  std::vector<size_t> repeated;
  for (size_t i = 0; i < a.size(); i++) {
    if (i == 0 || a[i] != a[i - 1]) { s[i] = a[i]; leftover[a[i]]--; } else repeated.push_back(i);
  }
  for (const auto &kv : leftover) for (uint32_t c = 0; c < kv.second; c++) { s[repeated.back()] = kv.first; repeated.pop_back(); }
  return repeated.empty();
}

int g_fail = 0;
void expect(bool ok, const char *what, uint64_t rows) { if (!ok) { printf("FAIL %s rows=%llu\n", what, (unsigned long long)rows); g_fail++; } }

void run_case(const char *name, const std::vector<Int> &in, const std::vector<Int> &tab, int want_passes = -1) {
  const uint64_t rows = in.size();
  std::vector<fe_t> iw(rows), tw(rows), pa(rows + 1), ps(rows + 1);
  for (uint64_t r = 0; r < rows; r++) { iw[r] = mont(in[r]); tw[r] = mont(tab[r]); }
  const fe_t guard = mont(small(0xabcdef));
  pa[rows] = guard; ps[rows] = guard;
  uint64_t missing = 0, want_missing = ~0ull; uint32_t passes = 0;
  std::vector<Int> a, s;
  const bool valid = restate(in, tab, a, s, want_missing);
  const int rc = permute(iw.data(), tw.data(), rows, pa.data(), ps.data(), &missing, &passes);
  expect(rc == (valid ? 0 : 1) && missing == want_missing, name, rows);
  expect(lk_eq(pa[rows], guard) && lk_eq(ps[rows], guard), name, rows);
  if (valid) for (uint64_t p = 0; p < rows; p++) if (canon(pa[p]) != a[p] || canon(ps[p]) != s[p] || !lk_eq(pa[p], mont(a[p]))) { expect(false, name, rows); break; }
  if (want_passes >= 0) expect((int)passes == want_passes, "pass count", rows);
}

}  // namespace

int main() {
  const uint64_t sizes[] = {1, 2, 63, 64, 65, 257, 4099, 65539};
  for (uint64_t rows : sizes) {
    std::vector<Int> in(rows), tab(rows);
    // a range table with a zero tail
    uint32_t bits = 1; while ((2ull << bits) <= rows) bits++;
    for (uint64_t r = 0; r < rows; r++) tab[r] = small(r < (1ull << bits) ? r : 0);
    for (uint64_t r = 0; r < rows; r++) in[r] = tab[next64() % rows];
    run_case("range_zero_tail", in, tab, rows == 1 ? 0 : (int)((bits + 7) / 8));   // the values 0 .. 2^bits - 1 differ in their low `bits` bits only
    // all inputs equal
    for (uint64_t r = 0; r < rows; r++) tab[r] = small(7 * r + 3);
    for (uint64_t r = 0; r < rows; r++) in[r] = tab[rows / 2];
    run_case("all_equal", in, tab);
    // a shuffle of distinct random values
    for (uint64_t r = 0; r < rows; r++) { tab[r] = random_int(); in[r] = tab[r]; }
    for (uint64_t r = rows - 1; r > 0; r--) std::swap(in[r], in[next64() % (r + 1)]);
    run_case("shuffle", in, tab);
    // duplicated table values, not adjacent
    const uint64_t d = std::max<uint64_t>(1, rows / 5);
    for (uint64_t r = 0; r < rows; r++) tab[r] = tab[r % d];
    for (uint64_t r = 0; r < rows; r++) in[r] = tab[next64() % std::max<uint64_t>(1, d / 2)];
    run_case("duplicated_table", in, tab);
    // Montgomery order against canonical order
    Int lo = random_int(), hi = lo, lo2 = lo; lo2[0] ^= 1; hi[7] ^= 1;
    const Int pool[] = {small(0), small(1), r_minus(1), r_minus(2), bit(64), bit(128), bit(192), lo, lo2, hi, bit(253), bit(32), bit(224)};
    for (uint64_t r = 0; r < rows; r++) tab[r] = pool[r % (sizeof pool / sizeof pool[0])];
    for (uint64_t r = 0; r < rows; r++) in[r] = tab[next64() % rows];
    run_case("montgomery_order", in, tab);
    // a long run between short ones
    for (uint64_t r = 0; r < rows; r++) tab[r] = small(r + 1);
    for (uint64_t r = 0; r < rows; r++) in[r] = small(r < rows / 8 ? r + 1 : r < rows - rows / 8 ? rows / 8 + 1 : r + 1);
    for (uint64_t r = rows - 1; r > 0; r--) std::swap(in[r], in[next64() % (r + 1)]);
    run_case("straddling_run", in, tab);
    // keys that differ in one digit only
    Int base = random_int(); base[3] &= ~0xff00u;
    for (uint64_t r = 0; r < rows; r++) { tab[r] = base; tab[r][3] |= (uint32_t)(r % 256) << 8; }
    for (uint64_t r = 0; r < rows; r++) in[r] = tab[next64() % rows];
    run_case("one_digit", in, tab, rows == 1 ? 0 : 1);
    // a missing value at the first, a middle and the last row
    const uint64_t where[] = {0, rows / 2, rows - 1};
    for (uint64_t w : where) { std::vector<Int> bad = in; bad[w] = bit(200); run_case("missing", bad, tab); }
  }
  // the bodies on their own
  uint32_t a[8], o[8];
  for (int k = 0; k < 8; k++) { a[k] = 0x12345678u; o[k] = 0x12345678u; }
  o[2] |= 0x00800000u; a[2] &= ~0x00800000u;
  for (uint32_t pass = 0; pass < LP_PASSES; pass++) expect(lp_pass_needed(a, o, pass) == (pass == 10), "lp_pass_needed", pass);
  expect(lp_digit(0xa1b2c3d4u, 0) == 0xd4 && lp_digit(0xa1b2c3d4u, 7) == 0xa1 && lp_digit(0xa1b2c3d4u, 30) == 0xb2, "lp_digit", 0);
  expect(lp_leftover_of_row(5, 5, 2, 9) == LP_HEAD && lp_leftover_of_row(6, 5, 2, 9) == 9 - 1 - 3 && lp_leftover_count(4, 0) == 4 && lp_leftover_count(4, 9) == 3, "lp_leftover", 0);
  printf(g_fail ? "%d FAILED\n" : "all passed\n", g_fail);
  return g_fail ? 1 : 0;
}
#endif
