// lookup_permute_host_bench.cpp -- the host restatement that tools/bench_classic_lookup.py times mi355_fr_lookup_permute_dev against: what halo2 runs per lookup
// on the CPU [EXT-recalled halo2_proofs src/plonk/lookup/prover.rs, `permute_expression_pair`]: the input sorted by canonical value (here a parallel sort: T sorted
// runs merged pairwise), an ordered map of the table's values with their counts, the run heads taken out of it, the leftovers popped into the repeated rows from the
// back.  Values are canonical 256-bit integers (the conversion from Montgomery form is not timed).  Written here from scratch, host only.
//   lookup_permute_host_bench K CASE THREADS   CASE: range | tuple | zero.  Prints one JSON line: sort_ms, map_ms, place_ms, total_ms.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

struct W { uint64_t w[4]; };
static bool less_w(const W &a, const W &b) { for (int i = 3; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i]; return false; }
static bool eq_w(const W &a, const W &b) { return std::memcmp(a.w, b.w, 32) == 0; }
struct LessW { bool operator()(const W &a, const W &b) const { return less_w(a, b); } };
static uint64_t mix(uint64_t z) { z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static W small(uint64_t v) { return W{{v, 0, 0, 0}}; }
static W wide(uint64_t id) { if (!id) return small(0); W v; for (int i = 0; i < 4; i++) v.w[i] = mix(id * 4 + i + 0x1234567); v.w[3] &= (1ull << 60) - 1; return v; }

int main(int argc, char **argv) {
  if (argc < 4) { std::printf("usage: %s K range|tuple|zero THREADS\n", argv[0]); return 1; }
  const uint32_t k = (uint32_t)std::atoi(argv[1]); const std::string cs = argv[2]; const int T = std::max(1, std::atoi(argv[3]));
  const uint64_t n = 1ull << k, u = n - 7, tr = std::min<uint64_t>(1ull << (k - 1), u);
  std::vector<W> table(u), input(u);
  { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back([&, t]() {
      for (uint64_t r = u * t / T; r < u * (t + 1) / T; r++) {
        table[r] = r < tr ? (cs == "tuple" ? wide(r * 7 + 1) : small(r)) : small(0);
        const uint64_t row = cs == "zero" ? 0 : mix(r + 99) % tr;
        input[r] = cs == "tuple" ? (row ? wide(row * 7 + 1) : table[0]) : small(row);
      } }); for (auto &x : th) x.join(); }
  const auto t0 = std::chrono::steady_clock::now();
  // A': T sorted runs, then pairwise merges, each level on its own threads
  std::vector<W> a = input;
  { std::vector<uint64_t> cut(T + 1); for (int t = 0; t <= T; t++) cut[t] = u * t / T;
    { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back([&, t]() { std::sort(a.begin() + (long)cut[t], a.begin() + (long)cut[t + 1], less_w); }); for (auto &x : th) x.join(); }
    for (int step = 1; step < T; step *= 2) {
      std::vector<std::thread> th;
      for (int t = 0; t + step < T; t += 2 * step) th.emplace_back([&, t, step]() { std::inplace_merge(a.begin() + (long)cut[t], a.begin() + (long)cut[t + step], a.begin() + (long)cut[std::min(T, t + 2 * step)], less_w); });
      for (auto &x : th) x.join();
    } }
  const auto t1 = std::chrono::steady_clock::now();
  std::map<W, uint32_t, LessW> leftover;
  for (uint64_t r = 0; r < u; r++) leftover[table[r]]++;
  const auto t2 = std::chrono::steady_clock::now();
  std::vector<W> s(u); std::vector<uint64_t> repeated; uint64_t missing = 0;
  for (uint64_t i = 0; i < u; i++) {
    if (i == 0 || !eq_w(a[i], a[i - 1])) { s[i] = a[i]; auto it = leftover.find(a[i]); if (it == leftover.end() || !it->second) missing++; else it->second--; }
    else repeated.push_back(i);
  }
  for (const auto &kv : leftover) for (uint32_t c = 0; c < kv.second && !repeated.empty(); c++) { s[repeated.back()] = kv.first; repeated.pop_back(); }
  const auto t3 = std::chrono::steady_clock::now();
  auto ms = [](auto x, auto y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
  uint64_t fold = 0; for (uint64_t i = 0; i < u; i += 4097) fold ^= s[i].w[0] ^ a[i].w[1];
  std::printf("{\"k\": %u, \"case\": \"%s\", \"threads\": %d, \"sort_ms\": %.2f, \"map_ms\": %.2f, \"place_ms\": %.2f, \"total_ms\": %.2f, \"missing\": %llu, \"unplaced\": %zu, \"fold\": %llu}\n",
              k, cs.c_str(), T, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t0, t3), (unsigned long long)missing, repeated.size(), (unsigned long long)fold);
  return 0;
}
