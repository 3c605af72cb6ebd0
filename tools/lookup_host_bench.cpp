// lookup_host_bench.cpp -- the host restatement that tools/bench_lookup_multiplicities.py times the device call against: what a caller of create_proof would run per
// lookup if the library did not count the multiplicities [EXT-recalled halo2_proofs src/plonk/mv_lookup/prover.rs, `prepare`]: a hash map from each table value (32-byte
// word) to its first row, built by one thread, then every input cell looked up by T threads, counts by relaxed atomic adds.  Written here from scratch, host only.
//   lookup_host_bench K CASE THREADS   CASE: range | tuple | zero | mostly_zero.  Prints one JSON line: build_ms, probe_ms, total_ms.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

struct W { uint64_t w[4]; bool operator==(const W &o) const { return std::memcmp(w, o.w, 32) == 0; } };
static uint64_t mix(uint64_t z) { z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint64_t hash_w(const W &v) { return mix(v.w[0] ^ mix(v.w[1] ^ mix(v.w[2] ^ mix(v.w[3])))); }
static W word_of(uint64_t id) { if (!id) return W{{0, 0, 0, 0}}; W v; for (int i = 0; i < 4; i++) v.w[i] = mix(id * 4 + i + 0x1234567); v.w[3] &= (1ull << 60) - 1; return v; }

int main(int argc, char **argv) {
  if (argc < 4) { std::printf("usage: %s K range|tuple|zero|mostly_zero THREADS\n", argv[0]); return 1; }
  const uint32_t k = (uint32_t)std::atoi(argv[1]); const std::string cs = argv[2]; const int T = std::max(1, std::atoi(argv[3]));
  const uint64_t n = 1ull << k, u = n - 10, bits = k - 1, tr = std::min<uint64_t>(1ull << bits, u);
  std::vector<W> table(n), input(n);
  { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back([&, t]() {
      for (uint64_t r = n * t / T; r < n * (t + 1) / T; r++) {
        const uint64_t tid = r < tr ? (cs == "tuple" ? r * 7 + 1 : r) : 0;                           // range: value r (row 0 = 0), zero tail; tuple: distinct words
        table[r] = word_of(tid);
        const uint64_t h = mix(r + 99);
        const uint64_t row = cs == "zero" ? 0 : (cs == "mostly_zero" && h % 10 != 0) ? 0 : h % tr;
        input[r] = word_of(row < tr ? (cs == "tuple" ? row * 7 + 1 : row) : 0);
        if (cs == "tuple" && row == 0) input[r] = table[0];
      } }); for (auto &x : th) x.join(); }
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t S = 64; while (S < 2 * u) S <<= 1; const uint64_t mask = S - 1;
  std::vector<uint32_t> slot(S, 0xffffffffu);
  for (uint64_t r = 0; r < u; r++) {   // first occurrence: a value already present keeps its row
    uint64_t h = hash_w(table[r]) & mask;
    while (slot[h] != 0xffffffffu && !(table[slot[h]] == table[r])) h = (h + 1) & mask;
    if (slot[h] == 0xffffffffu) slot[h] = (uint32_t)r;
  }
  const auto t1 = std::chrono::steady_clock::now();
  std::vector<std::atomic<uint32_t>> cnt(n); for (auto &c : cnt) c.store(0, std::memory_order_relaxed);
  std::atomic<uint64_t> missing{0};
  { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back([&, t]() {
      for (uint64_t r = u * t / T; r < u * (t + 1) / T; r++) {
        uint64_t h = hash_w(input[r]) & mask;
        while (slot[h] != 0xffffffffu && !(table[slot[h]] == input[r])) h = (h + 1) & mask;
        if (slot[h] == 0xffffffffu) missing++; else cnt[slot[h]].fetch_add(1, std::memory_order_relaxed);
      } }); for (auto &x : th) x.join(); }
  const auto t2 = std::chrono::steady_clock::now();
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  uint64_t total = 0; for (auto &c : cnt) total += c.load();
  std::printf("{\"k\": %u, \"case\": \"%s\", \"threads\": %d, \"build_ms\": %.2f, \"probe_ms\": %.2f, \"total_ms\": %.2f, \"counted\": %llu, \"missing\": %llu}\n",
              k, cs.c_str(), T, ms(t0, t1), ms(t1, t2), ms(t0, t2), (unsigned long long)total, (unsigned long long)missing.load());
  return 0;
}
