// g1_codec_host_bench.cpp -- the host route the device codec replaces: g1_from_bytes / g1_to_bytes of include/mi355zk_halo2.hpp (8 x 32-bit CIOS field, square-and-multiply
// square root) over T threads.  Reads n compressed words from a file written by tools/bench_g1_codec.py, prints one JSON line.  usage: g1_codec_host_bench WORDS_FILE n [threads = 16]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mi355zk_halo2.hpp"

using namespace mi355zk::halo2;
using Clock = std::chrono::steady_clock;

int main(int argc, char **argv) {
  if (argc < 3) { std::printf("usage: %s WORDS_FILE n [threads]\n", argv[0]); return 1; }
  const uint64_t n = std::strtoull(argv[2], nullptr, 10); const int T = argc > 3 ? std::max(1, std::atoi(argv[3])) : 16;
  std::vector<G1Bytes> words(n); std::vector<G1Affine> pts(n); std::vector<G1Bytes> back(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(words.data(), 32, n, f) != n) { std::printf("cannot read %llu words from %s\n", (unsigned long long)n, argv[1]); return 1; }
  std::fclose(f);
  std::vector<int> bad(T, 0);
  auto run = [&](auto body) {
    const auto t0 = Clock::now();
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&, t]() { for (uint64_t i = n * t / T; i < n * (t + 1) / T; i++) body(i, t); });
    for (auto &x : th) x.join();
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
  };
  const double dec = run([&](uint64_t i, int t) { if (!g1_from_bytes(words[i], pts[i])) bad[t]++; });
  const double enc = run([&](uint64_t i, int) { back[i] = g1_to_bytes(pts[i]); });
  int nbad = 0; for (int b : bad) nbad += b;
  std::printf("{\"n\": %llu, \"threads\": %d, \"host_decompress_ms\": %.1f, \"host_compress_ms\": %.1f, \"rejected\": %d, \"round_trip\": %s}\n",
              (unsigned long long)n, T, dec, enc, nbad, back == words ? "true" : "false");
  return back == words && nbad == 0 ? 0 : 1;
}
