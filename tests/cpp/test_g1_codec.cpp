// test_g1_codec.cpp -- a COMPILED caller of the compressed-point codec and of the SerdeFormat::Processed params route (include/mi355zk_halo2.hpp:
// ParamsKZG::write_custom / read_custom, the batch g1_to_bytes / g1_from_bytes).  Links no oracle code: everything is compared with the library's own RawBytes
// route, which the Python tests hold to the oracle.
//
//   synthetic SRS on the device (mi355_srs_setup_dev) -> ParamsKZG -> write_custom(Processed) and write_custom(RawBytes) -> read_custom of both ->
//   the points of both (mi355_srs_read_host) byte for byte, g2 / s_g2, one commitment on each basis; batch codec round trip; a corrupted word is refused.
//
// usage: test_g1_codec [k = 14] [directory for the two files = /tmp].  Prints one JSON line with the timings; exit 0 = all equal, 1 = a mismatch, 2 = no GPU.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unistd.h>

#include "mi355zk_halo2.hpp"

using namespace mi355zk::halo2;
using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// halo2curves' G2 generator (the public BN254 twist generator: x.c0, x.c1, y.c0, y.c1, canonical 32-bit words, little-endian)
static std::array<uint8_t, 128> g2_generator() {
  static const uint32_t c[4][8] = {
      {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
      {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
      {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
      {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};
  std::array<uint8_t, 128> out{};
  for (int i = 0; i < 4; i++) { zk::fe_t v; for (int j = 0; j < 8; j++) v.l[j] = c[i][j]; v = zk::Fq::from_canonical(v); std::memcpy(out.data() + 32 * i, &v, 32); }
  return out;
}

int main(int argc, char **argv) {
  const uint32_t k = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 14;
  const std::string dir = argc > 2 ? argv[2] : "/tmp";
  if (k < 4 || k > 26) { std::printf("k must be in 4..26\n"); return 1; }
  if (mi355_init(0) != MI355_OK) { std::printf("mi355_init failed: %s\n", mi355_last_error()); return 2; }
  const uint64_t n = uint64_t(1) << k;
  const std::string raw = dir + "/mi355_g1_codec_" + std::to_string((long)getpid()) + ".raw", proc = dir + "/mi355_g1_codec_" + std::to_string((long)getpid()) + ".processed";
  int rc_main = 1;
  try {
    const Fr tau = detail::fr_from_u64(0x5343524F4C4C0C0Dull);
    Fr omega = detail::root_of_unity();
    for (uint32_t i = k; i < FR_S; i++) omega = detail::fr_mul(omega, omega);
    std::vector<G1Affine> g(n), gl(n);
    {
      DevicePoly dg(2 * n), dl(2 * n);   // 64 bytes per point
      check(mi355_srs_setup_dev(dg.p, dl.p, k, tau.data(), omega.data()));
      check(mi355_buf_download(g.data(), dg.p, n * 64)); check(mi355_buf_download(gl.data(), dl.p, n * 64));
    }
    ParamsKZG src(k, g, gl);
    src.g2 = g2_generator();
    check(mi355_g2_mul_host(src.g2.data(), tau.data(), src.s_g2.data()));
    auto t0 = Clock::now();
    src.write_custom(raw, SerdeFormat::RawBytes);
    const double write_raw_ms = ms_since(t0);
    t0 = Clock::now();
    src.write_custom(proc, SerdeFormat::Processed);
    const double write_processed_ms = ms_since(t0);
    t0 = Clock::now();
    auto a = ParamsKZG::read_custom(raw, SerdeFormat::RawBytes, true);
    const double load_raw_ms = ms_since(t0);
    t0 = Clock::now();
    auto b = ParamsKZG::read_custom(proc, SerdeFormat::Processed);
    const double load_processed_ms = ms_since(t0);
    bool ok = a->k == k && b->k == k;
    ok = ok && a->get_g() == g && b->get_g() == g && a->get_g_lagrange() == gl && b->get_g_lagrange() == gl;
    ok = ok && b->g2 == src.g2 && b->s_g2 == src.s_g2 && a->g2 == src.g2 && a->s_g2 == src.s_g2;
    std::vector<Fr> poly(n);
    for (uint64_t i = 0; i < n; i++) poly[i] = detail::fr_from_u64(i * 0x9E3779B97F4A7C15ull + 12345);
    ok = ok && a->commit(poly) == b->commit(poly) && a->commit_lagrange(poly) == b->commit_lagrange(poly) && b->commit(poly) == src.commit(poly);
    // the batch codec on host vectors, and the single-point host helpers on a sample
    t0 = Clock::now();
    const std::vector<G1Bytes> words = g1_to_bytes(gl);
    const double compress_ms = ms_since(t0);
    t0 = Clock::now();
    const std::vector<G1Affine> back = g1_from_bytes(words);
    const double decompress_ms = ms_since(t0);
    ok = ok && back == gl;
    for (uint64_t i = 0; i < n; i += std::max<uint64_t>(1, n / 64)) { G1Affine p; ok = ok && g1_to_bytes(gl[i]) == words[i] && g1_from_bytes(words[i], p) && p == gl[i]; }
    // a word that is no point: refused with its index, by the codec and by the loader
    bool refused = false, refused_file = false;
    {
      std::vector<G1Bytes> bad = words; G1Affine p;
      const uint64_t at = n / 2 + 1;
      for (int d = 1; d < 256 && g1_from_bytes(bad[at], p); d++) bad[at][0] = (uint8_t)(words[at][0] + d);
      try { (void)g1_from_bytes(bad); } catch (const Error &e) { refused = e.code == MI355_EBADARG && std::string(e.what()).find("word " + std::to_string(at)) != std::string::npos; }
      FILE *f = std::fopen(proc.c_str(), "r+b");
      if (f) { std::fseek(f, (long)(4 + 32 * at), SEEK_SET); std::fwrite(bad[at].data(), 1, 32, f); std::fclose(f); }
      try { (void)ParamsKZG::read_custom(proc, SerdeFormat::Processed); } catch (const Error &e) { refused_file = e.code == MI355_EBADARG && std::string(e.what()).find("g[" + std::to_string(at) + "]") != std::string::npos; }
    }
    ok = ok && refused && refused_file;
    std::printf("{\"ok\": %s, \"k\": %u, \"write_raw_ms\": %.3f, \"write_processed_ms\": %.3f, \"load_raw_ms\": %.3f, \"load_processed_ms\": %.3f, \"compress_host_ms\": %.3f, \"decompress_host_ms\": %.3f, "
                "\"refused_word\": %s, \"refused_file\": %s}\n",
                ok ? "true" : "false", k, write_raw_ms, write_processed_ms, load_raw_ms, load_processed_ms, compress_ms, decompress_ms, refused ? "true" : "false", refused_file ? "true" : "false");
    rc_main = ok ? 0 : 1;
  } catch (const std::exception &e) {
    std::printf("{\"ok\": false, \"error\": \"%s\"}\n", e.what());
  }
  std::remove(raw.c_str()); std::remove(proc.c_str());
  mi355_shutdown();
  return rc_main;
}
