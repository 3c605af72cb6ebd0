// g1codec_selftest.cpp -- TEST INFRASTRUCTURE: compiles the __host__ __device__ codec that k_g1_decompress / k_g1_compress run per lane (g1codec.hpp:
// the 9 x 29-bit square root with the plain C++ multiplier, which the device's chained multiplier equals bit for bit) and the host-side G2 codec of
// the Processed params loader for the CPU with plain g++, so that both can be checked against the oracle without a GPU.  Never shipped.
#include "../../scroll-prover_amd/csrc/g1codec.hpp"
using namespace zk;

// words: n x 32 B in, points: n x 64 B out, ok: n flags out
extern "C" void g1c_decompress(const void *words, void *points, uint8_t *ok, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) {
    uint32_t w[8]; memcpy(w, (const uint8_t *)words + 32 * i, 32);
    g1_affine_t p; ok[i] = g1_decompress_point(w, p) ? 1 : 0;
    memcpy((uint8_t *)points + 64 * i, &p, 64);
  }
}
extern "C" void g1c_compress(const void *points, void *words, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) {
    g1_affine_t p; memcpy(&p, (const uint8_t *)points + 64 * i, 64);
    uint32_t w[8]; g1_compress_point(p, w);
    memcpy((uint8_t *)words + 32 * i, w, 32);
  }
}
extern "C" int g2c_decompress(const void *word64, void *point128) {
  g2_affine_t p; const bool ok = g2_decompress_point((const uint8_t *)word64, p);
  memcpy(point128, &p, 128); return ok ? 1 : 0;
}
extern "C" void g2c_compress(const void *point128, void *word64) {
  g2_affine_t p; memcpy(&p, point128, 128);
  g2_compress_point(p, (uint8_t *)word64);
}
