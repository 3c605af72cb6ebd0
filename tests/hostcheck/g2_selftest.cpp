// g2_selftest.cpp -- TEST INFRASTRUCTURE: compiles the __host__ __device__ G2 code that the G2 MSM kernels run (g2.hpp: Fq2 with the
// product-scanning multiplier of fp_asm.hpp, XYZZ madd / add / dbl, normalisation) for the CPU with plain g++, so that it can be checked
// against the oracle without a GPU.  Never shipped, never linked into libmi355zk.so.
#include "../../scroll-prover_amd/csrc/g2.hpp"
#include <vector>
using namespace zk;

using F2 = Fq2ps;   // the flavour the MSM kernels instantiate

extern "C" void g2s_madd(void *acc_xyzz, const void *affine) { g2_xyzz_madd<F2>(*(g2_xyzz_t *)acc_xyzz, *(const g2_affine_t *)affine); }
extern "C" void g2s_add(void *acc_xyzz, const void *q_xyzz) { g2_xyzz_add<F2>(*(g2_xyzz_t *)acc_xyzz, *(const g2_xyzz_t *)q_xyzz); }
extern "C" void g2s_dbl(void *out_xyzz, const void *p_xyzz) { *(g2_xyzz_t *)out_xyzz = g2_xyzz_dbl<F2>(*(const g2_xyzz_t *)p_xyzz); }
extern "C" void g2s_to_affine(void *out_affine, const void *p_xyzz) { *(g2_affine_t *)out_affine = g2_xyzz_to_affine<F2>(*(const g2_xyzz_t *)p_xyzz); }
extern "C" int g2s_on_curve(const void *affine) { return g2_is_on_curve_b<F2>(*(const g2_affine_t *)affine, g2_twist_b()) ? 1 : 0; }

// The bucket method with the kernels' building blocks, for small n: signed c-bit digits of the canonical scalars (the k_msm_digits rule:
// a digit above 2^(c-1) becomes digit - 2^c with a carry), per window buckets filled by madd of (x, +-y), running sums with add, Horner
// with dbl, normalisation.  scalars: canonical 256-bit little-endian words.
extern "C" void g2s_bucket_msm(void *out_affine, const void *bases_v, const void *scalars_v, uint64_t n, uint32_t c) {
  const g2_affine_t *bases = (const g2_affine_t *)bases_v; const fe_t *k = (const fe_t *)scalars_v;
  const uint32_t W = (256 + c - 1) / c + 1, nb = 1u << (c - 1);
  std::vector<int32_t> dig(n * W);
  for (uint64_t i = 0; i < n; i++) {
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; w++) {
      uint32_t raw = carry;
      for (uint32_t b = 0; b < c; b++) { const uint32_t bit = w * c + b; if (bit < 256) raw += ((k[i].l[bit >> 5] >> (bit & 31)) & 1u) << b; }
      if (raw > nb) { dig[i * W + w] = (int32_t)raw - (int32_t)(1u << c); carry = 1; } else { dig[i * W + w] = (int32_t)raw; carry = 0; }
    }
  }
  g2_xyzz_t acc = g2_xyzz_identity();
  std::vector<g2_xyzz_t> bucket(nb);
  for (uint32_t w = W; w-- > 0;) {
    for (uint32_t j = 0; j < c; j++) acc = g2_xyzz_dbl<F2>(acc);
    for (auto &b : bucket) b = g2_xyzz_identity();
    for (uint64_t i = 0; i < n; i++) {
      const int32_t d = dig[i * W + w];
      if (d == 0) continue;
      g2_affine_t q = bases[i];
      if (d < 0) q.y = F2::neg(q.y);
      g2_xyzz_madd<F2>(bucket[(d < 0 ? -d : d) - 1], q);
    }
    g2_xyzz_t run = g2_xyzz_identity(), sum = g2_xyzz_identity();
    for (uint32_t b = nb; b-- > 0;) { g2_xyzz_add<F2>(run, bucket[b]); g2_xyzz_add<F2>(sum, run); }
    g2_xyzz_add<F2>(acc, sum);
  }
  *(g2_affine_t *)out_affine = g2_xyzz_to_affine<F2>(acc);
}
