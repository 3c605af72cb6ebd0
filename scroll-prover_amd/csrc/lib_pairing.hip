// lib_pairing.hip -- libmi355zk.so, the translation unit of the BN254 pairing (fq12.hpp, pairing.hpp): mi355_pairing_products_host.  A unit of its own: the tower
// code is the slowest thing in the library to compile, and lib_aux.hip should not pay for it.  Host logic only.
// kernel headers first: lib_common.hpp defines the macro `g` (the calling thread's device context), a name the kernels use for locals
#define ZK_G2_DEVICE_ONLY 1      // pairing.hpp needs the twist arithmetic of g2.hpp, not k_g2_mul (that kernel belongs to lib_aux.hip)
#include "pairing.hpp"
#include "lib_common.hpp"

using namespace mi355;

constexpr uint64_t PAIRING_MAX_PAIRS = 1ull << 20;   // 768 MiB of workspace; a verifier has 2 to 4

extern "C" {

int mi355_pairing_products_host(const void *p_g1affine_host, const void *q_g2affine_host, uint32_t groups, uint32_t pairs_per_group, void *gt_out_host, uint32_t *is_one_out_host) {
  return guarded([&]() -> int {
  const int slot = pick_replica_slot(); DevGuard lk(slot);
  CHK(need_init(slot));
  if (groups == 0) return MI355_OK;
  if (pairs_per_group == 0) return fail(MI355_EBADARG, "pairing_products: pairs_per_group must not be zero");
  if (!gt_out_host && !is_one_out_host) return fail(MI355_EBADARG, "pairing_products: both outputs are null");
  if (!p_g1affine_host || !q_g2affine_host) return fail(MI355_EBADARG, "pairing_products: null pointer");
  const uint64_t n64 = (uint64_t)groups * pairs_per_group;
  if (n64 > PAIRING_MAX_PAIRS) return fail(MI355_EBADARG, "pairing_products: more than 2^20 pairs in one call");
  const uint32_t n = (uint32_t)n64;
  // the workspace: the points, two values per pair (the fe12_t arrays packed), the outputs, the two indices the validation reports
  WsLayout L;
  const uint64_t off_p = L.take(n64 * sizeof(g1_affine_t)), off_q = L.take(n64 * sizeof(g2_affine_t)), off_a = L.take_exact(n64 * sizeof(fe12_t)), off_b = L.take_exact(n64 * sizeof(fe12_t)),
                 off_gt = L.take_exact((uint64_t)groups * sizeof(fe12_t)), off_one = L.take((uint64_t)groups * 4), off_bad = L.take(8);
  PoolBlock ws; CHK(ws.alloc(L.total(), slot));
  hipStream_t s = g.stream;
  g1_affine_t *P = (g1_affine_t *)ws.at(off_p); g2_affine_t *Q = (g2_affine_t *)ws.at(off_q);
  fe12_t *cur = (fe12_t *)ws.at(off_a), *nxt = (fe12_t *)ws.at(off_b), *gt = (fe12_t *)ws.at(off_gt);
  uint32_t *one = (uint32_t *)ws.at(off_one), *bad_dev = (uint32_t *)ws.at(off_bad), bad[2] = {~0u, ~0u};
  HIPCHK(hipMemcpyAsync(P, p_g1affine_host, n64 * sizeof(g1_affine_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(Q, q_g2affine_host, n64 * sizeof(g2_affine_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(bad_dev, 0xff, 8, s));
  const fe2_t b = g2_twist_b(), b3 = Fq2::add(Fq2::dbl(b), b);
  {
    Scope sc("pairing_validate");
    hipLaunchKernelGGL(k_pairing_validate, dim3(ceil_div(n, PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, s, (const g1_affine_t *)P, (const g2_affine_t *)Q, n, b, bad_dev);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(bad, bad_dev, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (bad[0] != ~0u || bad[1] != ~0u) {   // nothing else is launched
    const uint32_t i = std::min(bad[0], bad[1]);
    const char *what = bad[0] == i && bad[1] == i ? "P is not on the curve y^2 = x^3 + 3 and Q is not on the twist y^2 = x^3 + 3 / (9 + u)"
                     : bad[0] == i ? "P is not on the curve y^2 = x^3 + 3" : "Q is not on the twist y^2 = x^3 + 3 / (9 + u)";
    resolve_spans();
    return fail(MI355_EBADARG, "pairing_products: pair " + std::to_string(i) + " (group " + std::to_string(i / pairs_per_group) + ", pair " + std::to_string(i % pairs_per_group) + " of it): " + what);
  }
  {
    Scope sc("pairing_miller");
    hipLaunchKernelGGL(k_pairing_miller, dim3(ceil_div(n, PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, s, (const g1_affine_t *)P, (const g2_affine_t *)Q, n, b3, cur);
  }
  for (uint32_t len = pairs_per_group; len > 1; len = (len + 1) / 2) {
    Scope sc("pairing_reduce");
    hipLaunchKernelGGL(k_pairing_reduce, dim3(ceil_div((uint64_t)groups * ((len + 1) / 2), PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, s, (const fe12_t *)cur, nxt, groups, len);
    std::swap(cur, nxt);
  }
  {
    Scope sc("pairing_final_exp");
    hipLaunchKernelGGL(k_pairing_final_exp, dim3(ceil_div(groups, PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, s, (const fe12_t *)cur, groups, gt, one);
  }
  HIPCHK(hipGetLastError());
  if (gt_out_host) HIPCHK(hipMemcpyAsync(gt_out_host, gt, (uint64_t)groups * sizeof(fe12_t), hipMemcpyDeviceToHost, s));
  if (is_one_out_host) HIPCHK(hipMemcpyAsync(is_one_out_host, one, (uint64_t)groups * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  resolve_spans();
  return MI355_OK;
  });
}

}  // extern "C"
