// frpoly.hpp -- the Fr polynomial kernels that are not transforms: eval_polynomial, distribute_powers, the element-wise vector operations, the gate-shaped
// fused evaluation (k_fr_gate_eval), the coset-part interleave and the partial-sum reduction.  Launched by lib_ntt.hip only.  Arithmetic on the 9 x 29-bit
// unsaturated field (fp29.hpp) with the domain conventions of ntt29.hpp (data x * 2^256, constants y * 2^261), whose fr29_finish they share.  k_fr_gate_eval's products are the
// chained Fr29::mul_c, as in the NTT butterflies and the bucket accumulation (round 6 A/B: profiles/r06_gate_chain_ab.json).
#pragma once
#include "fp29.hpp"
#include "fp_asm.hpp"
#include "ntt29.hpp"

namespace zk {

#if defined(__HIPCC__)
// ---- eval_polynomial (halo2_proofs::arithmetic::eval_polynomial, step 9 of create_proof: evaluations at x * omega^rot):
// p(x) = sum_i c_i x^i as a streaming reduction: each thread runs Horner over a contiguous run of EVAL_RUN coefficients
// (one multiplication per 32-byte coefficient read: the one kernel of the path that is close to HBM-bound), scales by
// x^(start of run), then the block sums its values (wavefront shuffles + LDS) into one partial per block.
constexpr uint32_t EVAL_RUN = 64;   // coefficients per thread; a block covers 256 * EVAL_RUN consecutive coefficients
__device__ __forceinline__ fe29_t shfl_down_fe29(const fe29_t &v, uint32_t o) { fe29_t r; for (int i = 0; i < 9; i++) r.l[i] = __shfl_down(v.l[i], o); return r; }
__device__ __forceinline__ fe29_t fr29_pow_u64(const fe29_t &x, uint64_t e) {
  fe29_t r = Fr29::one(), sq = x;
  while (e) { if (e & 1) r = Fr29::mul(r, sq); e >>= 1; if (e) sq = Fr29::sqr(sq); }
  return r;
}
// Thread t of a block takes the coefficients base + t + 256 k (k < EVAL_RUN): loads are coalesced (consecutive lanes, consecutive
// 32-byte coefficients) and every thread runs Horner in the SAME y = x^256, so the per-coefficient cost is one multiplication;
// the thread-specific factor x^t and the block factor x^base (computed once per block, broadcast through LDS) are applied at the end.
__device__ __forceinline__ void eval_poly_partial_body(const fe_t *__restrict__ poly, uint64_t n, const fe_t &x_sat, fe_t *__restrict__ partial) {
  __shared__ uint32_t lds[5][9];
  const uint64_t base = (uint64_t)blockIdx.x * 256 * EVAL_RUN;
  const fe29_t x = Fr29::reduce_small(Fr29::from_sat(x_sat));          // x * 2^261, tight
  if (threadIdx.x < 64) {                                               // wave 0: x^base for the whole block (all lanes compute the same value)
    const fe29_t xb = fr29_pow_u64(x, base);
    if (threadIdx.x == 0) for (int k = 0; k < 9; k++) lds[4][k] = xb.l[k];
  }
  fe29_t y = x;
#pragma unroll
  for (int i = 0; i < 8; i++) y = Fr29::sqr(y);                        // x^256
  fe29_t acc = Fr29::zero();
  bool any = false;
  for (int k = EVAL_RUN - 1; k >= 0; k--) {
    const uint64_t i = base + threadIdx.x + 256ull * (uint32_t)k;
    if (any) acc = Fr29::mul(acc, y);                                  // tight, < 1.3 r
    if (i < n) {
      const fe29_t c = Fr29::from_sat_plain(g_load(&poly[i]));         // ABI domain (c * 2^256); products with x-powers keep it
      for (int q = 0; q < 9; q++) acc.l[q] += c.l[q];                  // lazy add: limbs < 2^30, value < 2.3 r
      any = true;
    }
  }
  acc = Fr29::mul(acc, fr29_pow_u64(x, threadIdx.x));                  // * x^t (<= 8 squarings + multiplications)
  __syncthreads();
  { fe29_t xb; for (int k = 0; k < 9; k++) xb.l[k] = lds[4][k]; acc = Fr29::mul(acc, xb); }   // * x^base, tight
  for (uint32_t o = 32; o >= 1; o >>= 1) {
    const fe29_t other = shfl_down_fe29(acc, o);
    acc = Fr29::carry(Fr29::add(acc, other));
    if (o == 4) acc = Fr29::reduce_small(Fr29::normalise(acc));         // after 4 doublings: < 16 * 1.3 r -> < 2 r
  }
  acc = Fr29::reduce_small(Fr29::normalise(acc));                       // < 8 * 2 r -> < 2 r
  if ((threadIdx.x & 63) == 0) for (int k = 0; k < 9; k++) lds[threadIdx.x >> 6][k] = acc.l[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < 4; w++) { fe29_t o; for (int k = 0; k < 9; k++) o.l[k] = lds[w][k]; acc = Fr29::carry(Fr29::add(acc, o)); }
    g_store(&partial[blockIdx.x], fr29_finish(Fr29::reduce_small(Fr29::normalise(acc))));   // canonical, ABI domain
  }
}
__global__ void __launch_bounds__(256) k_eval_poly_partial(const fe_t *__restrict__ poly, uint64_t n, fe_t x_sat, fe_t *__restrict__ partial) { eval_poly_partial_body(poly, n, x_sat, partial); }
// blockIdx.y = evaluation: step 9 of create_proof evaluates thousands of (polynomial, point) pairs at k = 20, each a 64-block launch whose ~100 us are
// latency (a serial Horner chain of 64 multiplications per thread behind a power ladder); one launch over all pairs is throughput-bound instead
__global__ void __launch_bounds__(256) k_eval_poly_partial_batch(const fe_t *const *__restrict__ polys, uint64_t n, const fe_t *__restrict__ points, fe_t *__restrict__ partial, uint64_t stride) {
  eval_poly_partial_body(polys[blockIdx.y], n, g_load(&points[blockIdx.y]), partial + stride * blockIdx.y);
}
// a[i] *= f^i  (halo2_proofs distribute_powers: the coset shift of coeff_to_extended_part / general coset FFTs).
// Same tiling as k_eval_poly_partial: thread t walks i = base + t + 256 k with a running power stepped by f^256.
// src == a: in place; otherwise a = src scaled (the coset transforms write the scaled copy straight into their destination: no separate copy)
// DistFactors: f, f^256 and f^(256 EVAL_RUN) in Montgomery (ABI) form, the two powers computed by the host (round 4: the in-kernel ladder
// f^base with a 64-bit exponent cost every block ~40 dependent multiplications before its first store -- 108 us for a 2^16-element call)
struct DistFactors { fe_t f, f256, fblock; };
__device__ __forceinline__ void distribute_powers_body(const fe_t *src, fe_t *a, uint64_t n, const DistFactors &F) {
  __shared__ uint32_t lds[9];
  const uint64_t base = (uint64_t)blockIdx.x * 256 * EVAL_RUN;
  const fe29_t f = Fr29::reduce_small(Fr29::from_sat(F.f));
  if (threadIdx.x < 64) { const fe29_t fb = fr29_pow_u64(Fr29::reduce_small(Fr29::from_sat(F.fblock)), blockIdx.x); if (threadIdx.x == 0) for (int k = 0; k < 9; k++) lds[k] = fb.l[k]; }   // (f^(256 EVAL_RUN))^block: a short exponent
  const fe29_t y = Fr29::reduce_small(Fr29::from_sat(F.f256));         // f^256
  fe29_t pw = fr29_pow_u64(f, threadIdx.x);
  __syncthreads();
  { fe29_t fb; for (int k = 0; k < 9; k++) fb.l[k] = lds[k]; pw = Fr29::mul(pw, fb); }   // f^(base + t), tight
  for (uint32_t k = 0; k < EVAL_RUN; k++) {
    const uint64_t i = base + threadIdx.x + 256ull * k;
    if (i >= n) break;
    g_store(&a[i], fr29_finish(Fr29::mul(Fr29::from_sat_plain(g_load(&src[i])), pw)));
    pw = Fr29::mul(pw, y);
  }
}
__global__ void __launch_bounds__(256) k_distribute_powers(const fe_t *src, fe_t *a, uint64_t n, DistFactors F) { distribute_powers_body(src, a, n, F); }
// blockIdx.y = polynomial: the coset shift of every polynomial of a coset part in ONE launch (mi355_coset_ntt_fr_batch_dev)
__global__ void __launch_bounds__(256) k_distribute_powers_batch(const fe_t *const *srcs, fe_t *const *dsts, uint64_t n, DistFactors F) { distribute_powers_body(srcs[blockIdx.y], dsts[blockIdx.y], n, F); }

// element-wise vector operations on device-resident polynomials (the pointwise steps between the transforms of the quotient
// construction): op 0 add, 1 sub, 2 mul; and data[i] *= table[i mod period] (division by the vanishing polynomial on
// the extended coset: halo2's t_evaluations have period 2^(extended_k - k)).  Streaming, 16 B/lane accesses, grid-stride.
// no __restrict__: dst may be one of the operands (each thread reads element i of both operands before it writes element i)
__global__ void __launch_bounds__(256) k_fr_vec_op(int op, fe_t *dst, const fe_t *a, const fe_t *b, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const fe_t x = g_load(&a[i]), y = g_load(&b[i]);
    fe_t r;
    if (op == 0) r = Fr::add(x, y);
    else if (op == 1) r = Fr::sub(x, y);
    else r = fr29_finish(Fr29::mul(Fr29::from_sat_plain(x), Fr29::from_sat(y)));   // (x 2^256)(y 2^261) / 2^261
    g_store(&dst[i], r);
  }
}
// dst = a + s * b (s a scalar): the linear combinations sum_i v^i p_i(X) of the multi-open argument, one polynomial at a time
__global__ void __launch_bounds__(256) k_fr_vec_axpy(fe_t *dst, const fe_t *a, const fe_t *b, fe_t s_sat, uint64_t n) {   // dst may alias a or b
  const fe29_t s = Fr29::from_sat(s_sat);   // s * 2^261: the product with b * 2^256 lands back in the ABI domain
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const fe_t sb = fr29_finish(Fr29::mul(Fr29::from_sat_plain(g_load(&b[i])), s));
    g_store(&dst[i], a ? Fr::add(g_load(&a[i]), sb) : sb);
  }
}
__global__ void __launch_bounds__(256) k_fr_vec_mul_periodic(fe_t *__restrict__ data, uint64_t n, const fe_t *__restrict__ table, uint32_t period_mask) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    g_store(&data[i], fr29_finish(Fr29::mul(Fr29::from_sat_plain(g_load(&data[i])), Fr29::from_sat(g_load(&table[i & period_mask])))));
}

// ---- gate-shaped fused evaluation (the operand shape of halo2's evaluate_h [EXT-recalled halo2_proofs src/plonk/evaluation.rs: GraphEvaluator /
// get_rotation_idx]): dst[i] (+)= sum_j c_j * prod_k p_{jk}[(i + r_jk) mod n] for a small term list, rotations included, in
// ONE pass -- every operand is read once per use and nothing but dst is written, instead of one full HBM round trip per add / mul of a chain of
// k_fr_vec_op launches.  The term list travels as a kernel argument (scalar loads, uniform across the wavefront).  n is a power of two (the
// extended domain, or one 2^k coset part of the scroll fork); rotations arrive already scaled (rot * 2^(extended_k - k) on the extended domain).
// Arithmetic: the first factor is re-sliced in the ABI domain (x 2^256), the coefficient and every further factor enter as y 2^261, so each
// Montgomery product (R' = 2^261) lands back in the ABI domain; term values (< 2 r) are summed lazily, carried every fourth term, and reduced
// once (<= 16 terms + dst: < 34 r, below reduce_small's 64 r).
constexpr uint32_t GATE_MAX_TERMS = 16, GATE_MAX_FACTORS = 48, GATE_MAX_POLYS = 24, GATE_MAX_TERM_LEN = 16;   // a degree-9 gate of the inner circuit (selector, coefficient, seven cells) is ONE term
struct GatePlan {
  const fe_t *poly[GATE_MAX_POLYS];
  fe_t coeff[GATE_MAX_TERMS];            // Montgomery (ABI) form (constant terms)
  fe29_t coeff29[GATE_MAX_TERMS];        // the same coefficient as c * 2^261 in 29-bit limbs (Fr29::from_sat, done once on the host: round 4 -- the kernel used to re-slice every general coefficient for every row)
  int32_t factor_rot[GATE_MAX_FACTORS];
  uint8_t factor_poly[GATE_MAX_FACTORS];
  uint8_t term_len[GATE_MAX_TERMS];      // factors per term (0: the constant c_j)
  uint8_t coeff_kind[GATE_MAX_TERMS];    // 0: general coefficient, 1: c_j = 1, 2: c_j = -1 (set by the host from the coefficient bytes)
  uint32_t n_terms, accumulate;
};
// dst carries no __restrict__: it may be one of the operands (un-rotated, checked by the host) and is read when G.accumulate is set
__global__ void __launch_bounds__(256) k_fr_gate_eval(fe_t *dst, GatePlan G, uint64_t n) {
  const uint64_t mask = n - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    fe29_t acc = Fr29::zero();
    uint32_t f = 0;
    for (uint32_t j = 0; j < G.n_terms; j++) {
      const uint32_t len = G.term_len[j];
      fe29_t t;
      if (len == 0) t = Fr29::from_sat_plain(G.coeff[j]);
      else {
        const fe_t x0 = g_load(&G.poly[G.factor_poly[f]][(i + (uint64_t)(int64_t)G.factor_rot[f]) & mask]);
        // unit coefficients (the common case in halo2 gates: a - b, z(wX) prod - z(X) prod): no multiplication by c_j; -1 negates the canonical first
        // factor instead (r - x, zero stays zero), so the term value stays a tight non-negative representative (< r) like every other
        const uint32_t kind = G.coeff_kind[j];
        if (kind == 0) t = Fr29::mul_c(Fr29::from_sat_plain(x0), G.coeff29[j]);
        else t = Fr29::from_sat_plain(kind == 2 ? Fr::neg(x0) : x0);
        for (uint32_t q = 1; q < len; q++)
          t = Fr29::mul_c(t, Fr29::from_sat(g_load(&G.poly[G.factor_poly[f + q]][(i + (uint64_t)(int64_t)G.factor_rot[f + q]) & mask])));
      }
      f += len;
      acc = Fr29::add(acc, t);
      if ((j & 3) == 3) acc = Fr29::carry(acc);
    }
    if (G.accumulate) acc = Fr29::add(acc, Fr29::from_sat_plain(g_load(&dst[i])));
    g_store(&dst[i], fr29_finish(Fr29::reduce_small(Fr29::normalise(acc))));
  }
}

// dst[i * Q + q] = parts[q][i]: the Q coset parts of the scroll fork's evaluate_h (part q = the evaluations at zeta * omega_ext^(q + Q i), i < n)
// laid out as the extended domain's natural order, which is what extended_to_coeff inverts.  Q <= 8 pointers travel as a kernel argument; a lane
// reads one 32-byte element per part (consecutive lanes, consecutive elements) and writes Q consecutive elements: both sides coalesced.
struct InterleavePlan { const fe_t *part[8]; uint32_t q; };
__global__ void __launch_bounds__(256) k_fr_interleave(fe_t *__restrict__ dst, InterleavePlan P, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    for (uint32_t q = 0; q < P.q; q++) g_store(&dst[i * P.q + q], g_load(&P.part[q][i]));
}

// sum of m canonical field elements (the per-block partials) by one workgroup; blockIdx.x = which vector (stride elements apart) of a batch
__global__ void __launch_bounds__(256) k_fr_sum(const fe_t *__restrict__ in_all, uint64_t m, fe_t *__restrict__ out_all, uint64_t stride = 0) {
  const fe_t *__restrict__ in = in_all + stride * blockIdx.x; fe_t *__restrict__ out = out_all + blockIdx.x;
  __shared__ fe_t lds[4];
  fe_t acc = Fr::zero();
  for (uint64_t i = threadIdx.x; i < m; i += blockDim.x) acc = Fr::add(acc, g_load(&in[i]));
  for (uint32_t o = 32; o >= 1; o >>= 1) { fe_t other; for (int k = 0; k < 8; k++) other.l[k] = __shfl_down(acc.l[k], o); acc = Fr::add(acc, other); }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) { for (uint32_t w = 1; w < 4; w++) acc = Fr::add(acc, lds[w]); g_store(out, acc); }
}
#endif  // __HIPCC__

}  // namespace zk
