// ntt29.hpp -- BN254 Fr number-theoretic transform for gfx950: LDS-tiled Cooley-Tukey in at most three global passes, on the 9 x 29-bit
// unsaturated field (fp29.hpp).  Stands in for halo2_proofs::arithmetic::best_fft (natural order in -> natural order out,
// a'[i] = sum_j a[j] w^(ij), no scaling) and the EvaluationDomain wrappers around it.
//
// Decomposition N = M1*M2*M3 (each M <= 2^10).  Level l < L ("strided pass"): every contiguous sub-problem of
// size S = M_l * T is viewed as an M_l x T matrix; a workgroup loads M_l rows x C adjacent columns (C*32 B
// contiguous per row -> coalesced), runs the size-M_l DFT of each column in LDS (radix-2 DIF stages grouped into register
// rounds, bit reversal undone on the way out), multiplies by the inter-level twiddle w_S^(col*k) and stores to the scratch
// buffer.  Level L ("final pass"): a workgroup loads C contiguous segments of M_L elements that differ in the FASTEST output
// digit, transforms them in LDS and scatters so that each store instruction writes C*32 B contiguous; this
// pass also applies the digit-reversal permutation, so it runs out of place (scratch -> destination).
// HBM traffic = 64 B per element per pass (2-3 passes; algorithmic minimum is one pass = 64*N bytes).
//
// Arithmetic inside the tile: one v_mad_u64_u32 per limb product and lazy additions; the butterfly and inter-level twiddle products are the chained multiplier
// Fr29::mul_c (fp29.hpp: 8.61 vs 8.86 ms at 2^26 against the compiler-scheduled Fr29::mul in round 3), the once-per-element pre / post factors Fr29::mul.
//   * data stay in the ABI domain (x * 2^256): they are only re-sliced (from_sat_plain) on load; twiddles are kept as
//     w * 2^261 mod r (canonical, SoA tables), so Montgomery products with R' = 2^261 land back in the x * 2^256 domain
//   * butterfly (DIF): sum = carry(u + v), dif = (u - v + 64 r) * w  -- no branch for w = 1 (table entry 0 is the unit)
//   * value growth: a sum doubles the bound; after stages 5 and 10 of a tile the sums are brought back below 2r with
//     reduce_small (no multiplication); differences come out of a multiplication (< 1.6 r).  Bounds: start < 1.4 r (a pass reads canonical
//     input or the previous pass's multiplication output),
//     <= 44.8 r before a reduction, 64 r is the limit of sub64 / reduce_small.  (Round 3: the trivial-twiddle differences of a tile's LAST stage
//     stay un-reduced, < 103 r, when their consumer allows it -- a pass then starts below 1.62 r and reaches 51.6 r before its reduction.)
//   * elements leave a pass through a multiplication (inter-level twiddle, or the ifft / coset factor) or reduce_small,
//     then (closing pass) one conditional subtraction: everything the caller sees is canonical, so results stay bit-exact; the strided passes
//     leave the tight multiplication output (< 1.4 r) in the scratch buffer as it is.
// Element layout in LDS and in the twiddle tables: 36 B per element as three planes (SoA) -- two 16-byte planes (limbs 0..3, limbs 4..7) and one
// 4-byte plane (limb 8) -- so that consecutive lanes touch consecutive 16-byte slots (conflict-free ds_read_b128 / ds_write_b128); a 4096-element
// tile is 144 KiB of the 160 KiB.
#pragma once
#include "fp29.hpp"
#include "fp_asm.hpp"
#include "ntt_types.hpp"

namespace zk {

#ifndef ZK_NTT_ODD_FIRST
#define ZK_NTT_ODD_FIRST 1   // see lds_dif29
#endif
#ifndef ZK_NTT_LAZY_LAST
#define ZK_NTT_LAZY_LAST true   // trivial-twiddle differences of a tile's last stage stay un-reduced (see lds_dif29_round)
#endif
// tw_in / has_in (round 6, the coset shift folded into the first pass): element (m, column) of the FIRST strided pass is multiplied by tw_in[m] = (f^(2^log_t))^m on load, and the
// pass's inter-level table (direct 2 layout) carries f^column next to w_S^(column k) -- together the f^i of distribute_powers, for one multiplication per element and no pass of its own
struct Ntt29Level { uint32_t log_m, log_t, split; Tw29 tw_m, tw_s_lo, tw_s_hi; uint32_t direct; Tw29 tw_in = {nullptr, nullptr, nullptr}; uint32_t has_in = 0; };   // direct 1: tw_s_lo holds every inter-level twiddle w_S^e (small levels), no lo x hi product; direct 2: tw_s_lo is the table [k][column] = w_S^(column k) of a big level, read like the data (8 adjacent columns per row)

// the same three planes, writable: an LDS tile, or a twiddle table while it is being built (Tw29 is the read-only view the passes get)
struct Soa29 { uint4 *lo; uint4 *hi; uint32_t *top; operator Tw29() const { return Tw29{lo, hi, top}; } };

ZK_HD uint32_t bitrev32(uint32_t x, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return bits ? (__brev(x) >> (32 - bits)) : 0;
#else
  uint32_t r = 0; for (uint32_t i = 0; i < bits; i++) { r = (r << 1) | ((x >> i) & 1); } return r;
#endif
}

#if defined(__HIPCC__)
// the one load and the one store of a 36-byte SoA element (P: Tw29 or Soa29)
template <class P> __device__ __forceinline__ fe29_t soa29_load(const P &T, uint64_t i) {
  const uint4 a = T.lo[i], b = T.hi[i]; fe29_t r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w; r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w; r.l[8] = T.top[i]; return r;
}
__device__ __forceinline__ void soa29_store(const Soa29 &T, uint64_t i, const fe29_t &v) {
  T.lo[i] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]); T.hi[i] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]); T.top[i] = v.l[8];
}
__device__ __forceinline__ Soa29 lds29_carve(uint4 *base, uint32_t elems) { Soa29 L; L.lo = base; L.hi = base + elems; L.top = reinterpret_cast<uint32_t *>(base + 2 * elems); return L; }
// u - v + 64 r, limb-wise, no carry: v limbs <= 2^30 - 2, value(v) < 63.9 r; result limbs < 2^31.4 (multiplication operand only)
__device__ __forceinline__ fe29_t fr29_sub64(const fe29_t &u, const fe29_t &v) {
  constexpr uint32_t c[9] = {0x40000040u, 0x43eb27deu, 0x5709143cu, 0x54243cdau, 0x4174a0cdu, 0x56d03029u, 0x49b85043u, 0x57098cffu, 0xc19139au};
  fe29_t r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = u.l[i] + c[i] - v.l[i];
  return r;
}
// canonical ABI element from a tight value (< 2r, exact limbs)
__device__ __forceinline__ fe_t fr29_finish(const fe29_t &t) { return Fr29::to_sat_plain(Fr29::cond_sub_p(t)); }

// One round = R consecutive radix-2 DIF stages done in registers: a work item owns the 2^R elements that differ only in the
// R index bits those stages pair up, so the tile makes one LDS round trip and one barrier per R stages (3 per 9-stage tile
// instead of 9) and each lane carries 2^(R-1) independent multiplications per stage (ILP instead of occupancy).
// LAST (the round that ends the tile, b_lo = 0): the twiddle of a butterfly then depends on its position inside the work item only, and
// 2^R - 1 of the R * 2^(R-1) butterflies have the twiddle 1 (7 of 12 for R = 3): their multiplication is dropped at compile time -- the
// difference is brought back below 2r with reduce_small instead (~40 instructions against ~220).  Over a 2^26 transform this removes
// 2.6 of the 17 multiplications per element.
template <int R, bool LAST> __device__ __forceinline__ void lds_dif29_round(const Soa29 &L, uint32_t log_m, uint32_t log_c, uint32_t sm, uint32_t sc,
                                                                const Tw29 &tw_m, bool col_fast, uint32_t s0, bool lazy_last) {
  constexpr uint32_t Q = 1u << R;
  const uint32_t M = 1u << log_m, C = 1u << log_c, b_lo = log_m - s0 - R, items = (M >> R) << log_c;
  for (uint32_t g = threadIdx.x; g < items; g += blockDim.x) {
    uint32_t c, rest;
    if (col_fast) { c = g & (C - 1); rest = g >> log_c; } else { rest = g & ((M >> R) - 1); c = g >> (log_m - R); }
    const uint32_t low = rest & ((1u << b_lo) - 1), base = ((rest >> b_lo) << (b_lo + R)) | low;
    // all twiddles of the round are fetched first (L1/L2 hits, but ~500 cycles each): R * 2^(R-1) independent loads in flight
    // while the LDS reads and the first multiplications run
    fe29_t tw[R][Q / 2];
#pragma unroll
    for (int t = 0; t < R; t++) {
      const uint32_t stage = s0 + t, bit = R - 1 - t;
      uint32_t n = 0;
#pragma unroll
      for (uint32_t q0 = 0; q0 < Q; q0++) {
        if (q0 & (1u << bit)) continue;
        if (LAST && (q0 & ((1u << bit) - 1)) == 0) { n++; continue; }   // twiddle 1: never loaded, never multiplied
        tw[t][n++] = soa29_load(tw_m, (low | ((q0 & ((1u << bit) - 1)) << b_lo)) << stage);
      }
    }
    fe29_t x[Q];
    // A sum of two CARRIED values needs no carry pass of its own: its limbs stay below 2^30 + 16, which the next stage's sum (32-bit limbs),
    // difference (fr29_sub64: u < 2^30.1, v <= 2^30 + 64) and the pass-closing multiplication all accept.  Only sums with an un-carried operand
    // are carried -- half the carry passes of a round.  Whether the operands of a butterfly are un-carried is a function of the stage and of
    // the index bits already processed in this round (values read from LDS count as un-carried: the previous round stores its last sums as
    // they are; a difference is a multiplication output): loose_t = (bit processed at stage t - 1 is 0) and not loose_(t-1), loose_0 = true.
    // Codegen note: the choice is written as a limb-wise select between the two variants below.  As `if (in_loose) sum = carry(sum)` on the
    // 36-byte value the compiler kept the butterfly operands in scratch memory (ScratchSize 240, 90 registers) and the transform took 29 ms
    // instead of 10; check `hipcc -S` (ScratchSize 0, 122 registers) after touching this loop.
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) x[q] = soa29_load(L, (base | (q << b_lo)) * sm + c * sc);
#pragma unroll
    for (int t = 0; t < R; t++) {
      const uint32_t stage = s0 + t, bit = R - 1 - t;
      const bool reduce_now = (stage == 4 || stage == 9);
      uint32_t n = 0;
#pragma unroll
      for (uint32_t q0 = 0; q0 < Q; q0++) {
        if (q0 & (1u << bit)) continue;
        const uint32_t q1 = q0 | (1u << bit);
        const fe29_t u = x[q0], v = x[q1];
        // both operands share the processed bits, hence one flag; R <= 3: stage 0 carries, stage 1 does not, stage 2 carries the sums of stage-1 sums
        static_assert(R <= 3, "closed form of the recurrence for three stages");
        const bool in_loose = t == 0 ? true : t == 1 ? false : !((q0 >> (R >= 2 ? R - 2 : 0)) & 1u);
        const fe29_t s_raw = Fr29::add(u, v), s_car = Fr29::carry(s_raw);
        fe29_t sum;
#pragma unroll
        for (int i = 0; i < 9; i++) sum.l[i] = in_loose ? s_car.l[i] : s_raw.l[i];   // a compile-time choice per butterfly: the unused variant is dead code
        if (reduce_now) sum = Fr29::reduce_small(Fr29::normalise(s_raw));            // normalise is the full carry propagation
        // u - v + 64 r < 103 r: reduce_small is exact up to 2^261 = 168 r (host-checked), result tight < 2 r.  In the LAST STAGE of the tile
        // (t == R - 1 of the closing round) the difference is left as it is: nothing adds to it any more, and both consumers accept a loose
        // value below 103 r with limbs < 2^31.4 -- the strided pass multiplies every output by a canonical twiddle (9 limb products
        // < 2^60.4 per column plus the reduction terms stay below 2^64; (103 r)(r) / 2^261 + r < 1.7 r), the closing pass ends with
        // reduce_small(normalise(.)) or a multiplication itself.  One reduction (~70 instructions) per butterfly of that stage saved.
        if (LAST && (q0 & ((1u << bit) - 1)) == 0) { x[q1] = (ZK_NTT_LAZY_LAST && lazy_last && t == R - 1) ? fr29_sub64(u, v) : Fr29::reduce_small(Fr29::normalise(fr29_sub64(u, v))); n++; }
        else x[q1] = Fr29::mul_c(fr29_sub64(u, v), tw[t][n++]);
        x[q0] = sum;
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) soa29_store(L, (base | (q << b_lo)) * sm + c * sc, x[q]);
  }
  __syncthreads();
}
// lazy_last: the consumer of the tile accepts loose last-stage differences (< 103 r): true for the strided passes (every output is multiplied
// by an inter-level twiddle that is canonical, or the product of two canonical table entries: (103 r)(1.006 r) / 2^261 + r < 1.62 r) and for a
// closing pass without post-scaling (it ends with reduce_small(normalise(.)), exact below 168 r); a closing pass that multiplies by a
// post-scaling constant (tight, < 2 r) needs the reduced value ((103 r)(2 r) / 2^261 + r would exceed the single conditional subtraction).
template <int RMAX> __device__ __forceinline__ void lds_dif29(const Soa29 &L, uint32_t log_m, uint32_t log_c, uint32_t sm, uint32_t sc, const Tw29 &tw_m, bool col_fast, bool lazy_last) {
  uint32_t s = 0;
  // an odd tile with radix-4 rounds takes its single radix-2 stage FIRST (round 3): the closing round is then a LAST radix-4 round, which drops the
  // unit twiddles of the last TWO stages (0.75 multiplications per element) instead of the last one (0.5) -- the round count stays the same
  if (ZK_NTT_ODD_FIRST && RMAX == 2 && (log_m & 1u) && log_m >= 3) { lds_dif29_round<1, false>(L, log_m, log_c, sm, sc, tw_m, col_fast, 0, false); s = 1; }
  while (s < log_m) {
    const uint32_t left = log_m - s;
    if (RMAX >= 3 && left >= 3 && left != 4) { if (left == 3) lds_dif29_round<3, true>(L, log_m, log_c, sm, sc, tw_m, col_fast, s, lazy_last); else lds_dif29_round<3, false>(L, log_m, log_c, sm, sc, tw_m, col_fast, s, false); s += 3; }
    else if (RMAX >= 2 && left >= 2) { if (left == 2) lds_dif29_round<2, true>(L, log_m, log_c, sm, sc, tw_m, col_fast, s, lazy_last); else lds_dif29_round<2, false>(L, log_m, log_c, sm, sc, tw_m, col_fast, s, false); s += 2; }
    else { if (left == 1) lds_dif29_round<1, true>(L, log_m, log_c, sm, sc, tw_m, col_fast, s, lazy_last); else lds_dif29_round<1, false>(L, log_m, log_c, sm, sc, tw_m, col_fast, s, false); s += 1; }
  }
}
__device__ __forceinline__ fe29_t load_input29(const fe_t *__restrict__ src, uint64_t gi, uint64_t src_len, const fe_t *__restrict__ pre3) {
  if (gi >= src_len) return Fr29::zero();
  fe29_t v = Fr29::from_sat_plain(g_load(&src[gi]));
  if (pre3) { const uint32_t r3 = (uint32_t)(gi % 3); if (r3) v = Fr29::mul(v, Fr29::from_sat(g_load(&pre3[r3]))); }   // factor (c_sat << 5) = c * 2^261 < 2^259: output < 1.3 r
  return v;
}

// Several equal-size transforms in one launch (round 4): blockIdx.y picks the vector.  Small transforms (2^19 .. 2^22: the many-column layers run
// thousands per proof) are one round of workgroups each, so between two launches the device ramps down and up again; batched, workgroups of the next
// vector start as those of the previous one finish.  srcs == nullptr: the single-vector launch.
struct NttBatch { const fe_t *const *srcs; fe_t *const *dsts; };
// source and destination in the ABI form (8 x 32)
template <int RMAX> __global__ void __launch_bounds__(RMAX >= 2 ? 512 : 1024) k_ntt29_strided(const fe_t *__restrict__ src, fe_t *__restrict__ dst, Ntt29Level L, uint32_t log_c,
                                                        uint64_t src_len, const fe_t *__restrict__ pre3, NttBatch batch) {
  extern __shared__ uint4 lds[];
  if (batch.srcs) { src = batch.srcs[blockIdx.y]; dst = batch.dsts[blockIdx.y]; }
  const uint32_t M = 1u << L.log_m, C = 1u << log_c, tile = M << log_c;
  const Soa29 S = lds29_carve(lds, tile);
  const uint32_t cb_per_sub = 1u << (L.log_t - log_c);
  const uint64_t sub = blockIdx.x >> (L.log_t - log_c);
  const uint32_t cb = blockIdx.x & (cb_per_sub - 1);
  const uint64_t base = (sub << (L.log_m + L.log_t)) + ((uint64_t)cb << log_c);
  for (uint32_t e = threadIdx.x; e < tile; e += blockDim.x) {
    const uint32_t c = e & (C - 1), m = e >> log_c;
    fe29_t v = load_input29(src, base + ((uint64_t)m << L.log_t) + c, src_len, pre3);
    // canonical input (< r, exact limbs) times a canonical table entry: tight (< 1.4 r), what a pass may start from (header); uniform branch (kernel argument)
    if (L.has_in) v = Fr29::mul_c(v, soa29_load(L.tw_in, m));
    soa29_store(S, e, v);
  }
  __syncthreads();
  lds_dif29<RMAX>(S, L.log_m, log_c, C, 1, L.tw_m, true, true);
  const uint32_t smask = (1u << L.split) - 1;
  for (uint32_t e = threadIdx.x; e < tile; e += blockDim.x) {
    const uint32_t c = e & (C - 1), k = e >> log_c;
    const fe29_t v = soa29_load(S, (bitrev32(k, L.log_m) << log_c) + c);
    const uint32_t ex = ((cb << log_c) + c) * k;     // inter-level twiddle w_S^(col * k); entry 0 of both tables is the unit
    // the passes are ALU-bound and leave most of the HBM bandwidth idle: a big level reads its twiddles from a 2^log_s-entry table laid out
    // like the data (coalesced) instead of multiplying two half-size table entries -- one multiplication per element less in the first pass
    const fe29_t w = L.direct == 2 ? soa29_load(L.tw_s_lo, ((uint32_t)k << L.log_t) + (cb << log_c) + c)
                   : L.direct ? soa29_load(L.tw_s_lo, ex) : Fr29::mul_c(soa29_load(L.tw_s_lo, ex & smask), soa29_load(L.tw_s_hi, ex >> L.split));
    // the strided passes only ever write the library's scratch buffer: their outputs stay the multiplication's tight value (< 1.4 r < 2^256, exact
    // limbs) re-sliced to 8 x 32 bits -- no conditional subtraction; the next pass starts from < 1.4 r (five doublings: < 45 r < the 64 r limit) and
    // only the closing pass, whose output the caller sees, makes everything canonical
    g_store(&dst[base + ((uint64_t)k << L.log_t) + c], Fr29::to_sat_plain(Fr29::mul_c(v, w)));
  }
}

template <int RMAX> __global__ void __launch_bounds__(RMAX >= 2 ? 512 : 1024) k_ntt29_final(const fe_t *__restrict__ src, fe_t *__restrict__ dst, uint32_t log_m, uint32_t log_a, uint32_t log_b,
                                                      uint32_t log_c, Tw29 tw_m, uint64_t src_len, const fe_t *__restrict__ pre3, const fe_t *__restrict__ post3, NttBatch batch) {
  extern __shared__ uint4 lds[];
  if (batch.srcs) { src = batch.srcs[blockIdx.y]; dst = batch.dsts[blockIdx.y]; }
  const uint32_t M = 1u << log_m, C = 1u << log_c, seg = M + 1, tile = M << log_c;
  const Soa29 S = lds29_carve(lds, seg << log_c);
  const uint32_t k2 = blockIdx.x & ((1u << log_b) - 1);
  const uint32_t k1_0 = (blockIdx.x >> log_b) << log_c;
  for (uint32_t e = threadIdx.x; e < tile; e += blockDim.x) {
    const uint32_t m = e & (M - 1), c = e >> log_m;
    const uint64_t q = ((uint64_t)(k1_0 + c) << log_b) + k2;
    soa29_store(S, c * seg + m, load_input29(src, (q << log_m) + m, src_len, pre3));
  }
  __syncthreads();
  lds_dif29<RMAX>(S, log_m, log_c, 1, seg, tw_m, false, post3 == nullptr);
  const uint32_t log_stride = log_a + log_b;  // N / M
  fe29_t post0 = Fr29::zero(), post1 = post0, post2 = post0;   // named (not an array): runtime-indexed arrays go to scratch
  if (post3) { post0 = Fr29::reduce_small(Fr29::from_sat(g_load(&post3[0]))); post1 = Fr29::reduce_small(Fr29::from_sat(g_load(&post3[1]))); post2 = Fr29::reduce_small(Fr29::from_sat(g_load(&post3[2]))); }   // c * 2^261, tight
  for (uint32_t e = threadIdx.x; e < tile; e += blockDim.x) {
    const uint32_t c = e & (C - 1), k = e >> log_c;
    const fe29_t v = soa29_load(S, c * seg + bitrev32(k, log_m));
    const uint64_t oi = (uint64_t)(k1_0 + c) + ((uint64_t)k2 << log_a) + ((uint64_t)k << log_stride);
    fe29_t t;
    if (post3) { const uint32_t r3 = (uint32_t)(oi % 3); t = Fr29::mul(v, r3 == 0 ? post0 : (r3 == 1 ? post1 : post2)); }
    else t = Fr29::reduce_small(Fr29::normalise(v));
    g_store(&dst[oi], fr29_finish(t));
  }
}

// ---- table builders (set-up, outside the timed paths)
// out[i] = base^(i * step) for i < count, 8 x 32 Montgomery form (the twiddles of the G1 DFT, g1fft.hpp; tiny)
__global__ void k_pow_table(fe_t *out, fe_t base, uint64_t step, uint32_t count) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  fe_t b = step == 1 ? base : Fr::pow_u64(base, step);
  g_store(&out[i], Fr::pow_u64(b, i));
}
// SoA twiddle table: entry i = (base^step)^i * 2^261 mod r, canonical 29-bit limbs
__global__ void k_pow_table29(uint4 *lo, uint4 *hi, uint32_t *top, fe_t base, uint64_t step, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const fe_t b = step == 1 ? base : Fr::pow_u64(base, step);
  fe_t m32; { constexpr uint32_t c[8] = {0x8fffff57u, 0x2fd4e156u, 0xa494b01au, 0x75bba827u, 0x819caa80u, 0x5301fa84u, 0x563d4475u, 0xdc83629u}; for (int q = 0; q < 8; q++) m32.l[q] = c[q]; }   // 32 in Montgomery form
  soa29_store(Soa29{lo, hi, top}, i, Fr29::from_sat_plain(FrPs::mul(Fr::pow_u64(b, i), m32)));   // (w * 2^256) * 32 = w * 2^261 mod r, canonical
}
// table [k][col] (col < 2^log_t) of base^(col k) * 2^261 mod r: the inter-level twiddles of a big level in the order the pass reads them
// use_col: the entry also carries colbase^col (the column part f^col of a folded coset shift; colbase in Montgomery form)
__global__ void k_pow_table29_2d(uint4 *lo, uint4 *hi, uint32_t *top, fe_t base, uint32_t log_t, uint64_t count, fe_t colbase = fe_t{}, int use_col = 0) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t k = i >> log_t, col = i & ((1ull << log_t) - 1);
  fe_t m32; { constexpr uint32_t c[8] = {0x8fffff57u, 0x2fd4e156u, 0xa494b01au, 0x75bba827u, 0x819caa80u, 0x5301fa84u, 0x563d4475u, 0xdc83629u}; for (int q = 0; q < 8; q++) m32.l[q] = c[q]; }   // 32 in Montgomery form
  fe_t e = Fr::pow_u64(base, k * col);
  if (use_col) e = FrPs::mul(e, Fr::pow_u64(colbase, col));
  soa29_store(Soa29{lo, hi, top}, i, Fr29::from_sat_plain(FrPs::mul(e, m32)));
}
// dst[i] = src[i] * d (d: Montgomery form of the ABI): a twiddle table with a constant folded in -- the inverse transform's divisor rides on
// the inter-level twiddles of its last strided pass instead of costing the closing pass one more multiplication per element
__global__ void k_scale_table29(const uint4 *slo, const uint4 *shi, const uint32_t *stop, uint4 *lo, uint4 *hi, uint32_t *top, fe_t d, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  soa29_store(Soa29{lo, hi, top}, i, Fr29::cond_sub_p(Fr29::normalise(Fr29::mul(soa29_load(Tw29{slo, shi, stop}, i), Fr29::from_sat(d)))));   // (w 2^261)(d 2^261) / 2^261, canonical
}
#endif  // __HIPCC__

}  // namespace zk
