// msm_plan.hpp -- everything lib_msm.hip decides about a bucket MSM BEFORE it touches the device, as plain C++ (no HIP): the window search (once, for the pass and for
// mi355_srs_precompute), the plan of one pass (PassPlan: window and key split, accumulate launch, fix-up form, sorter tiles, reduction chunking), the batch splitter's rule,
// the chunk count of the pipelined schedule and the slice cuts of the host-pointer schedule.  Inputs are values only (PlanIn: the knobs of knobs.hpp, the calling thread's
// options, the CU count), so tests/hostcheck/msm_plan_main.cpp runs the same functions without a device and tests/test_msm_plan_on_host.py compares every field with the
// restatement of tests/msm_plan_common.py.  A refusal is a status with its message; the planner never writes the error slot (the caller turns it into fail()).
// The `double` expressions of the cost model stay as they are written, in this order: the lengths at which the window changes depend on their rounding.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "knobs.hpp"

namespace zk {
// limits the kernels of msm.hpp and the planner share
constexpr int MSM_SCALAR_BITS = 255, MSM_MAX_C = 24;   // hard limit of the sorter (23 key bits); the automatic choices stop at ProcessKnobs::msm_auto_max_c
constexpr uint32_t SCAN_BLOCK = 1024, SCAN_ITEMS = 4;  // 4096 per workgroup
constexpr uint32_t SORT_MAX_BINS = 4096;
constexpr uint32_t SORT_SPLIT_TMAX = 128;   // entries of the block-start table of k_sort_l1_scatter_split (coarse bins >> spare key bits, at most 2048 >> 4)
constexpr uint32_t FIXUP_HUGE_MIN = 2048, FIXUP_SLICES = 64;   // SLICES <= 64: one wavefront folds the slice sums
constexpr uint32_t TREE_PER_THREAD = 4;
}  // namespace zk

namespace mi355zk {
using zk::MSM_SCALAR_BITS;

struct PlanIn {
  Knobs k; uint32_t auto_max_c = 22, chunk_min_log = 23;   // the device slot's knobs, ProcessKnobs::msm_auto_max_c, the pipeline threshold of mi355_msm_set_pipeline
  int force_c = 0; bool no_tables = false;                 // the calling thread's options (mi355_msm_set_window_bits)
  uint32_t cus = 256;                                      // compute units of the device
};
// what is group-specific to the plan: the bucket record's size, and G2 always takes the segmented fix-up at 100 % fill
struct MsmGroup { uint32_t rec_bytes; bool always_segmented; };
constexpr MsmGroup GROUP_G1{144, false}, GROUP_G2{256, true};
struct TableShape { int c = 0, w = 0; };   // the window tables of the basis; c = 0: none

inline uint32_t plan_ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
inline uint32_t plan_log2_ceil(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) l++; return l; }

// measured on MI355X, in units of one bucket addition (~0.07 ns at 14 G adds/s): sort ~0.18 per entry, bucket reduction ~8.2 per bucket
// (fix-up, running sums, tree); without window tables the result also waits for the serial Horner tail over the windows (255 doublings
// in one lane, ~2 ms = 3e7 units).  The ordering this model gives for c was re-checked against tools/bench_window_choice.py (k = 18 ... 24).
inline double msm_cost(uint64_t n, int c, bool shared) { const double W = (MSM_SCALAR_BITS + c - 1) / c, nb = (double)(1ull << (c - 1)); return 1.18 * W * (double)n + 8.2 * nb * (shared ? 1.0 : W) + (shared ? 0.0 : 3.0e7); }

// THE window search: the cheapest c in [4, max_c] for n points, with one shared bucket set (window tables) or a set per window; per-window sets above 6 GB of G1 records are skipped
inline int best_window(uint64_t n, uint32_t max_c, bool shared) {
  double best = 1e300; int best_c = 8;
  for (int c = 4; c <= (int)max_c; c++) {
    const double W = (MSM_SCALAR_BITS + c - 1) / c, nb = (double)(1ull << (c - 1));
    if (!shared && W * nb * GROUP_G1.rec_bytes > 6.0e9) continue;
    const double cost = msm_cost(n, c, shared);
    if (cost < best) { best = cost; best_c = c; }
  }
  return best_c;
}
// mi355_srs_precompute's automatic choice: tables that exist (inherited from the parent basis, or built with another width) stay when they are within 10 % of the best schedule
inline bool tables_close_enough(uint64_t n, int have_c, int best_c) { return msm_cost(n, have_c, true) <= 1.10 * msm_cost(n, best_c, true); }

enum class Fixup { Segmented, Quad, FourLanes, OneLane };   // one segmented reduction over the partial sums | the per-bucket kernel in its three forms

struct PassPlan {
  const char *refusal = nullptr;   // null: the pass can run; else the text of the MI355_EBADARG it is refused with (the fields below the shape are then unset)
  uint64_t n = 0; uint32_t M = 0;
  // shape: window bits, table use, sorter key split, entry / bucket counts
  bool shared = false; uint32_t c = 0, W = 0, fb = 0, cb_bits = 0, regions = 0; uint64_t emax = 0, nbuckets = 0;
  // accumulate launch: worst-case entries per thread (16 .. 4096, seg_factor segments per lane slot), workgroups, threads; the kernels derive the actual segment from the entry
  // count on the device (msm_seg_eff) out of seg_arg = worst-case segment | minimum << 13 | (fill percentage / 2) << 26
  uint32_t seg = 0, blocks = 0, tn = 0, seg_arg = 0;
  Fixup fixup = Fixup::Segmented; uint32_t big_cap = 0, huge_cap = 0, serial_max = 0, huge_min = 0;
  uint32_t t1 = 0, t2 = 0, tiles1 = 0, l2_tiles_max = 0;   // sorter: level-1 / level-2 tile in entries and their counts
  uint32_t chunk = 0, chunks_per_set = 0; bool quad_sums = false, quad_final = false; uint32_t tree_quad_max = 0;   // reduction tail
  bool ok() const { return !refusal; }
  uint32_t wpp() const { return shared ? 1 : W; }    // bucket sets per polynomial
  uint32_t sets() const { return M * wpp(); }
  bool tree_quad(uint32_t cnt) const { return (uint64_t)cnt * sets() <= tree_quad_max; }   // a tree level with cnt inputs per set, where the policy has the quad form
};
struct ForcedShape { uint32_t c; bool shared; };   // the slices of a host-sliced MSM must agree on the bucket layout: (c, shared) of the biggest slice

inline PassPlan plan_pass(const PlanIn &in, uint64_t n, uint32_t M, TableShape tab, MsmGroup grp, const ForcedShape *forced = nullptr) {
  const Knobs &k = in.k;
  PassPlan o; o.n = n; o.M = M;
  if (forced) { o.c = forced->c; o.shared = forced->shared; }
  else {
    o.c = (uint32_t)(in.force_c ? in.force_c : best_window(n, in.auto_max_c, false));
    // precomputed rows 2^(c w) P available and cheaper than the per-window schedule at this n -> all windows share one bucket set
    o.shared = tab.c && !in.force_c && !in.no_tables && msm_cost(n, tab.c, true) <= msm_cost(n, (int)o.c, false) && ((uint64_t)tab.w << plan_log2_ceil(n)) < (1ull << 31);
    if (o.shared) o.c = (uint32_t)tab.c;
  }
  o.W = (MSM_SCALAR_BITS + o.c - 1) / o.c;
  o.emax = (uint64_t)M * n * o.W;
  const uint32_t kb = o.c - 1; uint32_t fb = kb < k.sort_fb ? kb : k.sort_fb; if (kb - fb > 11) fb = kb - 11;
  o.fb = fb; o.cb_bits = kb - fb;
  const uint64_t sets = (uint64_t)M * (o.shared ? 1 : o.W);
  o.nbuckets = sets << kb;
  const uint64_t regions = sets << o.cb_bits; o.regions = (uint32_t)std::min<uint64_t>(regions, 0xffffffffu);
  if (o.emax >= (1ull << 32)) { o.refusal = "msm: n * windows must be < 2^32"; return o; }
  if (o.nbuckets >= (1ull << 31)) { o.refusal = "msm: too many buckets (split the batch)"; return o; }
  if (regions * 4 > 48 * 1024) { o.refusal = "msm: batch too large for the coarse histogram (split the batch)"; return o; }
  if (o.fb > 12 || (1u << o.cb_bits) > zk::SORT_MAX_BINS) { o.refusal = "msm: window bits out of range for the sorter"; return o; }

  const uint64_t want_threads = (uint64_t)in.cus * 256 * k.seg_factor;
  uint64_t seg = (o.emax + want_threads - 1) / want_threads; if (seg < 16) seg = 16; if (seg > 4096) seg = 4096;
  o.seg = (uint32_t)seg; o.blocks = plan_ceil_div(plan_ceil_div(o.emax, seg), 256); o.tn = o.blocks * 256;
  // with the segmented fix-up (two-partial buckets are cheap) the entries may spread over more threads than with the per-bucket kernels.  By shape (fixup_mode 2): big
  // bucket sets whose buckets are no longer than a segment straddle two accumulate threads as a rule -- the case the segmented reduction is measured faster in (2^24 ..
  // 2^26 with c = 22); everything else takes the per-bucket kernels
  const uint32_t nbuckets = (uint32_t)o.nbuckets;
  const bool segfix = grp.always_segmented || k.fixup_mode == 1 || (k.fixup_mode == 2 && nbuckets >= (1u << 19) && (uint64_t)o.seg * o.nbuckets >= o.emax);
  const uint32_t fill_pct = grp.always_segmented ? 100 : segfix ? k.seg_fill_segfix : k.seg_fill;
  o.seg_arg = o.seg | (std::min(k.seg_min, o.seg) << 13) | ((fill_pct / 2) << 26);
  // four lanes per bucket where buckets straddle many short segments (small and mid-size MSMs); with 2^19 buckets and more the extra threads cost more than the shorter
  // chains save (measured: +0.15 ms at 2^18, +0.5 ms at 2^21 buckets)
  o.fixup = segfix ? Fixup::Segmented : ((uint64_t)nbuckets * 4 <= k.tail_coop_max && (k.tail_coop_mask & 1u)) ? Fixup::Quad : nbuckets <= (1u << k.fixup_lanes_max_log) ? Fixup::FourLanes : Fixup::OneLane;
  o.serial_max = k.fixup_serial_max; o.huge_min = k.fixup_huge_min;
  o.big_cap = o.tn / k.fixup_serial_max + 2;
  o.huge_cap = o.tn / zk::FIXUP_HUGE_MIN + 2;   // buckets that span >= FIXUP_HUGE_MIN accumulate threads (at most tn / FIXUP_HUGE_MIN of them) get FIXUP_SLICES workgroups each

  o.t1 = k.sort_t1;                           // level-1 tile: 1024 threads x 8 or 16 entries (64 / 128 KiB of LDS staging)
  // split records (payload u32 + fine key u16 as two streams, sort_split): 6 bytes of staging per entry -> 24 576-entry tiles where the bin bookkeeping leaves room
  // (<= 1024 coarse bins); sort_split = 2: split records, 16 384-entry tiles
  if (k.sort_split == 1 && o.t1 == 16384 && (1u << o.cb_bits) <= 1024 && o.emax >= (1ull << 24)) o.t1 = 24576;
  // level-2 tile (6 B of LDS per entry next to the 3 x 2^fb words of bin bookkeeping): 16384 entries give twice the run length in `sorted` (fewer partial-line store
  // transactions, the limiter of this kernel) at one workgroup per CU; worth it for big sorts
  o.t2 = k.sort_t2 ? k.sort_t2 : (o.emax >= (1ull << 27) && o.fb <= 11 ? 16384 : 8192);
  o.tiles1 = plan_ceil_div(n, o.t1); o.l2_tiles_max = plan_ceil_div(o.emax, o.t2) + o.regions + 8;   // + 8: the XCD-aware tile order rounds the tile count up to a multiple of 8

  // running-sum chunk per reduce thread: every thread is one serial chain of 2*chunk additions plus a ~(c-1)-bit scalar multiple, so the chain is kept short (the kernel is
  // latency-bound) as long as there are enough buckets to give the GPU ~128k chains (measured at 2^21 buckets: 2.58 ms with 256k chains of 8 buckets, 2.11 ms with 128k of
  // 16, 2.63 ms with 64k of 32); bucket sets of small MSMs: chains down to reduce_min_chunk buckets -- the chain is then mostly the (c - 2)-bit multiple of the chunk sum,
  // ~26 instead of ~37 addition times at 2^16 buckets
  const uint32_t nb = 1u << kb, nsets = o.sets();
  uint32_t chunk = 64; while (chunk > nb) chunk >>= 1;
  while (chunk > k.reduce_min_chunk && (uint64_t)(nb / chunk) * nsets < k.reduce_chains) chunk >>= 1;
  o.chunk = chunk; o.chunks_per_set = nb / chunk;
  // latency form (a quad per logical thread: ~2.6x shorter dependent chain per addition) where the kernel cannot fill the GPU anyway; throughput form (one lane per thread)
  // for big bucket sets.  tail_coop_max = largest logical thread count that takes the quads, tail_coop_mask = which kernels may
  o.quad_sums = o.chunks_per_set * nsets <= k.tail_coop_max && (k.tail_coop_mask & 2u);
  o.tree_quad_max = (k.tail_coop_mask & 4u) ? k.tail_coop_max : 0;
  o.quad_final = k.tail_coop_max && (k.tail_coop_mask & 8u);
  return o;
}

// a batch that would overflow the 32-bit entry index, the coarse histogram's LDS or 8 GiB of bucket records runs as two half batches
inline bool must_split(const PassPlan &p, MsmGroup grp) { return !p.ok() || p.emax > (1ull << 29) || p.nbuckets * grp.rec_bytes > (8ull << 30); }

// Chunks of a pipelined MSM: the point range is cut into K slices [n k / K, n (k + 1) / K), every slice a complete MSM.  OFF by default (msm_chunks = 1).
inline uint32_t pipeline_chunks(const PlanIn &in, uint32_t M, uint64_t n) {
  if (in.k.msm_chunks <= 1 || M != 1 || n < (1ull << in.chunk_min_log)) return 1;
  uint32_t k = in.k.msm_chunks;
  while (k > 1 && n / k < ((1ull << in.chunk_min_log) >> 2)) k--;
  return k;
}

// Slice plan of the host-pointer MSM: the copy of slice k + 1 must fit under the compute of slice k.  PCIe moves a pair's 32 bytes ~1.7x faster than the GPU consumes them, so
// slices may GROW by that factor: a small first slice (its copy is the only exposed one), then x1.7 each -- 5 slices for 2^26 pairs instead of 8 equal ones.  Every extra slice
// costs bucket crossings in the accumulation (each bucket is visited once per slice) and a fix-up pass, which is why fewer, growing slices win (measured: 8 equal slices
// 86.7 ms).  Slice k = [cut[k], cut[k + 1]); one slice ({0, n}) for batches, small n, host_chunks = 1, a shape that is refused or more than 8 GiB of bucket sets.
// shape: the plan of the biggest slice, whose (c, shared) every slice takes and whose tail runs once over the folded sets.
struct HostSlices { std::vector<uint64_t> cut; PassPlan shape; uint32_t count() const { return (uint32_t)cut.size() - 1; } };
inline HostSlices host_slices(const PlanIn &in, uint64_t n, uint32_t M, TableShape tab, MsmGroup grp) {
  HostSlices hs; std::vector<uint64_t> &cut = hs.cut;
  if (M == 1 && n >= (1ull << in.k.host_slice_min_log) && in.k.host_chunks > 1) {
    double w = 1.0, tot = 0; std::vector<double> ws;
    const double first = 1.0 / 16.0;
    for (double rem = 1.0; rem > 1e-9 && ws.size() + 1 < in.k.host_chunks;) { const double take = std::min(rem, first * w); ws.push_back(take); rem -= take; w *= 1.7; tot += take; }
    if (tot < 1.0 - 1e-9) ws.push_back(1.0 - tot);
    cut.push_back(0); double acc = 0;
    const uint64_t align = n >= (1ull << 20) ? ~1023ull : ~0ull;
    for (size_t i = 0; i + 1 < ws.size(); i++) { acc += ws[i]; const uint64_t c = std::min<uint64_t>(n, (uint64_t)(acc * (double)n) & align); if (c > cut.back() && c < n) cut.push_back(c); }
    cut.push_back(n);
  }
  if (cut.size() > 2) {
    uint64_t biggest = 0; for (size_t k = 0; k + 1 < cut.size(); k++) biggest = std::max(biggest, cut[k + 1] - cut[k]);
    hs.shape = plan_pass(in, biggest, 1, tab, grp);
    if (hs.shape.ok() && hs.shape.nbuckets * hs.count() * grp.rec_bytes <= (8ull << 30)) return hs;
  }
  cut = {0, n};
  return hs;
}

}  // namespace mi355zk
