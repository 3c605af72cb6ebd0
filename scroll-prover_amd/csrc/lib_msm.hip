// lib_msm.hip -- libmi355zk.so, the MSM translation unit: launch orchestration of msm.hpp (digits -> two-level LDS counting sort ->
// segmented accumulation -> fix-up -> reduction tail), the host-pointer and sharded (multi-device) schedules, the C-ABI entry points
// mi355_msm_* / mi355_g1_sum_*, and the SRS entry points that launch kernels of msm.hpp (params-file loader with on-device validation,
// window-table build, synthetic SRS).  Host logic only; all arithmetic runs in the kernels.
// Three layers, each written once for G1 and G2:
//   plan    msm_plan.hpp (plain C++, tested on the CPU) decides everything about a pass before the device is touched; plan_in() below is the one place its inputs are read
//   pass    msm_pass<H>(PassPlan, PassArgs): workspace -> msm_sort_stage -> accumulate -> fix-up -> msm_reduce_tail; they read the plan and derive nothing
//   driver  msm_run<H> (prologue, the run record, host staging) -> msm_batch<H> (split in halves, schedule: one pass | pipelined chunks | host slices, delivery)
// H is the host-side policy (G1Pass / G2Pass: kernel policy of msm.hpp / msm_g2.hpp, base type, span and trace names, the accumulate launch).
// kernel headers first: lib_common.hpp defines the macro `g` (the calling thread's device context), a name the kernels use for locals
#define ZK_FRSCAN_DEVICE_ONLY 1   // msm.hpp needs the block scans of frscan.hpp, not its kernels (those belong to lib_aux.hip)
#include "msm.hpp"
#define ZK_G2_DEVICE_ONLY 1      // msm_g2.hpp needs the twist arithmetic of g2.hpp, not k_g2_mul (that kernel belongs to lib_aux.hip)
#include "msm_g2.hpp"
#include "msm_seg.hpp"           // after msm.hpp: the kernel loads its operands with load_affine
#include "lib_common.hpp"

namespace mi355 {
using mi355zk::Fixup; using mi355zk::PassPlan; using mi355zk::PlanIn; using mi355zk::TableShape;

static_assert(sizeof(fe_t) == 32 && sizeof(g1_affine_t) == 64 && sizeof(g1_jac_t) == 96, "ABI element sizes");
static_assert(sizeof(g1_xyzz_t) == 128 && sizeof(g1_xyzz29_t) == 144, "device record sizes (workspace layout, 16-byte vector accesses)");
static_assert(sizeof(g1_xyzz29_t) == mi355zk::GROUP_G1.rec_bytes && sizeof(g2_xyzz_t) == mi355zk::GROUP_G2.rec_bytes, "the planner's record sizes");

int msm_tu_init_device() {
  HIPCHK(hipFuncSetAttribute((const void *)k_sort_l1_scatter_split<24>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)k_sort_l1_scatter_split<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)k_sort_l1_scatter_split<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)k_sort_l2_scatter_split<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)k_sort_l2_scatter_split<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return MI355_OK;
}

// ------------------------------------------------------------------------------------------------ MSM: the pass
// what msm_plan.hpp plans from: the bound slot's knobs, the process's widest automatic window, the calling thread's options, the device's CU count
static PlanIn plan_in() {
  PlanIn in; in.k = static_cast<const mi355zk::Knobs &>(g); in.auto_max_c = g_proc.msm_auto_max_c; in.chunk_min_log = g.msm_chunk_min_log;
  in.force_c = t_opts.force_c; in.no_tables = t_opts.no_tables; in.cus = (uint32_t)g.prop.multiProcessorCount;
  return in;
}

struct PreTable { const g1_affine_t *table = nullptr; uint64_t row_stride = 0; int c = 0, w = 0; };   // table already offset to the slice start
static TableShape tab_of(const PreTable *pre) { return pre && pre->table ? TableShape{pre->c, pre->w} : TableShape{}; }
// the same tables for a point range that starts `lo` points further on (slices of a chunked MSM); null stays null
const PreTable *pre_advance(const PreTable *pre, uint64_t lo, PreTable &store) {
  if (!pre) return nullptr;
  store = *pre; if (store.table) store.table += lo;
  return &store;
}

// workspace roles of one pass: the policy's prefix ("msm." / "msm2."), the buffer's name, "#slot" for the second slot of a pipelined MSM
struct Roles {
  const char *prefix; std::string sfx;
  template <class T> int get(const char *name, size_t bytes, T *&ptr) const { return ws_get((std::string(prefix) + name + sfx).c_str(), bytes, (void **)&ptr); }
};

// One MSM pass is enqueued on three streams: a digits + sort (HBM-bound), b bucket accumulation (ALU-bound), c fix-up + bucket reduction
// (latency-bound).  With a == b == c this is the plain serial schedule.
struct MsmStreams { hipStream_t a, b, c; };
struct SpanNames { const char *total, *digits, *sort, *l1, *hist, *l2, *accumulate, *fixup, *tail; };   // tail = null: the fix-up's span covers the tail as well

// What one pass works on.  M commitments over the same basis slice run in one pass: (polynomial m, window w) is window m * W + w of one big bucket problem, so the
// per-call fixed costs (launches, the latency-bound reduction tail) are paid once per batch.
template <class H> struct PassArgs {
  const typename H::base_t *bases; uint64_t row_stride;   // row_stride != 0: `bases` is a window table T[w][i] with rows this many points apart (a plan with pl.shared)
  PolyPtrs inl; const fe_t *const *polys_dev;             // the M scalar vectors (msm_stage_polys)
  typename H::Ops::out_t *out;                            // device: M results
  MsmSlot *slot; MsmStreams st;
  uint32_t set_index = 0, set_count = 1;                  // this pass fills bucket set `set_index` of `set_count` (each nbuckets records)
  bool skip_tail = false;                                 // stop after the fix-up (the caller folds the sets and runs msm_reduce_tail once)
  bool normalise = true;
};

// The host side of a group: the kernel policy, the planner's view of it, names, and the one launch whose signature is group-specific.
struct G1Pass {
  using Ops = G1Ops; using base_t = g1_affine_t;
  static constexpr mi355zk::MsmGroup GROUP = mi355zk::GROUP_G1;
  static constexpr bool FOLD = true, G1_SCHEDULES = true;   // k and r - k are the same term up to the sign of the point; window tables, pipelined chunks, host slices
  static constexpr SpanNames SPAN{"msm_total", "msm_digits", "msm_sort", "sort_l1", "sort_hist", "sort_l2", "msm_accumulate", "msm_reduce", nullptr};
  static constexpr const char *TRACE = "msm_g1", *N_LIMIT = "msm: n must be < 2^31"; static constexpr double TRACE_BYTES = 96.0;
  static void accumulate(const PassPlan &pl, const PassArgs<G1Pass> &a, const uint32_t *sorted, const uint32_t *offsets, g1_xyzz29_t *buckets, g1_xyzz29_t *part, int32_t *part_id, hipStream_t s) {
    hipLaunchKernelGGL(k_msm_accumulate, dim3(pl.blocks), dim3(256), 0, s, a.bases, sorted, offsets, (uint32_t)pl.nbuckets, buckets, part, part_id, pl.seg_arg, log2_ceil(pl.n), a.row_stride);
  }
};
struct G2Pass {   // no window tables, slots or bucket sets; a twist point need not have order r (k_msm_g2_validate checks the curve equation only), so no folding of k
  using Ops = G2Ops; using base_t = g2_affine_t;
  static constexpr mi355zk::MsmGroup GROUP = mi355zk::GROUP_G2;
  static constexpr bool FOLD = false, G1_SCHEDULES = false;
  static constexpr SpanNames SPAN{"msm_g2_total", "msm_g2_digits", "msm_g2_sort", "g2_sort_l1", "g2_sort_hist", "g2_sort_l2", "msm_g2_accumulate", "msm_g2_fixup", "msm_g2_reduce"};
  static constexpr const char *TRACE = "msm_g2", *N_LIMIT = "msm_g2: n must be < 2^31"; static constexpr double TRACE_BYTES = 160.0;
  static void accumulate(const PassPlan &pl, const PassArgs<G2Pass> &a, const uint32_t *sorted, const uint32_t *offsets, g2_xyzz_t *buckets, g2_xyzz_t *part, int32_t *part_id, hipStream_t s) {
    hipLaunchKernelGGL(k_msm_g2_accumulate, dim3(pl.blocks), dim3(256), 0, s, a.bases, sorted, offsets, (uint32_t)pl.nbuckets, buckets, part, part_id, pl.seg_arg);
  }
};

// the bases of a G1 pass: the window table (rows row_stride points apart) where the plan shares one bucket set, else the points from `lo` on
static void g1_bases(PassArgs<G1Pass> &a, const PassPlan &pl, const g1_affine_t *bases, const PreTable *pre) {
  if (pl.shared) { a.bases = pre->table; a.row_stride = pre->row_stride; } else { a.bases = bases; a.row_stride = 0; }
}

// up to 8 polynomial pointers travel in the kernel argument; a longer array is staged through a buffer the library owns (the caller's
// array may be a temporary)
int msm_stage_polys(const fe_t *const *polys_host, uint32_t M, const Roles &ws, hipStream_t s, PolyPtrs &inl, const fe_t **&polys_dev) {
  if (M <= 8) { for (uint32_t m = 0; m < M; m++) inl.p[m] = polys_host[m]; return MI355_OK; }
  CHK(ws.get("polys", (size_t)M * sizeof(void *), polys_dev));
  g.polys_stage.assign(polys_host, polys_host + M);
  HIPCHK(hipMemcpyAsync(polys_dev, g.polys_stage.data(), (size_t)M * sizeof(void *), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return MI355_OK;
}

// launch(std::integral_constant<int, Q>): Q = 4 (a quad per logical thread, the latency form) where the plan asks for it and the policy
// has it, else Q = 1 (one lane per logical thread, the throughput form)
template <class G, class F> void with_lanes(bool quad, F &&launch) {
  if constexpr (G::QUAD) { if (quad) { launch(std::integral_constant<int, 4>{}); return; } }
  launch(std::integral_constant<int, 1>{});
}

// Stage A of one MSM pass: digits -> two-level counting sort of (window, bucket) keys.  It never looks at a point, so the G1 and the G2
// MSM share it (and its msm.* buffers: the sort stages of successive chunks run one after the other on one stream).  Out: offsets[nbuckets + 1]
// (exclusive bucket starts) and sorted[emax] (point index | sign << 31, grouped by bucket; with window tables the payload names a table row, see SortPlan::nshift).
template <class H> int msm_sort_stage(const PassPlan &pl, const MsmPlan &P, const PolyPtrs &inl, const fe_t *const *polys_dev, uint32_t *offsets, uint32_t *sorted, hipStream_t s) {
  const uint64_t emax = pl.emax;
  const uint32_t nbuckets = (uint32_t)pl.nbuckets, M = pl.M;
  // sort plan: fine bits fb (<= 12, LDS histogram of 2^fb bins), coarse bits = the rest
  SortPlan S; S.n = P.n; S.windows = M * P.windows; S.wpp = P.windows; S.nb = P.nb;
  S.fb = pl.fb; S.cb_bits = pl.cb_bits;
  S.shared = pl.shared ? 1 : 0; S.nshift = log2_ceil(pl.n);
  S.regions = pl.regions; S.t1 = pl.t1; S.t2 = pl.t2;
  const uint32_t tiles1 = pl.tiles1, l2_tiles_max = pl.l2_tiles_max;
  const uint32_t vwindows = M * P.windows;   // (polynomial, window) pairs

  uint32_t *enc, *hist, *cursor, *scan_sums, *coarse_hist, *coarse_off, *coarse_cursor, *tile_start;
  CHK(ws_get("msm.digits", emax * 4, (void **)&enc));
  uint32_t *pairs_lo = nullptr; uint16_t *pairs_hi = nullptr;
  CHK(ws_get("msm.pairs_lo", emax * 4 + 64, (void **)&pairs_lo)); CHK(ws_get("msm.pairs_hi", emax * 2 + 64, (void **)&pairs_hi));
  CHK(ws_get("msm.hist", ((size_t)nbuckets + 1) * 4, (void **)&hist));
  CHK(ws_get("msm.cursor", ((size_t)nbuckets + 1) * 4, (void **)&cursor));
  CHK(ws_get("msm.coarse_hist", ((size_t)S.regions + 1) * 4, (void **)&coarse_hist));
  CHK(ws_get("msm.coarse_off", ((size_t)S.regions + 1) * 4, (void **)&coarse_off));
  CHK(ws_get("msm.coarse_cursor", ((size_t)S.regions + 1) * 4, (void **)&coarse_cursor));
  CHK(ws_get("msm.tile_start", ((size_t)S.regions + 1) * 4, (void **)&tile_start));
  const uint32_t scan_n = nbuckets + 1, scan_blocks = ceil_div(scan_n, SCAN_BLOCK * SCAN_ITEMS);
  const uint32_t cscan_n = S.regions + 1, cscan_blocks = ceil_div(cscan_n, SCAN_BLOCK * SCAN_ITEMS);
  CHK(ws_get("msm.scan_sums", (size_t)(scan_blocks + cscan_blocks) * 4, (void **)&scan_sums));
  const int grid_stream = g.prop.multiProcessorCount * 8;
  {
    Scope sc(H::SPAN.digits, s);
    HIPCHK(hipMemsetAsync(coarse_hist, 0, ((size_t)S.regions + 1) * 4, s));
    const dim3 dgrid(grid_stream / M > 0 ? grid_stream / M : 1, M);
    hipLaunchKernelGGL(k_msm_digits<H::FOLD>, dgrid, dim3(256), (size_t)S.regions * 4, s, inl, polys_dev, enc, P, coarse_hist, S.fb, S.cb_bits, S.shared);
  }
  {
    Scope sc(H::SPAN.sort, s);
    HIPCHK(hipMemsetAsync(hist, 0, ((size_t)nbuckets + 1) * 4, s));
    hipLaunchKernelGGL(k_scan_partial, dim3(cscan_blocks), dim3(SCAN_BLOCK), 0, s, coarse_hist, scan_sums + scan_blocks, cscan_n);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(SCAN_BLOCK), 0, s, scan_sums + scan_blocks, cscan_blocks);
    hipLaunchKernelGGL(k_scan_final, dim3(cscan_blocks), dim3(SCAN_BLOCK), 0, s, coarse_hist, scan_sums + scan_blocks, coarse_off, coarse_cursor, cscan_n);
    {
      Scope s1(H::SPAN.l1, s);
      const uint32_t CBp = ((1u << S.cb_bits) + 1) & ~1u;
      const size_t lds1 = (size_t)(3 * CBp + 32 + SORT_SPLIT_TMAX) * 4 + (size_t)S.t1 * 6;
      if (S.t1 == 24576) hipLaunchKernelGGL(k_sort_l1_scatter_split<24>, dim3(tiles1 * vwindows), dim3(1024), lds1, s, enc, coarse_cursor, pairs_lo, pairs_hi, S);
      else if (S.t1 == 16384) hipLaunchKernelGGL(k_sort_l1_scatter_split<16>, dim3(tiles1 * vwindows), dim3(1024), lds1, s, enc, coarse_cursor, pairs_lo, pairs_hi, S);
      else hipLaunchKernelGGL(k_sort_l1_scatter_split<8>, dim3(tiles1 * vwindows), dim3(1024), lds1, s, enc, coarse_cursor, pairs_lo, pairs_hi, S);
    }
    hipLaunchKernelGGL(k_sort_tile_prefix, dim3(1), dim3(SCAN_BLOCK), 0, s, coarse_off, tile_start, S);
    { Scope s2(H::SPAN.hist, s);
    hipLaunchKernelGGL(k_sort_l2_hist_split, dim3(l2_tiles_max), dim3(256), 0, s, (const uint16_t *)pairs_hi, coarse_off, tile_start, hist, S); }
    hipLaunchKernelGGL(k_scan_partial, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, s, hist, scan_sums, scan_n);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(SCAN_BLOCK), 0, s, scan_sums, scan_blocks);
    hipLaunchKernelGGL(k_scan_final, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, s, hist, scan_sums, offsets, cursor, scan_n);
    {
      Scope s3(H::SPAN.l2, s);
      const size_t lds2 = (size_t)(3 * (1u << S.fb) + 32) * 4 + (size_t)S.t2 * 6;   // histogram / offsets / bases + staged indices (4 B) and their bins (2 B)
      if (S.t2 == 8192) hipLaunchKernelGGL(k_sort_l2_scatter_split<8>, dim3(l2_tiles_max), dim3(1024), lds2, s, (const uint32_t *)pairs_lo, (const uint16_t *)pairs_hi, coarse_off, tile_start, cursor, sorted, S);
      else hipLaunchKernelGGL(k_sort_l2_scatter_split<16>, dim3(l2_tiles_max), dim3(1024), lds2, s, (const uint32_t *)pairs_lo, (const uint16_t *)pairs_hi, coarse_off, tile_start, cursor, sorted, S);
    }
  }
  return MI355_OK;
}

// The fix-up of straddling buckets as ONE segmented reduction over the 2 * tn partial slots of the accumulate threads, level by level
// (64 slots -> 2 per level) until one wavefront holds the rest.
template <class G> int msm_segfix_levels(const int32_t *part_id, const typename G::rec_t *part, uint32_t tn, typename G::rec_t *buckets, hipStream_t s, const Roles &ws) {
  using rec_t = typename G::rec_t;
  uint32_t N = 2 * tn; const uint32_t waves1 = ceil_div(N, 64);
  const size_t cap = (size_t)2 * waves1 + (size_t)waves1 / 8 + 512;
  int32_t *lv_ids; rec_t *lv_recs;
  CHK(ws.get("segfix_ids", cap * 4, lv_ids)); CHK(ws.get("segfix_recs", cap * sizeof(rec_t), lv_recs));
  const int32_t *cur_ids = part_id; const rec_t *cur_recs = part; size_t used = 0;
  while (N > 64) {
    const uint32_t waves = ceil_div(N, 64);
    hipLaunchKernelGGL(k_msm_segfix<G>, dim3(ceil_div(N, 256)), dim3(256), 0, s, cur_ids, cur_recs, N, buckets, lv_ids + used, lv_recs + used, 0);
    cur_ids = lv_ids + used; cur_recs = lv_recs + used; used += (size_t)2 * waves; N = 2 * waves;
  }
  hipLaunchKernelGGL(k_msm_segfix<G>, dim3(1), dim3(64), 0, s, cur_ids, cur_recs, N, buckets, (int32_t *)nullptr, (rec_t *)nullptr, 1);
  return MI355_OK;
}

// The per-bucket fix-up (G1 only): k_msm_fixup in the plan's form lists the buckets whose span is too long for it; a workgroup per listed bucket, and FIXUP_SLICES
// workgroups per giant one, sum those.
struct FixupLists {
  uint32_t *big_list, *big_count, *huge_list, *huge_count; g1_xyzz29_t *huge_part;
  int get(const PassPlan &pl, const Roles &ws) {
    CHK(ws.get("big_list", ((size_t)pl.big_cap * 3 + 1) * 4, big_list)); big_count = big_list + (size_t)pl.big_cap * 3;
    CHK(ws.get("huge_list", ((size_t)pl.huge_cap * 3 + 1) * 4, huge_list)); huge_count = huge_list + (size_t)pl.huge_cap * 3;
    return ws.get("huge_part", (size_t)pl.huge_cap * FIXUP_SLICES * sizeof(g1_xyzz29_t), huge_part);
  }
};
static void msm_fixup_per_bucket(const PassPlan &pl, const FixupLists &fl, const uint32_t *offsets, g1_xyzz29_t *buckets, g1_xyzz29_t *part, int32_t *part_id, hipStream_t s) {
  const uint32_t nbuckets = (uint32_t)pl.nbuckets;
  auto fixup = [&](auto kernel, uint64_t threads) {
    hipLaunchKernelGGL(kernel, dim3(ceil_div(threads, 256)), dim3(256), 0, s, offsets, nbuckets, buckets, part, part_id, pl.seg_arg, pl.tn, fl.big_list, fl.big_count, pl.big_cap, fl.huge_list, fl.huge_count, pl.huge_cap, pl.serial_max, pl.huge_min);
  };
  if (pl.fixup == Fixup::Quad) fixup(k_msm_fixup<4, 4>, (uint64_t)nbuckets * 16);
  else if (pl.fixup == Fixup::FourLanes) fixup(k_msm_fixup<4, 1>, (uint64_t)nbuckets * 4);
  else fixup(k_msm_fixup<1, 1>, nbuckets);
  hipLaunchKernelGGL(k_msm_fixup_big, dim3(pl.big_cap), dim3(256), 0, s, buckets, part, part_id, fl.big_list, fl.big_count);
  hipLaunchKernelGGL(k_msm_fixup_huge, dim3(pl.huge_cap * FIXUP_SLICES), dim3(256), 0, s, part, part_id, fl.huge_list, fl.huge_count, fl.huge_part, pl.huge_cap);
  hipLaunchKernelGGL(k_msm_fixup_huge_fold, dim3(pl.huge_cap), dim3(64), 0, s, buckets, fl.huge_list, fl.huge_count, (const g1_xyzz29_t *)fl.huge_part);
}

// The reduction tail of one MSM pass: sum_b (b + 1) B[b] per bucket set by short chunked running sums, a multi-block tree per set, the
// Horner over windows (none with window tables) and the result in the caller's form (G1: Jacobian, normalised on request; G2: affine).
template <class G> int msm_reduce_tail(const PassPlan &pl, const typename G::rec_t *buckets, typename G::out_t *out_dev, bool normalise, hipStream_t s, const Roles &ws) {
  using rec_t = typename G::rec_t;
  const uint32_t nb = 1u << (pl.c - 1), wpp = pl.wpp(), sets = pl.sets(), chunks_per_set = pl.chunks_per_set, nchunks = chunks_per_set * sets;
  rec_t *chunk_out, *tree_a, *tree_b, *window_sums;
  CHK(ws.get("chunk_out", (size_t)nchunks * sizeof(rec_t), chunk_out));
  { const size_t lvl = (size_t)ceil_div(chunks_per_set, 64 * TREE_PER_THREAD) * sets + 1;   // 64: the quad form's logical threads per block (an upper bound for the one-lane form)
    CHK(ws.get("tree_a", lvl * sizeof(rec_t), tree_a)); CHK(ws.get("tree_b", lvl * sizeof(rec_t), tree_b)); }
  CHK(ws.get("window_sums", (size_t)sets * sizeof(rec_t), window_sums));
  with_lanes<G>(pl.quad_sums, [&](auto q) {
    constexpr int Q = decltype(q)::value;
    hipLaunchKernelGGL((k_msm_bucket_reduce<G, Q>), dim3(ceil_div((uint64_t)nchunks * Q, 128)), dim3(128), 0, s, buckets, chunk_out, nb, sets, pl.chunk);
  });
  // tree-sum the chunk results per set, ping-ponging between two small buffers
  const rec_t *cur = chunk_out; uint32_t cnt = chunks_per_set; rec_t *bufs[2] = {tree_a, tree_b}; int which = 0;
  while (true) {
    const bool coop = G::QUAD && pl.tree_quad(cnt);
    const uint32_t outn = ceil_div(cnt, (coop ? 64u : 256u) * TREE_PER_THREAD);
    rec_t *dst = outn == 1 ? window_sums : bufs[which];
    with_lanes<G>(coop, [&](auto q) { hipLaunchKernelGGL((k_msm_tree_sum<G, decltype(q)::value>), dim3(outn, sets), dim3(256), 0, s, cur, cnt, dst, outn); });
    if (outn == 1) break;
    cur = dst; cnt = outn; which ^= 1;
  }
  with_lanes<G>(pl.quad_final, [&](auto q) {
    hipLaunchKernelGGL((k_msm_final<G, decltype(q)::value>), dim3(pl.M), dim3(64), 0, s, (const rec_t *)window_sums, wpp, pl.shared ? 0u : pl.c, out_dev, normalise ? 1 : 0);
  });
  HIPCHK(hipGetLastError());
  return MI355_OK;
}

// One pass of the plan, for either group.  A pipelined MSM (st.a != st.b) alternates two slots: a slot's buffers are reused only after the events of the chunk that
// used it before.  The whole tail runs on the group's bucket records (G1: the 29-bit field, never converted to the saturated form on the way).
template <class H> int msm_pass(const PassPlan &pl, const PassArgs<H> &a) {
  using G = typename H::Ops; using rec_t = typename G::rec_t;
  if (!pl.ok()) return fail(MI355_EBADARG, pl.refusal);
  MsmSlot &slot = *a.slot; const MsmStreams &st = a.st;
  const bool piped = st.a != st.b;
  const Roles ws{G::ROLE, slot.id ? "#" + std::to_string(slot.id) : std::string()};
  const uint32_t nbuckets = (uint32_t)pl.nbuckets, tn = pl.tn;
  MsmPlan P; P.n = (uint32_t)pl.n; P.c = pl.c; P.windows = pl.W; P.nb = 1u << (pl.c - 1); P.seg = pl.seg; P.batch = pl.M;
  uint32_t *offsets, *sorted; rec_t *buckets, *part; int32_t *part_id;
  // per-slot: what the accumulation and the reduction of this chunk read while the next chunk is being sorted
  CHK(ws.get("offsets", ((size_t)nbuckets + 1) * 4, offsets));
  CHK(ws.get("sorted", pl.emax * 4, sorted));
  CHK(ws.get("buckets", (size_t)nbuckets * a.set_count * sizeof(rec_t), buckets));
  buckets += (size_t)nbuckets * a.set_index;
  CHK(ws.get("part", (size_t)tn * 2 * sizeof(rec_t), part));
  CHK(ws.get("part_id", (size_t)tn * 2 * 4, part_id));
  constexpr bool PER_BUCKET = !H::GROUP.always_segmented;   // the group has the per-bucket fix-up kernels
  FixupLists fl{};
  if constexpr (PER_BUCKET) CHK(fl.get(pl, ws));
  {
    hipStream_t s = st.a;
    // the accumulation and the fix-up of the chunk that used this slot before must be done with `sorted` / `offsets`
    if (piped && slot.used) { HIPCHK(hipStreamWaitEvent(s, slot.acc_done, 0)); HIPCHK(hipStreamWaitEvent(s, slot.red_done, 0)); }
    CHK(msm_sort_stage<H>(pl, P, a.inl, a.polys_dev, offsets, sorted, s));
    if (piped) { HIPCHK(hipEventRecord(slot.sorted, s)); HIPCHK(hipStreamWaitEvent(st.b, slot.sorted, 0)); }
  }
  {
    hipStream_t s = st.b;
    // the reduction of the chunk that used this slot before must be done with `buckets` / `part`
    if (piped && slot.used) HIPCHK(hipStreamWaitEvent(s, slot.red_done, 0));
    {
      Scope sc(H::SPAN.accumulate, s);
      HIPCHK(hipMemsetAsync(buckets, 0, (size_t)nbuckets * sizeof(rec_t), s));   // all zero = the XYZZ identity: empty buckets
      H::accumulate(pl, a, sorted, offsets, buckets, part, part_id, s);
    }
    if (piped) { HIPCHK(hipEventRecord(slot.acc_done, s)); HIPCHK(hipStreamWaitEvent(st.c, slot.acc_done, 0)); }
  }
  {
    hipStream_t s = st.c;
    Scope sc(H::SPAN.fixup, s);
    if constexpr (PER_BUCKET) { HIPCHK(hipMemsetAsync(fl.big_count, 0, 4, s)); HIPCHK(hipMemsetAsync(fl.huge_count, 0, 4, s)); }
    if (pl.fixup == Fixup::Segmented) CHK(msm_segfix_levels<G>(part_id, part, tn, buckets, s, ws));
    else if constexpr (PER_BUCKET) msm_fixup_per_bucket(pl, fl, offsets, buckets, part, part_id, s);
    if (!a.skip_tail) {
      if (H::SPAN.tail) { sc.close(); Scope tail(H::SPAN.tail, s); CHK(msm_reduce_tail<G>(pl, buckets, a.out, a.normalise, s, ws)); }
      else CHK(msm_reduce_tail<G>(pl, buckets, a.out, a.normalise, s, ws));
    }
  }
  if (piped) HIPCHK(hipEventRecord(slot.red_done, st.c));
  slot.used = true;
  HIPCHK(hipGetLastError());
  g.run.c = (int)pl.c; g.run.windows = (int)pl.W; g.run.entries += pl.emax; g.run.shared = pl.shared;
  return MI355_OK;
}

// ------------------------------------------------------------------------------------------------ MSM: the driver
// The M results of a finished schedule go to the caller: into device memory in stream order (the call returns without waiting), or into
// host memory once the stream has drained.  what / count: the trace line's "<what>=<count>".
template <class out_t> int msm_deliver(CallTrace &tr, const out_t *out_dev, uint32_t M, void *out_host, void *out_dev_user, hipStream_t s, const char *what, uint32_t count) {
  if (out_dev_user) {   // asynchronous: the caller's stream order protects the result
    HIPCHK(hipMemcpyAsync(out_dev_user, out_dev, (size_t)M * sizeof(out_t), hipMemcpyDeviceToDevice, s));
    if (g.profiling) resolve_spans();
    tr.done(" (device result)");
    return MI355_OK;
  }
  HIPCHK(hipMemcpyAsync(out_host, out_dev, (size_t)M * sizeof(out_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  resolve_spans();
  { char buf[64]; snprintf(buf, sizeof buf, " %s=%u c=%d W=%d", what, count, g.run.c, g.run.windows); tr.done(buf); }
  return MI355_OK;
}

// Chunks of a pipelined G1 MSM: the point range is cut into K slices, every slice is a complete MSM over its part of the basis (and of the
// window tables) with a plan of its own, and the memory-bound sort of slice k + 1 runs under the ALU-bound accumulation of slice k; the K partial
// results (out_dev + M ...) are added at the end.  OFF by default (MI355_MSM_CHUNKS / mi355_msm_set_pipeline): on MI355X the accumulation holds every wave slot
// for its whole run, so the sort of the next slice barely progresses next to it -- measured 74.9 ms (1 chunk), 75.6 (2), 80.2 (4), 91.1 (8) at 2^26.
static int msm_pipelined(const PlanIn &in, const g1_affine_t *bases, const fe_t *const *polys, uint32_t M, uint64_t n, uint32_t K, g1_jac_t *out_dev, const PreTable *pre, hipStream_t s) {
  // the side streams start after everything already queued on the caller's stream (the scalars may still be in flight there)
  HIPCHK(hipEventRecord(g.ev_fork, s));
  HIPCHK(hipStreamWaitEvent(g.aux_stream[0], g.ev_fork, 0)); HIPCHK(hipStreamWaitEvent(g.aux_stream[1], g.ev_fork, 0));
  const MsmStreams st{g.aux_stream[0], s, g.aux_stream[1]};
  for (uint32_t k = 0; k < K; k++) {
    const uint64_t lo = n * k / K, hi = n * (k + 1) / K;
    PreTable pk; const PreTable *pp = pre_advance(pre, lo, pk);
    const PassPlan pl = plan_pass(in, hi - lo, M, tab_of(pp), G1Pass::GROUP);
    PassArgs<G1Pass> a{nullptr, 0, {}, nullptr, out_dev + (size_t)(k + 1) * M, &g.msm_slot[k & 1], st};
    g1_bases(a, pl, bases + lo, pp);
    a.inl.p[0] = polys[0] + lo;   // pipelined MSMs are single-polynomial (pipeline_chunks)
    a.normalise = false;
    CHK(msm_pass<G1Pass>(pl, a));
  }
  HIPCHK(hipStreamWaitEvent(s, g.msm_slot[0].red_done, 0)); HIPCHK(hipStreamWaitEvent(s, g.msm_slot[1].red_done, 0));
  HIPCHK(hipEventRecord(g.ev_fork, st.a)); HIPCHK(hipStreamWaitEvent(s, g.ev_fork, 0));   // join the sort stream too
  hipLaunchKernelGGL(k_g1_sum_strided, dim3(M), dim3(64), 0, s, out_dev + M, K, M, out_dev, t_opts.normalise ? 1 : 0);
  return MI355_OK;
}

// M MSMs over one basis in device memory, scalars in device memory; the results go to out_host, or with out_dev_user stay in device memory (the call then returns
// without waiting for the stream).  A batch the plan says must split runs as two half batches; else one pass, or for G1 the pipelined chunks.
template <class H> int msm_batch(const typename H::base_t *bases, const fe_t *const *polys, uint32_t M, uint64_t n, void *out_host, const PreTable *pre, void *out_dev_user) {
  using G = typename H::Ops; using out_t = typename G::out_t;
  const PlanIn in = plan_in();
  const PassPlan pl = plan_pass(in, n, M, tab_of(pre), H::GROUP);
  if (M > 1 && mi355zk::must_split(pl, H::GROUP)) {
    const uint32_t h = M / 2;
    CHK(msm_batch<H>(bases, polys, h, n, out_host, pre, out_dev_user));
    return msm_batch<H>(bases, polys + h, M - h, n, out_host ? (char *)out_host + (size_t)h * sizeof(out_t) : nullptr, pre,
                        out_dev_user ? (char *)out_dev_user + (size_t)h * sizeof(out_t) : nullptr);
  }
  uint32_t K = 1;
  if constexpr (H::G1_SCHEDULES) K = mi355zk::pipeline_chunks(in, M, n);
  CallTrace tr(H::TRACE, (uint64_t)M * n, H::TRACE_BYTES);
  const Roles ws{G::ROLE, ""};
  out_t *out_dev; CHK(ws.get("out", (size_t)(K + 1) * M * sizeof(out_t), out_dev));
  hipStream_t s = g.stream;
  Scope total(H::SPAN.total, s);
  if (K == 1) {
    PassArgs<H> a{bases, 0, {}, nullptr, out_dev, &g.msm_slot[0], {s, s, s}};
    if constexpr (H::G1_SCHEDULES) g1_bases(a, pl, bases, pre);
    const fe_t **polys_dev = nullptr;
    CHK(msm_stage_polys(polys, M, ws, s, a.inl, polys_dev)); a.polys_dev = polys_dev;
    a.normalise = t_opts.normalise;
    CHK(msm_pass<H>(pl, a));
  } else if constexpr (H::G1_SCHEDULES) CHK(msm_pipelined(in, bases, polys, M, n, K, out_dev, pre, s));
  HIPCHK(hipGetLastError());
  total.close();
  g.msm_slot[0].used = g.msm_slot[1].used = false;
  return msm_deliver(tr, out_dev, M, out_host, out_dev_user, s, "batch", M);
}

// Host slices of a big single G1 MSM (mi355zk::host_slices): slice k + 1 crosses PCIe on the copy stream while slice k is sorted and accumulated; every slice fills its
// OWN bucket set with the common layout (c, W, table rows) of hs.shape, the K sets are added bucket by bucket and the latency-bound reduction tail runs once.  (The
// pipelined device-resident schedule above pays a tail per slice; here the slices only differ from the one-pass MSM by K - 1 extra bucket records per bucket.)
static int msm_host_sliced(const PlanIn &in, const mi355zk::HostSlices &hs, const g1_affine_t *bases, const fe_t *scalars_host, fe_t *sc, uint64_t n, void *out_host, const PreTable *pre, void *out_dev_user) {
  const uint32_t K = hs.count();
  const mi355zk::ForcedShape forced{hs.shape.c, hs.shape.shared};
  hipStream_t s = g.stream;
  CallTrace tr("msm_g1_host", n, 96.0);
  g1_jac_t *out_dev; CHK(ws_get("msm.out", 2 * sizeof(g1_jac_t), (void **)&out_dev));
  Scope total("msm_total", s);
  // the staging buffer may still be read by work queued earlier on the compute stream
  HIPCHK(hipEventRecord(g.ev_fork, s)); HIPCHK(hipStreamWaitEvent(g.copy_stream, g.ev_fork, 0));
  for (uint32_t k = 0; k < K; k++) {
    const uint64_t lo = hs.cut[k], hi = hs.cut[k + 1];
    // pageable source: the call blocks this thread while the DMA runs, which is exactly when the GPU works on the slices queued before
    HIPCHK(hipMemcpyAsync(sc + lo, scalars_host + lo, (hi - lo) * sizeof(fe_t), hipMemcpyHostToDevice, g.copy_stream));
    HIPCHK(hipEventRecord(g.ev_copy[k & 3], g.copy_stream));
    HIPCHK(hipStreamWaitEvent(s, g.ev_copy[k & 3], 0));
    PreTable pk; const PreTable *pp = pre_advance(pre, lo, pk);
    const PassPlan pl = plan_pass(in, hi - lo, 1, tab_of(pp), G1Pass::GROUP, &forced);
    PassArgs<G1Pass> a{nullptr, 0, {}, nullptr, out_dev, &g.msm_slot[0], {s, s, s}, k, K, true};
    g1_bases(a, pl, bases + lo, pp);
    a.inl.p[0] = sc + lo;
    CHK(msm_pass<G1Pass>(pl, a));
  }
  g.msm_slot[0].used = false;
  const Roles ws{G1Ops::ROLE, ""};
  g1_xyzz29_t *buckets; CHK(ws.get("buckets", (size_t)hs.shape.nbuckets * K * sizeof(g1_xyzz29_t), buckets));
  {
    Scope sc2("msm_reduce", s);
    hipLaunchKernelGGL(k_msm_bucket_fold, dim3(ceil_div(hs.shape.nbuckets, 256)), dim3(256), 0, s, buckets, (uint32_t)hs.shape.nbuckets, K);
    CHK(msm_reduce_tail<G1Ops>(hs.shape, buckets, out_dev, t_opts.normalise, s, ws));
  }
  total.close();
  g.run.host_slices = (int)K;
  return msm_deliver(tr, out_dev, 1, out_host, out_dev_user, s, "host slices", K);   // sharded MSM: the partial stays on the device, in stream order
}

// A top-level MSM on the bound device: the one place the run record starts.  Scalars in host memory (G1) are staged first -- big single MSMs in growing slices that
// overlap their compute (msm_host_sliced), everything else (batches, small sizes) as one copy followed by the device-resident path.
enum ScalarLoc { SCALARS_HOST = 0, SCALARS_DEV = 1 };
template <class H> int msm_run(const typename H::base_t *bases, const fe_t *const *polys, ScalarLoc loc, uint32_t M, uint64_t n, void *out_host, const PreTable *pre = nullptr, void *out_dev_user = nullptr) {
  using out_t = typename H::Ops::out_t;
  if (M == 0) return MI355_OK;
  if (n == 0) {
    if (out_dev_user) { HIPCHK(hipMemsetAsync(out_dev_user, 0, (size_t)M * sizeof(out_t), g.stream)); return MI355_OK; }
    memset(out_host, 0, (size_t)M * sizeof(out_t)); return MI355_OK;
  }
  if (n >= (1ull << 31)) return fail(MI355_EBADARG, H::N_LIMIT);
  g.run.begin();
  if constexpr (H::G1_SCHEDULES) if (loc == SCALARS_HOST) {
    fe_t *sc; CHK(ws_get("io.scalars", (size_t)M * n * sizeof(fe_t), (void **)&sc));
    const PlanIn in = plan_in();
    const mi355zk::HostSlices hs = mi355zk::host_slices(in, n, M, tab_of(pre), H::GROUP);
    if (hs.count() > 1) return msm_host_sliced(in, hs, bases, polys[0], sc, n, out_host, pre, out_dev_user);
    std::vector<const fe_t *> ptrs(M);
    for (uint32_t m = 0; m < M; m++) { ptrs[m] = sc + (size_t)m * n; HIPCHK(hipMemcpyAsync(sc + (size_t)m * n, polys[m], n * sizeof(fe_t), hipMemcpyHostToDevice, g.stream)); }
    return msm_batch<H>(bases, ptrs.data(), M, n, out_host, pre, out_dev_user);
  }
  return msm_batch<H>(bases, polys, M, n, out_host, pre, out_dev_user);
}

// ------------------------------------------------------------------------------------------------ G2 MSM
// every base on the twist (device pass), then the MSMs (one device, one stream, the pass with the G2 policy; the window comes from the G1 cost model, workspace roles
// msm2.* hold 256-byte records; out_host: M x 128 B, normalised G2Affine).  EBADARG names the first base that is not on the twist.
static int msm_g2_run(const g2_affine_t *bases, const fe_t *const *polys, uint32_t M, uint64_t n, void *out_host) {
  if (n) {
    uint32_t *bad; CHK(ws_get("msm2.validate", 4, (void **)&bad));
    Scope sc("msm_g2_validate", g.stream);
    HIPCHK(hipMemsetAsync(bad, 0xff, 4, g.stream));
    const uint32_t blocks = std::min<uint64_t>(ceil_div(n, 256), (uint64_t)g.prop.multiProcessorCount * 8);
    hipLaunchKernelGGL(k_msm_g2_validate, dim3(blocks), dim3(256), 0, g.stream, bases, n, g2_twist_b(), bad);
    HIPCHK(hipGetLastError());
    uint32_t first_bad = 0xffffffffu;
    HIPCHK(hipMemcpyAsync(&first_bad, bad, 4, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    sc.close();
    if (first_bad != 0xffffffffu) return fail(MI355_EBADARG, "msm_g2: base " + std::to_string(first_bad) + " is not on the twist y^2 = x^3 + 3 / (9 + u)");
  }
  return msm_run<G2Pass>(bases, polys, SCALARS_DEV, M, n, out_host);
}

// The MSM entry points (G1 and G2) open the same way: no exception across the boundary, the MSM lock, an initialised library, and -- null_error being the text for a
// null argument the caller found, or null -- MI355_EBADARG before anything runs.
template <class F> int msm_entry(const char *null_error, F body, const char *who = __builtin_FUNCTION()) {
  return guarded([&]() -> int {
    MsmGuard lk;
    CHK(need_init());
    if (null_error) return fail(MI355_EBADARG, null_error);
    return body();
  }, who);
}
const char *batch_null_error(const char *who_null, const char *who_poly, bool other_null, const void *const *scalars, uint32_t batch, uint64_t n) {
  if (other_null || (batch && !scalars)) return who_null;
  for (uint32_t m = 0; m < batch; m++) if (n && !scalars[m]) return who_poly;
  return nullptr;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

// Prover::load_params for one degree: stream a RawBytes params file into device memory (two pinned staging buffers: the read of chunk
// i + 1 overlaps the DMA of chunk i), optionally validate every point on the device, register both bases as library-owned handles.
// flags bit 1: the file is SerdeFormat::Processed -- the compressed words take the same route and are decompressed chunk by chunk on the device.
static int stream_file_to_device(FILE *f, void *dev, size_t bytes, void *pinned[2], size_t chunk) {
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; i++) { HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)); HIPCHK(hipEventRecord(ev[i], g.stream)); }
  size_t done = 0; int which = 0; int rc = MI355_OK;
  while (done < bytes && rc == MI355_OK) {
    const size_t len = std::min(chunk, bytes - done);
    if (hipEventSynchronize(ev[which]) != hipSuccess) { rc = fail(MI355_EHIP, "srs_load_params_file: event wait failed"); break; }   // the previous copy out of this staging buffer has finished
    if (fread(pinned[which], 1, len, f) != len) { rc = fail(MI355_EBADARG, "srs_load_params_file: short read"); break; }
    if (hipMemcpyAsync((char *)dev + done, pinned[which], len, hipMemcpyHostToDevice, g.stream) != hipSuccess || hipEventRecord(ev[which], g.stream) != hipSuccess) { (void)hipGetLastError(); rc = fail(MI355_EHIP, "srs_load_params_file: copy failed"); break; }
    done += len; which ^= 1;
  }
  (void)hipStreamSynchronize(g.stream);
  for (int i = 0; i < 2; i++) (void)hipEventDestroy(ev[i]);
  return rc;
}
// SerdeFormat::Processed: the 32-byte words of one shard.  Chunk i + 1 is read and copied (a stream of its own) while chunk i is decompressed on the library
// stream straight into the shard: two pinned host buffers, the two halves of one pooled device block.  *bad_out: the smallest rejected index of the basis, or ~0.
static int stream_processed_to_shard(FILE *f, const Shard &sh, void *pinned[2], size_t chunk_pts, unsigned long long *bad_out) {
  PoolBlock stage; CHK(stage.alloc(2 * chunk_pts * 32, sh.slot));
  struct Side {   // the copy stream and the events of the two halves.  Declared after the block: on every return both streams are drained, these go, and then the block is freed
    hipStream_t cs = nullptr; hipEvent_t copied[2] = {nullptr, nullptr}, used[2] = {nullptr, nullptr};
    ~Side() {
      if (cs) (void)hipStreamSynchronize(cs);
      (void)hipStreamSynchronize(g.stream);
      for (int i = 0; i < 2; i++) { if (copied[i]) (void)hipEventDestroy(copied[i]); if (used[i]) (void)hipEventDestroy(used[i]); }
      if (cs) (void)hipStreamDestroy(cs);
    }
  } sd;
  unsigned long long *err; CHK(ws_get("g1codec.err", 8, (void **)&err));
  HIPCHK(hipMemsetAsync(err, 0xff, 8, g.stream));
  HIPCHK(hipStreamCreateWithFlags(&sd.cs, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) {
    HIPCHK(hipEventCreateWithFlags(&sd.copied[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&sd.used[i], hipEventDisableTiming));
    HIPCHK(hipEventRecord(sd.copied[i], sd.cs)); HIPCHK(hipEventRecord(sd.used[i], g.stream));
  }
  uint64_t done = 0; int which = 0;
  while (done < sh.n) {
    const uint64_t len = std::min<uint64_t>(chunk_pts, sh.n - done);
    char *half = stage.at((uint64_t)which * chunk_pts * 32);
    HIPCHK(hipEventSynchronize(sd.copied[which]));                       // the previous copy out of this pinned buffer has finished
    if (fread(pinned[which], 1, len * 32, f) != len * 32) return fail(MI355_EBADARG, "srs_load_params_file: short read");
    HIPCHK(hipStreamWaitEvent(sd.cs, sd.used[which], 0));                // the kernel that read this half of the device block has finished
    HIPCHK(hipMemcpyAsync(half, pinned[which], len * 32, hipMemcpyHostToDevice, sd.cs));
    HIPCHK(hipEventRecord(sd.copied[which], sd.cs));
    HIPCHK(hipStreamWaitEvent(g.stream, sd.copied[which], 0));
    CHK(launch_g1_decompress(half, sh.dev + done, len, sh.lo + done, err));
    HIPCHK(hipEventRecord(sd.used[which], g.stream));
    done += len; which ^= 1;
  }
  HIPCHK(hipMemcpyAsync(bad_out, err, 8, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return MI355_OK;
}
int mi355_srs_load_params_file(const char *path, uint32_t flags, uint32_t *k_out, uint64_t *g_handle_out, uint64_t *g_lagrange_handle_out, void *g2_out, void *s_g2_out) {
  return guarded([&]() -> int {
  AllGuard lk;
  CHK(need_init());
  if (!path || !k_out || !g_handle_out || !g_lagrange_handle_out) return fail(MI355_EBADARG, "srs_load_params_file: null pointer");
  FILE *f = fopen(path, "rb");
  if (!f) return fail(MI355_EBADARG, std::string("srs_load_params_file: cannot open ") + path);
  uint8_t hdr[4];
  int rc = MI355_OK; Srs sg, sl; void *pinned[2] = {nullptr, nullptr};
  do {
    if (fread(hdr, 1, 4, f) != 4) { rc = fail(MI355_EBADARG, "srs_load_params_file: empty file"); break; }
    const uint32_t k = (uint32_t)hdr[0] | ((uint32_t)hdr[1] << 8) | ((uint32_t)hdr[2] << 16) | ((uint32_t)hdr[3] << 24);
    if (k == 0 || k > 28) { rc = fail(MI355_EBADARG, "srs_load_params_file: k out of range (not a RawBytes params file)"); break; }
    const bool processed = (flags & 2u) != 0;   // SerdeFormat::Processed: 32-byte compressed G1 words, 64-byte compressed G2 points
    const uint64_t n = 1ull << k, want = processed ? 4 + 2 * n * 32 + 128 : 4 + 2 * n * sizeof(g1_affine_t) + 256;
    if (fseek(f, 0, SEEK_END) != 0 || (uint64_t)ftell(f) != want) {
      rc = fail(MI355_EBADARG, processed ? "srs_load_params_file: file length does not match 4 + 2 * 2^k * 32 + 128 (not a Processed params file of this k)"
                                         : "srs_load_params_file: file length does not match 4 + 2 * 2^k * 64 + 256 (load_params rejects it too)");
      break;
    }
    fseek(f, 4, SEEK_SET);
    const size_t chunk = std::min<uint64_t>(64ull << 20, n * (processed ? 32 : sizeof(g1_affine_t)));
    sg.n = sl.n = n; sg.mem = std::make_shared<SrsMem>(); sl.mem = std::make_shared<SrsMem>();
    if (srs_alloc(*sg.mem, n) != MI355_OK || srs_alloc(*sl.mem, n) != MI355_OK) { (void)hipGetLastError(); rc = fail(MI355_EOOM, "srs_load_params_file: device allocation failed"); break; }
    bool okp = true;
    for (int i = 0; i < 2; i++) okp = okp && hipHostMalloc(&pinned[i], chunk, hipHostMallocPortable) == hipSuccess;
    if (!okp) { rc = fail(MI355_EOOM, "srs_load_params_file: pinned staging allocation failed"); break; }
    for (Srs *b : {&sg, &sl}) for (auto &sh : b->mem->sh) {   // the file holds g then g_lagrange, each in point order = shard order
      if (rc != MI355_OK) break;
      if ((rc = bind_ctx(sh.slot)) != MI355_OK) break;
      if (!processed) { rc = stream_file_to_device(f, sh.dev, sh.n * sizeof(g1_affine_t), pinned, chunk); continue; }
      unsigned long long bad = ~0ull;
      rc = stream_processed_to_shard(f, sh, pinned, chunk / 32, &bad);
      if (rc == MI355_OK && bad != ~0ull)
        rc = fail(MI355_EBADARG, std::string("srs_load_params_file: ") + (b == &sg ? "g" : "g_lagrange") + "[" + std::to_string(bad) + "] is not the compressed form of a G1 point");
    }
    if (rc != MI355_OK) break;
    if (processed) {   // a decompressed point is on the curve by construction: bit 0 has nothing left to check
      uint8_t tail[128]; uint8_t g2v[128], sg2v[128];
      if (fread(tail, 1, 128, f) != 128) { rc = fail(MI355_EBADARG, "srs_load_params_file: short read (g2 / s_g2)"); break; }
      if (!g2_decode_host(tail, g2v)) { rc = fail(MI355_EBADARG, "srs_load_params_file: g2 is not the compressed form of a point of the twist"); break; }
      if (!g2_decode_host(tail + 64, sg2v)) { rc = fail(MI355_EBADARG, "srs_load_params_file: s_g2 is not the compressed form of a point of the twist"); break; }
      if (g2_out) memcpy(g2_out, g2v, 128);
      if (s_g2_out) memcpy(s_g2_out, sg2v, 128);
      *k_out = k;
      *g_handle_out = srs_insert(sg);
      *g_lagrange_handle_out = srs_insert(sl);
      break;
    }
    uint8_t tail[256];
    if (fread(tail, 1, 256, f) != 256) { rc = fail(MI355_EBADARG, "srs_load_params_file: short read (g2 / s_g2)"); break; }
    if (g2_out) memcpy(g2_out, tail, 128);
    if (s_g2_out) memcpy(s_g2_out, tail + 128, 128);
    if (flags & 1u) {
      uint64_t nbad_total = 0;
      for (Srs *b : {&sg, &sl}) for (auto &sh : b->mem->sh) {
        if ((rc = bind_ctx(sh.slot)) != MI355_OK) break;
        uint32_t *bad = nullptr;
        if (ws_get("io.validate", 4, (void **)&bad) != MI355_OK) { rc = MI355_EHIP; break; }
        (void)hipMemsetAsync(bad, 0, 4, g.stream);
        hipLaunchKernelGGL(k_g1_validate, dim3(g.prop.multiProcessorCount * 8), dim3(256), 0, g.stream, sh.dev, sh.n, bad);
        uint32_t nbad = 0;
        if (hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, g.stream) != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess) { rc = fail(MI355_EHIP, "srs_load_params_file: validation failed to run"); break; }
        nbad_total += nbad;
      }
      if (rc != MI355_OK) break;
      if (nbad_total) { rc = fail(MI355_EBADARG, "srs_load_params_file: " + std::to_string(nbad_total) + " point(s) are not on the curve"); break; }
    }
    *k_out = k;
    *g_handle_out = srs_insert(sg);
    *g_lagrange_handle_out = srs_insert(sl);
  } while (false);
  fclose(f);
  for (int i = 0; i < 2; i++) if (pinned[i]) (void)hipHostFree(pinned[i]);
  const std::string keep = g_err;
  (void)bind_ctx(0);
  if (rc != MI355_OK) g_err = keep;
  return rc;   // on failure the shared_ptrs in sg / sl free whatever was allocated
  });
}
int mi355_srs_precompute(uint64_t handle, uint64_t n_hint, int c) {
  return guarded([&]() -> int {
  AllGuard lk;
  CHK(need_init());
  Srs *sp; CHK(srs_find(handle, &sp, "srs_precompute"));
  SrsMem &mem = *sp->mem;
  if (n_hint == 0 || n_hint > sp->n) n_hint = sp->n;
  size_t live = 0; for (const auto &sh : mem.sh) if (sh.lo < sp->n) live++;
  const uint64_t per_shard = std::max<uint64_t>(1, n_hint / std::max<size_t>(1, live));
  const bool automatic = c == 0;
  if (automatic) c = mi355zk::best_window(per_shard, g_proc.msm_auto_max_c, true);   // best shared-bucket window for MSMs of n_hint points (per shard), within the sorter's key range
  if (c < 2 || c > MSM_MAX_C) return fail(MI355_EBADARG, "srs_precompute: window bits out of range");
  if (sp->tab) {
    if (sp->tab->c == c) return MI355_OK;
    // tables inherited from the parent basis (or built earlier with another width) stay when they are within 10 % of the best schedule
    if (automatic && mi355zk::tables_close_enough(per_shard, sp->tab->c, c)) return MI355_OK;
  }
  const int W = (MSM_SCALAR_BITS + c - 1) / c;
  auto tab = std::make_shared<SrsTables>();
  tab->c = c; tab->w = W;
  tab->pre.assign(mem.sh.size(), nullptr); tab->stride.assign(mem.sh.size(), 0); tab->slot.assign(mem.sh.size(), 0);
  for (size_t i = 0; i < mem.sh.size(); i++) {
    const Shard &sh = mem.sh[i];
    tab->slot[i] = sh.slot;
    if (sh.lo >= sp->n) continue;
    const uint64_t cnt = std::min(sh.n, sp->n - sh.lo);   // a prefix view tabulates only its own points
    CHK(bind_ctx(sh.slot));
    CHK(dev_malloc((void **)&tab->pre[i], (size_t)W * cnt * sizeof(g1_affine_t), "srs_precompute (window table)", mi355zk::MEM_WINDOW_TABLES));
    tab->stride[i] = cnt;
    hipLaunchKernelGGL(k_srs_precompute, dim3(ceil_div(cnt, 256)), dim3(256), 0, g.stream, sh.dev, tab->pre[i], cnt, (uint32_t)W, (uint32_t)c);
    HIPCHK(hipGetLastError());
  }
  for (const auto &sh : mem.sh) { CHK(bind_ctx(sh.slot)); HIPCHK(hipStreamSynchronize(g.stream)); }
  sp->tab = tab;   // the previous tables (if any) are freed here unless another handle still shares them
  return bind_ctx(0);
  });
}

// ---- MSM
// the pieces of [off, off + n) of a registered basis, one per shard that intersects it
struct Piece { int slot; const g1_affine_t *bases; PreTable pre; uint64_t a /* first scalar of the call */, cnt; };
static int srs_pieces(uint64_t handle, uint64_t off, uint64_t n, std::vector<Piece> &out) {
  Srs *sp; CHK(srs_find(handle, &sp, "msm"));
  if (off > sp->n || n > sp->n - off) return fail(MI355_EBADARG, "msm: base_offset + n exceeds the registered basis (best_multiexp panics on length mismatch)");
  const SrsMem &mem = *sp->mem;
  for (size_t i = 0; i < mem.sh.size(); i++) {
    const Shard &sh = mem.sh[i];
    const uint64_t lo = std::max(off, sh.lo), hi = std::min(off + n, sh.lo + sh.n);
    if (hi <= lo) continue;
    Piece p; p.slot = sh.slot; p.bases = sh.dev + (lo - sh.lo); p.a = lo - off; p.cnt = hi - lo;
    if (sp->tab && sp->tab->pre[i] && hi - sh.lo <= sp->tab->stride[i]) { p.pre.table = sp->tab->pre[i] + (lo - sh.lo); p.pre.row_stride = sp->tab->stride[i]; p.pre.c = sp->tab->c; p.pre.w = sp->tab->w; }
    out.push_back(p);
  }
  if (out.empty()) { Piece p; p.slot = 0; p.bases = nullptr; p.a = 0; p.cnt = 0; out.push_back(p); }   // n == 0
  return MI355_OK;
}

// Sharded MSM: every device that owns part of the point range computes the partial sum over its shard on its own stream, driven by
// its own host thread (copies from pageable memory block the issuing thread, so one thread per device keeps the PCIe links busy in parallel);
// the M x 96-byte partials are exchanged with ONE ncclAllGather per device (grouped) and folded + normalised on the primary device.
// polys: M pointers to n scalars each, host memory or device memory of any bound device.
static int msm_multi(const std::vector<Piece> &pieces, const fe_t *const *polys, ScalarLoc loc, uint32_t M, void *out_host) {
  const int D = g_ndev;
  const MsmOpts opts = t_opts;
  std::vector<int> rcs(D, MI355_OK); std::vector<std::string> errs(D);
  std::vector<const Piece *> by_slot(D, nullptr);
  for (const auto &p : pieces) by_slot[p.slot] = &p;
  // device-resident scalars may still be in flight on their owner's stream: the other devices' copies must wait for it
  std::vector<int> owner(M, 0);
  if (loc == SCALARS_DEV) {
    bool seen[MAX_DEV] = {false};
    for (uint32_t m = 0; m < M; m++) { owner[m] = slot_of(polys[m]); seen[owner[m]] = true; }
    if (D > 1) for (int s = 0; s < D; s++) if (seen[s]) { CHK(bind_ctx(s)); HIPCHK(hipStreamSynchronize(g.stream)); }
  }
  auto work = [&](int slot) {
    t_opts = opts; t_opts.normalise = false;            // partials are folded (and normalised once) after the exchange
    SlotHeld held(slot);                                // the entry point's MsmGuard holds this slot's lock on the worker's behalf
    auto body = [&]() -> int {
      CHK(bind_ctx(slot));
      g1_jac_t *send; CHK(ws_get("xchg.send", (size_t)M * sizeof(g1_jac_t), (void **)&send));
      const Piece *p = by_slot[slot];
      if (!p || p->cnt == 0) { HIPCHK(hipMemsetAsync(send, 0, (size_t)M * sizeof(g1_jac_t), g.stream)); return MI355_OK; }
      std::vector<const fe_t *> ptrs(M);
      if (loc == SCALARS_HOST) {   // this device's slice of every polynomial crosses its own PCIe link, chunk-overlapped with the compute
        for (uint32_t m = 0; m < M; m++) ptrs[m] = polys[m] + p->a;
        return msm_run<G1Pass>(p->bases, ptrs.data(), SCALARS_HOST, M, p->cnt, nullptr, &p->pre, send);
      }
      // device-resident scalars: a polynomial that lives on this (physical) device is read in place; one that lives on another bound device --
      // the primary as a rule, any device with mi355_buf_alloc(.., slot) -- crosses xGMI into a staging buffer first
      fe_t *sc = nullptr;
      for (uint32_t m = 0; m < M; m++) {
        const int o = owner[m];
        if (g_ctx[o].device == g.device) { ptrs[m] = polys[m] + p->a; continue; }
        if (!sc) CHK(ws_get("io.scalars", (size_t)M * p->cnt * sizeof(fe_t), (void **)&sc));
        ptrs[m] = sc + (size_t)m * p->cnt;
        HIPCHK(hipMemcpyPeerAsync(sc + (size_t)m * p->cnt, g.device, polys[m] + p->a, g_ctx[o].device, p->cnt * sizeof(fe_t), g.stream));
      }
      return msm_run<G1Pass>(p->bases, ptrs.data(), SCALARS_DEV, M, p->cnt, nullptr, &p->pre, send);
    };
    rcs[slot] = guarded(body, "msm shard worker");
    if (rcs[slot] != MI355_OK) errs[slot] = g_err;
  };
  {
    // every started worker is joined on every path (a std::thread that is destroyed while joinable terminates the process)
    struct Joiner { std::vector<std::thread> th; ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); } } workers;
    workers.th.reserve(D);
    for (int s = 1; s < D; s++) workers.th.emplace_back(work, s);
    work(0);
  }
  t_opts = opts;
  CHK(bind_ctx(0));
  for (int s = 0; s < D; s++) if (rcs[s] != MI355_OK) return fail(rcs[s], "device slot " + std::to_string(s) + ": " + errs[s]);
  // ---- exchange: D x M x 96 bytes
  const size_t part_bytes = (size_t)M * sizeof(g1_jac_t);
  std::vector<g1_jac_t *> send(D), recv(D);
  for (int s = 0; s < D; s++) { CHK(bind_ctx(s)); CHK(ws_get("xchg.send", part_bytes, (void **)&send[s])); CHK(ws_get("xchg.recv", part_bytes * D, (void **)&recv[s])); }
  if (g_ctx[0].comm) {
    int r = g_rccl.GroupStart(); if (r != 0) return rccl_fail("ncclGroupStart", r);
    for (int s = 0; s < D; s++) {
      CHK(bind_ctx(s));
      r = g_rccl.AllGather(send[s], recv[s], part_bytes, /* ncclUint8 */ 1, g_ctx[s].comm, g_ctx[s].stream);
      if (r != 0) { (void)g_rccl.GroupEnd(); return rccl_fail("ncclAllGather", r); }
    }
    r = g_rccl.GroupEnd(); if (r != 0) return rccl_fail("ncclGroupEnd", r);
    g_ctx[0].run.exchange = "rccl_allgather";
  } else {
    // several slots on one physical device (test mode): no communicator can exist; the partials are copied device-to-device
    for (int s = 0; s < D; s++) {
      CHK(bind_ctx(s)); HIPCHK(hipEventRecord(g.ev_xchg, g.stream));
      CHK(bind_ctx(0)); HIPCHK(hipStreamWaitEvent(g.stream, g_ctx[s].ev_xchg, 0));
      HIPCHK(hipMemcpyAsync((char *)recv[0] + part_bytes * s, send[s], part_bytes, hipMemcpyDeviceToDevice, g.stream));
    }
    g_ctx[0].run.exchange = "device_copy";
  }
  CHK(bind_ctx(0));
  g1_jac_t *res; CHK(ws_get("xchg.result", part_bytes, (void **)&res));
  hipLaunchKernelGGL(k_g1_sum_strided, dim3(M), dim3(64), 0, g.stream, (const g1_jac_t *)recv[0], (uint32_t)D, M, res, opts.normalise ? 1 : 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_host, res, part_bytes, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  for (int s = D - 1; s >= 0; s--) { CHK(bind_ctx(s)); if (s) HIPCHK(hipStreamSynchronize(g.stream)); resolve_spans(); }
  g_ctx[0].run.devices = D;   // the primary's record holds its own shard's plan (msm_run) and the whole call's devices and exchange
  return MI355_OK;
}
static bool single_device_call(const std::vector<Piece> &pieces) { return pieces.size() == 1 && pieces[0].slot == 0 && !g_proc.multi_force; }

// host scalars, one device: staged in groups of at most 4 GiB of scalars (msm_run copies a group, or cuts a big single MSM into slices that overlap their compute)
static int msm_host_groups(const Piece &p, const fe_t *const *scalars_host, uint32_t M, uint64_t n, void *out_g1_host) {
  const uint32_t group_max = (uint32_t)std::max<uint64_t>(1, (4ull << 30) / (n * sizeof(fe_t)));
  for (uint32_t m0 = 0; m0 < M; m0 += group_max) {
    const uint32_t mg = std::min(group_max, M - m0);
    CHK(msm_run<G1Pass>(p.bases, scalars_host + m0, SCALARS_HOST, mg, n, (char *)out_g1_host + (size_t)m0 * sizeof(g1_jac_t), &p.pre));
  }
  return MI355_OK;
}
// resident scalars, one device
static int msm_dev_resident(const Piece &p, const void *const *scalars_dev, uint32_t M, uint64_t n, void *out_g1_host) {
  // Every scalar block is marked as used by queued work (slot_of's `touch`), with one device as with several: an upload into a block whose only
  // use since mi355_buf_alloc was as an MSM input must wait for the compute stream, not take the "fresh block" path.
  // Several devices bound, basis on the primary only: scalars that live on another device are read through peer access, after their producer;
  // when peer access to that device could not be enabled they are staged on the primary first (hipMemcpyPeerAsync needs no peer mapping).
  std::vector<const fe_t *> ptrs(M);
  fe_t *stage = nullptr; size_t staged = 0;
  for (uint32_t m = 0; m < M; m++) {
    const int o = slot_of(scalars_dev[m], true);
    ptrs[m] = (const fe_t *)scalars_dev[m];
    if (g_ndev > 1 && o != 0) {
      CHK(bind_ctx(o)); HIPCHK(hipStreamSynchronize(g.stream));
      if (!g_peer_ok[0][o]) {
        CHK(bind_ctx(0));
        if (!stage) CHK(ws_get("io.scalars", (size_t)M * n * sizeof(fe_t), (void **)&stage));
        HIPCHK(hipMemcpyPeerAsync(stage + staged, g.device, scalars_dev[m], g_ctx[o].device, n * sizeof(fe_t), g.stream));
        ptrs[m] = stage + staged; staged += n;
      }
    }
  }
  CHK(bind_ctx(0));
  return msm_run<G1Pass>(p.bases, ptrs.data(), SCALARS_DEV, M, n, out_g1_host, &p.pre);
}
// mi355_msm_g1_host / _dev and their batch forms: one piece on the primary device runs there, anything else is the sharded MSM
static int msm_dispatch(uint64_t srs_handle, uint64_t base_offset, const void *const *scalars, ScalarLoc loc, uint32_t M, uint64_t n, void *out_g1_host) {
  std::vector<Piece> pieces; CHK(srs_pieces(srs_handle, base_offset, n, pieces));
  if (M == 0 || n == 0) { if (M) memset(out_g1_host, 0, (size_t)M * sizeof(g1_jac_t)); return MI355_OK; }
  if (!single_device_call(pieces)) return msm_multi(pieces, (const fe_t *const *)scalars, loc, M, out_g1_host);
  return loc == SCALARS_HOST ? msm_host_groups(pieces[0], (const fe_t *const *)scalars, M, n, out_g1_host) : msm_dev_resident(pieces[0], scalars, M, n, out_g1_host);
}


int mi355_msm_g1_dev(uint64_t srs_handle, uint64_t base_offset, const void *scalars_dev, uint64_t n, void *out_g1_host) {
  return msm_entry(!out_g1_host || (n && !scalars_dev) ? "msm: null pointer" : nullptr, [&]() -> int {
  return msm_dispatch(srs_handle, base_offset, &scalars_dev, SCALARS_DEV, 1, n, out_g1_host);
  });
}
int mi355_msm_g1_dev_async(uint64_t srs_handle, uint64_t base_offset, const void *scalars_dev, uint64_t n, void *out_g1_dev) {
  return msm_entry(!out_g1_dev || (n && !scalars_dev) ? "msm: null pointer" : nullptr, [&]() -> int {
  std::vector<Piece> pieces; CHK(srs_pieces(srs_handle, base_offset, n, pieces));
  if (pieces.size() != 1 || pieces[0].slot != 0) return fail(MI355_EBADARG, "msm_g1_dev_async: the range must lie on the primary device (one process per GPU drives its own shard)");
  const fe_t *sc = (const fe_t *)scalars_dev;
  (void)slot_of(scalars_dev, true); (void)slot_of(out_g1_dev, true);   // both blocks now carry queued work: a later upload into either waits for the compute stream
  return msm_run<G1Pass>(pieces[0].bases, &sc, SCALARS_DEV, 1, n, nullptr, &pieces[0].pre, out_g1_dev);
  });
}
int mi355_g1_sum_dev(const void *pts_dev, uint64_t n, void *out_g1_host) {
  return guarded([&]() -> int {
  const int slot = slot_of(pts_dev);
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (!out_g1_host || (n && !pts_dev) || n > (1u << 20)) return fail(MI355_EBADARG, "g1_sum: bad argument");
  g1_jac_t *dev; CHK(ws_get("io.g1sum", sizeof(g1_jac_t), (void **)&dev));
  hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(64), 0, g.stream, (const g1_jac_t *)pts_dev, (uint32_t)n, dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_g1_host, dev, sizeof(g1_jac_t), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return MI355_OK;
  });
}
int mi355_msm_g1_host(uint64_t srs_handle, uint64_t base_offset, const void *scalars_host, uint64_t n, void *out_g1_host) {
  return msm_entry(!out_g1_host || (n && !scalars_host) ? "msm: null pointer" : nullptr, [&]() -> int {
  return msm_dispatch(srs_handle, base_offset, &scalars_host, SCALARS_HOST, 1, n, out_g1_host);
  });
}
int mi355_msm_g1_batch_dev(uint64_t srs_handle, uint64_t base_offset, const void *const *scalars_dev, uint32_t batch, uint64_t n, void *out_g1_host) {
  return msm_entry(batch_null_error("msm_batch: null pointer", "msm_batch: null polynomial pointer", !out_g1_host, scalars_dev, batch, n), [&]() -> int {
  return msm_dispatch(srs_handle, base_offset, scalars_dev, SCALARS_DEV, batch, n, out_g1_host);
  });
}
int mi355_msm_g1_batch_host(uint64_t srs_handle, uint64_t base_offset, const void *const *scalars_host, uint32_t batch, uint64_t n, void *out_g1_host) {
  return msm_entry(batch_null_error("msm_batch: null pointer", "msm_batch: null polynomial pointer", !out_g1_host, scalars_host, batch, n), [&]() -> int {
  return msm_dispatch(srs_handle, base_offset, scalars_host, SCALARS_HOST, batch, n, out_g1_host);
  });
}
int mi355_msm_set_pipeline(uint32_t chunks, uint32_t min_log_n) {
  return guarded([&]() -> int {
  AllGuard lk;
  if (chunks > 16 || min_log_n > 31) return fail(MI355_EBADARG, "msm_set_pipeline: chunks <= 16, min_log_n <= 31");
  for (int s = 0; s < std::max(1, g_ndev); s++) { g_ctx[s].msm_chunks = chunks ? chunks : 1; g_ctx[s].msm_chunk_min_log = chunks ? min_log_n : 23; }
  return MI355_OK;
  });
}
int mi355_msm_g1_adhoc_host(const void *bases_host, const void *scalars_host, uint64_t n, void *out_g1_host) {
  return msm_entry(!out_g1_host || (n && (!scalars_host || !bases_host)) ? "msm: null pointer" : nullptr, [&]() -> int {
  fe_t *sc = nullptr; g1_affine_t *bs = nullptr;
  if (n) {
    CHK(ws_get("io.scalars", n * sizeof(fe_t), (void **)&sc)); CHK(ws_get("io.bases", n * sizeof(g1_affine_t), (void **)&bs));
    HIPCHK(hipMemcpyAsync(sc, scalars_host, n * sizeof(fe_t), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(bs, bases_host, n * sizeof(g1_affine_t), hipMemcpyHostToDevice, g.stream));
  }
  const fe_t *poly = sc;
  return msm_run<G1Pass>(bs, &poly, SCALARS_DEV, 1, n, out_g1_host);
  });
}
// Many short MSMs in one launch (msm_seg.hpp: a wavefront per segment, no bucket pipeline).  The argument checks read host memory only and come before
// the device is asked for; one upload per array, one launch, one download.
int mi355_msm_g1_segmented_host(const void *bases_affine_host, const void *scalars_host, const uint64_t *offsets_host, uint32_t segments, void *out_g1affine_host) {
  return guarded([&]() -> int {
  if (segments > (1u << 20)) return fail(MI355_EBADARG, "msm_segmented: more than 2^20 segments");
  uint64_t total = 0;
  if (segments) {
    if (!offsets_host || !out_g1affine_host) return fail(MI355_EBADARG, "msm_segmented: null pointer");
    if (offsets_host[0] != 0) return fail(MI355_EBADARG, "msm_segmented: offsets[0] must be 0");
    for (uint32_t s = 0; s < segments; s++) if (offsets_host[s + 1] < offsets_host[s]) return fail(MI355_EBADARG, "msm_segmented: offsets decrease at segment " + std::to_string(s));
    total = offsets_host[segments];
    if (total > (1ull << 24)) return fail(MI355_EBADARG, "msm_segmented: more than 2^24 terms (this entry point is for many SHORT segments)");
    if (total && (!bases_affine_host || !scalars_host)) return fail(MI355_EBADARG, "msm_segmented: null pointer");
  }
  MsmGuard lk;
  CHK(need_init());
  if (segments == 0) return MI355_OK;
  if (total == 0) { memset(out_g1affine_host, 0, (size_t)segments * sizeof(g1_affine_t)); return MI355_OK; }   // every segment empty: identities
  CallTrace tr("msm_g1_segmented", total, 96.0);
  hipStream_t s = g.stream;
  fe_t *sc; g1_affine_t *bs, *out_dev; uint64_t *off;
  CHK(ws_get("io.scalars", total * sizeof(fe_t), (void **)&sc)); CHK(ws_get("io.bases", total * sizeof(g1_affine_t), (void **)&bs));
  CHK(ws_get("msmseg.offsets", ((size_t)segments + 1) * 8, (void **)&off)); CHK(ws_get("msmseg.out", (size_t)segments * sizeof(g1_affine_t), (void **)&out_dev));
  HIPCHK(hipMemcpyAsync(sc, scalars_host, total * sizeof(fe_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(bs, bases_affine_host, total * sizeof(g1_affine_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(off, offsets_host, ((size_t)segments + 1) * 8, hipMemcpyHostToDevice, s));
  {
    Scope sp("msm_segmented", s);
    hipLaunchKernelGGL(k_msm_g1_segmented, dim3(segments), dim3(SEGMSM_LANES), 0, s, (const g1_affine_t *)bs, (const fe_t *)sc, (const uint64_t *)off, out_dev);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(out_g1affine_host, out_dev, (size_t)segments * sizeof(g1_affine_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  resolve_spans();
  { char buf[48]; snprintf(buf, sizeof buf, " segments=%u", segments); tr.done(buf); }
  return MI355_OK;
  });
}
int mi355_g1_sum_host(const void *pts_host, uint64_t n, void *out_g1_host) {
  return guarded([&]() -> int {
  DevGuard lk(0);
  CHK(need_init());
  if (!out_g1_host || (n && !pts_host) || n > (1u << 20)) return fail(MI355_EBADARG, "g1_sum: bad argument");
  g1_jac_t *dev; CHK(ws_get("io.g1sum", (n + 1) * sizeof(g1_jac_t), (void **)&dev));
  if (n) HIPCHK(hipMemcpyAsync(dev + 1, pts_host, n * sizeof(g1_jac_t), hipMemcpyHostToDevice, g.stream));
  hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(64), 0, g.stream, dev + 1, (uint32_t)n, dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_g1_host, dev, sizeof(g1_jac_t), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return MI355_OK;
  });
}
// The two setters below act on the CALLING THREAD only (thread-local options): concurrent callers never see each other's settings.
int mi355_msm_set_window_bits(int c) {
  return guarded([&]() -> int {
  if (c == -1) { t_opts.force_c = 0; t_opts.no_tables = true; return MI355_OK; }   // automatic window, window tables ignored
  if (c != 0 && (c < 2 || c > MSM_MAX_C)) return fail(MI355_EBADARG, "window bits must be 0 (auto), -1 (auto, no window tables) or in [2, 24]");
  t_opts.force_c = c; t_opts.no_tables = false; return MI355_OK;
  });
}
int mi355_msm_set_normalise(int on) { t_opts.normalise = on != 0; return MI355_OK; }
int mi355_msm_last_plan(int *c_out, int *windows_out, uint64_t *entries_out) {
  return guarded([&]() -> int {
  DevGuard lk(0);
  const Ctx &p = g_ctx[0];
  if (c_out) *c_out = p.run.c; if (windows_out) *windows_out = p.run.windows; if (entries_out) *entries_out = p.run.entries; return MI355_OK;
  });
}
// how the last MSM ran: device slots that took part, the exchange ("none" | "rccl_allgather" | "device_copy"), whether the window tables
// (one shared bucket set) were used, and the number of point-range slices of the host-pointer path
int mi355_msm_last_run(int *devices_out, const char **exchange_out, int *shared_tables_out, int *host_slices_out) {
  return guarded([&]() -> int {
  DevGuard lk(0);
  const MsmRunRecord &r = g_ctx[0].run;
  if (devices_out) *devices_out = r.devices; if (exchange_out) *exchange_out = r.exchange;
  if (shared_tables_out) *shared_tables_out = r.shared ? 1 : 0; if (host_slices_out) *host_slices_out = r.host_slices;
  return MI355_OK;
  });
}

// ---- G2 MSM (single device; bases checked on the twist, not for subgroup membership)
int mi355_msm_g2_adhoc_host(const void *bases_g2affine_host, const void *scalars_host, uint64_t n, void *out_g2affine_host) {
  return msm_entry(!out_g2affine_host || (n && (!scalars_host || !bases_g2affine_host)) ? "msm_g2: null pointer" : nullptr, [&]() -> int {
  if (n >= (1ull << 31)) return fail(MI355_EBADARG, "msm_g2: n must be < 2^31");
  fe_t *sc = nullptr; g2_affine_t *bs = nullptr;
  if (n) {
    CHK(ws_get("io.scalars", n * sizeof(fe_t), (void **)&sc)); CHK(ws_get("io.g2_bases", n * sizeof(g2_affine_t), (void **)&bs));
    HIPCHK(hipMemcpyAsync(sc, scalars_host, n * sizeof(fe_t), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(bs, bases_g2affine_host, n * sizeof(g2_affine_t), hipMemcpyHostToDevice, g.stream));
  }
  const fe_t *p = sc;
  return msm_g2_run(bs, &p, 1, n, out_g2affine_host);
  });
}
// device-resident bases and scalars: both must live on the primary device (the G2 MSM runs on one device)
static int g2_dev_operand(const void *p) {
  if (slot_of(p, true) != 0) return fail(MI355_EBADARG, "msm_g2: bases and scalars must live on the primary device (G2 MSMs run on one device)");
  return MI355_OK;
}
int mi355_msm_g2_dev(const void *bases_g2affine_dev, const void *scalars_dev, uint64_t n, void *out_g2affine_host) {
  return msm_entry(!out_g2affine_host || (n && (!scalars_dev || !bases_g2affine_dev)) ? "msm_g2: null pointer" : nullptr, [&]() -> int {
  if (n) { CHK(g2_dev_operand(bases_g2affine_dev)); CHK(g2_dev_operand(scalars_dev)); }
  CHK(bind_ctx(0));
  const fe_t *p = (const fe_t *)scalars_dev;
  return msm_g2_run((const g2_affine_t *)bases_g2affine_dev, &p, 1, n, out_g2affine_host);
  });
}
int mi355_msm_g2_batch_dev(const void *bases_g2affine_dev, const void *const *scalars_dev, uint32_t batch, uint64_t n, void *out_g2affine_host) {
  return msm_entry(batch_null_error("msm_g2_batch: null pointer", "msm_g2_batch: null polynomial pointer", !out_g2affine_host || (batch && n && !bases_g2affine_dev), scalars_dev, batch, n), [&]() -> int {
  if (batch && n) { CHK(g2_dev_operand(bases_g2affine_dev)); for (uint32_t m = 0; m < batch; m++) CHK(g2_dev_operand(scalars_dev[m])); }
  CHK(bind_ctx(0));
  if (batch == 0) return MI355_OK;
  return msm_g2_run((const g2_affine_t *)bases_g2affine_dev, (const fe_t *const *)scalars_dev, batch, n, out_g2affine_host);
  });
}

// ---- synthetic SRS
static int ensure_fixed_base_table() {
  if (g.fixed_base_table) return MI355_OK;
  CHK(dev_malloc((void **)&g.fixed_base_table, 32 * 256 * sizeof(g1_affine_t), "fixed-base table", mi355zk::MEM_FIXED_TABLES));
  hipLaunchKernelGGL(k_fixed_base_table, dim3(1), dim3(256), 0, g.stream, g.fixed_base_table);
  HIPCHK(hipGetLastError());
  return MI355_OK;
}
int mi355_g1_fixed_base_mul_dev(void *points_dev, const void *scalars_dev, uint64_t n) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({points_dev, scalars_dev}, &slot, "fixed_base_mul"));
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (!points_dev || !scalars_dev) return fail(MI355_EBADARG, "fixed_base_mul: null pointer");
  CHK(ensure_fixed_base_table());
  hipLaunchKernelGGL(k_fixed_base_mul, dim3(ceil_div(n, 256)), dim3(256), 0, g.stream, g.fixed_base_table, (const fe_t *)scalars_dev, (g1_affine_t *)points_dev, n);
  HIPCHK(hipGetLastError());
  return MI355_OK;
  });
}
int mi355_srs_setup_dev(void *g_dev, void *g_lagrange_dev, uint32_t k, const void *tau, const void *omega) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({g_dev, g_lagrange_dev}, &slot, "srs_setup"));
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (!g_dev || !g_lagrange_dev || !tau || !omega || k > 28) return fail(MI355_EBADARG, "srs_setup: bad argument");
  CHK(ensure_fixed_base_table());
  const uint64_t n = 1ull << k;
  fe_t *sc; CHK(ws_get("srs.scalars", 2 * n * sizeof(fe_t), (void **)&sc));
  fe_t t, w; memcpy(&t, tau, 32); memcpy(&w, omega, 32);
  // (tau^n - 1) / n: one-off constant, formed on the host with the same limb code
  fe_t nn = Fr::zero(); nn.l[0] = (uint32_t)n; nn.l[1] = (uint32_t)(n >> 32);
  const fe_t tn1_over_n = Fr::mul(Fr::sub(Fr::pow_u64(t, n), Fr::one()), Fr::inv(Fr::from_canonical(nn)));
  hipLaunchKernelGGL(k_srs_scalars, dim3(ceil_div(n, 256)), dim3(256), 0, g.stream, sc, sc + n, t, w, tn1_over_n, n);
  hipLaunchKernelGGL(k_fixed_base_mul, dim3(ceil_div(n, 256)), dim3(256), 0, g.stream, g.fixed_base_table, sc, (g1_affine_t *)g_dev, n);
  hipLaunchKernelGGL(k_fixed_base_mul, dim3(ceil_div(n, 256)), dim3(256), 0, g.stream, g.fixed_base_table, sc + n, (g1_affine_t *)g_lagrange_dev, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(g.stream));
  return MI355_OK;
  });
}

}  // extern "C"
