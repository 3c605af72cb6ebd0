// knobs.hpp -- the environment variables mi355_init / mi355_init_multi read, as ONE table: name, field, default, acceptance rule with its bounds, meaning.  Plain C++, no HIP: the
// structs and the table are generated from the two lists below, apply_knobs() walks the table over any lookup function (getenv in lib_core.hip, an injected map in
// tests/hostcheck/knobs_main.cpp).  DESIGN.md section 10 is the same table for readers, with the variables that are deliberately read elsewhere (per launch, per process, lazily);
// tests/test_knob_table.py keeps the two and the getenv literals of csrc/ in step.
//
// Rules (v = atoi(e) unless stated; a value a rule rejects leaves the default, and atoi's leniency is part of the contract: "12abc" is 12, "abc" and "" are 0):
//   Range      lo <= v <= hi                         RangeLong  the same with atol (bounds beyond int)
//   RangePow2  Range, and v a power of two           AtLeast    v >= lo
//   Set        v == lo or v == hi                    FirstChar  the first character is a digit lo..hi; the value is that digit
//   Mask       v & hi, always accepted               ZeroOff    0 when the first character is '0', else 1
//   NonZeroOn  v != 0, always accepted ("abc" turns off)
#pragma once
#include <cstdint>
#include <cstdlib>

// X(field, default, "NAME", rule, lo, hi, "meaning") -- per device slot (Ctx derives from Knobs; lib_msm.hip / lib_ntt.hip read them as g.<field>)
#define MI355_DEVICE_KNOBS(X) \
  X(trace, 0, "MI355_TRACE", FirstChar, 1, 1, "1: one stderr line per MSM / NTT call (host wall time; device transforms are synchronised for it); 2 is read lazily by roctx_bind") \
  X(aux_prio_high, 1, "MI355_AUX_PRIO", ZeroOff, 0, 1, "side streams of the pipelined MSM at the highest stream priority (0: the lowest)") \
  X(msm_chunks, 1, "MI355_MSM_CHUNKS", Range, 1, 16, "point-range slices of the pipelined MSM schedule (also mi355_msm_set_pipeline; 1 = off)") \
  X(reduce_chains, 131072, "MI355_REDUCE_CHAINS", AtLeast, 1024, 0, "target number of running-sum chains of the bucket reduction") \
  X(seg_fill, 40, "MI355_SEG_FILL", Range, 2, 100, "share (%) of the launched accumulate threads the entries are spread over, per-bucket fix-up (above 100 the segments would not cover the entries)") \
  X(seg_fill_segfix, 40, "MI355_SEG_FILL_SEGFIX", Range, 2, 100, "the same share with the segmented fix-up") \
  X(seg_min, 16, "MI355_SEG_MIN", Range, 1, 4096, "shortest accumulate segment (entries per thread) when few digits are non-zero") \
  X(fixup_mode, 2, "MI355_FIXUP_MODE", FirstChar, 0, 2, "2: fix-up by shape (plan_pass, msm_plan.hpp); 0: per-bucket kernels; 1: one segmented reduction over the partial sums (k_msm_segfix)") \
  X(fixup_huge_min, 2048, "MI355_FIXUP_HUGE_MIN", RangeLong, 2048, 0x7fffffffL, "bucket spans from this many accumulate threads on are summed by several workgroups") \
  X(fixup_serial_max, 32, "MI355_FIXUP_SERIAL_MAX", Range, 1, 1024, "bucket spans (in accumulate threads) above this go to the workgroup-per-bucket fix-up") \
  X(fixup_lanes_max_log, 17, "MI355_FIXUP_LANES_MAX_LOG", Range, 0, 31, "bucket sets up to 2^this records take the four-lanes-per-bucket fix-up") \
  X(tail_coop_mask, 15, "MI355_TAIL_COOP_MASK", Mask, 0, 15, "which tail kernels may take the quad form (1 fix-up, 2 running sums, 4 trees, 8 final Horner)") \
  X(tail_coop_max, 65536, "MI355_TAIL_COOP_MAX", RangeLong, 0, 1L << 24, "reduction-tail kernels with at most this many logical threads run the quad-cooperative point addition; 0 disables") \
  X(reduce_min_chunk, 4, "MI355_REDUCE_MIN_CHUNK", RangePow2, 1, 64, "shortest running-sum chain (buckets per reduce thread) small bucket sets are cut into") \
  X(sort_fb, 11, "MI355_SORT_FB", Range, 9, 12, "fine (level-2) key bits of the sorter") \
  X(sort_split, 1, "MI355_SORT_SPLIT", FirstChar, 1, 2, "level-1 output as two streams: 1 = 24 576-entry tiles where the bin bookkeeping leaves room, 2 = 16 384-entry tiles") \
  X(seg_factor, 16, "MI355_SEG_FACTOR", Range, 1, 256, "accumulate threads per lane slot (segment length = entries / (CUs * 256 * factor))") \
  X(sort_t2, 0, "MI355_SORT_T2", Set, 8192, 16384, "level-2 tile of the sorter (default 0: by size)") \
  X(sort_t1, 16384, "MI355_SORT_T1", Set, 8192, 8192, "8192 selects the smaller level-1 tile (2 workgroups per CU)") \
  X(ntt_direct2_max_log, 25, "MI355_NTT_DIRECT2_MAX_LOG", Range, 0, 28, "levels up to 2^this elements read their inter-level twiddles from a full [k][column] table (36 B per element, HBM permitting); 0 disables") \
  X(ntt_direct2_min_log, 0, "MI355_NTT_DIRECT2_MIN_LOG", Range, 0, 28, "levels below 2^this elements gather their inter-level twiddles from one 1-D table instead") \
  X(ntt_fold_scale, 1, "MI355_NTT_FOLD_SCALE", ZeroOff, 0, 1, "0: the inverse transform's divisor stays a multiplication in the closing pass") \
  X(ntt_coset_fold_max_log, 26, "MI355_NTT_COSET_FOLD_MAX_LOG", Range, 0, 28, "coset transforms up to 2^this fold distribute_powers into their first pass (one 36 B x 2^log_n table per coset factor, HBM permitting); 0: always the separate pass") \
  X(ntt_batch_max_log, 22, "MI355_NTT_BATCH_MAX_LOG", Range, 0, 28, "the batch entry points run transforms up to 2^this as batched launches (blockIdx.y = polynomial); 0: always the loop of single transforms") \
  X(ntt_two_level_max_log, 18, "MI355_NTT_TWO_LEVEL_MAX_LOG", Range, 9, 20, "transforms up to 2^this run as two passes instead of three") \
  X(ntt_tile_log, 11, "MI355_NTT_TILE_LOG", Range, 8, 12, "log2 of the LDS tile in elements") \
  X(host_batch_overlap, 1, "MI355_HOST_BATCH_OVERLAP", NonZeroOn, 0, 1, "0: the host-pointer batch transforms copy and compute one item at a time (no helper thread)") \
  X(host_chunks, 8, "MI355_HOST_CHUNKS", Range, 1, 64, "upper bound on the point-range slices of the host-pointer MSM (1 = one copy, then compute)") \
  X(host_slice_min_log, 22, "MI355_HOST_SLICE_MIN_LOG", Range, 4, 31, "smallest log2(n) the host-pointer MSM cuts into slices (tests lower it)")
// per process (mi355_init_multi; the library reads them as g_proc.<field>)
#define MI355_PROCESS_KNOBS(X) \
  X(allow_dup_devices, 0, "MI355_ALLOW_DUP_DEVICES", FirstChar, 1, 1, "test mode: one physical device may fill several slots (exchange by device copies instead of RCCL)") \
  X(multi_force, 0, "MI355_MULTI_FORCE", FirstChar, 1, 1, "take the sharded MSM path (partials + exchange + fold) even with one device") \
  X(msm_auto_max_c, 22, "MI355_MSM_AUTO_MAX_C", Range, 16, 24, "widest window the automatic choices may take (explicit requests may always use up to 24)") \
  X(shard_min_log, 14, "MI355_SHARD_MIN_LOG", Range, 0, 30, "a basis with fewer than 2^this points per device stays on the primary device (tests lower it)")

namespace mi355zk {

#define MI355_KNOB_FIELD(field, dflt, ...) uint32_t field = dflt;
struct Knobs { MI355_DEVICE_KNOBS(MI355_KNOB_FIELD) };
struct ProcessKnobs { MI355_PROCESS_KNOBS(MI355_KNOB_FIELD) };
struct AllKnobs : Knobs, ProcessKnobs {};
#undef MI355_KNOB_FIELD

enum class KnobRule { Range, RangeLong, RangePow2, AtLeast, Set, FirstChar, Mask, ZeroOff, NonZeroOn };
struct KnobRow { const char *name; uint32_t AllKnobs::*field; uint32_t dflt; KnobRule rule; long lo, hi; const char *meaning; };
#define MI355_KNOB_ROW(field, dflt, name, rule, lo, hi, meaning) {name, &AllKnobs::field, dflt, KnobRule::rule, lo, hi, meaning},
inline const KnobRow KNOB_TABLE[] = {MI355_DEVICE_KNOBS(MI355_KNOB_ROW) MI355_PROCESS_KNOBS(MI355_KNOB_ROW)};
#undef MI355_KNOB_ROW

// every variable the lookup knows overrides its field of `k` (a freshly constructed AllKnobs: the defaults) when its rule accepts the string
inline void apply_knobs(AllKnobs &k, const char *(*lookup)(const char *)) {
  for (const KnobRow &r : KNOB_TABLE) {
    const char *e = lookup(r.name);
    if (!e) continue;
    uint32_t &f = k.*r.field;
    const int v = r.rule == KnobRule::RangeLong ? 0 : atoi(e);   // atoi is undefined beyond int: the long rows never call it
    switch (r.rule) {
      case KnobRule::Range: if (v >= r.lo && v <= r.hi) f = (uint32_t)v; break;
      case KnobRule::RangeLong: { const long w = atol(e); if (w >= r.lo && w <= r.hi) f = (uint32_t)w; } break;
      case KnobRule::RangePow2: if (v >= r.lo && v <= r.hi && (v & (v - 1)) == 0) f = (uint32_t)v; break;
      case KnobRule::AtLeast: if (v >= r.lo) f = (uint32_t)v; break;
      case KnobRule::Set: if (v == r.lo || v == r.hi) f = (uint32_t)v; break;
      case KnobRule::FirstChar: if (e[0] >= '0' + r.lo && e[0] <= '0' + r.hi) f = (uint32_t)(e[0] - '0'); break;
      case KnobRule::Mask: f = (uint32_t)v & (uint32_t)r.hi; break;
      case KnobRule::ZeroOff: f = e[0] == '0' ? 0u : 1u; break;
      case KnobRule::NonZeroOn: f = v != 0; break;
    }
  }
}

}  // namespace mi355zk
