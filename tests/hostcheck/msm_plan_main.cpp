// msm_plan_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around the MSM launch planner (scroll-prover_amd/csrc/msm_plan.hpp).  tests/test_msm_plan_on_host.py builds it
// with -fsanitize=address,undefined, feeds it one case per line on stdin and compares the line it prints for each with tests/msm_plan_common.py.  Never shipped.
// A case is a list of key=value words.  op = plan | leaves | chunks | slices | window; n, M, tab_c (0: no tables), rec (144 | 256), forced_c / forced_shared (forced_c = 0: none),
// force_c, no_tables, cus, chunk_min_log, have_c; every other key is an environment name of csrc/knobs.hpp and goes through apply_knobs like the real environment.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../scroll-prover_amd/csrc/msm_plan.hpp"

using namespace mi355zk;

static std::map<std::string, std::string> g_case;
static const char *lookup(const char *name) { auto it = g_case.find(name); return it == g_case.end() ? nullptr : it->second.c_str(); }
static uint64_t num(const char *key, uint64_t dflt) { const char *v = lookup(key); return v ? strtoull(v, nullptr, 10) : dflt; }

static std::string words(const char *s) { std::string r = s ? s : "-"; for (char &ch : r) if (ch == ' ') ch = '_'; return r; }
static const char *fixup_name(Fixup f) { return f == Fixup::Segmented ? "segmented" : f == Fixup::Quad ? "quad" : f == Fixup::FourLanes ? "four_lanes" : "one_lane"; }

static void print_plan(const PassPlan &p, MsmGroup grp) {
  std::printf("refusal=%s must_split=%d n=%llu M=%u shared=%d c=%u W=%u fb=%u cb_bits=%u regions=%u entries=%llu buckets=%llu", words(p.refusal).c_str(), must_split(p, grp) ? 1 : 0,
              (unsigned long long)p.n, p.M, p.shared ? 1 : 0, p.c, p.W, p.fb, p.cb_bits, p.regions, (unsigned long long)p.emax, (unsigned long long)p.nbuckets);
  if (p.ok())
    std::printf(" seg=%u blocks=%u tn=%u seg_arg=%u fixup_kind=%s big_cap=%u huge_cap=%u t1=%u t2=%u tiles1=%u l2_tiles_max=%u chunk=%u chunks_per_set=%u quad_sums=%d tree_quad_max=%u quad_final=%d",
                p.seg, p.blocks, p.tn, p.seg_arg, fixup_name(p.fixup), p.big_cap, p.huge_cap, p.t1, p.t2, p.tiles1, p.l2_tiles_max, p.chunk, p.chunks_per_set, p.quad_sums ? 1 : 0, p.tree_quad_max,
                p.quad_final ? 1 : 0);
}
// the batch sizes msm_batch (lib_msm.hip) runs a batch of M as
static void leaves(const PlanIn &in, uint64_t n, uint32_t M, TableShape tab, MsmGroup grp, std::string &out) {
  if (M > 1 && must_split(plan_pass(in, n, M, tab, grp), grp)) { leaves(in, n, M / 2, tab, grp, out); leaves(in, n, M - M / 2, tab, grp, out); return; }
  out += (out.empty() ? "" : ",") + std::to_string(M);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    g_case.clear();
    std::istringstream in_words(line); std::string w;
    while (in_words >> w) { const size_t eq = w.find('='); if (eq != std::string::npos) g_case[w.substr(0, eq)] = w.substr(eq + 1); }
    AllKnobs all; apply_knobs(all, lookup);
    PlanIn in; in.k = all; in.auto_max_c = all.msm_auto_max_c; in.chunk_min_log = (uint32_t)num("chunk_min_log", 23);
    in.force_c = (int)num("force_c", 0); in.no_tables = num("no_tables", 0) != 0; in.cus = (uint32_t)num("cus", 256);
    const uint64_t n = num("n", 0); const uint32_t M = (uint32_t)num("M", 1);
    const int tab_c = (int)num("tab_c", 0);
    const TableShape tab{tab_c, tab_c ? (MSM_SCALAR_BITS + tab_c - 1) / tab_c : 0};
    const MsmGroup grp = num("rec", 144) == 256 ? GROUP_G2 : GROUP_G1;
    const std::string op = lookup("op") ? lookup("op") : "";
    if (op == "plan") {
      const ForcedShape forced{(uint32_t)num("forced_c", 0), num("forced_shared", 0) != 0};
      print_plan(plan_pass(in, n, M, tab, grp, forced.c ? &forced : nullptr), grp);
    } else if (op == "leaves") {
      std::string out; leaves(in, n, M, tab, grp, out); std::printf("leaves=%s", out.c_str());
    } else if (op == "chunks") {
      std::printf("chunks=%u", pipeline_chunks(in, M, n));
    } else if (op == "slices") {
      const HostSlices hs = host_slices(in, n, M, tab, grp);
      std::string cuts; for (uint64_t c : hs.cut) cuts += (cuts.empty() ? "" : ",") + std::to_string(c);
      std::printf("cuts=%s slices=%u shape_c=%u shape_shared=%d shape_buckets=%llu", cuts.c_str(), hs.count(), hs.count() > 1 ? hs.shape.c : 0, hs.count() > 1 && hs.shape.shared ? 1 : 0,
                  hs.count() > 1 ? (unsigned long long)hs.shape.nbuckets : 0ull);
    } else if (op == "window") {   // mi355_srs_precompute's automatic choice for a per-shard hint, and whether tables of have_c stay
      const int best = best_window(n, in.auto_max_c, true); const int have = (int)num("have_c", 0);
      std::printf("best=%d keep=%d", best, have && tables_close_enough(n, have, best) ? 1 : 0);
    } else { std::printf("unknown-op"); }
    std::printf("\n");
  }
  return 0;
}
