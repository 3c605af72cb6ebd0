// knobs_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around the knob table (scroll-prover_amd/csrc/knobs.hpp).  tests/test_knob_table.py builds it with
// -fsanitize=address,undefined and runs it; every case prints one line "name ok|WRONG ..." and the exit code is the number of cases that went wrong.  Never shipped.
// The "before" is parse_before(): the getenv lines init_ctx and mi355_init_multi carried until the table replaced them, VERBATIM (getenv is a macro for the injected lookup
// there, `g` a struct with the member initialisers Ctx had, the three globals locals with the values mi355_init_multi reset them to).  For every variable of the table and every
// input string -- unset, "", the bounds of its rule and their neighbours, "-1", "abc", "12abc", every member of every set / power-of-two / first-character rule with near-misses;
// nothing beyond int, where atoi is undefined -- the table must yield field for field what those lines yield, touch no field but the variable's own, and start from the same defaults.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../scroll-prover_amd/csrc/knobs.hpp"

using namespace mi355zk;
static int g_wrong = 0;
static void verdict(const std::string &name, bool ok, const std::string &why = "") {
  if (ok) std::printf("%s ok\n", name.c_str());
  else { std::printf("%s WRONG %s\n", name.c_str(), why.c_str()); g_wrong++; }
}

static std::map<std::string, std::string> g_env;
static const char *lookup(const char *name) { auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }

// ---- before: the members as Ctx declared them (the two the old code kept in locals or globals are added with the value the old code gave them when the variable is unset)
struct Before {
  uint32_t host_slice_min_log = 22; uint32_t host_batch_overlap = 1; uint32_t host_chunks = 8; uint32_t msm_chunks = 1;
  uint32_t sort_t2 = 0; uint32_t seg_factor = 16; uint32_t sort_fb = 11; uint32_t sort_split = 1; uint32_t reduce_chains = 131072; uint32_t seg_fill = 40, seg_fill_segfix = 40;
  uint32_t seg_min = 16; uint32_t fixup_mode = 2; uint32_t fixup_huge_min = 2048; uint32_t fixup_serial_max = 32; uint32_t fixup_lanes_max_log = 17; uint32_t tail_coop_mask = 15;
  uint32_t tail_coop_max = 65536; uint32_t reduce_min_chunk = 4; uint32_t sort_t1 = 16384; uint32_t ntt_direct2_max_log = 25; uint32_t ntt_coset_fold_max_log = 26;
  uint32_t ntt_direct2_min_log = 0; uint32_t ntt_fold_scale = 1; uint32_t ntt_batch_max_log = 22; uint32_t ntt_two_level_max_log = 18; uint32_t ntt_tile_log = 11; bool trace = false;
  // not Ctx members before
  uint32_t aux_prio_high = 1, allow_dup_devices = 0, multi_force = 0, msm_auto_max_c = 22, shard_min_log = 14;
};
constexpr int MSM_MAX_C = 24;
static Before parse_before() {
  Before g;
  bool g_force_exchange; int g_auto_max_c; uint32_t g_shard_min_log;
#define getenv lookup
  { const char *e = getenv("MI355_AUX_PRIO"); const bool high = !(e && e[0] == '0'); g.aux_prio_high = high; }
  { const char *e = getenv("MI355_MSM_CHUNKS"); if (e) { int v = atoi(e); if (v >= 1 && v <= 16) g.msm_chunks = (uint32_t)v; } }
  { const char *e = getenv("MI355_TRACE"); g.trace = e && e[0] == '1'; }
  { const char *e = getenv("MI355_REDUCE_CHAINS"); if (e) { int v = atoi(e); if (v >= 1024) g.reduce_chains = (uint32_t)v; } }
  { const char *e = getenv("MI355_SEG_FILL"); if (e) { int v = atoi(e); if (v >= 2 && v <= 100) g.seg_fill = (uint32_t)v; } }
  { const char *e = getenv("MI355_SEG_FILL_SEGFIX"); if (e) { int v = atoi(e); if (v >= 2 && v <= 100) g.seg_fill_segfix = (uint32_t)v; } }
  { const char *e = getenv("MI355_SEG_MIN"); if (e) { int v = atoi(e); if (v >= 1 && v <= 4096) g.seg_min = (uint32_t)v; } }
  { const char *e = getenv("MI355_FIXUP_MODE"); if (e && e[0] >= '0' && e[0] <= '2') g.fixup_mode = (uint32_t)(e[0] - '0'); }
  { const char *e = getenv("MI355_FIXUP_HUGE_MIN"); if (e) { long v = atol(e); if (v >= 2048 && v <= 0x7fffffffL) g.fixup_huge_min = (uint32_t)v; } }
  { const char *e = getenv("MI355_FIXUP_SERIAL_MAX"); if (e) { int v = atoi(e); if (v >= 1 && v <= 1024) g.fixup_serial_max = (uint32_t)v; } }
  { const char *e = getenv("MI355_FIXUP_LANES_MAX_LOG"); if (e) { int v = atoi(e); if (v >= 0 && v <= 31) g.fixup_lanes_max_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_TAIL_COOP_MASK"); if (e) g.tail_coop_mask = (uint32_t)atoi(e) & 15u; }
  { const char *e = getenv("MI355_TAIL_COOP_MAX"); if (e) { long v = atol(e); if (v >= 0 && v <= (1l << 24)) g.tail_coop_max = (uint32_t)v; } }
  { const char *e = getenv("MI355_REDUCE_MIN_CHUNK"); if (e) { int v = atoi(e); if (v >= 1 && v <= 64 && (v & (v - 1)) == 0) g.reduce_min_chunk = (uint32_t)v; } }
  { const char *e = getenv("MI355_SORT_FB"); if (e) { int v = atoi(e); if (v >= 9 && v <= 12) g.sort_fb = (uint32_t)v; } }
  { const char *e = getenv("MI355_SORT_SPLIT"); if (e && e[0] >= '1' && e[0] <= '2') g.sort_split = (uint32_t)(e[0] - '0'); }
  { const char *e = getenv("MI355_SEG_FACTOR"); if (e) { int v = atoi(e); if (v >= 1 && v <= 256) g.seg_factor = (uint32_t)v; } }
  { const char *e = getenv("MI355_SORT_T2"); if (e) { int v = atoi(e); if (v == 8192 || v == 16384) g.sort_t2 = (uint32_t)v; } }
  { const char *e = getenv("MI355_SORT_T1"); if (e && atoi(e) == 8192) g.sort_t1 = 8192; }
  { const char *e = getenv("MI355_NTT_DIRECT2_MAX_LOG"); if (e) { int v = atoi(e); if (v >= 0 && v <= 28) g.ntt_direct2_max_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_NTT_DIRECT2_MIN_LOG"); if (e) { int v = atoi(e); if (v >= 0 && v <= 28) g.ntt_direct2_min_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_NTT_FOLD_SCALE"); if (e) g.ntt_fold_scale = e[0] == '0' ? 0u : 1u; }
  { const char *e = getenv("MI355_NTT_COSET_FOLD_MAX_LOG"); if (e) { int v = atoi(e); if (v >= 0 && v <= 28) g.ntt_coset_fold_max_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_NTT_BATCH_MAX_LOG"); if (e) { int v = atoi(e); if (v >= 0 && v <= 28) g.ntt_batch_max_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_NTT_TWO_LEVEL_MAX_LOG"); if (e) { int v = atoi(e); if (v >= 9 && v <= 20) g.ntt_two_level_max_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_NTT_TILE_LOG"); if (e) { int v = atoi(e); if (v >= 8 && v <= 12) g.ntt_tile_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_HOST_BATCH_OVERLAP"); if (e) g.host_batch_overlap = atoi(e) != 0; }
  { const char *e = getenv("MI355_HOST_CHUNKS"); if (e) { int v = atoi(e); if (v >= 1 && v <= 64) g.host_chunks = (uint32_t)v; } }
  { const char *e = getenv("MI355_HOST_SLICE_MIN_LOG"); if (e) { int v = atoi(e); if (v >= 4 && v <= 31) g.host_slice_min_log = (uint32_t)v; } }
  { const char *e = getenv("MI355_ALLOW_DUP_DEVICES"); g.allow_dup_devices = !(!(e && e[0] == '1')); }   // was: if (!(e && e[0] == '1')) return fail(...)
  { const char *e = getenv("MI355_MULTI_FORCE"); g_force_exchange = e && e[0] == '1'; }
  { const char *e = getenv("MI355_MSM_AUTO_MAX_C"); g_auto_max_c = 22; if (e) { int v = atoi(e); if (v >= 16 && v <= MSM_MAX_C) g_auto_max_c = v; } }
  { const char *e = getenv("MI355_SHARD_MIN_LOG"); g_shard_min_log = 14; if (e) { int v = atoi(e); if (v >= 0 && v <= 30) g_shard_min_log = (uint32_t)v; } }
#undef getenv
  g.multi_force = g_force_exchange; g.msm_auto_max_c = (uint32_t)g_auto_max_c; g.shard_min_log = g_shard_min_log;
  return g;
}

// field-for-field comparison, driven by the lists that generate the structs (a field added to knobs.hpp without a line above does not compile here)
static std::string differences(const Before &o, const AllKnobs &n) {
  std::string d;
#define CMP(field, dflt, name, ...) if ((uint32_t)o.field != n.field) d += std::string(" ") + name + ": before " + std::to_string((uint32_t)o.field) + " table " + std::to_string(n.field);
  MI355_DEVICE_KNOBS(CMP) MI355_PROCESS_KNOBS(CMP)
#undef CMP
  return d;
}

int main() {
  const size_t rows = sizeof(KNOB_TABLE) / sizeof(KNOB_TABLE[0]);
  verdict("table_has_33_rows", rows == 33, std::to_string(rows));
  { std::set<std::string> names; for (const KnobRow &r : KNOB_TABLE) names.insert(r.name); verdict("names_are_distinct", names.size() == rows); }

  // defaults: the structs' initialisers, the rows' default column and the members Ctx had
  { g_env.clear(); AllKnobs n; const AllKnobs fresh; apply_knobs(n, lookup);
    std::string d = differences(Before(), fresh) + differences(parse_before(), n);
    for (const KnobRow &r : KNOB_TABLE) if (fresh.*r.field != r.dflt) d += std::string(" row default of ") + r.name;
    verdict("defaults_equal_the_earlier_initialisers", d.empty(), d); }

  // the inputs: a common list for every variable, plus the bounds of the variable's own row and their neighbours
  std::vector<std::string> common = {"", "0", "1", "2", "3", "-1", "-2", "abc", "12abc", "1abc", "0abc", "2x", " 1", "+1", "01", "00", "09", "1.5", "/", ":", "9", "10",
                                     "4", "5", "7", "8", "15", "16", "17", "31", "32", "33", "48", "63", "64", "65", "100", "101", "127", "128", "255", "256", "257", "1023", "1024", "1025",
                                     "2047", "2048", "2049", "4095", "4096", "4097", "8191", "8192", "8193", "16383", "16384", "16385", "65535", "65536", "131072",
                                     "16777215", "16777216", "16777217", "2147483646", "2147483647", "-2147483648"};
  size_t cases = 0;
  for (const KnobRow &r : KNOB_TABLE) {
    std::vector<std::string> in = common;
    for (long b : {r.lo - 1, r.lo, r.lo + 1, r.hi - 1, r.hi, r.hi + 1}) if (b >= INT_MIN && b <= INT_MAX) in.push_back(std::to_string(b));
    std::string d; bool accepted_something = false;
    for (const std::string &v : in) {
      g_env.clear(); g_env[r.name] = v;
      AllKnobs n; apply_knobs(n, lookup);
      const std::string diff = differences(parse_before(), n);
      if (!diff.empty()) d += " [\"" + v + "\":" + diff + "]";
      for (const KnobRow &other : KNOB_TABLE) if (&other != &r && n.*other.field != other.dflt) d += " [\"" + v + "\" moved " + other.name + "]";
      accepted_something = accepted_something || n.*r.field != r.dflt;
      cases++;
    }
    if (!accepted_something) d += " no input changed the field";
    verdict(r.name, d.empty(), d);
  }
  // every variable at once: the rows do not interfere
  { g_env.clear(); for (const KnobRow &r : KNOB_TABLE) g_env[r.name] = r.rule == KnobRule::FirstChar || r.rule == KnobRule::ZeroOff || r.rule == KnobRule::NonZeroOn ? (r.dflt ? "0" : "1") : std::to_string(r.rule == KnobRule::Mask ? 5 : r.lo);
    AllKnobs n; apply_knobs(n, lookup); const std::string d = differences(parse_before(), n); verdict("all_set_together", d.empty(), d); }
  std::printf("# %zu single-variable cases\n", cases);
  return g_wrong;
}
