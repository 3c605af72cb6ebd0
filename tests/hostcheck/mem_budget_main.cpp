// mem_budget_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around MemLedger (scroll-prover_amd/csrc/mem_budget.hpp), the ledger behind dev_malloc / dev_free and
// mi355_mem_set_limit / _usage / _reset_peak.  tests/test_mem_budget_on_host.py builds it with -fsanitize=address,undefined and runs it; every property prints one line
// "name ok|WRONG ..." and the exit code is the number of properties that went wrong.  Never shipped.
// Random charge / release / reclaim sequences on two slots go through the ledger's OWN decision (reserve_step): the driver below only plays the part lib_core.hip plays around
// it -- it "allocates" from a counter where the library calls hipMalloc, keeps freed buffer blocks as a pool that the first reclaim gives back, keeps optional tables that the
// second reclaim gives back -- and a plain model (sums over what the driver holds) says what every step must have decided.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../scroll-prover_amd/csrc/mem_budget.hpp"

using namespace mi355zk;

static std::map<std::string, int> g_fail;   // property -> violations
static void expect(const char *prop, bool ok) { g_fail[prop] += ok ? 0 : 1; }

struct Block { uintptr_t p; uint64_t bytes; MemClass cls; };
struct Driver {
  MemLedger L;
  std::mt19937_64 rng;
  uintptr_t next = 1 << 20;
  std::vector<Block> live[2], pooled[2], optional[2];   // what the "library" holds per slot: in use | freed buffer blocks | optional tables
  uint64_t limit[2] = {0, 0}, peak[2] = {0, 0}, refused[2] = {0, 0}, reclaims[2] = {0, 0};
  bool allocator_fails_sometimes = true;
  explicit Driver(uint64_t seed) : rng(seed) {}

  static uint64_t sum(const std::vector<Block> &v) { uint64_t n = 0; for (const auto &b : v) n += b.bytes; return n; }
  uint64_t model_held(int s) const { return sum(live[s]) + sum(pooled[s]) + sum(optional[s]); }
  uint64_t model_class(int s, int c) const { uint64_t n = 0; for (const auto *v : {&live[s], &pooled[s], &optional[s]}) for (const auto &b : *v) if (b.cls == c) n += b.bytes; return n; }
  bool model_fits(int s, uint64_t bytes) const { return limit[s] == 0 || model_held(s) + bytes <= limit[s]; }

  uint64_t drop(int s, std::vector<Block> &v) {
    uint64_t freed = 0;
    for (const auto &b : v) { MemLedger::Rec r; expect("release_finds_what_was_bound", L.release((void *)b.p, &r) && r.bytes == b.bytes && r.slot == s && r.cls == b.cls); freed += b.bytes; }
    v.clear(); L.reclaimed(s, freed); if (freed) reclaims[s]++;
    return freed;
  }
  // dev_malloc without HIP; returns whether the request was served
  bool alloc(int s, MemClass cls, uint64_t bytes, MemMode mode) {
    const MemSlot before_other = L.slot[1 - s];
    const uint64_t pool_bytes = sum(pooled[s]), opt_bytes = sum(optional[s]);
    // what the plain model expects
    const bool fits0 = model_fits(s, bytes);
    const bool fits1 = limit[s] == 0 || model_held(s) - pool_bytes + bytes <= limit[s];
    const bool fits2 = limit[s] == 0 || model_held(s) - pool_bytes - opt_bytes + bytes <= limit[s];
    const bool want_ok = fits0 || (mode != MemMode::Spare && fits1) || (mode == MemMode::Required && fits2);
    const int want_reclaims = fits0 || mode == MemMode::Spare ? 0 : (fits1 || mode == MemMode::Headroom) ? 1 : 2;
    int stage = 0; bool ok = false;
    for (;;) {
      const MemSlot snap = L.slot[s];
      const MemStep st = L.reserve_step(s, cls, bytes, stage, mode);
      if (st == MemStep::Charged) { ok = true; break; }
      if (st == MemStep::Refused) {
        bool same = snap.held == L.slot[s].held && snap.high_water == L.slot[s].high_water && snap.limit == L.slot[s].limit && snap.reclaims == L.slot[s].reclaims;
        for (int c = 0; c < MEM_CLASSES; c++) same = same && snap.by_class[c] == L.slot[s].by_class[c];
        expect("a_refusal_changes_nothing", same && L.slot[s].refused_bytes == snap.refused_bytes + (mode == MemMode::Required ? bytes : 0));
        if (mode == MemMode::Required) refused[s] += bytes;
        const std::string msg = L.describe_refusal(s, bytes, "test");
        expect("refusal_names_limit_held_and_request", msg.find(std::to_string(limit[s])) != std::string::npos && msg.find(std::to_string(model_held(s))) != std::string::npos && msg.find(std::to_string(bytes)) != std::string::npos && msg.find("ntt_optional") != std::string::npos);
        break;
      }
      expect("reclaim_order_pool_then_tables_then_refuse", (st == MemStep::ReclaimPool && stage == 0) || (st == MemStep::ReclaimTables && stage == 1 && mode == MemMode::Required));
      if (st == MemStep::ReclaimPool) drop(s, pooled[s]); else drop(s, optional[s]);
      if (++stage > 2) { expect("reclaim_order_pool_then_tables_then_refuse", false); break; }
    }
    expect("reclaim_order_pool_then_tables_then_refuse", stage == want_reclaims);
    expect("decision_matches_the_plain_model", ok == want_ok);
    expect("limit_zero_refuses_nothing", limit[s] != 0 || (ok && stage == 0));
    expect("spare_requests_reclaim_nothing", mode != MemMode::Spare || stage == 0);
    if (ok) {
      if (allocator_fails_sometimes && rng() % 16 == 0) { L.cancel(s, cls, bytes); ok = false; }   // the allocator failed after all: the reservation is returned
      else { const Block b{next, bytes, cls}; next += bytes + 256; L.bind((void *)b.p, s, cls, bytes); (cls == MEM_NTT_OPTIONAL ? optional[s] : live[s]).push_back(b); }
      peak[s] = std::max(peak[s], model_held(s) + (ok ? 0 : bytes));
    }
    const MemSlot &o = L.slot[1 - s]; bool same = o.held == before_other.held && o.high_water == before_other.high_water && o.limit == before_other.limit && o.reclaims == before_other.reclaims && o.refused_bytes == before_other.refused_bytes;
    for (int c = 0; c < MEM_CLASSES; c++) same = same && o.by_class[c] == before_other.by_class[c];
    expect("slots_are_independent", same);
    return ok;
  }
  void free_one(int s) {
    if (live[s].empty()) return;
    const size_t i = rng() % live[s].size(); const Block b = live[s][i]; live[s].erase(live[s].begin() + (long)i);
    if (b.cls == MEM_BUF) { pooled[s].push_back(b); return; }   // mi355_buf_free: the block stays held, in the pool
    expect("release_finds_what_was_bound", L.release((void *)b.p));
    expect("second_release_is_refused", !L.release((void *)b.p));
  }
  void check() {
    for (int s = 0; s < 2; s++) {
      const MemSlot &m = L.slot[s]; uint64_t by = 0; bool classes = true;
      for (int c = 0; c < MEM_CLASSES; c++) { by += m.by_class[c]; classes = classes && m.by_class[c] == model_class(s, c); }
      expect("held_equals_sum_of_classes", m.held == by);
      expect("held_is_what_the_driver_holds", m.held == model_held(s) && classes);
      expect("high_water_is_the_peak_since_reset", m.high_water == peak[s] && m.high_water >= m.held);
      expect("counters_match", m.refused_bytes == refused[s] && m.reclaims == reclaims[s] && m.limit == limit[s]);
      expect("room_is_min_of_free_and_limit_minus_held", L.room(s, 1000) == (limit[s] == 0 ? 1000 : std::min<uint64_t>(1000, limit[s] > model_held(s) ? limit[s] - model_held(s) : 0)));
    }
    size_t blocks = 0; for (int s = 0; s < 2; s++) blocks += live[s].size() + pooled[s].size() + optional[s].size();
    expect("held_is_what_the_driver_holds", L.recs.size() == blocks);
  }
};

static void run(uint64_t seed) {
  Driver D(seed);
  const uint64_t sizes[6] = {256, 4096, 36864, 131072, 262144, 1 << 20};
  uint64_t held_at_limit_set[2] = {0, 0}; bool limited_since[2] = {false, false};
  for (int step = 0; step < 3000; step++) {
    const int s = (int)(D.rng() & 1); const unsigned op = (unsigned)(D.rng() % 64);
    const uint64_t last_peak = D.L.slot[s].high_water;
    bool reset = false;
    if (op < 30) {
      const unsigned k = (unsigned)(D.rng() % 10);
      const MemClass cls = k < 5 ? MEM_BUF : k < 6 ? MEM_WORKSPACE : k < 8 ? MEM_NTT_OPTIONAL : k < 9 ? MEM_NTT_REQUIRED : MEM_SRS;
      const MemMode mode = cls == MEM_NTT_OPTIONAL ? MemMode::Spare : (cls == MEM_BUF || cls == MEM_WORKSPACE) && D.rng() % 4 == 0 ? MemMode::Headroom : MemMode::Required;
      const uint64_t held_before = D.L.slot[s].held, pool_before = Driver::sum(D.pooled[s]) + Driver::sum(D.optional[s]);
      D.alloc(s, cls, sizes[D.rng() % 6], mode);
      if (D.limit[s]) expect("held_never_exceeds_a_limit_it_was_under", held_before > D.limit[s] || D.L.slot[s].held <= D.limit[s]);
      if (limited_since[s] && held_before > D.limit[s]) expect("lowered_limit_refuses_but_frees_only_by_reclaim", D.L.slot[s].held <= held_before && held_before - D.L.slot[s].held <= pool_before);
    }
    else if (op < 56) D.free_one(s);
    else if (op < 58) { D.drop(s, D.pooled[s]); }                                  // mi355_buf_trim
    else if (op < 62) {
      const unsigned how = (unsigned)(D.rng() % 4);
      const uint64_t h = D.model_held(s);
      D.limit[s] = how == 0 ? 0 : how == 1 ? h / 2 : how == 2 ? h + sizes[D.rng() % 6] * 3 : h;   // none | below held | a little room | exactly held
      const MemSlot snap = D.L.slot[s];
      D.L.set_limit(s, D.limit[s]); held_at_limit_set[s] = h; limited_since[s] = D.limit[s] != 0;
      expect("set_limit_frees_nothing", D.L.slot[s].held == snap.held && D.L.slot[s].high_water == snap.high_water && D.L.recs.size() == D.live[0].size() + D.live[1].size() + D.pooled[0].size() + D.pooled[1].size() + D.optional[0].size() + D.optional[1].size());
    }
    else { D.L.reset_peak(s); D.peak[s] = D.model_held(s); reset = true; }
    if (!reset) expect("high_water_is_monotone_until_reset", D.L.slot[s].high_water >= last_peak);
    D.check();
  }
  (void)held_at_limit_set;
  // everything goes back: nothing is held, the peak stays until it is reset
  for (int s = 0; s < 2; s++) { D.L.set_limit(s, 0); D.limit[s] = 0; while (!D.live[s].empty()) D.free_one(s); D.drop(s, D.pooled[s]); D.drop(s, D.optional[s]); }
  D.check();
  expect("all_released_nothing_held", D.L.slot[0].held == 0 && D.L.slot[1].held == 0 && D.L.recs.empty());
}

int main() {
  for (const char *p : {"held_equals_sum_of_classes", "held_is_what_the_driver_holds", "held_never_exceeds_a_limit_it_was_under", "high_water_is_monotone_until_reset", "high_water_is_the_peak_since_reset",
                        "reclaim_order_pool_then_tables_then_refuse", "a_refusal_changes_nothing", "slots_are_independent", "limit_zero_refuses_nothing", "lowered_limit_refuses_but_frees_only_by_reclaim",
                        "set_limit_frees_nothing", "decision_matches_the_plain_model", "spare_requests_reclaim_nothing", "refusal_names_limit_held_and_request", "release_finds_what_was_bound",
                        "second_release_is_refused", "counters_match", "room_is_min_of_free_and_limit_minus_held", "all_released_nothing_held"}) g_fail[p] = 0;
  for (uint64_t seed = 1; seed <= 8; seed++) run(seed);
  // a fixed case of every outcome, so that no property above passes for want of an event
  {
    Driver D(99); D.allocator_fails_sometimes = false;
    D.alloc(0, MEM_BUF, 1000, MemMode::Required); D.alloc(0, MEM_BUF, 1000, MemMode::Required); D.check(); D.alloc(0, MEM_NTT_OPTIONAL, 500, MemMode::Spare); D.alloc(0, MEM_SRS, 700, MemMode::Required);
    D.pooled[0].push_back(D.live[0][0]); D.live[0].erase(D.live[0].begin());                     // mi355_buf_free of the first block
    const uint64_t h = D.model_held(0), pool = Driver::sum(D.pooled[0]), opt = Driver::sum(D.optional[0]);
    D.limit[0] = h; D.L.set_limit(0, h);
    const bool a = D.alloc(0, MEM_WORKSPACE, pool ? pool : 1, MemMode::Required);                 // only by giving the pool back
    const bool b = D.alloc(0, MEM_WORKSPACE, opt ? opt : 1, MemMode::Required);                   // only by giving the tables back
    const bool c = D.alloc(0, MEM_WORKSPACE, 1, MemMode::Required);                               // nothing left to give
    D.check();
    expect("reclaim_order_pool_then_tables_then_refuse", pool == 1000 && opt == 500 && a && b && !c && D.pooled[0].empty() && D.optional[0].empty());
    D.limit[0] = 1; D.L.set_limit(0, 1);
    const uint64_t held = D.L.slot[0].held;
    expect("lowered_limit_refuses_but_frees_only_by_reclaim", !D.alloc(0, MEM_BUF, 1, MemMode::Required) && D.L.slot[0].held == held);
    D.limit[0] = 0; D.L.set_limit(0, 0);
    expect("limit_zero_refuses_nothing", D.alloc(0, MEM_BUF, uint64_t(1) << 40, MemMode::Required) || true);
    D.check();
  }
  int wrong = 0;
  for (auto &kv : g_fail) { if (kv.second) { std::printf("%s WRONG %d violations\n", kv.first.c_str(), kv.second); wrong++; } else std::printf("%s ok\n", kv.first.c_str()); }
  return wrong;
}
