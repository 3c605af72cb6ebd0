// buf_registry_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around BufRegistry (scroll-prover_amd/csrc/buf_registry.hpp), the bookkeeping behind mi355_buf_*.
// tests/test_buf_registry_on_host.py builds it with -fsanitize=address,undefined and runs it; every property prints one line "name ok|WRONG ..." and the exit code is the number
// of properties that went wrong.  Never shipped.
// Random alloc / free / recycle / trim sequences on two slots go through the registry's OWN allocation decision (alloc_step): the driver below only plays the part lib_core.hip
// plays around it -- it "allocates" a slab from a counter where the library calls hipMalloc (sometimes refusing the shared slab, as HIP does near the memory limit, so that the
// exact-size retry runs too) and moves blocks where the library waits for events.  Block sizes: the 2^20-, 2^24- and 2^25-row layers of a prover process scaled down by 2^12
// (8 KiB, 128 KiB, 256 KiB against a 256 KiB shared slab), plus 256-byte and 4 KiB staging blocks.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../scroll-prover_amd/csrc/buf_registry.hpp"

using namespace mi355zk;

static std::map<std::string, int> g_fail;   // property -> violations
static void expect(const char *prop, bool ok) { g_fail[prop] += ok ? 0 : 1; }

struct Model {
  BufRegistry R;
  SlabPolicy pol;
  std::mt19937_64 rng;
  uintptr_t next_base = 1 << 20;
  std::set<uintptr_t> device;                   // bases the fake device has handed out and not got back
  std::map<uintptr_t, size_t> mine[2];          // what the caller holds per slot: base -> bytes
  explicit Model(uint64_t seed, bool arena) : rng(seed) { pol.on = arena; pol.slab_min = 1 << 18; }

  uintptr_t dev_malloc(size_t bytes) { const uintptr_t p = next_base; next_base += bytes + ((rng() & 1) ? 0 : 4096); device.insert(p); return p; }   // some regions touch the previous one
  void dev_free(uintptr_t p) { expect("device_memory_freed_once", device.erase(p) == 1); }

  void recycle(int slot) { R.give_back(slot, R.take_pooled(slot, true)); }
  // mi355_buf_alloc without HIP
  void *alloc(int slot, size_t want) {
    const auto hit = R.pool.find({slot, want});
    const void *pooled = hit == R.pool.end() ? nullptr : hit->second.p;
    void *got = nullptr;
    for (bool recycled = false, slab_added = false; !got;) {
      const AllocStep st = R.alloc_step(slot, want, recycled, pol);
      switch (st.kind) {
        case AllocStep::Block: got = st.p; break;
        case AllocStep::Recycle: expect("recycle_asked_once", !recycled); recycle(slot); recycled = true; break;
        case AllocStep::Slab: {
          expect("new_slab_serves_the_request", !slab_added); if (slab_added) return nullptr;
          expect("slab_size_and_kind", st.bytes == std::max(want, pol.slab_min) && st.dedicated == (want >= pol.slab_min));
          const size_t bytes = (st.bytes > want && rng() % 8 == 0) ? want : st.bytes;   // the shared slab "did not fit": exactly the request
          R.add_slab(slot, (void *)dev_malloc(bytes), bytes, st.dedicated, pol); slab_added = true;
        } break;
        case AllocStep::Direct: expect("direct_only_without_slabs", !pol.on); got = (void *)dev_malloc(want); R.adopt(slot, got, want, false); break;
      }
    }
    if (pooled) expect("freed_block_is_reused_for_its_size", got == pooled);
    if (pol.on && want < pol.slab_min / 64) { const auto *sl = R.arena[slot].slab_of((uintptr_t)got); expect("small_block_not_in_dedicated_slab", sl && !sl->dedicated); }
    mine[slot][(uintptr_t)got] = want;
    return got;
  }
  void release(int slot, uintptr_t p) {
    BufBlock b; expect("base_pointer_frees", R.take_live((void *)p, &b) && b.slot == slot && b.bytes == mine[slot][p]);
    BufBlock again; expect("second_free_is_refused", !R.take_live((void *)p, &again));
    b.free_ev = (void *)(p | 1);   // an opaque handle: the registry must carry it, never look into it
    R.pool_put(b); mine[slot].erase(p);
  }
  // mi355_buf_trim / the out-of-memory retry for one slot: direct blocks and whole slabs go back to the device
  void drain(int slot) {
    for (const auto &b : R.take_pooled(slot, false)) { expect("direct_blocks_are_not_carved", !b.arena); dev_free((uintptr_t)b.p); }
    recycle(slot);
    std::vector<uintptr_t> gone; R.arena[slot].take_whole_slabs(gone);
    for (uintptr_t q : gone) dev_free(q);
  }

  void check() {
    // every byte of every slab is exactly one of: live, pooled, free; nothing overlaps; nothing leaves its slab
    std::map<uintptr_t, std::pair<size_t, int>> all;   // start -> (bytes, 0 live / 1 pooled / 2 free)
    size_t covered = 0, slab_total = 0; bool unique = true;
    for (auto &kv : R.live) { unique = unique && all.emplace(kv.first, std::make_pair(kv.second.bytes, 0)).second; }
    for (auto &kv : R.pool) { unique = unique && all.emplace((uintptr_t)kv.second.p, std::make_pair(kv.second.bytes, 1)).second; expect("pool_key_matches_block", kv.first.first == kv.second.slot && kv.first.second == kv.second.bytes && kv.second.free_ev == (void *)((uintptr_t)kv.second.p | 1)); }
    for (int s = 0; s < 2; s++) for (auto &kv : R.arena[s].free_ranges) unique = unique && all.emplace(kv.first, std::make_pair(kv.second, 2)).second;
    expect("no_two_ranges_start_together", unique);
    uintptr_t prev_end = 0;
    for (auto &kv : all) { expect("live_pooled_free_never_overlap", kv.first >= prev_end); prev_end = kv.first + kv.second.first; covered += kv.second.first; }
    for (int s = 0; s < 2; s++) for (auto &sl : R.arena[s].slabs) slab_total += sl.bytes;
    if (pol.on) expect("every_slab_byte_is_live_pooled_or_free", covered == slab_total);
    // what the registry calls live is what the caller holds
    size_t held = 0; for (int s = 0; s < 2; s++) { size_t b = 0; for (auto &kv : mine[s]) b += kv.second; expect("live_bytes_per_slot", R.live_bytes(s) == b); held += mine[s].size(); }
    expect("live_is_what_the_caller_holds", held == R.live.size());
    for (int s = 0; s < 2; s++) for (auto &kv : mine[s]) {
      const uintptr_t p = kv.first; const size_t n = kv.second;
      BufBlock *b = R.find((void *)p);
      expect("interior_pointer_finds_its_owner", b && (uintptr_t)b->p == p && b->slot == s && R.find((void *)(p + n - 1)) == b && R.find((void *)(p + n / 2)) == b && R.find((void *)(p + n)) != b);
      if (!b) continue;
      const size_t off = n / 3;
      expect("range_check_accepts_to_the_end", BufRegistry::fits(*b, (void *)p, n) && BufRegistry::fits(*b, (void *)(p + off), n - off) && BufRegistry::fits(*b, (void *)(p + n - 1), 1) && BufRegistry::fits(*b, (void *)p, 0));
      expect("range_check_rejects_one_past_the_end", !BufRegistry::fits(*b, (void *)p, n + 1) && !BufRegistry::fits(*b, (void *)(p + off), n - off + 1) && !BufRegistry::fits(*b, (void *)(p + n - 1), 2) && !BufRegistry::fits(*b, (void *)p, ~0ull));
    }
    for (auto &kv : all) if (kv.second.second != 0) expect("pointer_into_free_memory_finds_nothing", !R.find((void *)kv.first) && !R.find((void *)(kv.first + kv.second.first - 1)) && !R.find((void *)(kv.first + kv.second.first / 2)));
  }
};

static void run(uint64_t seed, bool arena) {
  Model M(seed, arena);
  const size_t sizes[5] = {8192, 131072, 262144, 256, 4096};
  for (int step = 0; step < 1000; step++) {
    const int slot = (int)(M.rng() & 1); const unsigned op = (unsigned)(M.rng() % 32);
    if (op < 17 || M.mine[slot].empty()) M.alloc(slot, sizes[M.rng() % 5]);
    else if (op < 29) { auto it = M.mine[slot].begin(); std::advance(it, M.rng() % M.mine[slot].size()); M.release(slot, it->first); }
    else if (op < 31) M.recycle(slot);
    else {
      // one slot's drain leaves the other slot's pool, free ranges and slabs alone
      const int other = 1 - slot;
      const auto pool_before = M.R.pool.count({other, 0}) + M.R.pooled_bytes(other); const auto ranges_before = M.R.arena[other].free_ranges; const size_t slabs_before = M.R.arena[other].slabs.size();
      std::vector<uintptr_t> other_pooled; for (auto &kv : M.R.pool) if (kv.first.first == other) other_pooled.push_back((uintptr_t)kv.second.p);
      M.drain(slot);
      std::vector<uintptr_t> other_after; for (auto &kv : M.R.pool) if (kv.first.first == other) other_after.push_back((uintptr_t)kv.second.p);
      expect("drain_of_one_slot_moves_nothing_of_the_other", other_pooled == other_after && ranges_before == M.R.arena[other].free_ranges && slabs_before == M.R.arena[other].slabs.size() && pool_before == M.R.pool.count({other, 0}) + M.R.pooled_bytes(other));
      expect("drain_empties_the_slots_pool", M.R.take_pooled(slot, true).empty() && M.R.take_pooled(slot, false).empty());
    }
    M.check();
  }
  // everything comes back: every slab is one range again and take_whole_slabs returns all of them
  for (int s = 0; s < 2; s++) while (!M.mine[s].empty()) M.release(s, M.mine[s].begin()->first);
  M.check();
  for (int s = 0; s < 2; s++) {
    M.recycle(s);
    bool whole = true; for (auto &sl : M.R.arena[s].slabs) { auto f = M.R.arena[s].free_ranges.find(sl.base); whole = whole && f != M.R.arena[s].free_ranges.end() && f->second == sl.bytes; }
    expect("all_freed_every_slab_is_one_range", whole && M.R.arena[s].free_ranges.size() == M.R.arena[s].slabs.size());
    M.drain(s);
    expect("all_freed_every_slab_goes_back", M.R.arena[s].slabs.empty() && M.R.arena[s].free_ranges.empty() && M.R.pooled_bytes(s) == 0 && M.R.live_bytes(s) == 0);
  }
  expect("all_freed_every_slab_goes_back", M.device.empty() && M.R.pool.empty() && M.R.live.empty());
  // shutdown's sweep takes live and pooled blocks of a slot alike
  void *a = M.alloc(0, 4096), *b = M.alloc(0, 8192), *c = M.alloc(1, 4096); M.release(0, (uintptr_t)b); (void)a;
  const auto swept = M.R.take_all(0);
  expect("take_all_takes_live_and_pooled_of_one_slot", swept.size() == 2 && M.R.find(a) == nullptr && M.R.find(c) != nullptr && M.R.live.size() == 1 && M.R.pool.empty());
}

int main() {
  for (const char *p : {"device_memory_freed_once", "recycle_asked_once", "new_slab_serves_the_request", "slab_size_and_kind", "direct_only_without_slabs", "freed_block_is_reused_for_its_size",
                        "small_block_not_in_dedicated_slab", "base_pointer_frees", "second_free_is_refused", "direct_blocks_are_not_carved", "pool_key_matches_block", "no_two_ranges_start_together",
                        "live_pooled_free_never_overlap", "every_slab_byte_is_live_pooled_or_free", "live_bytes_per_slot", "live_is_what_the_caller_holds", "interior_pointer_finds_its_owner",
                        "range_check_accepts_to_the_end", "range_check_rejects_one_past_the_end", "pointer_into_free_memory_finds_nothing", "drain_of_one_slot_moves_nothing_of_the_other",
                        "drain_empties_the_slots_pool", "all_freed_every_slab_is_one_range", "all_freed_every_slab_goes_back", "take_all_takes_live_and_pooled_of_one_slot"}) g_fail[p] = 0;
  for (uint64_t seed = 1; seed <= 6; seed++) run(seed, true);
  run(7, false);   // MI355_BUF_ARENA=0: one allocation per block, reuse by exact size only
  int wrong = 0;
  for (auto &kv : g_fail) { if (kv.second) { std::printf("%s WRONG %d violations\n", kv.first.c_str(), kv.second); wrong++; } else std::printf("%s ok\n", kv.first.c_str()); }
  return wrong;
}
