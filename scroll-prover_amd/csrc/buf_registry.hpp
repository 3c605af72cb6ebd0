// buf_registry.hpp -- the bookkeeping behind mi355_buf_* (lib_core.hip "resident buffers"): which blocks are live, which wait in the pool, which ranges of which slab are free
// (slab_ranges.hpp), and where the next block comes from.  Plain C++, no HIP and no lock: lib_core.hip owns the device memory, the events (opaque handles here), the stream
// synchronisation and the one mutex every call below runs under, so the same code runs under tests/hostcheck/buf_registry_main.cpp against a byte map.
//
// Allocation order: a pooled block of exactly this size on this slot; else (slabs on) a range carved from the slot's free ranges; else, once, "recycle": the caller moves the slot's
// pooled carved blocks into the free ranges after their last use has completed and asks again; else a new slab -- max(want, slab_min) bytes, dedicated when the request alone is at
// least a shared slab (small blocks are never carved out of a dedicated slab, slab_ranges.hpp) -- after which the caller asks again.  With slabs off every miss is one allocation of
// its own ("direct").  A range only becomes free after the block it came from is quiescent, so a carved block is as fresh as one straight from the allocator.
#pragma once
#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "slab_ranges.hpp"

namespace mi355zk {

// free_ev: recorded on the owner's compute stream when the block last went back to the pool -- the only work an upload into the recycled block has to wait for.  used: the block
// has been passed to a library call since it was allocated (an upload into it must then wait for the whole compute stream).  arena: carved from a slab, not an allocation of its own.
struct BufBlock { void *p = nullptr; size_t bytes = 0; int slot = 0; void *free_ev = nullptr; bool used = false; bool arena = false; };
struct SlabPolicy { bool on = true; size_t slab_min = (size_t)1 << 30; };   // MI355_BUF_ARENA, MI355_BUF_SLAB_MB
struct AllocStep {
  enum Kind { Block, Recycle, Slab, Direct } kind;
  void *p;             // Block: the block, already registered as live
  size_t bytes;        // Slab: size of a shared or dedicated slab (near the memory limit the caller may give up the head-room and add a slab of exactly `want`); Direct: want
  bool dedicated;      // Slab: what to pass to add_slab
};

struct BufRegistry {
  static constexpr int MAX_SLOTS = 16;
  std::map<uintptr_t, BufBlock> live;                          // by base address
  std::multimap<std::pair<int, size_t>, BufBlock> pool;        // free blocks by (slot, size)
  SlabRanges arena[MAX_SLOTS];                                 // per slot: its slabs and their quiescent free ranges

  // the live block that holds p (any interior pointer), or null
  BufBlock *find(const void *p) {
    auto it = live.upper_bound((uintptr_t)p);
    if (it == live.begin()) return nullptr;
    --it;
    return (uintptr_t)p < it->first + it->second.bytes ? &it->second : nullptr;
  }
  // [p, p + bytes) stays inside b (p lies in b).  Blocks are carved next to each other inside slabs: an overrun lands in a neighbouring LIVE polynomial, not in a fault
  static bool fits(const BufBlock &b, const void *p, uint64_t bytes) { return bytes <= b.bytes - (uint64_t)((uintptr_t)p - (uintptr_t)b.p); }

  AllocStep alloc_step(int slot, size_t want, bool recycled, const SlabPolicy &pol) {
    auto it = pool.find({slot, want});
    if (it != pool.end()) { BufBlock b = it->second; pool.erase(it); b.used = false; live[(uintptr_t)b.p] = b; return {AllocStep::Block, b.p, want, false}; }
    if (!pol.on) return {AllocStep::Direct, nullptr, want, false};
    if (const uintptr_t p = arena[slot].carve(want)) { adopt(slot, (void *)p, want, true); return {AllocStep::Block, (void *)p, want, false}; }
    if (!recycled) return {AllocStep::Recycle, nullptr, 0, false};
    return {AllocStep::Slab, nullptr, std::max(want, pol.slab_min), want >= pol.slab_min};
  }
  void add_slab(int slot, void *base, size_t bytes, bool dedicated, const SlabPolicy &pol) {
    arena[slot].small_limit = pol.slab_min / 64;   // 16 MiB with the default 1 GiB slabs: staging blocks, pointer tables, short vectors
    arena[slot].add_slab((uintptr_t)base, bytes, dedicated);
  }
  void adopt(int slot, void *p, size_t bytes, bool from_arena) { BufBlock b; b.p = p; b.bytes = bytes; b.slot = slot; b.arena = from_arena; live[(uintptr_t)p] = b; }
  // mi355_buf_free: p must be the BASE of a live block; it leaves `live` (the caller records its free event and hands it to pool_put)
  bool take_live(const void *p, BufBlock *out) { auto it = live.find((uintptr_t)p); if (it == live.end()) return false; *out = it->second; live.erase(it); return true; }
  void pool_put(const BufBlock &b) { pool.insert({{b.slot, b.bytes}, b}); }
  // the pooled blocks of one slot leave the pool: the carved ones (to go back to their slab) or the directly allocated ones (to go back to the allocator)
  std::vector<BufBlock> take_pooled(int slot, bool carved) {
    std::vector<BufBlock> out;
    for (auto it = pool.lower_bound({slot, 0}); it != pool.end() && it->first.first == slot;) { if (it->second.arena == carved) { out.push_back(it->second); it = pool.erase(it); } else ++it; }
    return out;
  }
  // shutdown: every block of the slot, live or pooled
  std::vector<BufBlock> take_all(int slot) {
    std::vector<BufBlock> out = take_pooled(slot, true), direct = take_pooled(slot, false);
    out.insert(out.end(), direct.begin(), direct.end());
    for (auto it = live.begin(); it != live.end();) { if (it->second.slot == slot) { out.push_back(it->second); it = live.erase(it); } else ++it; }
    return out;
  }
  void give_back(int slot, const std::vector<BufBlock> &carved) { for (const auto &b : carved) arena[slot].insert((uintptr_t)b.p, b.bytes); }
  bool holds_carved(int slot) const {   // something of this slot could still go back to the allocator through its slabs
    if (!arena[slot].free_ranges.empty()) return true;
    for (auto it = pool.lower_bound({slot, 0}); it != pool.end() && it->first.first == slot; ++it) if (it->second.arena) return true;
    return false;
  }
  size_t live_bytes(int slot) const { size_t n = 0; for (const auto &kv : live) if (kv.second.slot == slot) n += kv.second.bytes; return n; }
  size_t pooled_bytes(int slot) const {   // pooled blocks plus the free ranges of the slabs: held by the library, reusable, not live
    size_t n = arena[slot].free_bytes();
    for (auto it = pool.lower_bound({slot, 0}); it != pool.end() && it->first.first == slot; ++it) n += it->second.bytes;
    return n;
  }
};

}  // namespace mi355zk
