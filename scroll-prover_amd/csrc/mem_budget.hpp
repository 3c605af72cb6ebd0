// mem_budget.hpp -- the ledger of the device memory the library holds from HIP (lib_core.hip: dev_malloc / dev_free, the only two functions that name hipMalloc / hipFree), and
// the limit a caller sets on it (mi355_mem_set_limit / _usage / _reset_peak).  Plain C++, no HIP and no lock: lib_core.hip owns the allocations, the reclaiming itself and the one
// mutex every call below runs under, so the same code runs under tests/hostcheck/mem_budget_main.cpp against a plain model.
//
// Per device slot and per class the ledger records every byte between a successful reserve and its release.  A slot keeps: held (the sum of its classes), the high-water mark
// of held since the last reset, the limit (0 = none), how many reclaims freed something, and the bytes of the requests it refused.
//
// The decision of an allocation, one step per call (as BufRegistry::alloc_step): with no limit, or while held + bytes stays within it, the bytes are charged BEFORE any HIP
// call -- under a limit the real HBM is never approached.  Otherwise the caller is told what to give back, in this order, and asks again after each:
//   1. the slot's pooled blocks and whole free slabs (pool_release_slot);
//   2. the optional NTT tables (folded coset shifts, divisor-scaled tables, 2-D inter-level tables: every pass has a table-free form with the same bits);
// and when that made no room the request is refused: nothing changes but the refused counter.  oom_step is the same order for a real hipErrorOutOfMemory with no limit set.
// What an allocation may reclaim depends on what it is:
//   Required   everything above; a refusal is counted and reported (MI355_EOOM naming the limit, the held bytes by class and the request)
//   Headroom   a convenience on top of a required size (the head-room of a shared slab or of a workspace block): the pool only; the exact size is tried next, so a refusal is not counted
//   Spare      an optional table: nothing is reclaimed for it and a refusal is quiet (the caller takes the table-free form of the pass)
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>

namespace mi355zk {

enum MemClass : int {
  MEM_BUF = 0,         // slabs and direct mi355_buf blocks: live, pooled or free ranges
  MEM_WORKSPACE,       // the workspace arena (Ctx::ws)
  MEM_NTT_REQUIRED,    // the power tables every plan needs
  MEM_NTT_OPTIONAL,    // coset-fold, divisor-scaled and 2-D inter-level tables: reclaimable
  MEM_SRS,             // SRS shards and the result of mi355_srs_downsize
  MEM_WINDOW_TABLES,   // mi355_srs_precompute: the caller's handle owns them; counted, never reclaimed
  MEM_FIXED_TABLES,    // the fixed-base table and the Poseidon tables
  MEM_CLASSES
};
inline const char *mem_class_name(int c) {
  static const char *const names[MEM_CLASSES] = {"buffers", "workspace", "ntt_required", "ntt_optional", "srs", "window_tables", "fixed_tables"};
  return c >= 0 && c < MEM_CLASSES ? names[c] : "?";
}
enum class MemMode { Required, Headroom, Spare };
enum class MemStep { Charged, ReclaimPool, ReclaimTables, Refused };

struct MemSlot { uint64_t by_class[MEM_CLASSES] = {}; uint64_t held = 0, high_water = 0, limit = 0, reclaims = 0, refused_bytes = 0; };

struct MemLedger {
  static constexpr int MAX_SLOTS = 16;
  struct Rec { uint64_t bytes; int slot; MemClass cls; };
  MemSlot slot[MAX_SLOTS];
  std::unordered_map<uintptr_t, Rec> recs;   // every allocation the library holds, by base address

  static MemStep after(int stage, MemMode mode) {   // what follows `stage` reclaims that made no room
    if (mode == MemMode::Spare) return MemStep::Refused;
    if (stage == 0) return MemStep::ReclaimPool;
    if (stage == 1 && mode == MemMode::Required) return MemStep::ReclaimTables;
    return MemStep::Refused;
  }
  // stage: how many reclaims the caller has run for this request (0, 1, 2).  Charged: the bytes are held from now on (bind() or cancel() follows the HIP call)
  MemStep reserve_step(int s, MemClass c, uint64_t bytes, int stage, MemMode mode) {
    MemSlot &m = slot[s];
    if (m.limit == 0 || (bytes <= m.limit && m.held <= m.limit - bytes)) {
      m.by_class[c] += bytes; m.held += bytes; if (m.held > m.high_water) m.high_water = m.held;
      return MemStep::Charged;
    }
    const MemStep next = after(stage, mode);
    if (next == MemStep::Refused && mode == MemMode::Required) m.refused_bytes += bytes;
    return next;
  }
  // a real out-of-memory error of the allocator after a successful reserve: the same order; the caller retries the allocation after each reclaim that freed something
  static MemStep oom_step(int stage, MemMode mode) { return after(stage, mode); }
  void cancel(int s, MemClass c, uint64_t bytes) { MemSlot &m = slot[s]; m.by_class[c] -= bytes; m.held -= bytes; }   // the HIP call failed after all: the high-water mark keeps what was reserved
  void bind(const void *p, int s, MemClass c, uint64_t bytes) { recs[(uintptr_t)p] = Rec{bytes, s, c}; }
  // the allocation at p leaves the ledger; false (and nothing changes) when the library does not hold it
  bool release(const void *p, Rec *out = nullptr) {
    auto it = recs.find((uintptr_t)p);
    if (it == recs.end()) return false;
    const Rec r = it->second; recs.erase(it);
    cancel(r.slot, r.cls, r.bytes);
    if (out) *out = r;
    return true;
  }
  void reclaimed(int s, uint64_t freed) { if (freed) slot[s].reclaims++; }
  void set_limit(int s, uint64_t bytes) { slot[s].limit = bytes; }   // below held: new charges are refused, nothing is freed
  void reset_peak(int s) { slot[s].high_water = slot[s].held; }
  // what "free" means to a builder of optional tables: min(free HBM, limit - held)
  uint64_t room(int s, uint64_t free_hbm) const { const MemSlot &m = slot[s]; if (!m.limit) return free_hbm; const uint64_t r = m.held >= m.limit ? 0 : m.limit - m.held; return r < free_hbm ? r : free_hbm; }
  std::string describe_refusal(int s, uint64_t bytes, const char *what) const {
    const MemSlot &m = slot[s]; char b[160];
    std::snprintf(b, sizeof b, "%s: %llu bytes refused by the memory limit of %llu bytes on device slot %d: held %llu (", what, (unsigned long long)bytes, (unsigned long long)m.limit, s, (unsigned long long)m.held);
    std::string out = b;
    for (int c = 0; c < MEM_CLASSES; c++) { std::snprintf(b, sizeof b, "%s%s %llu", c ? ", " : "", mem_class_name(c), (unsigned long long)m.by_class[c]); out += b; }
    return out + ")";
  }
};

}  // namespace mi355zk
