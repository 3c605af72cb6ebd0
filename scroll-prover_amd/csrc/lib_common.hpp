// lib_common.hpp -- host-side state shared by the translation units of libmi355zk.so (lib_core / lib_msm / lib_ntt / lib_aux / lib_pairing .hip): device contexts with their
// knobs (knobs.hpp), streams and events, the per-device locks, SRS handles, the workspace arena, the slot look-ups of the resident-buffer registry, HIP-event profiling and the
// error plumbing of the C-ABI (include/mi355zk.h).  Host logic only; no kernel is declared here -- every lib_*.hip includes the kernel headers it launches and nothing else, so a
// change to one kernel family rebuilds one translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <condition_variable>
#include <unordered_map>
#include <vector>

#include "../../include/mi355zk.h"
#include "fp.hpp"
#include "g1.hpp"
#include "g1_29.hpp"
#include "ntt_types.hpp"
#include "ws_layout.hpp"
#include "knobs.hpp"
#include "msm_plan.hpp"
#include "mem_budget.hpp"

namespace mi355 {
using namespace zk;
using mi355zk::WsLayout;
using mi355zk::MemClass;
using mi355zk::MemMode;

extern thread_local std::string g_err;
int fail(int code, const std::string &msg);

#define HIPCHK(expr)                                                                                                     \
  do {                                                                                                                   \
    hipError_t _e = (expr);                                                                                              \
    if (_e != hipSuccess) {                                                                                              \
      char _b[512]; snprintf(_b, sizeof _b, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);  \
      (void)hipGetLastError();                                                                                           \
      return ::mi355::fail(_e == hipErrorOutOfMemory ? MI355_EOOM : MI355_EHIP, _b);                                     \
    }                                                                                                                    \
  } while (0)
#define CHK(expr) do { int _r = (expr); if (_r != MI355_OK) return _r; } while (0)

// A registered basis.  One device: ONE shard holding all n points.  mi355_init_multi with D devices: shard d = points [lo, lo + n) on device slot d
// (fixed point-range shards); window tables are per shard (row stride = shard length).  The device memory (SrsMem) is shared
// between a handle and its prefix views (mi355_srs_register_prefix) and freed with the last of them.
struct Shard { int slot = 0; uint64_t lo = 0, n = 0; g1_affine_t *dev = nullptr; bool owned = false; };
void free_shards(std::vector<Shard> &sh);
struct SrsMem { std::vector<Shard> sh; ~SrsMem() { free_shards(sh); } };
// window tables T[w][i] = 2^(c w) P_i, one allocation per shard (pre[i] belongs to shard i of the basis, rows `stride[i]` points apart).
// A prefix view starts out sharing its parent's tables and gets private ones only when a much smaller n calls for another window width.
struct SrsTables { std::vector<g1_affine_t *> pre; std::vector<uint64_t> stride; std::vector<int> slot; int c = 0, w = 0; ~SrsTables(); };
struct Srs { uint64_t n = 0; std::shared_ptr<SrsMem> mem; std::shared_ptr<SrsTables> tab; };
struct Buf { void *p = nullptr; size_t cap = 0; };
struct NttPlan {
  uint32_t log_n = 0, levels = 0, log_m[3] = {0, 0, 0};
  uint32_t split[2] = {0, 0};
  uint32_t direct2[2] = {0, 0};
  std::map<std::string, Tw29> scaled;   // the last strided level's direct twiddle table times a constant (key: the 32 bytes of the constant)
  // the tables of a coset shift folded into the first pass, per coset factor f (key: its 32 bytes): in[m] = (f^(2^log_t))^m, s2d[k][column] = w_S^(column k) f^column
  struct CosetTw { Tw29 in, s2d; };
  std::map<std::string, CosetTw> coset;
  // twiddles as w * 2^261 mod r in 29-bit limbs (SoA) for the kernels of ntt29.hpp; tw29_s_lo[l] of a big level is the 2^log_s-entry table [k][column]
  Tw29 tw29_m[3] = {}, tw29_s_lo[2] = {}, tw29_s_hi[2] = {};
  std::vector<void *> owned;
  // which of `owned` are optional (csrc/mem_budget.hpp, MEM_NTT_OPTIONAL): the s2d + in tables of `coset`, the tables of `scaled`, the 2-D level tables of direct2.  They can be
  // given back at any time no transform is in flight (ntt_reclaim_optional): every pass has its table-free form with the same bits
  std::vector<void *> optional;
};
struct Prof { double ms = 0; uint64_t launches = 0; };

// How the last MSM ran: window bits, windows, sorted entries (all passes of the call), one shared bucket set (window tables), point-range slices of the host-pointer schedule,
// device slots that took part and how their partials were exchanged ("none" | "rccl_allgather" | "device_copy").  begin() where a top-level call starts on a device
// (msm_run, lib_msm.hip); every pass adds itself.
struct MsmRunRecord {
  int c = 0, windows = 0; uint64_t entries = 0; bool shared = false; int host_slices = 1, devices = 1; const char *exchange = "none";
  void begin() { entries = 0; host_slices = 1; devices = 1; exchange = "none"; }
};
struct MsmSlot { int id = 0; hipEvent_t sorted = nullptr, acc_done = nullptr, red_done = nullptr; bool used = false; };   // per-chunk buffers + events of the pipelined MSM

struct Span { std::string name; hipEvent_t a, b; };
// One bound device.  The environment knobs (seg_fill, ntt_tile_log, trace, ...) are the Knobs base: csrc/knobs.hpp is their table, DESIGN.md section 10 their description.
struct Ctx : mi355zk::Knobs {
  bool inited = false;
  int slot = 0;                 // index in g_ctx (0 = primary)
  int device = -1;
  hipDeviceProp_t prop;
  // streams (ctx_streams below lists the owned ones once, for init_ctx / destroy_ctx / sync_streams).  `stream` is the compute stream: own_stream, or the caller's (mi355_set_stream)
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipStream_t aux_stream[2] = {nullptr, nullptr};   // side streams of the pipelined MSM (sort | reduction); the accumulation stays on `stream`
  hipStream_t copy_stream = nullptr;   // the chunked copy of the host-pointer MSM (msm_host_sliced) and the resident-buffer uploads (mi355_buf_upload)
  // events (ctx_events below lists them once), all without timing
  MsmSlot msm_slot[2];
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_xchg = nullptr;
  hipEvent_t ev_xchg2 = nullptr;   // recorded behind a cross-slot mi355_buf_copy on the destination's stream; the source slot's stream waits for it
  hipEvent_t ev_copy[4] = {};
  hipEvent_t ev_up[8] = {}; uint32_t up_next = 0;   // uploads on copy_stream (ring: several threads may upload at once), under the upload mutex
  hipEvent_t ev_up_fork = nullptr;   // mi355_buf_upload into a block in use: recorded on the compute stream, awaited by the copy stream (upload mutex)
  void *comm = nullptr;         // ncclComm_t of this device (mi355_init_multi with distinct devices)
  std::vector<const fe_t *> polys_stage;
  uint32_t msm_chunk_min_log = 23;   // mi355_msm_set_pipeline
  std::map<std::string, Buf> ws;           // grow-only workspace arena, keyed by role
  std::map<std::string, NttPlan> ntt_plans;  // key = log_n | omega bytes
  int ntt_pins = 0;             // transforms in flight on the calling thread that hold pointers into ntt_plans: the optional tables are not reclaimed meanwhile (PlanPin, lib_ntt.hip)
  g1_affine_t *fixed_base_table = nullptr;
  bool profiling = false;
  std::vector<Span> spans;      // profiling: (name, start, stop) event pairs resolved after the stream is idle
  std::map<std::string, Prof> prof;
  MsmRunRecord run;             // how the last MSM on this slot ran (mi355_msm_last_plan / _last_run read slot 0's)
};
// The streams a context owns, in creation order, and every event it owns: init_ctx creates from these lists and destroy_ctx destroys from them, so a new member is named once.
enum : unsigned { SYNC_COMPUTE = 1, SYNC_AUX = 2, SYNC_COPY = 4 };
struct CtxStream { hipStream_t *s; unsigned kind; };
inline std::vector<CtxStream> ctx_streams(Ctx &c) { return {{&c.own_stream, SYNC_COMPUTE}, {&c.aux_stream[0], SYNC_AUX}, {&c.aux_stream[1], SYNC_AUX}, {&c.copy_stream, SYNC_COPY}}; }
inline std::vector<hipEvent_t *> ctx_events(Ctx &c) {
  std::vector<hipEvent_t *> v = {&c.ev_fork, &c.ev_xchg, &c.ev_xchg2, &c.ev_up_fork};
  for (auto &m : c.msm_slot) { v.push_back(&m.sorted); v.push_back(&m.acc_done); v.push_back(&m.red_done); }
  for (auto &e : c.ev_copy) v.push_back(&e);
  for (auto &e : c.ev_up) v.push_back(&e);
  return v;
}
// waits for the streams of `which` (SYNC_COMPUTE is c.stream, the caller's stream included; streams not yet created are skipped); every stream is waited for, the first error is returned
hipError_t sync_streams(Ctx &c, unsigned which);

// One context per bound device; slot 0 is the primary.  LOCKING (round 3): one mutex PER DEVICE SLOT instead of one for the library.
//   * an entry point that works on one device (every transform, scan, evaluation, element-wise operation, buffer copy) holds that slot's
//     lock only, so callers on different devices -- rayon workers of one prover -- run concurrently;
//   * MSM entry points hold slot 0 and, with several devices bound, every other slot as well (the point range is sharded over all of them);
//   * lifecycle and SRS management (init, shutdown, register, release, precompute, downsize, profile control) hold every slot.
// Locks are always taken in ascending slot order.  The SRS handle table is read under slot 0's lock and written under all of them.
// `g` names the context the CURRENT THREAD works on (bind_ctx), which is why the pointer is thread-local: API threads and the per-device
// worker threads of sharded MSMs / batched transforms each have their own.
constexpr int MAX_DEV = 16;
extern std::mutex g_ctx_mu[MAX_DEV];
extern std::mutex g_upload_mu[MAX_DEV];
extern Ctx g_ctx[MAX_DEV];
extern int g_ndev;
extern bool g_dup_devices;     // test mode: the same physical device bound to several slots (exchange by device copies instead of RCCL)
extern bool g_peer_ok[MAX_DEV][MAX_DEV];   // [s][t]: kernels on slot s may read memory of slot t directly
extern mi355zk::ProcessKnobs g_proc;   // the per-process knobs of mi355_init_multi (csrc/knobs.hpp): shard_min_log, multi_force, msm_auto_max_c
extern thread_local Ctx *g_cur;
#define g (*::mi355::g_cur)
extern std::unordered_map<uint64_t, Srs> &g_srs;   // heap-allocated, never destroyed (no HIP calls from static destruction)
extern uint64_t g_next_handle;

// t_slots_held: bit s is set while the CALLING THREAD works under slot s's lock -- it took the lock through one of the guards below, or it is a worker thread of a call
// that did (SlotHeld).  mi355_buf_alloc, the one allocation path that runs without the lock, reads it to know whether reclaiming the optional NTT tables needs the lock first.
extern thread_local uint32_t t_slots_held;
struct SlotHeld {   // a worker thread of an entry point that holds `slot`'s lock on its behalf
  const uint32_t bit, was;
  explicit SlotHeld(int slot) : bit(1u << slot), was(t_slots_held & (1u << slot)) { t_slots_held |= bit; }
  ~SlotHeld() { if (!was) t_slots_held &= ~bit; }
  SlotHeld(const SlotHeld &) = delete; SlotHeld &operator=(const SlotHeld &) = delete;
};
struct DevGuard {   // one device slot
  std::unique_lock<std::mutex> lk; const uint32_t bit;
  explicit DevGuard(int slot) : lk(g_ctx_mu[slot]), bit(1u << slot) { t_slots_held |= bit; }
  ~DevGuard() { t_slots_held &= ~bit; }
};
struct AllGuard {   // every slot, ascending
  std::unique_lock<std::mutex> lk[MAX_DEV];
  AllGuard() { for (int i = 0; i < MAX_DEV; i++) lk[i] = std::unique_lock<std::mutex>(g_ctx_mu[i]); t_slots_held = (1u << MAX_DEV) - 1; }
  ~AllGuard() { t_slots_held = 0; }
};
struct MsmGuard {   // slot 0, plus every other bound slot when the process drives several devices
  std::unique_lock<std::mutex> lk[MAX_DEV]; uint32_t bits = 1;
  MsmGuard() { lk[0] = std::unique_lock<std::mutex>(g_ctx_mu[0]); for (int i = 1; i < g_ndev && i < MAX_DEV; i++) { lk[i] = std::unique_lock<std::mutex>(g_ctx_mu[i]); bits |= 1u << i; } t_slots_held |= bits; }
  ~MsmGuard() { t_slots_held &= ~bits; }
};

// One pooled mi355_buf block, back in the pool when its owner leaves scope -- on every exit path, so the body of an entry point uses HIPCHK / CHK and plain returns.  Declare it
// AFTER the DevGuard: the block then goes back (its free event is recorded on the owner's stream, behind everything queued so far) before the device lock is released.  The
// result of mi355_buf_free is ignored, and g_err is written by fail() alone: the error text of a failed body survives the destructor unless the free itself fails (it can,
// after a sticky HIP error in the body: its event record then writes its own text).
struct PoolBlock {
  void *p = nullptr; int slot = 0;
  PoolBlock() = default;
  PoolBlock(const PoolBlock &) = delete; PoolBlock &operator=(const PoolBlock &) = delete;
  ~PoolBlock() { if (p) (void)mi355_buf_free(p); }
  int alloc(uint64_t bytes, int slot_) { slot = slot_; return mi355_buf_alloc(bytes, slot_, &p); }   // binds slot_'s context on the calling thread (need_init)
  char *at(uint64_t off) const { return (char *)p + off; }
  // host memory -> the block, on the copy stream (mi355_buf_upload: work queued afterwards on the compute stream waits for it); the owner's context is bound again afterwards
  int upload(uint64_t off, const void *src_host, uint64_t bytes);
};

// per-THREAD MSM options (mi355_msm_set_normalise / _set_window_bits): a rayon worker that asks for un-normalised partial sums must not
// change what another worker's commit returns (SURVEY 8b "Threading")
struct MsmOpts { bool normalise = true; int force_c = 0; bool no_tables = false; };
extern thread_local MsmOpts t_opts;

inline void use_ctx(int slot) { g_cur = &g_ctx[slot]; }
// Every compute entry point starts here.  The HIP current device is per host thread and calls arrive from whichever thread runs
// create_proof (rayon workers included, SURVEY 8b "Threading"), so the bound device is re-selected on the calling thread each time.
int bind_ctx(int slot);
int need_init(int slot = 0);
inline int PoolBlock::upload(uint64_t off, const void *src_host, uint64_t bytes) { CHK(mi355_buf_upload(at(off), src_host, bytes)); return need_init(slot); }

// MI355_TRACE: per-call counters for the integrator (metrics / logging)
struct CallTrace {
  const char *what; uint64_t n; double bytes_per_unit; std::chrono::steady_clock::time_point t0;
  CallTrace(const char *w, uint64_t n_, double bpu) : what(w), n(n_), bytes_per_unit(bpu), t0(std::chrono::steady_clock::now()) {}
  void done(const char *extra = "") {
    if (!g.trace) return;
    (void)hipStreamSynchronize(g.stream);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "[mi355zk] %s n=%llu %.3f ms %.2f M units/s %.1f GB/s algorithmic%s\n", what, (unsigned long long)n, ms, n / ms / 1e3, n * bytes_per_unit / ms / 1e6, extra);
  }
};

int ws_get(const char *role, size_t bytes, void **out);
// The one pair through which the library takes device memory from HIP and gives it back (csrc/mem_budget.hpp is the ledger they keep).  dev_malloc allocates on the current
// context's device: under a limit (mi355_mem_set_limit) the ledger decides BEFORE any HIP call; a request that does not fit, and a real out-of-memory error, first get the
// slot's pooled blocks and free slabs back, then the optional NTT tables, and only then MI355_EOOM.  cls: what the ledger books the bytes under.  mode: what may be reclaimed
// for the request and whether a refusal is reported (MemMode).  slot_locked: the calling thread works under the slot's lock -- true everywhere but in mi355_buf_alloc.
// dev_free takes any pointer dev_malloc returned (nullptr is ignored) and returns its size; the caller has bound the owning device and drained the streams that may still use it.
int dev_malloc(void **out, size_t bytes, const char *what, MemClass cls, MemMode mode = MemMode::Required, bool slot_locked = true);
size_t dev_free(void *p);
// min(free HBM, limit - held) of the current context's device: what a builder of optional tables may count on (0 when the runtime cannot say); *total_out: the device's HBM
size_t dev_room(size_t *total_out);
// lib_ntt.hip: gives the optional tables of every plan of `c` back (after draining its compute and auxiliary streams); returns the bytes freed, 0 while a transform is in
// flight.  Called under c's slot lock only, with c's device bound.
size_t ntt_reclaim_optional(Ctx &c);

// ---- profiling: a list of (name, start, stop) event pairs per context, resolved after the stream is idle
struct Scope {
  bool on; hipEvent_t a = nullptr, b = nullptr; std::string name; hipStream_t st;
  Scope(const char *n, hipStream_t s = nullptr) : on(g.profiling), name(n), st(s ? s : g.stream) { if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, st); } }
  void close() { if (on) { (void)hipEventRecord(b, st); g.spans.push_back({name, a, b}); on = false; } }
  ~Scope() { close(); }
};
void resolve_spans();
inline int finish_async() { if (g.profiling) resolve_spans(); return MI355_OK; }

inline uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
inline uint32_t log2_ceil(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) l++; return l; }

// No exception may cross the C boundary (the Rust callers are `extern "C"` and would abort): every multi-line entry point runs inside
// this guard, which turns allocation failures and anything else the host-side C++ might throw into error codes.
// MI355_TRACE=2: every entry point runs inside a roctx range named after it ("wrap every FFI call in a roctx range"), so a
// rocprofv3 --marker-trace timeline of a real proof shows which create_proof call each kernel belongs to.  The marker library
// (librocprofiler-sdk-roctx.so.1, else libroctx64.so.4) is dlopen()ed on first use; without it, or with MI355_TRACE != 2, this costs one load.
struct Roctx { int state = 0; int (*push)(const char *) = nullptr; int (*pop)() = nullptr; };
extern Roctx g_roctx;
void roctx_bind();
struct ApiRange {
  bool on;
  explicit ApiRange(const char *name) : on(false) { if (g_roctx.state == 0) roctx_bind(); if (g_roctx.state == 2) { g_roctx.push(name); on = true; } }
  ~ApiRange() { if (on) g_roctx.pop(); }
};
template <class F> int guarded(F body, const char *who = __builtin_FUNCTION()) {
  ApiRange range(who);
  try { return body(); }
  catch (const std::bad_alloc &) { return fail(MI355_EOOM, "host allocation failed"); }
  catch (const std::exception &e) { return fail(MI355_EHIP, std::string("unexpected host exception: ") + e.what()); }
  catch (...) { return fail(MI355_EHIP, "unexpected host exception"); }
}

// ---- RCCL, bound lazily (lib_core.hip)
struct Rccl {
  void *lib = nullptr;
  int (*CommInitAll)(void **, int, const int *) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
extern Rccl g_rccl;
int rccl_fail(const char *what, int rc);

// ---- SRS bookkeeping (lib_core.hip; no kernels)
std::vector<Shard> plan_shards(uint64_t n);
int srs_find(uint64_t handle, Srs **out, const char *who);
uint64_t srs_insert(const Srs &s);
int srs_alloc(SrsMem &mem, uint64_t n);
int srs_scatter_from_primary(SrsMem &mem, const g1_affine_t *src_dev, uint64_t n, bool alias_shard0);
int srs_gather_to_primary(const Srs &sr, uint64_t n, const g1_affine_t **out);

// ---- resident buffers (mi355_buf_*, lib_core.hip over buf_registry.hpp): which device slot owns a device pointer.  Pointers handed out by mi355_buf_alloc are
// looked up in the registry; anything else (a torch tensor, an SRS pointer) is asked of the HIP runtime when several devices are bound.
// `touch` marks a registered block as used by queued work (an upload into it must then wait for the compute stream).
int slot_of(const void *dev_ptr, bool touch = true);
int buf_check_range(const void *dev_ptr, uint64_t bytes, const char *who);   // MI355_EBADARG when [dev_ptr, dev_ptr + bytes) leaves the library block that holds dev_ptr
// the slot that owns ALL of the given device pointers (null pointers ignored); MI355_EBADARG when they live on different devices
int common_slot(std::initializer_list<const void *> ptrs, int *slot_out, const char *who);
// the same over a host table of `count` device pointers (the columns of a witness, the vectors of a batch); touch as in slot_of
int common_slot(const void *const *ptrs, size_t count, bool touch, int *slot_out, const char *who);
// round-robin choice of a device for a host-pointer call (replicas: any bound device can run it); prefers a device whose lock is free
int pick_replica_slot();

// ---- per-translation-unit hooks called by init_ctx (dynamic-LDS limits of the kernels that TU launches)
int msm_tu_init_device();
int ntt_tu_init_device();
int aux_tu_init_device();
// twiddle table out[i] = (base^step)^i on the current context's stream (kernel in ntt29.hpp; used by the G1 DFT as well)
int launch_pow_table(fe_t *out, const fe_t &base, uint64_t step, uint32_t count);
// the G1 point codec (kernels in g1codec.hpp, launched by lib_aux.hip; the Processed params loader of lib_msm.hip uses it chunk by chunk): queue the decompression of
// n 32-byte words into n affine points on the current context's stream; a rejected word leaves base + its index in *err_dev by atomicMin (the caller presets ~0)
int launch_g1_decompress(const void *bytes_dev, void *affine_out_dev, uint64_t n, uint64_t base, unsigned long long *err_dev);
// the two G2 points of a Processed params file, decoded on the host (64 bytes -> 128-byte G2Affine); false for a word that is no point of the twist
bool g2_decode_host(const uint8_t in[64], void *g2affine_out);

// ---- small helpers shared by the transform entry points (lib_ntt.hip, lib_aux.hip)
inline int check_ntt_args(const void *data, uint32_t log_n, const void *omega) {
  if (!data || !omega) return fail(MI355_EBADARG, "ntt: null pointer");
  if (log_n > 28) return fail(MI355_EBADARG, "ntt: log_n > 28");
  return MI355_OK;
}
struct NttHostArgs { uint32_t log_n; const void *omega; const void *divisor; };
// host buffer -> this context's staging buffer `role` -> body(dev) -> host buffer, synchronous (the device lock is held by the caller)
inline int with_host_io(void *data_host, size_t in_bytes, size_t out_bytes, size_t dev_bytes, const char *role, int (*body)(void *dev, void *ud), void *ud) {
  void *dev; CHK(ws_get(role, dev_bytes, &dev));
  HIPCHK(hipMemcpyAsync(dev, data_host, in_bytes, hipMemcpyHostToDevice, g.stream));
  CHK(body(dev, ud));
  HIPCHK(hipMemcpyAsync(data_host, dev, out_bytes, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  resolve_spans();
  return MI355_OK;
}

}  // namespace mi355
