// ws_layout_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around WsLayout (scroll-prover_amd/csrc/ws_layout.hpp), the bump allocator that places the fields of the
// pooled workspace blocks of lib_aux.hip / lib_pairing.hip.  tests/test_ws_layout_on_host.py builds it with -fsanitize=address,undefined and runs it; every case prints one
// line "name ok|WRONG ..." and the exit code is the number of cases that went wrong.  Never shipped.
//   * random sequences of field sizes: every take() offset a multiple of 256, no two fields overlap, last end <= total() < last end + 256;
//   * the sizes 0, 1, 255, 256, 257 and a field of 2^40 bytes (offsets are 64-bit);
//   * the six entry points laid out with it: total() against the byte count each computed by hand before (written out below as plain arithmetic).
// The *_layout functions below are COPIES of the take / take_exact sequences in lib_aux.hip and lib_pairing.hip (those need HIP; this program must not): a field added or
// reordered in an entry point has to be repeated here by hand.  What they pin is that WsLayout reproduces the earlier byte counts for these sequences; the entry points' own
// layouts are pinned by the GPU tests that assert on pooled and workspace bytes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../scroll-prover_amd/csrc/ws_layout.hpp"

using mi355zk::WsLayout;
static int g_wrong = 0;
static void verdict(const char *name, bool ok, uint64_t got = 0, uint64_t want = 0) {
  if (ok) std::printf("%s ok\n", name);
  else { std::printf("%s WRONG got %llu want %llu\n", name, (unsigned long long)got, (unsigned long long)want); g_wrong++; }
}
static uint64_t al(uint64_t b) { return (b + 255) & ~255ull; }   // the rounding the hand-written chains used
static uint64_t cdiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
static uint32_t log2_ceil(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) l++; return l; }

// ---- the layouts as the entry points build them, retyped (the order of the take calls is the order of the fields in the block)
static uint64_t lookup_layout(uint64_t n, uint64_t S) { WsLayout L; L.take(8); L.take(S * 4); L.take_exact(n * 4); return L.total(); }
static uint64_t sigma_layout(uint64_t n_cols, uint64_t n_lo, uint64_t n_hi, uint64_t stage) {
  WsLayout L; L.take(n_cols * 8); L.take_exact(n_cols * 32); L.take_exact(n_lo * 32); L.take_exact(n_hi * 32); L.take_exact(stage * 8); L.take_exact(stage * 8); return L.total();
}
static uint64_t nonzero_layout(uint64_t batch, uint64_t cap, uint64_t nblocks) {
  WsLayout L; L.take(batch * 8); L.take(batch * 8); L.take(batch * cap * 8); L.take(batch * nblocks * 4); L.take(batch * nblocks * 4); return L.total();
}
static uint64_t copy_layout(uint64_t n_cols, uint64_t cap, uint64_t max_blocks, uint64_t stage) {
  WsLayout L; L.take(n_cols * 8); L.take(8); L.take(cap * 8); L.take(max_blocks * 4); L.take(max_blocks * 4); L.take(stage * 8); L.take(stage * 8); return L.total();
}
static uint64_t pairing_layout(uint64_t n, uint64_t groups) {
  WsLayout L; L.take(n * 64); L.take(n * 128); L.take_exact(n * 384); L.take_exact(n * 384); L.take_exact(groups * 384); L.take(groups * 4); L.take(8); return L.total();
}
static uint64_t poseidon_layout(uint64_t n_words, uint64_t jobs, uint64_t n_sq) {
  WsLayout L; L.take(n_words * 32); L.take((jobs + 1) * 8); L.take((jobs + 1) * 8); L.take(n_sq * 4); L.take(n_sq * 32); return L.total();
}

int main() {
  // ---- random sequences
  {
    std::mt19937_64 rng(20240611);
    const uint64_t edge[5] = {0, 1, 255, 256, 257};
    bool aligned = true, disjoint = true, total_ok = true;
    for (int seq = 0; seq < 4000; seq++) {
      WsLayout L; const int fields = 1 + (int)(rng() % 12);
      std::vector<std::pair<uint64_t, uint64_t>> f;   // [start, end)
      for (int i = 0; i < fields; i++) {
        const int bits = (int)(rng() % 36); uint64_t sz = rng() & ((1ull << bits) - 1);
        if (rng() % 8 == 0) sz = (sz & ~255ull) + edge[rng() % 5];
        const uint64_t off = L.take(sz);
        aligned = aligned && off % 256 == 0;
        f.push_back({off, off + sz});
      }
      for (size_t i = 0; i < f.size(); i++) for (size_t j = i + 1; j < f.size(); j++)
        if (f[i].first < f[j].second && f[j].first < f[i].second && f[i].first != f[i].second && f[j].first != f[j].second) disjoint = false;
      for (size_t i = 1; i < f.size(); i++) if (f[i].first < f[i - 1].second) disjoint = false;   // fields come in order
      total_ok = total_ok && L.total() >= f.back().second && L.total() < f.back().second + 256;
    }
    verdict("random_take_offsets_aligned", aligned);
    verdict("random_take_fields_disjoint", disjoint);
    verdict("random_take_total_bounds", total_ok);
    // take and take_exact mixed: still in order and disjoint, total() = the last end rounded as its call says
    bool mixed = true;
    for (int seq = 0; seq < 4000; seq++) {
      WsLayout L; uint64_t prev_end = 0, want_total = 0;
      for (int i = 0; i < 10; i++) {
        const uint64_t sz = rng() & ((1ull << (rng() % 30)) - 1); const bool exact = rng() & 1;
        const uint64_t off = exact ? L.take_exact(sz) : L.take(sz);
        mixed = mixed && off >= prev_end && off == want_total;
        prev_end = off + sz; want_total = off + (exact ? sz : al(sz));
      }
      mixed = mixed && L.total() == want_total;
    }
    verdict("random_mixed_in_order", mixed);
  }
  // ---- the edge sizes
  {
    WsLayout L;
    const uint64_t o0 = L.take(0), o1 = L.take(1), o255 = L.take(255), o256 = L.take(256), o257 = L.take(257), obig = L.take(1ull << 40), after = L.take(1);
    verdict("size_0_takes_no_room", o0 == 0 && o1 == 0);
    verdict("size_1", o255 == 256, o255, 256);
    verdict("size_255", o256 == 512, o256, 512);
    verdict("size_256", o257 == 768, o257, 768);
    verdict("size_257", obig == 1280, obig, 1280);
    verdict("size_2_pow_40", after == 1280 + (1ull << 40), after, 1280 + (1ull << 40));
    verdict("total_past_2_pow_40", L.total() == 1280 + (1ull << 40) + 256, L.total(), 1280 + (1ull << 40) + 256);
    WsLayout E; const uint64_t e0 = E.take_exact(1ull << 40), e1 = E.take_exact(3), e2 = E.take(5);
    verdict("take_exact_is_exact", e0 == 0 && e1 == (1ull << 40) && e2 == (1ull << 40) + 3 && E.total() == (1ull << 40) + 3 + 256, E.total(), (1ull << 40) + 259);
  }
  // ---- the six entry points against the byte counts of the hand-written offset chains they replace
  bool ok = true;
  // lookup multiplicities: 256 B of error word, the slots (S = max(64, next power of two >= 2 x table_rows)) rounded, 4 B per row of m as they are
  for (uint64_t n : {1ull, 1000ull, (1ull << 20) + 5, (1ull << 31) - 1}) for (uint64_t table_rows : {(uint64_t)0, (uint64_t)1, (uint64_t)33, (uint64_t)1000, n}) {
    if (table_rows > n) continue;
    const uint64_t S = std::max<uint64_t>(64, 1ull << log2_ceil(2 * table_rows));
    const uint64_t off_slots = 256, off_cnt = off_slots + ((S * 4 + 255) & ~255ull), bytes = off_cnt + n * 4;
    if (lookup_layout(n, S) != bytes) { ok = false; verdict("lookup_bytes", false, lookup_layout(n, S), bytes); }
  }
  verdict("lookup_bytes_unchanged", ok); ok = true;
  // permutation sigma: the pointers rounded, then the three power tables and the two staged lists packed
  for (uint64_t n_cols : {1ull, 5ull, 37ull}) for (uint32_t log_n : {1u, 10u, 16u, 28u}) for (uint64_t count : {0ull, 1ull, 4097ull, (1ull << 22) + 1}) {
    const uint32_t lo_bits = (log_n + 1) / 2; const uint64_t n_lo = 1ull << lo_bits, n_hi = 1ull << (log_n - lo_bits), stage = std::min<uint64_t>(count, 1ull << 22);
    const uint64_t off_dpow = (n_cols * 8 + 255) & ~255ull, off_lo = off_dpow + n_cols * 32, off_hi = off_lo + n_lo * 32, off_cells = off_hi + n_hi * 32, off_images = off_cells + stage * 8,
                   bytes = off_images + stage * 8;
    if (sigma_layout(n_cols, n_lo, n_hi, stage) != bytes) { ok = false; verdict("sigma_bytes", false, sigma_layout(n_cols, n_lo, n_hi, stage), bytes); }
  }
  verdict("sigma_bytes_unchanged", ok); ok = true;
  // nonzero rows: five rounded fields (CHECK_TILE = 1024 elements per workgroup)
  for (uint64_t batch : {1ull, 3ull, 70000ull}) for (uint64_t n : {1ull, 1024ull, (1ull << 20) + 5}) for (uint64_t cap : {0ull, 16ull, 65536ull}) {
    const uint64_t nblocks = cdiv(n, 1024);
    const uint64_t off_tot = al(batch * 8), off_rows = off_tot + al(batch * 8), off_cnt = off_rows + al(batch * cap * 8), off_pre = off_cnt + al(batch * nblocks * 4), bytes = off_pre + al(batch * nblocks * 4);
    if (nonzero_layout(batch, cap, nblocks) != bytes) { ok = false; verdict("nonzero_bytes", false, nonzero_layout(batch, cap, nblocks), bytes); }
  }
  verdict("nonzero_rows_bytes_unchanged", ok); ok = true;
  // copy check: the pointers, 256 B of total, the failed list, count + prefix per workgroup of the staged piece, the two staged lists (at most 2^22 entries)
  for (uint64_t n_cols : {1ull, 5ull, 33ull}) for (uint64_t cap : {0ull, 16ull, 65536ull}) for (uint64_t count : {0ull, 1ull, 1025ull, (1ull << 22) + 1}) {
    const uint64_t stage = std::min<uint64_t>(count, 1ull << 22), max_blocks = cdiv(stage, 1024);
    const uint64_t off_tot = al(n_cols * 8), off_failed = off_tot + 256, off_cnt = off_failed + al(cap * 8), off_pre = off_cnt + al(max_blocks * 4), off_cells = off_pre + al(max_blocks * 4),
                   off_images = off_cells + al(stage * 8), bytes = off_images + al(stage * 8);
    if (copy_layout(n_cols, cap, max_blocks, stage) != bytes) { ok = false; verdict("copy_bytes", false, copy_layout(n_cols, cap, max_blocks, stage), bytes); }
  }
  verdict("copy_check_bytes_unchanged", ok); ok = true;
  // pairing products: G1 points (64 B) and G2 points (128 B) rounded, three arrays of 384-byte values packed, the flags rounded, 256 B for the two indices
  for (uint64_t groups : {1ull, 3ull, 1000ull}) for (uint64_t per : {1ull, 2ull, 5ull, 1048ull}) {
    const uint64_t n = groups * per;
    const uint64_t off_q = al(n * 64), off_a = off_q + al(n * 128), off_b = off_a + n * 384, off_gt = off_b + n * 384, off_one = off_gt + groups * 384, off_bad = off_one + al(groups * 4), bytes = off_bad + 256;
    if (pairing_layout(n, groups) != bytes) { ok = false; verdict("pairing_bytes", false, pairing_layout(n, groups), bytes); }
  }
  verdict("pairing_bytes_unchanged", ok); ok = true;
  // Poseidon transcripts: five rounded fields
  for (uint64_t jobs : {1ull, 7ull, 1ull << 20}) for (uint64_t n_words : {0ull, 1ull, 1001ull, 1ull << 24}) for (uint64_t n_sq : {1ull, 9ull, 1ull << 24}) {
    const uint64_t off_woff = al(n_words * 32), off_soff = off_woff + al((jobs + 1) * 8), off_sq = off_soff + al((jobs + 1) * 8), off_out = off_sq + al(n_sq * 4), bytes = off_out + al(n_sq * 32);
    if (poseidon_layout(n_words, jobs, n_sq) != bytes) { ok = false; verdict("poseidon_bytes", false, poseidon_layout(n_words, jobs, n_sq), bytes); }
  }
  verdict("poseidon_bytes_unchanged", ok);
  std::printf("wrong %d\n", g_wrong);
  return g_wrong;
}
