// lib_aux.hip -- libmi355zk.so, the translation unit of the kernels either side of MSM / NTT: the DFT over G1 points
// (g1fft.hpp: g_to_lagrange, ParamsKZG::downsize), the multiplicative scans of the permutation / lookup arguments and kate_division
// (frscan.hpp), Curve::batch_normalize, the one G2 scalar multiple of ParamsKZG::setup (g2.hpp), the multiplicities of the mv-lookup argument
// (lookup.hpp), the sigma columns of the permutation argument (perm.hpp), the compressed-point codec of G1 (g1codec.hpp), the two reductions of the witness
// check (check.hpp), the prover's randomness (frrand.hpp), the Poseidon transcripts of a batch of verifiers (poseidon.hpp) and their scalar sides (frprog.hpp).  Host logic only.
// The shape of an entry point: guarded([&] { slot + DevGuard; need_init; argument checks; WsLayout names the fields of the workspace; PoolBlock owns it; the body calls
// HIPCHK / CHK and returns where it fails -- the block goes back to the pool on every path; finish_async() }).  The exception: mi355_buf_upload_packed / _sparse take no
// DevGuard and do not call finish_async() -- like mi355_buf_upload, which they stand in for, they only queue (see "narrow uploads" below).
// kernel headers first: lib_common.hpp defines the macro `g` (the calling thread's device context), a name the kernels use for locals
#include "g1fft.hpp"
#include "frscan.hpp"
#include "g2.hpp"
#include "lookup.hpp"
#include "lookup_permute.hpp"
#include "perm.hpp"
#include "g1codec.hpp"
#include "check.hpp"
#include "frrand.hpp"
#include "poseidon.hpp"
#include "frprog.hpp"
#include "lib_common.hpp"
#include <thread>

namespace mi355 {

static_assert(sizeof(g2_affine_t) == 128, "G2Affine is 128 bytes (x.c0, x.c1, y.c0, y.c1)");

int aux_tu_init_device() {
  HIPCHK(hipFuncSetAttribute((const void *)k_fr_prefix_product<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)k_fr_prefix_product<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)(k_fr_prefix_product<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)(k_fr_prefix_product<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)k_fr_linrec<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  HIPCHK(hipFuncSetAttribute((const void *)k_fr_linrec<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return MI355_OK;
}

// DFT over G1 points (g1fft.hpp).  in: n x (96 B Jacobian | 64 B affine), out likewise (may alias in); scale: optional Fr (Montgomery).
int g1fft_impl(const void *in, int in_jac, void *out, int out_jac, uint32_t log_n, const void *omega, const void *scale_host) {
  const uint32_t n = 1u << log_n, half = std::max(1u, n / 2);
  g1_xyzz_t *work; fe_t *tw; fe_t scale = Fr::zero(); if (scale_host) memcpy(&scale, scale_host, 32);
  CHK(ws_get("g1fft.work", (size_t)n * sizeof(g1_xyzz_t), (void **)&work));
  CHK(ws_get("g1fft.tw", (size_t)half * sizeof(fe_t), (void **)&tw));
  hipStream_t s = g.stream;
  fe_t w; memcpy(&w, omega, 32);
  Scope total("g1_fft");
  CHK(launch_pow_table(tw, w, 1, half));   // kernel of ntt29.hpp, launched by lib_ntt.hip on this context's stream
  if (in_jac) hipLaunchKernelGGL(k_g1fft_load<1>, dim3(ceil_div(n, 256)), dim3(256), 0, s, in, work, log_n);
  else hipLaunchKernelGGL(k_g1fft_load<0>, dim3(ceil_div(n, 256)), dim3(256), 0, s, in, work, log_n);
  for (uint32_t st = 0; st < log_n; st++) hipLaunchKernelGGL(k_g1fft_stage, dim3(ceil_div(n / 2, 256)), dim3(256), 0, s, work, tw, log_n, st);
  if (out_jac) hipLaunchKernelGGL(k_g1fft_store<1>, dim3(ceil_div(n, 256)), dim3(256), 0, s, work, out, log_n, scale, scale_host ? 1 : 0);
  else hipLaunchKernelGGL(k_g1fft_store<0>, dim3(ceil_div(n, 256)), dim3(256), 0, s, work, out, log_n, scale, scale_host ? 1 : 0);
  HIPCHK(hipGetLastError());
  return MI355_OK;
}

// data[i] <- data[i]^-1 (zeros kept): tile products -> (recursively) their inverses -> per-tile completion
int batch_invert_impl(fe_t *data, uint64_t n, int level) {
  const uint32_t tiles = (uint32_t)ceil_div(n, FRSCAN_TILE);
  hipStream_t s = g.stream;
  if (tiles <= 32) { hipLaunchKernelGGL(k_fr_batch_invert<0>, dim3(tiles), dim3(FRSCAN_THREADS), 0, s, data, n, (fe_t *)nullptr); return MI355_OK; }
  fe_t *tile_prod; const std::string role = "frscan.inv_tiles" + std::to_string(level);
  CHK(ws_get(role.c_str(), (size_t)tiles * sizeof(fe_t), (void **)&tile_prod));
  hipLaunchKernelGGL(k_fr_batch_invert<1>, dim3(tiles), dim3(FRSCAN_THREADS), 0, s, data, n, tile_prod);
  CHK(batch_invert_impl(tile_prod, tiles, level + 1));
  hipLaunchKernelGGL(k_fr_batch_invert<2>, dim3(tiles), dim3(FRSCAN_THREADS), 0, s, data, n, tile_prod);
  return MI355_OK;
}

// P_j = src_j + m * P_(j-1) over n elements (dst may alias src); reverse: index j lives at memory position n - 1 - j
int linrec_impl(const fe_t *src, fe_t *dst, uint64_t n, const fe_t &m, bool reverse, int level) {
  const uint32_t tiles = (uint32_t)ceil_div(n, FRSCAN_TILE);
  const size_t lds = (size_t)(FRSCAN_THREADS * 65) * 4;
  hipStream_t s = g.stream;
  if (tiles <= 1) { hipLaunchKernelGGL(k_fr_linrec<1>, dim3(1), dim3(FRSCAN_THREADS), lds, s, src, dst, n, m, reverse ? 1 : 0, (fe_t *)nullptr); return MI355_OK; }
  fe_t *tile_tot; const std::string role = "frscan.linrec" + std::to_string(level);
  CHK(ws_get(role.c_str(), (size_t)tiles * sizeof(fe_t), (void **)&tile_tot));
  hipLaunchKernelGGL(k_fr_linrec<0>, dim3(tiles), dim3(FRSCAN_THREADS), lds, s, src, dst, n, m, reverse ? 1 : 0, tile_tot);
  CHK(linrec_impl(tile_tot, tile_tot, tiles, Fr::pow_u64(m, FRSCAN_TILE), false, level + 1));   // the value of the recurrence at every tile end
  hipLaunchKernelGGL(k_fr_linrec<1>, dim3(tiles), dim3(FRSCAN_THREADS), lds, s, src, dst, n, m, reverse ? 1 : 0, tile_tot);
  return MI355_OK;
}

// workgroups of a grid-stride launch over n elements: enough to cover them, at most per_cu_cap per compute unit of the bound device (0: no such cap) and 65535 x 4 in all;
// a positive value of the environment variable env_override replaces the count (tests: the result of a grid-stride kernel must not depend on its grid)
static uint32_t grid_blocks(uint64_t n, uint32_t threads, uint32_t per_cu_cap = 0, const char *env_override = nullptr) {
  uint64_t blocks = std::min<uint64_t>(ceil_div(n, threads), per_cu_cap ? (uint64_t)g.prop.multiProcessorCount * per_cu_cap : 65535u * 4);
  if (const char *e = env_override ? getenv(env_override) : nullptr) { const long v = atol(e); if (v > 0) blocks = std::min<uint64_t>((uint64_t)v, 65535u * 4); }
  return (uint32_t)std::max<uint64_t>(1, blocks);
}
// ---- G1 point codec (g1codec.hpp).  Grid: grid-stride over at most 16 workgroups per CU; MI355_G1_CODEC_BLOCKS overrides the workgroup count (tests run the
// error reporting at two grid sizes; the result must not depend on it)
int launch_g1_decompress(const void *bytes_dev, void *affine_out_dev, uint64_t n, uint64_t base, unsigned long long *err_dev) {
  if (!n) return MI355_OK;
  Scope sc("g1_decompress");
  hipLaunchKernelGGL(k_g1_decompress, dim3(grid_blocks(n, G1CODEC_THREADS, 16, "MI355_G1_CODEC_BLOCKS")), dim3(G1CODEC_THREADS), 0, g.stream, (const uint4 *)bytes_dev, (uint4 *)affine_out_dev, n, base, err_dev);
  sc.close();
  HIPCHK(hipGetLastError());
  return MI355_OK;
}
static int launch_g1_compress(const void *affine_dev, void *bytes_out_dev, uint64_t n) {
  if (!n) return MI355_OK;
  Scope sc("g1_compress");
  hipLaunchKernelGGL(k_g1_compress, dim3(grid_blocks(n, G1CODEC_THREADS, 16, "MI355_G1_CODEC_BLOCKS")), dim3(G1CODEC_THREADS), 0, g.stream, (const uint4 *)affine_dev, (uint4 *)bytes_out_dev, n);
  sc.close();
  HIPCHK(hipGetLastError());
  return MI355_OK;
}
bool g2_decode_host(const uint8_t in[64], void *g2affine_out) {
  g2_affine_t p; const bool ok = g2_decompress_point(in, p);
  memcpy(g2affine_out, &p, sizeof p);
  return ok;
}
static bool ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
  const char *x = (const char *)a, *y = (const char *)b;
  return x < y + b_bytes && y < x + a_bytes;
}
static int g1codec_bad_index(uint64_t bad, uint64_t *first_bad_out) {
  if (first_bad_out) *first_bad_out = bad;
  return fail(MI355_EBADARG, "g1_decompress: word " + std::to_string(bad) + " is not the compressed form of a G1 point (x >= q, x^3 + 3 a non-residue, or the identity with the sign bit set)");
}
// the argument checks a _dev / _host pair shares (n != 0); the alignment rule binds device pointers only: the host forms stage through the library's own buffers
static int g1codec_check_args(const char *who, const void *in, uint64_t in_each, const void *out, uint64_t out_each, uint64_t n, bool dev) {
  if (!in || !out) return fail(MI355_EBADARG, std::string(who) + ": null pointer");
  if (n >= (1ull << 32)) return fail(MI355_EBADARG, std::string(who) + ": n must be < 2^32");
  if (ranges_overlap(in, n * in_each, out, n * out_each)) return fail(MI355_EBADARG, std::string(who) + ": input and output must not overlap");
  if (dev && (((uintptr_t)in | (uintptr_t)out) & 15)) return fail(MI355_EBADARG, std::string(who) + ": device pointers must be 16-byte aligned");
  return MI355_OK;
}
// Curve::batch_normalize: the host form stages input and output side by side on the device, so only device operands can overlap
static int g1norm_check_args(const void *jac, const void *affine, uint64_t n, bool dev) {
  if (n && (!jac || !affine)) return fail(MI355_EBADARG, "g1_batch_normalize: null pointer");
  if (n >= (1ull << 31)) return fail(MI355_EBADARG, "g1_batch_normalize: n must be < 2^31");
  if (dev && n && ranges_overlap(jac, n * sizeof(g1_jac_t), affine, n * sizeof(g1_affine_t))) return fail(MI355_EBADARG, "g1_batch_normalize: input and output must not overlap");
  return MI355_OK;
}
// ---- a host table of `count` device pointers (the columns of a witness, the vectors of a batch).  common_slot (lib_core.hip) names the device slot that owns them before the
// lock is taken (null entries are skipped there and refused here); check_ptr_table, after the entry point's scalar checks: every entry non-null, 16-byte aligned, and
// bytes_each bytes from it inside the library block that holds it.
static int check_ptr_table(const void *const *ptrs, uint32_t count, uint64_t bytes_each, const char *who, const char *noun) {
  for (uint32_t j = 0; j < count; j++) {
    if (!ptrs[j]) return fail(MI355_EBADARG, std::string(who) + ": null " + noun + " " + std::to_string(j));
    if ((uintptr_t)ptrs[j] & 15) return fail(MI355_EBADARG, std::string(who) + ": " + noun + " " + std::to_string(j) + " is not 16-byte aligned");
    CHK(buf_check_range(ptrs[j], bytes_each, who));
  }
  return MI355_OK;
}
constexpr uint64_t G1CODEC_HOST_CHUNK = 1ull << 22;   // points per staged chunk of the host-pointer forms (128 + 256 MiB of workspace at most)

}  // namespace mi355

using namespace mi355;

// dst[i] = product (ADD: sum) of src[j], j < i: tile totals -> scan of the totals by one workgroup -> per-tile completion
template <bool ADD> int prefix_scan_entry(void *dst_dev, const void *src_dev, uint64_t n, void *total_out_host, const char *what) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({dst_dev, src_dev}, &slot, what)); DevGuard lk(slot);
  CHK(need_init(slot));
  if (n && (!dst_dev || !src_dev)) return fail(MI355_EBADARG, std::string(what) + ": null pointer");
  if (n >= (1ull << 40)) return fail(MI355_EBADARG, std::string(what) + ": n too large");
  const uint32_t tiles = (uint32_t)ceil_div(n, FRSCAN_TILE);
  fe_t *tile_prod, *tile_prefix, *total;
  CHK(ws_get("frscan.tile_prod", ((size_t)tiles + 1) * sizeof(fe_t), (void **)&tile_prod));
  CHK(ws_get("frscan.tile_prefix", ((size_t)tiles + 1) * sizeof(fe_t), (void **)&tile_prefix));
  CHK(ws_get("frscan.total", sizeof(fe_t), (void **)&total));
  const size_t lds = (size_t)(FRSCAN_THREADS * 65) * 4;
  hipStream_t s = g.stream;
  if (tiles) hipLaunchKernelGGL((k_fr_prefix_product<0, ADD>), dim3(tiles), dim3(FRSCAN_THREADS), lds, s, (const fe_t *)src_dev, (fe_t *)dst_dev, n, tile_prod, (const fe_t *)tile_prefix);
  hipLaunchKernelGGL(k_fr_scan_tiles<ADD>, dim3(1), dim3(FRSCAN_THREADS), 0, s, (const fe_t *)tile_prod, tile_prefix, tiles, total);
  if (tiles) hipLaunchKernelGGL((k_fr_prefix_product<1, ADD>), dim3(tiles), dim3(FRSCAN_THREADS), lds, s, (const fe_t *)src_dev, (fe_t *)dst_dev, n, tile_prod, (const fe_t *)tile_prefix);
  HIPCHK(hipGetLastError());
  if (total_out_host) { HIPCHK(hipMemcpyAsync(total_out_host, total, sizeof(fe_t), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
  return MI355_OK;
  });
}

// scan of n u32 under OP (0: sum, 1: max) for mi355_fr_lookup_permute_dev (lookup_permute.hpp; in may be out); aux: room for the totals of every level (lp_scan_aux_words)
static uint64_t lp_scan_aux_words(uint64_t n) { uint64_t w = 0; while (n > 1) { n = (n + LP_SCAN_TILE - 1) / LP_SCAN_TILE; w += n; } return w + 1; }
template <int OP, bool INCL> static void lp_scan(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t *aux, hipStream_t s) {
  const uint32_t tiles = ceil_div(n, LP_SCAN_TILE);
  hipLaunchKernelGGL((k_lp_scan_tile<OP, INCL>), dim3(tiles), dim3(LP_THREADS), 0, s, in, out, n, aux);
  if (tiles <= 1) return;
  lp_scan<OP, false>(aux, aux, tiles, aux + tiles, s);
  hipLaunchKernelGGL(k_lp_scan_fix<OP>, dim3(tiles), dim3(LP_THREADS), 0, s, out, n, (const uint32_t *)aux);
}

extern "C" {

// Curve::batch_normalize: n Jacobian points (96 B, any representative) -> n affine points (64 B); k_g1_batch_normalize (frscan.hpp)
int mi355_g1_batch_normalize_dev(const void *jac_dev, void *affine_dev, uint64_t n) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({jac_dev, affine_dev}, &slot, "g1_batch_normalize")); DevGuard lk(slot);
  CHK(need_init(slot));
  CHK(g1norm_check_args(jac_dev, affine_dev, n, true));
  if (n) {
    hipLaunchKernelGGL(k_g1_batch_normalize, dim3(ceil_div(n, FRSCAN_THREADS)), dim3(FRSCAN_THREADS), 0, g.stream, (const g1_jac_t *)jac_dev, (g1_affine_t *)affine_dev, n);
    HIPCHK(hipGetLastError());
  }
  return finish_async();
  });
}
int mi355_g1_batch_normalize_host(const void *jac_host, void *affine_host, uint64_t n) {
  return guarded([&]() -> int {
  const int slot = pick_replica_slot(); DevGuard lk(slot);
  CHK(need_init(slot));
  CHK(g1norm_check_args(jac_host, affine_host, n, false));
  if (!n) return MI355_OK;
  char *dev; CHK(ws_get("io.g1norm", n * (sizeof(g1_jac_t) + sizeof(g1_affine_t)), (void **)&dev));
  g1_jac_t *in = (g1_jac_t *)dev; g1_affine_t *out = (g1_affine_t *)(dev + n * sizeof(g1_jac_t));
  HIPCHK(hipMemcpyAsync(in, jac_host, n * sizeof(g1_jac_t), hipMemcpyHostToDevice, g.stream));
  hipLaunchKernelGGL(k_g1_batch_normalize, dim3(ceil_div(n, FRSCAN_THREADS)), dim3(FRSCAN_THREADS), 0, g.stream, (const g1_jac_t *)in, out, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(affine_host, out, n * sizeof(g1_affine_t), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return MI355_OK;
  });
}
// ---- G1Affine::from_bytes / to_bytes over arrays (g1codec.hpp)
int mi355_g1_decompress_dev(const void *bytes_dev, void *affine_out_dev, uint64_t n, uint64_t *first_bad_out) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({affine_out_dev, bytes_dev}, &slot, "g1_decompress")); DevGuard lk(slot);
  CHK(need_init(slot));
  if (first_bad_out) *first_bad_out = ~0ull;
  if (n == 0) return MI355_OK;
  CHK(g1codec_check_args("g1_decompress", bytes_dev, 32, affine_out_dev, sizeof(g1_affine_t), n, true));
  unsigned long long *err; CHK(ws_get("g1codec.err", 8, (void **)&err));
  HIPCHK(hipMemsetAsync(err, 0xff, 8, g.stream));
  CHK(launch_g1_decompress(bytes_dev, affine_out_dev, n, 0, err));
  unsigned long long bad = ~0ull;
  HIPCHK(hipMemcpyAsync(&bad, err, 8, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (bad != ~0ull) return g1codec_bad_index(bad, first_bad_out);
  return finish_async();
  });
}
int mi355_g1_decompress_host(const void *bytes_host, void *affine_out_host, uint64_t n, uint64_t *first_bad_out) {
  return guarded([&]() -> int {
  const int slot = pick_replica_slot(); DevGuard lk(slot);
  CHK(need_init(slot));
  if (first_bad_out) *first_bad_out = ~0ull;
  if (n == 0) return MI355_OK;
  CHK(g1codec_check_args("g1_decompress", bytes_host, 32, affine_out_host, sizeof(g1_affine_t), n, false));
  const uint64_t chunk = std::min(n, G1CODEC_HOST_CHUNK);
  char *dev; CHK(ws_get("io.g1codec", chunk * (32 + sizeof(g1_affine_t)) + 256, (void **)&dev));
  unsigned long long *err = (unsigned long long *)dev; char *in = dev + 256, *out = in + chunk * 32;
  HIPCHK(hipMemsetAsync(err, 0xff, 8, g.stream));
  for (uint64_t lo = 0; lo < n; lo += chunk) {
    const uint64_t len = std::min(chunk, n - lo);
    HIPCHK(hipMemcpyAsync(in, (const char *)bytes_host + lo * 32, len * 32, hipMemcpyHostToDevice, g.stream));
    CHK(launch_g1_decompress(in, out, len, lo, err));
    HIPCHK(hipMemcpyAsync((char *)affine_out_host + lo * sizeof(g1_affine_t), out, len * sizeof(g1_affine_t), hipMemcpyDeviceToHost, g.stream));
  }
  unsigned long long bad = ~0ull;
  HIPCHK(hipMemcpyAsync(&bad, err, 8, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  resolve_spans();
  if (bad != ~0ull) return g1codec_bad_index(bad, first_bad_out);
  return MI355_OK;
  });
}
int mi355_g1_compress_dev(const void *affine_dev, void *bytes_out_dev, uint64_t n) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({bytes_out_dev, affine_dev}, &slot, "g1_compress")); DevGuard lk(slot);
  CHK(need_init(slot));
  if (n == 0) return MI355_OK;
  CHK(g1codec_check_args("g1_compress", affine_dev, sizeof(g1_affine_t), bytes_out_dev, 32, n, true));
  CHK(launch_g1_compress(affine_dev, bytes_out_dev, n));
  return finish_async();
  });
}
int mi355_g1_compress_host(const void *affine_host, void *bytes_out_host, uint64_t n) {
  return guarded([&]() -> int {
  const int slot = pick_replica_slot(); DevGuard lk(slot);
  CHK(need_init(slot));
  if (n == 0) return MI355_OK;
  CHK(g1codec_check_args("g1_compress", affine_host, sizeof(g1_affine_t), bytes_out_host, 32, n, false));
  const uint64_t chunk = std::min(n, G1CODEC_HOST_CHUNK);
  char *dev; CHK(ws_get("io.g1codec", chunk * (32 + sizeof(g1_affine_t)) + 256, (void **)&dev));
  char *out = dev + 256, *in = out + chunk * 32;
  for (uint64_t lo = 0; lo < n; lo += chunk) {
    const uint64_t len = std::min(chunk, n - lo);
    HIPCHK(hipMemcpyAsync(in, (const char *)affine_host + lo * sizeof(g1_affine_t), len * sizeof(g1_affine_t), hipMemcpyHostToDevice, g.stream));
    CHK(launch_g1_compress(in, out, len));
    HIPCHK(hipMemcpyAsync((char *)bytes_out_host + lo * 32, out, len * 32, hipMemcpyDeviceToHost, g.stream));
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  resolve_spans();
  return MI355_OK;
  });
}
// ---- DFT over G1 points (best_fft::<Fr, G1>, g_to_lagrange)
int mi355_g1_fft_dev(void *points_jac_dev, uint32_t log_n, const void *omega) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({points_jac_dev}, &slot, "g1_fft")); DevGuard lk(slot);
  CHK(need_init(slot)); CHK(check_ntt_args(points_jac_dev, log_n, omega));
  CHK(g1fft_impl(points_jac_dev, 1, points_jac_dev, 1, log_n, omega, nullptr));
  return finish_async();
  });
}
int mi355_g1_fft_host(void *points_jac_host, uint32_t log_n, const void *omega) {
  return guarded([&]() -> int {
  const int slot = pick_replica_slot(); DevGuard lk(slot);
  CHK(need_init(slot)); CHK(check_ntt_args(points_jac_host, log_n, omega));
  NttHostArgs a{log_n, omega, nullptr};
  const size_t bytes = sizeof(g1_jac_t) << log_n;
  return with_host_io(points_jac_host, bytes, bytes, bytes, "io.g1fft", [](void *dev, void *ud) { auto *a = (NttHostArgs *)ud; return g1fft_impl(dev, 1, dev, 1, a->log_n, a->omega, nullptr); }, &a);
  });
}
int mi355_g_to_lagrange_dev(const void *g_affine_dev, void *g_lagrange_affine_dev, uint32_t log_n, const void *omega_inv, const void *n_inv) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({g_affine_dev, g_lagrange_affine_dev}, &slot, "g_to_lagrange")); DevGuard lk(slot);
  CHK(need_init(slot)); CHK(check_ntt_args(g_affine_dev, log_n, omega_inv));
  if (!g_lagrange_affine_dev || !n_inv) return fail(MI355_EBADARG, "g_to_lagrange: null pointer");
  CHK(g1fft_impl(g_affine_dev, 0, g_lagrange_affine_dev, 0, log_n, omega_inv, n_inv));
  return finish_async();
  });
}
int mi355_srs_downsize(uint64_t g_handle, uint32_t k, const void *omega_inv, const void *n_inv, uint64_t *g_lagrange_handle_out) {
  return guarded([&]() -> int {
  AllGuard lk;
  CHK(need_init());
  Srs *sp; CHK(srs_find(g_handle, &sp, "srs_downsize"));
  if (!omega_inv || !n_inv || !g_lagrange_handle_out || k > 28 || (1ull << k) > sp->n) return fail(MI355_EBADARG, "srs_downsize: bad argument (2^k must not exceed the registered basis)");
  const uint64_t n = 1ull << k;
  for (int sl = 1; sl < g_ndev; sl++) { CHK(bind_ctx(sl)); HIPCHK(hipStreamSynchronize(g.stream)); }
  CHK(bind_ctx(0));
  const g1_affine_t *src; CHK(srs_gather_to_primary(*sp, n, &src));
  g1_affine_t *res; CHK(dev_malloc((void **)&res, n * sizeof(g1_affine_t), "srs_downsize", mi355zk::MEM_SRS));
  int rc = g1fft_impl(src, 0, res, 0, k, omega_inv, n_inv);
  if (rc == MI355_OK) rc = finish_async();
  if (rc == MI355_OK && hipStreamSynchronize(g.stream) != hipSuccess) rc = fail(MI355_EHIP, "srs_downsize: stream synchronize failed");
  Srs s; s.n = n; s.mem = std::make_shared<SrsMem>();
  if (rc == MI355_OK) {
    if (plan_shards(n).size() == 1) { Shard one; one.slot = 0; one.lo = 0; one.n = n; one.dev = res; one.owned = true; s.mem->sh.push_back(one); res = nullptr; }
    else rc = srs_scatter_from_primary(*s.mem, res, n, false);
  }
  if (res) { (void)bind_ctx(0); dev_free(res); }
  if (rc != MI355_OK) return rc;
  *g_lagrange_handle_out = srs_insert(s); return MI355_OK;
  });
}
int mi355_fr_kate_division_dev(void *dst_dev, const void *poly_dev, uint64_t n, const void *z) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({dst_dev, poly_dev}, &slot, "fr_kate_division")); DevGuard lk(slot);
  CHK(need_init(slot));
  if (!z || n == 0 || !poly_dev || (n > 1 && !dst_dev)) return fail(MI355_EBADARG, "fr_kate_division: null pointer or empty polynomial");
  if (n >= (1ull << 40)) return fail(MI355_EBADARG, "fr_kate_division: n too large");
  if (n == 1) return MI355_OK;   // a constant: the quotient is empty
  fe_t m; memcpy(&m, z, 32);
  CHK(linrec_impl((const fe_t *)poly_dev + 1, (fe_t *)dst_dev, n - 1, m, true, 0));
  HIPCHK(hipGetLastError());
  return MI355_OK;
  });
}
int mi355_fr_batch_invert_dev(void *data_dev, uint64_t n) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({data_dev}, &slot, "fr_batch_invert")); DevGuard lk(slot);
  CHK(need_init(slot));
  if (n && !data_dev) return fail(MI355_EBADARG, "fr_batch_invert: null pointer");
  if (n >= (1ull << 40)) return fail(MI355_EBADARG, "fr_batch_invert: n too large");
  if (n == 0) return MI355_OK;
  CHK(batch_invert_impl((fe_t *)data_dev, n, 0));
  HIPCHK(hipGetLastError());
  return MI355_OK;
  });
}
int mi355_fr_prefix_product_dev(void *dst_dev, const void *src_dev, uint64_t n, void *total_out_host) { return prefix_scan_entry<false>(dst_dev, src_dev, n, total_out_host, "fr_prefix_product"); }
int mi355_fr_prefix_sum_dev(void *dst_dev, const void *src_dev, uint64_t n, void *total_out_host) { return prefix_scan_entry<true>(dst_dev, src_dev, n, total_out_host, "fr_prefix_sum"); }
// ---- G2: s_g2 = tau * G2 of ParamsKZG::setup (the only G2 arithmetic on the path)
int mi355_g2_mul_host(const void *p_affine_host, const void *scalar, void *out_affine_host) {
  return guarded([&]() -> int {
  const int slot = pick_replica_slot(); DevGuard lk(slot);
  CHK(need_init(slot));
  if (!p_affine_host || !scalar || !out_affine_host) return fail(MI355_EBADARG, "g2_mul: null pointer");
  g2_affine_t *dev; CHK(ws_get("g2.io", 2 * sizeof(g2_affine_t) + 16, (void **)&dev));
  uint32_t *flag = reinterpret_cast<uint32_t *>(dev + 2);
  fe_t k; memcpy(&k, scalar, 32);
  HIPCHK(hipMemcpyAsync(dev, p_affine_host, sizeof(g2_affine_t), hipMemcpyHostToDevice, g.stream));
  hipLaunchKernelGGL(k_g2_mul, dim3(1), dim3(64), 0, g.stream, (const g2_affine_t *)dev, k, dev + 1, flag);
  HIPCHK(hipGetLastError());
  uint32_t ok = 0; g2_affine_t res;
  HIPCHK(hipMemcpyAsync(&res, dev + 1, sizeof res, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(&ok, flag, 4, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (!ok) return fail(MI355_EBADARG, "g2_mul: the point is not on the twist y^2 = x^3 + 3 / (9 + u)");
  memcpy(out_affine_host, &res, sizeof res);
  return MI355_OK;
  });
}

// ---- narrow uploads: a witness column as W-byte integers or as (index, value) pairs of its non-zero cells instead of n 32-byte words.  The narrow data crosses PCIe through
// mi355_buf_upload (copy stream, no device lock) into a pooled staging block; the expansion kernel is queued on the owner's compute stream WITHOUT the device lock (it touches
// no context state; HIP streams accept work from several threads) and the call returns without waiting for it: calls issued afterwards on that device are ordered behind it.
// staging blocks come in size classes (powers of two up to 1 MiB, then whole MiB): column after column of slightly different size -- the pairs of a sparse column -- then hits
// the exact-size pool instead of missing it and recycling the pool (which synchronises the copy stream and the free events on the uploader thread)
static uint64_t stage_class(uint64_t bytes) {
  if (bytes <= (1ull << 20)) { uint64_t c = 4096; while (c < bytes) c <<= 1; return c; }
  return (bytes + (1ull << 20) - 1) & ~((1ull << 20) - 1);
}
int mi355_buf_upload_packed(void *dst_dev, const void *src_host, uint64_t n, uint32_t width_bytes) {
  return guarded([&]() -> int {
  if (n == 0) return MI355_OK;
  if (!dst_dev || !src_host) return fail(MI355_EBADARG, "buf_upload_packed: null pointer");
  if (width_bytes != 1 && width_bytes != 2 && width_bytes != 4 && width_bytes != 8) return fail(MI355_EBADARG, "buf_upload_packed: width must be 1, 2, 4 or 8 bytes");
  if (n > (1ull << 32)) return fail(MI355_EBADARG, "buf_upload_packed: more than 2^32 cells");   // also keeps n * width_bytes and n * 32 far from overflow
  CHK(buf_check_range(dst_dev, n * sizeof(fe_t), "buf_upload_packed"));
  const int slot = slot_of(dst_dev);
  PoolBlock stage; CHK(stage.alloc(stage_class(n * width_bytes), slot));
  CHK(stage.upload(0, src_host, n * width_bytes));
  hipStream_t s = g_ctx[slot].stream; const dim3 grid(grid_blocks(n, 256)); const uint8_t *src = (const uint8_t *)stage.p;
  switch (width_bytes) {
    case 1: hipLaunchKernelGGL(k_expand_packed<1>, grid, dim3(256), 0, s, (fe_t *)dst_dev, src, n); break;
    case 2: hipLaunchKernelGGL(k_expand_packed<2>, grid, dim3(256), 0, s, (fe_t *)dst_dev, src, n); break;
    case 4: hipLaunchKernelGGL(k_expand_packed<4>, grid, dim3(256), 0, s, (fe_t *)dst_dev, src, n); break;
    default: hipLaunchKernelGGL(k_expand_packed<8>, grid, dim3(256), 0, s, (fe_t *)dst_dev, src, n); break;
  }
  HIPCHK(hipGetLastError());
  return MI355_OK;   // the block goes back to the pool here; its reuse waits for the kernel queued above
  });
}
int mi355_buf_upload_sparse(void *dst_dev, uint64_t n, const uint32_t *idx_host, const void *vals_host, uint64_t count) {
  return guarded([&]() -> int {
  if (n == 0) return MI355_OK;
  if (!dst_dev || (count && (!idx_host || !vals_host))) return fail(MI355_EBADARG, "buf_upload_sparse: null pointer");
  if (count > n || n > (1ull << 32)) return fail(MI355_EBADARG, "buf_upload_sparse: more pairs than cells, or more than 2^32 cells");
  CHK(buf_check_range(dst_dev, n * sizeof(fe_t), "buf_upload_sparse"));
  const int slot = slot_of(dst_dev);
  CHK(need_init(slot));
  hipStream_t s = g_ctx[slot].stream;
  if (count == 0) { HIPCHK(hipMemsetAsync(dst_dev, 0, n * sizeof(fe_t), s)); return MI355_OK; }
  const uint64_t idx_bytes = (count * 4 + 31) & ~31ull;
  PoolBlock stage; CHK(stage.alloc(stage_class(idx_bytes + count * sizeof(fe_t)), slot));
  CHK(stage.upload(0, idx_host, count * 4));
  CHK(stage.upload(idx_bytes, vals_host, count * sizeof(fe_t)));
  HIPCHK(hipMemsetAsync(dst_dev, 0, n * sizeof(fe_t), s));
  hipLaunchKernelGGL(k_scatter_fr, dim3(grid_blocks(count, 256)), dim3(256), 0, s, (fe_t *)dst_dev, n, (const uint32_t *)stage.p, (const fe_t *)stage.at(idx_bytes), count);
  HIPCHK(hipGetLastError());
  return MI355_OK;   // as above: the block's reuse waits for the scatter
  });
}
// host helper for the sparse form: the non-zero cells of a column of n 32-byte words as (index, value) pairs, in index order; `threads` workers scan disjoint ranges
// (zero is zero in Montgomery form too, so the scan needs no arithmetic).  idx_out / vals_out must hold n entries in the worst case; pure host code, no device.
int mi355_host_compact_nonzero(const void *src_host, uint64_t n, uint32_t *idx_out, void *vals_out, uint64_t *count_out, int threads) {
  return guarded([&]() -> int {
  if (!count_out || (n && (!src_host || !idx_out || !vals_out))) return fail(MI355_EBADARG, "host_compact_nonzero: null pointer");
  if (n > (1ull << 32)) return fail(MI355_EBADARG, "host_compact_nonzero: more than 2^32 cells");
  const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, threads), std::max<uint64_t>(1, n >> 16)));
  const uint64_t *w = (const uint64_t *)src_host; uint64_t *vo = (uint64_t *)vals_out;
  std::vector<uint64_t> cnt(T + 1, 0);
  auto nz = [&](uint64_t i) { return (w[4 * i] | w[4 * i + 1] | w[4 * i + 2] | w[4 * i + 3]) != 0; };
  auto range = [&](int t, uint64_t &lo, uint64_t &hi) { lo = n * t / T; hi = n * (t + 1) / T; };
  auto count_job = [&](int t) { uint64_t lo, hi; range(t, lo, hi); uint64_t c = 0; for (uint64_t i = lo; i < hi; i++) c += nz(i); cnt[t + 1] = c; };
  { std::vector<std::thread> th; for (int t = 1; t < T; t++) th.emplace_back(count_job, t); count_job(0); for (auto &x : th) x.join(); }
  for (int t = 0; t < T; t++) cnt[t + 1] += cnt[t];
  auto write_job = [&](int t) { uint64_t lo, hi; range(t, lo, hi); uint64_t o = cnt[t]; for (uint64_t i = lo; i < hi; i++) if (nz(i)) { idx_out[o] = (uint32_t)i; memcpy(vo + 4 * o, w + 4 * i, 32); o++; } };
  { std::vector<std::thread> th; for (int t = 1; t < T; t++) th.emplace_back(write_job, t); write_job(0); for (auto &x : th) x.join(); }
  *count_out = cnt[T];
  return MI355_OK;
  });
}

// ---- the multiplicity column m of the mv-lookup argument (lookup.hpp): hash set of the table rows -> counts per row -> Montgomery Fr.  Workspace: ONE pooled
// mi355_buf block (PoolBlock; WsLayout: the error word, 4 B per slot for the next power of two >= 2 x table_rows, 4 B per row of m: ~12 B per row), back in the pool
// on every return (mi355_mem_info counts it; mi355_buf_trim gives it back to HIP).  Synchronous: the error word is read back before the call returns.
int mi355_fr_lookup_multiplicities_dev(void *m_dev, uint64_t n, const void *table_dev, uint64_t table_rows, const void *const *inputs_dev, uint32_t n_inputs, uint64_t input_rows,
                                       uint32_t flags, uint64_t *missing_out) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({m_dev, table_dev}, &slot, "fr_lookup_multiplicities"));
  for (uint32_t c = 0; inputs_dev && c < n_inputs; c++) { int s2; CHK(common_slot({m_dev, table_dev, inputs_dev[c]}, &s2, "fr_lookup_multiplicities")); }
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (missing_out) *missing_out = ~0ull;
  if (n == 0) return MI355_OK;
  if (!m_dev || !table_dev || (n_inputs && !inputs_dev)) return fail(MI355_EBADARG, "fr_lookup_multiplicities: null pointer");
  for (uint32_t c = 0; c < n_inputs; c++) if (!inputs_dev[c] && input_rows) return fail(MI355_EBADARG, "fr_lookup_multiplicities: null input column " + std::to_string(c));
  if (n >= (1ull << 31)) return fail(MI355_EBADARG, "fr_lookup_multiplicities: n must be < 2^31");
  if (table_rows > n || input_rows > n) return fail(MI355_EBADARG, "fr_lookup_multiplicities: table_rows and input_rows must not exceed n");
  if (n_inputs >= (1u << 24)) return fail(MI355_EBADARG, "fr_lookup_multiplicities: more than 2^24 input columns");
  if ((uint64_t)n_inputs * input_rows >= (1ull << 32)) return fail(MI355_EBADARG, "fr_lookup_multiplicities: n_inputs x input_rows must be < 2^32 (u32 counts)");
  if (flags & ~1u) return fail(MI355_EBADARG, "fr_lookup_multiplicities: unknown flag bits");
  const bool last = flags & 1u;
  const uint64_t S = std::max<uint64_t>(64, 1ull << log2_ceil(2 * table_rows));
  const uint32_t mask = (uint32_t)(S - 1);
  WsLayout L; const uint64_t off_err = L.take(8), off_slots = L.take(S * 4), off_cnt = L.take_exact(n * 4);
  PoolBlock ws; CHK(ws.alloc(L.total(), slot));
  hipStream_t s = g.stream;
  unsigned long long *err = (unsigned long long *)ws.at(off_err), err_host = ~0ull; uint32_t *slots = (uint32_t *)ws.at(off_slots), *cnt = (uint32_t *)ws.at(off_cnt);
  HIPCHK(hipMemsetAsync(ws.p, 0xff, off_cnt, s));   // the error word and the empty slots
  HIPCHK(hipMemsetAsync(cnt, 0, n * 4, s));
  Scope sc("lookup_multiplicities");
  const fe_t *T = (const fe_t *)table_dev;
  if (table_rows) {
    const dim3 grid(grid_blocks(table_rows, LK_THREADS));
    if (last) hipLaunchKernelGGL(k_lk_insert<true>, grid, dim3(LK_THREADS), 0, s, T, table_rows, slots, mask);
    else hipLaunchKernelGGL(k_lk_insert<false>, grid, dim3(LK_THREADS), 0, s, T, table_rows, slots, mask);
  }
  // ~8 192 waves per column at most (one resident wave per SIMD slot of the chip, a few over): the hot row of each is one atomic at the end
  const uint64_t wave_rows = std::max<uint64_t>(2048, (ceil_div(input_rows, 8192) + 63) & ~63ull);
  const uint64_t waves = ceil_div(input_rows, wave_rows);
  for (uint32_t c = 0; c < n_inputs && input_rows; c++)
    hipLaunchKernelGGL(k_lk_probe, dim3(ceil_div(waves, LK_THREADS / 64)), dim3(LK_THREADS), 0, s, (const fe_t *)inputs_dev[c], input_rows, (uint64_t)c, T, (const uint32_t *)slots, mask, cnt, err, wave_rows);
  hipLaunchKernelGGL(k_expand_packed<4>, dim3(grid_blocks(n, 256)), dim3(256), 0, s, (fe_t *)m_dev, (const uint8_t *)cnt, n);
  sc.close();
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&err_host, err, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (err_host != ~0ull) {
    if (missing_out) *missing_out = err_host;
    return fail(MI355_EBADARG, "fr_lookup_multiplicities: input " + std::to_string(err_host >> 40) + ", row " + std::to_string(err_host & ((1ull << 40) - 1)) + " is not in the table");
  }
  return finish_async();
  });
}

// ---- the permuted columns A' and S' of the classic lookup argument (lookup_permute.hpp).  The argument checks read host memory and the buffer registry only and
// come before the device is asked for.  Workspace: ONE pooled mi355_buf block (PoolBlock; WsLayout): two header blocks, 4 B per hash slot (the next power of two
// >= 2 x rows), two counts per row, two (key word, row) ping-pong pairs per row -- the key words serve again as the run / owner maps of the expansion --, five
// u32 per row of scans, 1 KiB of histogram per 2 048 rows and the totals of the scans: 52 .. 60 B per row.  Synchronous, two synchronisations: one after the
// counts (the missing row, the number of distinct values and the digits that need a pass come back), one at the end.
int mi355_fr_lookup_permute_dev(void *perm_input, void *perm_table, const void *input, const void *table, uint64_t rows, uint64_t *missing_out) {
  return guarded([&]() -> int {
  if (missing_out) *missing_out = ~0ull;
  if (rows >= (1ull << 31)) return fail(MI355_EBADARG, "fr_lookup_permute: rows must be < 2^31");
  const uint64_t bytes = rows * sizeof(fe_t);
  if (rows) {
    if (!perm_input || !perm_table || !input || !table) return fail(MI355_EBADARG, "fr_lookup_permute: null pointer");
    if (((uintptr_t)perm_input | (uintptr_t)perm_table | (uintptr_t)input | (uintptr_t)table) & 15) return fail(MI355_EBADARG, "fr_lookup_permute: device pointers must be 16-byte aligned");
    if (ranges_overlap(perm_input, bytes, perm_table, bytes)) return fail(MI355_EBADARG, "fr_lookup_permute: the two outputs must not overlap");
    for (const void *out : {(const void *)perm_input, (const void *)perm_table})
      if (ranges_overlap(out, bytes, input, bytes) || ranges_overlap(out, bytes, table, bytes)) return fail(MI355_EBADARG, "fr_lookup_permute: an output must not overlap an input");
    for (const void *p : {(const void *)perm_input, (const void *)perm_table, input, table}) CHK(buf_check_range(p, bytes, "fr_lookup_permute"));
  }
  int slot; CHK(common_slot({perm_input, perm_table, input, table}, &slot, "fr_lookup_permute"));
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (rows == 0) return MI355_OK;
  const uint64_t S = std::max<uint64_t>(64, 1ull << log2_ceil(2 * rows));
  const uint32_t mask = (uint32_t)(S - 1), nblk_max = ceil_div(rows, LP_CHUNK);
  const uint64_t hist_words = 256ull * nblk_max;
  WsLayout L;
  const uint64_t off_ones = L.take(sizeof(LpHeadOnes)), off_slots = L.take(S * 4), off_zero = L.take(sizeof(LpHeadZero)), off_tcnt = L.take(rows * 4), off_icnt = L.take(rows * 4), off_end_zero = L.total();
  uint64_t off_key[2], off_val[2], off_arr[5];
  for (int i = 0; i < 2; i++) { off_key[i] = L.take(rows * 4); off_val[i] = L.take(rows * 4); }
  for (int i = 0; i < 5; i++) off_arr[i] = L.take(rows * 4);
  const uint64_t off_hist = L.take(hist_words * 4), off_aux = L.take(lp_scan_aux_words(std::max<uint64_t>(rows, hist_words)) * 4);
  PoolBlock ws; CHK(ws.alloc(L.total(), slot));
  hipStream_t s = g.stream;
  LpHeadOnes *ones = (LpHeadOnes *)ws.at(off_ones), ones_host; LpHeadZero *zero = (LpHeadZero *)ws.at(off_zero), zero_host;
  uint32_t *slots = (uint32_t *)ws.at(off_slots), *tcnt = (uint32_t *)ws.at(off_tcnt), *icnt = (uint32_t *)ws.at(off_icnt), *hist = (uint32_t *)ws.at(off_hist), *aux = (uint32_t *)ws.at(off_aux);
  uint32_t *key[2] = {(uint32_t *)ws.at(off_key[0]), (uint32_t *)ws.at(off_key[1])}, *val[2] = {(uint32_t *)ws.at(off_val[0]), (uint32_t *)ws.at(off_val[1])};
  uint32_t *in_cells = (uint32_t *)ws.at(off_arr[0]), *left = (uint32_t *)ws.at(off_arr[1]), *heads = (uint32_t *)ws.at(off_arr[2]), *run_start = (uint32_t *)ws.at(off_arr[3]), *left_start = (uint32_t *)ws.at(off_arr[4]);
  const fe_t *T = (const fe_t *)table, *A = (const fe_t *)input;
  HIPCHK(hipMemsetAsync(ws.at(off_ones), 0xff, off_zero - off_ones, s));       // the error words, the AND of the keys, the empty slots
  HIPCHK(hipMemsetAsync(ws.at(off_zero), 0, off_end_zero - off_zero, s));      // the number of distinct values, the OR of the keys, the counts
  {
    Scope sc("lookup_permute");
    hipLaunchKernelGGL(k_lk_insert<false>, dim3(grid_blocks(rows, LK_THREADS)), dim3(LK_THREADS), 0, s, T, rows, slots, mask);
    const uint64_t wave_rows = std::max<uint64_t>(2048, (ceil_div(rows, 8192) + 63) & ~63ull);
    const dim3 probe_grid(ceil_div(ceil_div(rows, wave_rows), LK_THREADS / 64));
    hipLaunchKernelGGL(k_lk_probe, probe_grid, dim3(LK_THREADS), 0, s, T, rows, (uint64_t)0, T, (const uint32_t *)slots, mask, tcnt, &ones->err_table, wave_rows);
    hipLaunchKernelGGL(k_lk_probe, probe_grid, dim3(LK_THREADS), 0, s, A, rows, (uint64_t)0, T, (const uint32_t *)slots, mask, icnt, &ones->err, wave_rows);
    hipLaunchKernelGGL(k_lp_compact, dim3(grid_blocks(rows, LP_THREADS, 8)), dim3(LP_THREADS), 0, s, T, rows, (const uint32_t *)tcnt, val[0], ones, zero);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&ones_host, ones, sizeof ones_host, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&zero_host, zero, sizeof zero_host, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ones_host.err != ~0ull) {
    if (missing_out) *missing_out = ones_host.err;
    return fail(MI355_EBADARG, "fr_lookup_permute: input row " + std::to_string(ones_host.err) + " is not in the table");
  }
  const uint32_t D = zero_host.distinct;
  if (D == 0 || D > rows || ones_host.err_table != ~0ull) return fail(MI355_EHIP, "fr_lookup_permute: the table's hash set is inconsistent");
  {
    Scope sc("lookup_permute");
    // LSD radix sort of the distinct values by canonical key; the passes that would move nothing are skipped
    const uint32_t nblk = ceil_div(D, LP_CHUNK);
    int cur = 0;
    for (uint32_t word = 0; word < 8; word++) {
      if (ones_host.key_and[word] == zero_host.key_or[word]) continue;
      hipLaunchKernelGGL(k_lp_gather, dim3(grid_blocks(D, LP_THREADS)), dim3(LP_THREADS), 0, s, T, rows, (const uint32_t *)val[cur], D, word, key[cur]);
      for (uint32_t pass = 4 * word; pass < 4 * word + 4; pass++) {
        if (!lp_pass_needed(ones_host.key_and, zero_host.key_or, pass)) continue;
        Scope one_pass("lookup_permute_pass");   // its launch count in the profile is the number of passes that ran
        hipLaunchKernelGGL(k_lp_hist, dim3(nblk), dim3(LP_THREADS), 0, s, (const uint32_t *)key[cur], D, pass, hist, nblk);
        lp_scan<0, false>(hist, hist, 256ull * nblk, aux, s);
        hipLaunchKernelGGL(k_lp_scatter, dim3(nblk), dim3(LP_THREADS), 0, s, (const uint32_t *)key[cur], (const uint32_t *)val[cur], key[cur ^ 1], val[cur ^ 1], D, pass, (const uint32_t *)hist, nblk);
        cur ^= 1;
      }
    }
    const uint32_t *sorted = val[cur];
    uint32_t *run_of_row = key[0], *owner_of_left = key[1];   // the key words are done with
    const dim3 gd(grid_blocks(D, LP_THREADS));
    hipLaunchKernelGGL(k_lp_counts, gd, dim3(LP_THREADS), 0, s, sorted, D, rows, (const uint32_t *)tcnt, (const uint32_t *)icnt, in_cells, left, heads);
    lp_scan<0, false>(in_cells, run_start, D, aux, s);
    lp_scan<0, false>(left, left_start, D, aux, s);
    lp_scan<0, false>(heads, heads, D, aux, s);               // heads[i]: the runs in front of run i
    HIPCHK(hipMemsetAsync(run_of_row, 0, rows * 4, s));
    HIPCHK(hipMemsetAsync(owner_of_left, 0, rows * 4, s));
    hipLaunchKernelGGL(k_lp_mark, gd, dim3(LP_THREADS), 0, s, D, rows, (const uint32_t *)in_cells, (const uint32_t *)left, (const uint32_t *)run_start, (const uint32_t *)left_start, run_of_row, owner_of_left);
    lp_scan<1, true>(run_of_row, run_of_row, rows, aux, s);
    lp_scan<1, true>(owner_of_left, owner_of_left, rows, aux, s);
    hipLaunchKernelGGL(k_lp_expand, dim3(grid_blocks(rows, LP_THREADS)), dim3(LP_THREADS), 0, s, T, sorted, rows, D, (const uint32_t *)run_of_row, (const uint32_t *)owner_of_left,
                       (const uint32_t *)run_start, (const uint32_t *)heads, (const uint32_t *)left_start, (const uint32_t *)left, (fe_t *)perm_input, (fe_t *)perm_table);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  return finish_async();
  });
}

// ---- the sigma columns of the permutation argument from the copy mapping (perm.hpp).  The mapping is checked on the host first (perm_check): on MI355_EBADARG nothing has
// been uploaded or launched.  Workspace: ONE pooled mi355_buf block (PoolBlock; WsLayout) -- the column pointers, the three power tables (n_cols + 2 x 2^(log_n / 2) words, packed)
// and a staging area for at most PERM_STAGE overrides (16 B each) -- back in the pool on every return.  Longer lists go through the staging area piece by piece: an upload into it waits for the
// kernel that reads the previous piece (mi355_buf_upload into a block in use).  Synchronous: the call returns when the columns are written.
constexpr uint64_t PERM_STAGE = 1ull << 22;
int mi355_fr_permutation_sigma_dev(void *const *sigma_dev, uint32_t n_cols, uint32_t log_n, const void *delta, const void *omega, const uint64_t *cells_host,
                                   const uint64_t *images_host, uint64_t count, uint32_t flags) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot(sigma_dev, n_cols, true, &slot, "fr_permutation_sigma"));
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (n_cols == 0 || n_cols > 65535u * PERM_COL_TILE) return fail(MI355_EBADARG, "fr_permutation_sigma: n_cols must be 1 .. " + std::to_string(65535u * PERM_COL_TILE));
  if (log_n > PERM_MAX_LOG_N) return fail(MI355_EBADARG, "fr_permutation_sigma: log_n > 28");
  if (!sigma_dev || !delta || !omega || (count && (!cells_host || !images_host))) return fail(MI355_EBADARG, "fr_permutation_sigma: null pointer");
  if (flags & ~PERM_FLAG_TRUSTED) return fail(MI355_EBADARG, "fr_permutation_sigma: unknown flag bits");
  const uint64_t n = 1ull << log_n, total = (uint64_t)n_cols * n;
  CHK(check_ptr_table(sigma_dev, n_cols, n * sizeof(fe_t), "fr_permutation_sigma", "column"));
  { uint64_t bad = 0; std::string why; if (perm_check(cells_host, images_host, count, total, flags, &bad, &why)) return fail(MI355_EBADARG, "fr_permutation_sigma: override " + std::to_string(bad) + ": " + why); }
  const uint32_t lo_bits = perm_lo_bits(log_n), n_lo = 1u << lo_bits, n_hi = 1u << (log_n - lo_bits);
  const uint64_t stage = std::min(count, PERM_STAGE);
  WsLayout L;
  const uint64_t off_cols = L.take((uint64_t)n_cols * 8), off_dpow = L.take_exact((uint64_t)n_cols * sizeof(fe_t)), off_lo = L.take_exact((uint64_t)n_lo * sizeof(fe_t)),
                 off_hi = L.take_exact((uint64_t)n_hi * sizeof(fe_t)), off_cells = L.take_exact(stage * 8), off_images = L.take_exact(stage * 8);
  PoolBlock ws; CHK(ws.alloc(L.total(), slot));
  hipStream_t s = g.stream;
  fe_t *const *cols = (fe_t *const *)ws.at(off_cols); fe_t *dpow = (fe_t *)ws.at(off_dpow), *tw_lo = (fe_t *)ws.at(off_lo), *tw_hi = (fe_t *)ws.at(off_hi);
  CHK(ws.upload(off_cols, sigma_dev, (uint64_t)n_cols * 8));
  fe_t d, w; memcpy(&d, delta, 32); memcpy(&w, omega, 32);
  const PermTables T{tw_lo, tw_hi, dpow, lo_bits};
  {
    Scope sc("permutation_sigma");
    CHK(launch_pow_table(dpow, d, 1, n_cols)); CHK(launch_pow_table(tw_lo, w, 1, n_lo)); CHK(launch_pow_table(tw_hi, w, n_lo, n_hi));
    hipLaunchKernelGGL(k_perm_identity, dim3(ceil_div(n, PERM_THREADS), ceil_div(n_cols, PERM_COL_TILE)), dim3(PERM_THREADS), 0, s, cols, n_cols, log_n, T, d);
  }
  HIPCHK(hipGetLastError());
  for (uint64_t lo = 0; lo < count; lo += stage) {
    const uint64_t len = std::min(stage, count - lo);
    CHK(ws.upload(off_cells, cells_host + lo, len * 8)); CHK(ws.upload(off_images, images_host + lo, len * 8));
    Scope sc("permutation_sigma");
    hipLaunchKernelGGL(k_perm_override, dim3(grid_blocks(len, PERM_THREADS)), dim3(PERM_THREADS), 0, s, cols, log_n, T, (const uint64_t *)ws.at(off_cells), (const uint64_t *)ws.at(off_images), len);
    sc.close();
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(s));
  return finish_async();
  });
}

// ---- the reductions of the witness check (check.hpp): count + the smallest `cap` failing indices, ascending.  Three launches per vector batch / staged piece --
// count per workgroup, scan of the counts, ranked write -- and ONE synchronisation at the end, when the totals and the indices come back.  Workspace: ONE pooled
// mi355_buf block (PoolBlock; WsLayout: the pointer table, the totals, the index lists, 8 B per workgroup of CHECK_TILE elements; copy_check: two lists of at most
// CHECK_STAGE entries), back in the pool on every return.
constexpr uint64_t CHECK_STAGE = 1ull << 22;   // a multiple of CHECK_TILE
int mi355_fr_nonzero_rows_dev(const void *const *vecs_dev, uint32_t batch, uint64_t n, uint32_t cap, uint64_t *counts_out_host, uint64_t *rows_out_host) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot(vecs_dev, batch, true, &slot, "fr_nonzero_rows"));
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (batch == 0 || n == 0) return fail(MI355_EBADARG, "fr_nonzero_rows: batch and n must not be zero");
  if (n >= (1ull << 40)) return fail(MI355_EBADARG, "fr_nonzero_rows: n too large");
  if (cap > CHECK_MAX_CAP) return fail(MI355_EBADARG, "fr_nonzero_rows: cap " + std::to_string(cap) + " exceeds " + std::to_string(CHECK_MAX_CAP));
  if (!vecs_dev || !counts_out_host || (cap && !rows_out_host)) return fail(MI355_EBADARG, "fr_nonzero_rows: null pointer");
  CHK(check_ptr_table(vecs_dev, batch, n * sizeof(fe_t), "fr_nonzero_rows", "vector"));
  const uint32_t nblocks = (uint32_t)ceil_div(n, CHECK_TILE);
  WsLayout L;
  const uint64_t off_vecs = L.take((uint64_t)batch * 8), off_tot = L.take((uint64_t)batch * 8), off_rows = L.take((uint64_t)batch * cap * 8), off_cnt = L.take((uint64_t)batch * nblocks * 4),
                 off_pre = L.take((uint64_t)batch * nblocks * 4);
  PoolBlock ws; CHK(ws.alloc(L.total(), slot));
  hipStream_t s = g.stream;
  CHK(ws.upload(off_vecs, vecs_dev, (uint64_t)batch * 8));
  const fe_t *const *vecs = (const fe_t *const *)ws.at(off_vecs); unsigned long long *tot = (unsigned long long *)ws.at(off_tot); uint64_t *rows = (uint64_t *)ws.at(off_rows);
  uint32_t *cnt = (uint32_t *)ws.at(off_cnt), *pre = (uint32_t *)ws.at(off_pre);
  HIPCHK(hipMemsetAsync(tot, 0, (uint64_t)batch * 8, s));
  if (cap) HIPCHK(hipMemsetAsync(rows, 0xff, (uint64_t)batch * cap * 8, s));
  {
    Scope sc("nonzero_rows");
    for (uint32_t v0 = 0; v0 < batch; v0 += 65535) {   // blockIdx.y = vector
      const uint32_t nv = std::min<uint32_t>(65535, batch - v0); const uint64_t o = (uint64_t)v0 * nblocks;
      hipLaunchKernelGGL(k_fr_nonzero_rows<0>, dim3(nblocks, nv), dim3(CHECK_THREADS), 0, s, vecs + v0, n, cap, cnt + o, (const uint32_t *)(pre + o), rows + (uint64_t)v0 * cap);
      hipLaunchKernelGGL(k_check_scan, dim3(nv), dim3(CHECK_THREADS), 0, s, (const uint32_t *)(cnt + o), pre + o, nblocks, tot + v0);
      if (cap) hipLaunchKernelGGL(k_fr_nonzero_rows<1>, dim3(nblocks, nv), dim3(CHECK_THREADS), 0, s, vecs + v0, n, cap, cnt + o, (const uint32_t *)(pre + o), rows + (uint64_t)v0 * cap);
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(counts_out_host, tot, (uint64_t)batch * 8, hipMemcpyDeviceToHost, s));
  if (cap) HIPCHK(hipMemcpyAsync(rows_out_host, rows, (uint64_t)batch * cap * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return finish_async();
  });
}
int mi355_fr_copy_check_dev(const void *const *cols_dev, uint32_t n_cols, uint32_t log_n, const uint64_t *cells_host, const uint64_t *images_host, uint64_t count, uint32_t cap,
                            uint64_t *n_failed_out, uint64_t *failed_t_out_host) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot(cols_dev, n_cols, true, &slot, "fr_copy_check"));
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (n_cols == 0) return fail(MI355_EBADARG, "fr_copy_check: n_cols must not be zero");
  if (log_n > PERM_MAX_LOG_N) return fail(MI355_EBADARG, "fr_copy_check: log_n > 28");
  if (cap > CHECK_MAX_CAP) return fail(MI355_EBADARG, "fr_copy_check: cap " + std::to_string(cap) + " exceeds " + std::to_string(CHECK_MAX_CAP));
  if (!cols_dev || !n_failed_out || (cap && !failed_t_out_host) || (count && (!cells_host || !images_host))) return fail(MI355_EBADARG, "fr_copy_check: null pointer");
  const uint64_t n = 1ull << log_n, total = (uint64_t)n_cols * n;
  CHK(check_ptr_table(cols_dev, n_cols, n * sizeof(fe_t), "fr_copy_check", "column"));
  // a cell >= n_cols * n would be a load outside the columns: the range check of perm_check (the bijection is not this call's business: any list of pairs may be compared)
  { uint64_t bad = 0; std::string why; if (perm_check(cells_host, images_host, count, total, PERM_FLAG_TRUSTED, &bad, &why)) return fail(MI355_EBADARG, "fr_copy_check: pair " + std::to_string(bad) + ": " + why); }
  const uint64_t stage = std::min(count, CHECK_STAGE); const uint32_t max_blocks = (uint32_t)ceil_div(stage, CHECK_TILE);
  WsLayout L;
  const uint64_t off_cols = L.take((uint64_t)n_cols * 8), off_tot = L.take(8), off_failed = L.take((uint64_t)cap * 8), off_cnt = L.take((uint64_t)max_blocks * 4), off_pre = L.take((uint64_t)max_blocks * 4),
                 off_cells = L.take(stage * 8), off_images = L.take(stage * 8);
  PoolBlock ws; CHK(ws.alloc(L.total(), slot));
  hipStream_t s = g.stream;
  CHK(ws.upload(off_cols, cols_dev, (uint64_t)n_cols * 8));
  const fe_t *const *cols = (const fe_t *const *)ws.at(off_cols); unsigned long long *tot = (unsigned long long *)ws.at(off_tot); uint64_t *failed = (uint64_t *)ws.at(off_failed);
  uint32_t *cnt = (uint32_t *)ws.at(off_cnt), *pre = (uint32_t *)ws.at(off_pre);
  const uint64_t *cells = (const uint64_t *)ws.at(off_cells), *images = (const uint64_t *)ws.at(off_images);
  HIPCHK(hipMemsetAsync(tot, 0, 8, s));
  if (cap) HIPCHK(hipMemsetAsync(failed, 0xff, (uint64_t)cap * 8, s));
  for (uint64_t lo = 0; lo < count; lo += stage) {   // an upload into the staging area waits for the kernels that read the previous piece (mi355_buf_upload into a block in use)
    const uint64_t len = std::min(stage, count - lo); const uint32_t nblocks = (uint32_t)ceil_div(len, CHECK_TILE);
    CHK(ws.upload(off_cells, cells_host + lo, len * 8)); CHK(ws.upload(off_images, images_host + lo, len * 8));
    Scope sc("copy_check");
    hipLaunchKernelGGL(k_fr_copy_check<0>, dim3(nblocks), dim3(CHECK_THREADS), 0, s, cols, log_n, cells, images, len, lo, cap, cnt, (const uint32_t *)pre, failed);
    hipLaunchKernelGGL(k_check_scan, dim3(1), dim3(CHECK_THREADS), 0, s, (const uint32_t *)cnt, pre, nblocks, tot);
    if (cap) hipLaunchKernelGGL(k_fr_copy_check<1>, dim3(nblocks), dim3(CHECK_THREADS), 0, s, cols, log_n, cells, images, len, lo, cap, cnt, (const uint32_t *)pre, failed);
    sc.close();
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(n_failed_out, tot, 8, hipMemcpyDeviceToHost, s));
  if (cap) HIPCHK(hipMemcpyAsync(failed_t_out_host, failed, (uint64_t)cap * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return finish_async();
  });
}

// ---- the prover's randomness (frrand.hpp): ChaCha20 blocks reduced to Fr.  Asynchronous on the library stream of the device that owns the destination.  The key is a
// kernel argument and nothing else: it is never copied into an error text, a trace line or a range name.  A draw whose block counters would wrap 2^64 is refused before
// the device is looked at: a (key, stream) pair must never repeat a block.  Grid: grid-stride over at most 8 workgroups per CU; MI355_FR_RANDOM_BLOCKS overrides the
// workgroup count (tests make every lane loop; the result must not depend on it).
static frrand_key_t frrand_key(const uint8_t *key32) { frrand_key_t k; memcpy(k.w, key32, 32); return k; }   // little-endian host: bytes -> words
int mi355_fr_random_dev(void *dst, uint64_t n, const uint8_t *key32, uint64_t stream, uint64_t counter0) {
  return guarded([&]() -> int {
  if (counter0 + n < counter0) return fail(MI355_EBADARG, "fr_random: counter0 + n wraps 2^64 (a stream must never repeat a block)");
  int slot; CHK(common_slot({dst}, &slot, "fr_random")); DevGuard lk(slot);
  CHK(need_init(slot));
  if (n == 0) return MI355_OK;
  if (!dst || !key32) return fail(MI355_EBADARG, "fr_random: null pointer");
  if (n >= (1ull << 40)) return fail(MI355_EBADARG, "fr_random: n too large");
  if ((uintptr_t)dst & 15) return fail(MI355_EBADARG, "fr_random: device pointers must be 16-byte aligned");
  CHK(buf_check_range(dst, n * sizeof(fe_t), "fr_random"));
  Scope sc("fr_random");
  hipLaunchKernelGGL(k_fr_random, dim3(grid_blocks(n, FRRAND_THREADS, 8, "MI355_FR_RANDOM_BLOCKS")), dim3(FRRAND_THREADS), 0, g.stream, (fe_t *)dst, n, frrand_key(key32), stream, counter0);
  sc.close();
  HIPCHK(hipGetLastError());
  return finish_async();
  });
}
int mi355_fr_random_rows_dev(void *const *cols, uint32_t n_cols, uint64_t row0, uint32_t rows, const uint8_t *key32, uint64_t stream, uint64_t counter0) {
  return guarded([&]() -> int {
  const uint64_t total = (uint64_t)n_cols * rows;
  if (counter0 + total < counter0) return fail(MI355_EBADARG, "fr_random_rows: counter0 + n_cols * rows wraps 2^64 (a stream must never repeat a block)");
  // the columns are looked up WITHOUT marking their blocks as in use: a witness upload into the other rows of a column (create_proof: rows [0, u + 1) cross the link while
  // rows [u + 1, n) are drawn) then keeps its fresh-block ordering instead of waiting for everything queued on the compute stream.  Disjoint rows need no order; calls
  // queued afterwards on the compute stream see both.
  int slot; CHK(common_slot(cols, n_cols, false, &slot, "fr_random_rows"));
  DevGuard lk(slot);
  CHK(need_init(slot));
  if (total == 0) return MI355_OK;
  if (!cols || !key32) return fail(MI355_EBADARG, "fr_random_rows: null pointer");
  if (row0 >= (1ull << 40)) return fail(MI355_EBADARG, "fr_random_rows: row0 too large");
  CHK(check_ptr_table(cols, n_cols, (row0 + rows) * sizeof(fe_t), "fr_random_rows", "column"));
  PoolBlock ws; CHK(ws.alloc(stage_class((uint64_t)n_cols * 8), slot));
  CHK(ws.upload(0, cols, (uint64_t)n_cols * 8));
  Scope sc("fr_random");
  hipLaunchKernelGGL(k_fr_random_rows, dim3(grid_blocks(total, FRRAND_THREADS, 8, "MI355_FR_RANDOM_BLOCKS")), dim3(FRRAND_THREADS), 0, g.stream, (fe_t *const *)ws.p, n_cols, row0, rows, frrand_key(key32), stream, counter0);
  sc.close();
  HIPCHK(hipGetLastError());
  return finish_async();   // the block goes back to the pool here; its reuse waits for the kernel queued above
  });
}
// Fr::from_uniform_bytes over an array: src 64-byte little-endian integers, dst their residues mod r as Montgomery words
int mi355_fr_from_u512_dev(void *dst, const void *src, uint64_t n) {
  return guarded([&]() -> int {
  int slot; CHK(common_slot({dst, src}, &slot, "fr_from_u512")); DevGuard lk(slot);
  CHK(need_init(slot));
  if (n == 0) return MI355_OK;
  if (!dst || !src) return fail(MI355_EBADARG, "fr_from_u512: null pointer");
  if (n >= (1ull << 40)) return fail(MI355_EBADARG, "fr_from_u512: n too large");
  if (((uintptr_t)dst | (uintptr_t)src) & 15) return fail(MI355_EBADARG, "fr_from_u512: device pointers must be 16-byte aligned");
  if (ranges_overlap(src, n * 64, dst, n * sizeof(fe_t))) return fail(MI355_EBADARG, "fr_from_u512: input and output must not overlap");
  CHK(buf_check_range(dst, n * sizeof(fe_t), "fr_from_u512"));
  Scope sc("fr_from_u512");
  hipLaunchKernelGGL(k_fr_from_u512, dim3(grid_blocks(n, FRRAND_THREADS, 8, "MI355_FR_RANDOM_BLOCKS")), dim3(FRRAND_THREADS), 0, g.stream, (fe_t *)dst, (const uint4 *)src, n);
  sc.close();
  HIPCHK(hipGetLastError());
  return finish_async();
  });
}

// ---- many Poseidon transcripts in one launch (poseidon.hpp: one lane per job).  The argument checks read host memory only and come before the device is asked for; the
// constants are the library's own (generated and checked once per process, uploaded once per device slot); one staging block, one launch, one download.
int mi355_poseidon_transcripts_host(const void *words_host, const uint64_t *word_offsets_host, const uint32_t *squeeze_at_host, const uint64_t *squeeze_offsets_host,
                                    uint32_t jobs, void *challenges_out_host) {
  return guarded([&]() -> int {
  if (jobs > (1u << 20)) return fail(MI355_EBADARG, "poseidon_transcripts: more than 2^20 jobs");
  uint64_t n_words = 0, n_sq = 0;
  if (jobs) {
    if (!word_offsets_host || !squeeze_offsets_host) return fail(MI355_EBADARG, "poseidon_transcripts: null pointer");
    if (word_offsets_host[0] != 0) return fail(MI355_EBADARG, "poseidon_transcripts: word_offsets[0] must be 0");
    if (squeeze_offsets_host[0] != 0) return fail(MI355_EBADARG, "poseidon_transcripts: squeeze_offsets[0] must be 0");
    for (uint32_t j = 0; j < jobs; j++) {
      if (word_offsets_host[j + 1] < word_offsets_host[j]) return fail(MI355_EBADARG, "poseidon_transcripts: word_offsets decrease at job " + std::to_string(j));
      if (squeeze_offsets_host[j + 1] < squeeze_offsets_host[j]) return fail(MI355_EBADARG, "poseidon_transcripts: squeeze_offsets decrease at job " + std::to_string(j));
    }
    n_words = word_offsets_host[jobs]; n_sq = squeeze_offsets_host[jobs];
    if (n_words > (1ull << 24)) return fail(MI355_EBADARG, "poseidon_transcripts: more than 2^24 words");
    if (n_sq > (1ull << 24)) return fail(MI355_EBADARG, "poseidon_transcripts: more than 2^24 squeezes");
    if ((n_words && !words_host) || (n_sq && (!squeeze_at_host || !challenges_out_host))) return fail(MI355_EBADARG, "poseidon_transcripts: null pointer");
    for (uint32_t j = 0; j < jobs; j++) {
      const uint64_t len = word_offsets_host[j + 1] - word_offsets_host[j]; uint32_t prev = 0;
      for (uint64_t q = squeeze_offsets_host[j]; q < squeeze_offsets_host[j + 1]; q++) {
        const uint32_t p = squeeze_at_host[q];
        if (p < prev) return fail(MI355_EBADARG, "poseidon_transcripts: squeeze positions decrease in job " + std::to_string(j) + " (squeeze " + std::to_string(q - squeeze_offsets_host[j]) + ")");
        if (p > len) return fail(MI355_EBADARG, "poseidon_transcripts: squeeze position " + std::to_string(p) + " exceeds the " + std::to_string(len) + " words of job " + std::to_string(j));
        prev = p;
      }
    }
    uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = FrP::mod(i);
    for (uint64_t i = 0; i < n_words; i++) if (Fr::w_geq(((const fe_t *)words_host)[i].l, m)) return fail(MI355_EBADARG, "poseidon_transcripts: word " + std::to_string(i) + " is not below r");
  }
  MsmGuard lk;
  CHK(need_init());
  if (jobs == 0 || n_sq == 0) return MI355_OK;   // nothing to squeeze: nothing is launched, nothing is written
  CallTrace tr("poseidon_transcripts", n_words, 32.0);
  hipStream_t s = g.stream;
  bool fresh; { const auto it = g.ws.find("poseidon.tables"); fresh = it == g.ws.end() || !it->second.p; }   // shutdown clears the arena: the next call uploads again
  fe_t *tab; CHK(ws_get("poseidon.tables", (size_t)POS_TABLE_WORDS * sizeof(fe_t), (void **)&tab));
  if (fresh) {
    const std::vector<fe_t> &t = poseidon_tables();
    const hipError_t e = hipMemcpyAsync(tab, t.data(), t.size() * sizeof(fe_t), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { g.ws.erase("poseidon.tables"); dev_free(tab); HIPCHK(e); }
  }
  WsLayout L;
  const uint64_t off_words = L.take(n_words * sizeof(fe_t)), off_woff = L.take(((uint64_t)jobs + 1) * 8), off_soff = L.take(((uint64_t)jobs + 1) * 8), off_sq = L.take(n_sq * 4),
                 off_out = L.take(n_sq * sizeof(fe_t));
  char *dev; CHK(ws_get("io.poseidon", L.total(), (void **)&dev));
  if (n_words) HIPCHK(hipMemcpyAsync(dev + off_words, words_host, n_words * sizeof(fe_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dev + off_woff, word_offsets_host, ((size_t)jobs + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dev + off_soff, squeeze_offsets_host, ((size_t)jobs + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dev + off_sq, squeeze_at_host, n_sq * 4, hipMemcpyHostToDevice, s));
  {
    Scope sp("poseidon_transcripts", s);
    hipLaunchKernelGGL(k_poseidon_transcripts, dim3(ceil_div(jobs, POS_LANES)), dim3(POS_LANES), 0, s, (const fe_t *)tab, (const fe_t *)(dev + off_words), (const uint64_t *)(dev + off_woff),
                       (const uint32_t *)(dev + off_sq), (const uint64_t *)(dev + off_soff), jobs, (fe_t *)(dev + off_out));
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(challenges_out_host, dev + off_out, n_sq * sizeof(fe_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  resolve_spans();
  { char buf[64]; snprintf(buf, sizeof buf, " jobs=%u squeezes=%llu", jobs, (unsigned long long)n_sq); tr.done(buf); }
  return MI355_OK;
  });
}

// ---- one straight-line Fr program for many jobs (frprog.hpp: one lane per job).  The argument checks (frprog_check) read host memory only and come before the device is asked
// for.  Workspace: ONE pooled mi355_buf block (PoolBlock; WsLayout) -- the program, the constants, the inputs, the register file ((n_regs - n_consts) x jobs rounded up to 64
// words), the output register list, the outputs and the flag words -- back in the pool on every return.  One launch, two downloads, synchronous.
int mi355_fr_program_host(const uint32_t *code_host, uint32_t n_instr, uint32_t n_regs, const void *consts_host, uint32_t n_consts, const void *inputs_host, uint32_t n_inputs,
                          uint32_t jobs, const uint32_t *out_regs_host, uint32_t n_outputs, void *outputs_host, uint32_t *flags_out_host) {
  return guarded([&]() -> int {
  { std::string why;
    if (!frprog_check(code_host, n_instr, n_regs, consts_host, n_consts, inputs_host, n_inputs, jobs, out_regs_host, n_outputs, outputs_host, flags_out_host, why)) return fail(MI355_EBADARG, "fr_program: " + why); }
  const int slot = pick_replica_slot(); DevGuard lk(slot);
  CHK(need_init(slot));
  if (jobs == 0) return MI355_OK;   // nothing is launched, nothing is written
  CallTrace tr("fr_program", (uint64_t)jobs * n_instr, 32.0);
  const uint64_t stride = frprog_stride(jobs);
  WsLayout L;
  const uint64_t off_code = L.take((uint64_t)n_instr * 16), off_consts = L.take((uint64_t)n_consts * sizeof(fe_t)), off_in = L.take((uint64_t)jobs * n_inputs * sizeof(fe_t)),
                 off_regs = L.take((uint64_t)(n_regs - n_consts) * stride * sizeof(fe_t)), off_oregs = L.take((uint64_t)n_outputs * 4),
                 off_out = L.take((uint64_t)jobs * n_outputs * sizeof(fe_t)), off_flags = L.take((uint64_t)jobs * 4);
  PoolBlock ws; CHK(ws.alloc(L.total(), slot));
  hipStream_t s = g.stream;
  if (n_instr) HIPCHK(hipMemcpyAsync(ws.at(off_code), code_host, (size_t)n_instr * 16, hipMemcpyHostToDevice, s));
  if (n_consts) HIPCHK(hipMemcpyAsync(ws.at(off_consts), consts_host, (size_t)n_consts * sizeof(fe_t), hipMemcpyHostToDevice, s));
  if (n_inputs) HIPCHK(hipMemcpyAsync(ws.at(off_in), inputs_host, (size_t)jobs * n_inputs * sizeof(fe_t), hipMemcpyHostToDevice, s));
  if (n_outputs) HIPCHK(hipMemcpyAsync(ws.at(off_oregs), out_regs_host, (size_t)n_outputs * 4, hipMemcpyHostToDevice, s));
  {
    Scope sp("fr_program", s);
    hipLaunchKernelGGL(k_fr_program, dim3(ceil_div(jobs, FRP_LANES)), dim3(FRP_LANES), 0, s, (const uint32_t *)ws.at(off_code), n_instr, (const fe_t *)ws.at(off_consts), n_consts,
                       (const fe_t *)ws.at(off_in), n_inputs, jobs, (fe_t *)ws.at(off_regs), stride, (const uint32_t *)ws.at(off_oregs), n_outputs, (fe_t *)ws.at(off_out),
                       (uint32_t *)ws.at(off_flags));
  }
  HIPCHK(hipGetLastError());
  if (n_outputs) HIPCHK(hipMemcpyAsync(outputs_host, ws.at(off_out), (size_t)jobs * n_outputs * sizeof(fe_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(flags_out_host, ws.at(off_flags), (size_t)jobs * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  resolve_spans();
  { char buf[64]; snprintf(buf, sizeof buf, " jobs=%u instructions=%u registers=%u", jobs, n_instr, n_regs); tr.done(buf); }
  return MI355_OK;
  });
}

}  // extern "C"
