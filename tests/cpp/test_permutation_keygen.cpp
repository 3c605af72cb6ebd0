// test_permutation_keygen.cpp -- a COMPILED caller of keygen (include/mi355zk_plonk.hpp) that checks the device route of the permutation's sigma columns
// (keygen(..., device_sigma = true): one mi355_fr_permutation_sigma_dev call from the copy mapping, Circuit::pairs fed through halo2::PermutationAssembly)
// against the default route, where Circuit::sigma_column builds every column on the host and uploads it.
//
// One layer in one process: synthetic SRS, the builder's circuit instance; keygen + create_proof by the default route, that key dropped, then keygen + create_proof
// by the device route on the same circuit.  Both the verifying keys and the proofs must be the same bytes.
//
//   --protocol FILE     a PlonkProtocol JSON (scroll-prover_amd/protocols.py or tests/golden/)
//   --out DIR           vk_host.bin, vk_device.bin, proof_host.bin, proof_device.bin, instances.bin and result.json
//   --keygen-only       no proofs: the two keys and the wall time of their sigma stages
//   --sigma-only COLS K PCT   no protocol: the sigma stage of the default route alone (Circuit::sigma_column + upload, column by column) for COLS permutation columns of
//                       2^K rows with PCT % of the cells in copy pairs -- the host figure tools/bench_permutation_sigma.py sets the device call against
// Prints one JSON line; exit code 0 = both routes ran, 1 = they did not, 2 = no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mi355zk_plonk.hpp"

using namespace mi355zk::plonk;
using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
static void write_file(const std::string &path, const void *p, size_t bytes) { std::ofstream f(path, std::ios::binary); if (!f) throw std::invalid_argument("cannot write " + path); f.write(static_cast<const char *>(p), (std::streamsize)bytes); }

// the default route's sigma stage on a synthetic permutation: what keygen does per sigma column, nothing else
static int sigma_only(uint32_t cols, uint32_t k, uint32_t pct, int threads) {
  { const int rc = mi355_init(0); if (rc != MI355_OK) { std::printf("mi355_init failed (%d): %s\n", rc, mi355_last_error()); return 2; } }
  int rc_main = 1;
  try {
    const mi355zk::halo2::EvaluationDomain dom(2, k);
    Protocol P; P.k = k; P.n = uint64_t(1) << k; P.omega = dom.omega;
    const uint64_t n = P.n;
    Circuit C; C.pr = &P; C.threads = threads;
    const Fr delta = fr_pow(fr_u64(7), uint64_t(1) << 28);
    { Fr dp = fr_one(); for (uint32_t j = 0; j < cols; j++) { C.pcols.push_back({j, j, dp}); dp = fr_mul(dp, delta); } }
    C.omega_pow.resize(n); { Fr w = fr_one(); for (uint64_t i = 0; i < n; i++) { C.omega_pow[i] = w; w = fr_mul(w, P.omega); } }
    // pairs (j, r) <-> (j + 1, r) over every second column, rows r with r % 100 < pct
    for (uint32_t j = 0; j + 1 < cols; j += 2) for (uint64_t r = 0; r < n; r++) if (r % 100 < pct) C.pairs.push_back({j, r, j + 1, r});
    DevicePoly lag(n, 0); std::vector<Fr> sig;
    C.sigma_column(0, sig); check(mi355_buf_upload(lag.p, sig.data(), n * 32)); check(mi355_synchronize());   // warm-up: page faults of `sig`, the first upload
    const auto t0 = Clock::now();
    for (uint32_t j = 0; j < cols; j++) { C.sigma_column(j, sig); check(mi355_buf_upload(lag.p, sig.data(), n * 32)); }
    check(mi355_synchronize());
    const double ms = ms_since(t0);
    std::printf("{\"sigma_only\": true, \"n_cols\": %u, \"k\": %u, \"density_pct\": %u, \"copy_pairs\": %zu, \"threads\": %d, \"host_sigma_ms\": %.3f, \"ok\": true}\n", cols, k, pct, C.pairs.size(), threads, ms);
    rc_main = 0;
  } catch (const std::exception &e) { std::printf("FAILED with exception: %s\n", e.what()); rc_main = 1; }
  (void)mi355_shutdown();
  std::fflush(stdout);
  return rc_main;
}

int main(int argc, char **argv) {
  std::string protocol_path, out_dir;
  int threads = 8; uint64_t seed = 1; bool keygen_only = false;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto nexts = [&]() -> std::string { return i + 1 < argc ? std::string(argv[++i]) : std::string(); };
    if (a == "--protocol") protocol_path = nexts(); else if (a == "--out") out_dir = nexts(); else if (a == "--threads") threads = std::atoi(nexts().c_str());
    else if (a == "--seed") seed = (uint64_t)std::atoll(nexts().c_str()); else if (a == "--keygen-only") keygen_only = true;
    else if (a == "--sigma-only" && i + 3 < argc) { const uint32_t c = (uint32_t)std::atoi(argv[i + 1]), kk = (uint32_t)std::atoi(argv[i + 2]), pc = (uint32_t)std::atoi(argv[i + 3]); if (c == 0 || kk > 28 || pc > 100) { std::printf("--sigma-only COLS K PCT\n"); return 1; } return sigma_only(c, kk, pc, std::max(1, std::min(16, threads))); }
    else { std::printf("usage: %s --protocol FILE --out DIR [--keygen-only] [--threads T] [--seed S] | [--threads T] --sigma-only COLS K PCT\n", argv[0]); return 1; }
  }
  if (protocol_path.empty() || out_dir.empty()) { std::printf("--protocol and --out are required\n"); return 1; }
  threads = std::max(1, std::min(16, threads));
  Protocol P;
  try { P.load(protocol_path); } catch (const std::exception &e) { std::printf("cannot load the protocol: %s\n", e.what()); return 1; }
  const uint32_t k = P.k, Q = P.Q; const uint64_t n = P.n;
  const TranscriptKind transcript = reference_transcript(P);
  const Fr tau = fr_u64(0x5343524F4C4C0001ull + (uint64_t)(P.layer < 0 ? 0 : P.layer));   // the key test_plonk_replay.cpp uses: the tests verify with the same tau
  { const int rc = mi355_init(0); if (rc != MI355_OK) { std::printf("mi355_init failed (%d): %s\n", rc, mi355_last_error()); return 2; } }
  int rc_main = 1;
  try {
    const mi355zk::halo2::EvaluationDomain dom(Q + 1, k);
    uint64_t hg = 0, hl = 0;
    {
      DevicePoly g(2 * n, 0), gl(2 * n, 0);
      check(mi355_srs_setup_dev(g.p, gl.p, k, tau.data(), dom.omega.data()));
      check(mi355_srs_register_dev(g.p, n, 1, &hg)); check(mi355_srs_register_dev(gl.p, n, 1, &hl));
      check(mi355_synchronize());
    }
    check(mi355_buf_trim());
    uint64_t hbm_free = 0; check(mi355_mem_info(0, &hbm_free, nullptr, nullptr, nullptr, nullptr));
    const PkSizes sz = pk_sizes(P);
    const bool resident = sz.base_bytes + sz.coset_bytes + sz.working_bytes <= 0.94 * (double)hbm_free;   // test_plonk_replay.cpp's `--pk-cosets auto`
    CircuitOptions co; co.seed = seed; co.threads = threads;
    auto C = build_circuit(P, co);
    ProofOptions opt; opt.threads = threads; opt.packed_multiplicities = true; opt.transcript = transcript;   // test_plonk_replay.cpp's defaults
    std::vector<uint8_t> vk[2], proof[2]; double sigma_ms[2] = {0, 0}, keygen_ms[2] = {0, 0}, prep_ms = 0;
    for (int route = 0; route < 2; route++) {   // 0: host, 1: device
      const auto t0 = Clock::now();
      auto pk = keygen(P, *C, hl, resident, 1, route == 1);
      keygen_ms[route] = ms_since(t0); sigma_ms[route] = pk->sigma_ms; if (route == 1) prep_ms = pk->sigma_host_prep_ms;
      vk[route] = pk->vk;
      if (!keygen_only) proof[route] = create_proof(hg, hl, *pk, *C, opt).proof;
      pk.reset();
      check(mi355_buf_trim());
    }
    const char *names[2] = {"host", "device"};
    for (int route = 0; route < 2; route++) {
      write_file(out_dir + "/vk_" + names[route] + ".bin", vk[route].data(), vk[route].size());
      if (!keygen_only) write_file(out_dir + "/proof_" + names[route] + ".bin", proof[route].data(), proof[route].size());
    }
    write_file(out_dir + "/instances.bin", C->instances.data(), C->instances.size() * 32);
    char line[2048];
    std::snprintf(line, sizeof line,
      "{\"layer\": %d, \"k\": %u, \"perm_columns\": %zu, \"copy_pairs\": %zu, \"transcript\": \"%s\", \"pk_cosets\": \"%s\", \"keygen_only\": %s, \"vk_equal\": %s, \"proof_equal\": %s, "
      "\"proof_bytes\": %zu, \"sigma_ms\": {\"host\": %.3f, \"device\": %.3f, \"device_host_prep\": %.3f}, \"keygen_ms\": {\"host\": %.2f, \"device\": %.2f}, \"ok\": true}",
      P.layer, k, C->pcols.size(), C->pairs.size(), transcript_name(transcript), resident ? "resident" : "on-the-fly", keygen_only ? "true" : "false",
      vk[0] == vk[1] ? "true" : "false", proof[0] == proof[1] ? "true" : "false", proof[1].size(), sigma_ms[0], sigma_ms[1], prep_ms, keygen_ms[0], keygen_ms[1]);
    std::printf("%s\n", line);
    write_file(out_dir + "/result.json", line, std::strlen(line));
    rc_main = 0;
    check(mi355_srs_release(hg)); check(mi355_srs_release(hl));
  } catch (const std::exception &e) { std::printf("FAILED with exception: %s\n", e.what()); rc_main = 1; }
  (void)mi355_shutdown();
  std::fflush(stdout);
  return rc_main;
}
