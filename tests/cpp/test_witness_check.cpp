// test_witness_check.cpp -- a COMPILED caller of plonk::check_witness (include/mi355zk_plonk.hpp): MockProver::verify for a PlonkProtocol on the device.
//
// One layer in one process: the builder's circuit instance, optionally with cells changed AFTER it was built (so that constraints no longer hold), dumped for the CPU
// yardstick (tests/witness_check_common.py), then -- on the device -- synthetic SRS, keygen, check_witness, and with --prove a create_proof under
// ProofOptions::check_witness.
//
//   --protocol FILE     a PlonkProtocol JSON (scroll-prover_amd/protocols.py or tests/golden/)
//   --out DIR           the dumped inputs (dump_circuit), check.json, and with --prove: prove.json, vk.bin, instances.bin, proof.bin, proof_plain.bin
//   --corrupt SPEC      advice:<col>:<row>[:<delta>] or instance:<i>[:<delta>]: adds delta (default 1) to that cell before the dump and keygen; may be repeated
//   --builder-only      only the dumped inputs; no device is touched
//   --no-dump           the inputs are not dumped (full-size runs: a layer-4 instance at k = 26 is tens of gigabytes on disk)
//   --prove             create_proof with check_witness = true: {"threw", "message", "proof_written"}; when it did not throw, the proof and the proof of the same
//                       run without the check (proof_plain.bin: the same bytes)
//   --cap N             failures reported per gate / for the copies (CheckOptions::cap); --seed S, --fill F, --threads T as the replay
// check.json: {"check_ms": .., "failures": [{"kind", "index", "row", "count", "col_a", "col_b", "row_b"}, ..]}.
// Prints one JSON line; exit code 0 = the check ran (whatever it found), 1 = it did not, 2 = no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mi355zk_plonk.hpp"

using namespace mi355zk::plonk;
using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
static void write_file(const std::string &path, const void *p, size_t bytes) { std::ofstream f(path, std::ios::binary); if (!f) throw std::invalid_argument("cannot write " + path); f.write(static_cast<const char *>(p), (std::streamsize)bytes); }
static std::string json_escape(const std::string &s) { std::string o; for (char c : s) { if (c == '"' || c == '\\') o.push_back('\\'); if ((unsigned char)c >= 32) o.push_back(c); } return o; }

struct Corruption { bool instance; uint64_t col, row, delta; };
static bool parse_spec(const std::string &spec, Corruption &c) {
  std::vector<std::string> f; size_t p = 0;
  for (;;) { const size_t q = spec.find(':', p); f.push_back(spec.substr(p, q == std::string::npos ? q : q - p)); if (q == std::string::npos) break; p = q + 1; }
  auto num = [](const std::string &s, uint64_t &v) { if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos) return false; v = std::strtoull(s.c_str(), nullptr, 10); return true; };
  c.delta = 1; c.col = 0;
  if (f[0] == "advice" && (f.size() == 3 || f.size() == 4)) { c.instance = false; return num(f[1], c.col) && num(f[2], c.row) && (f.size() == 3 || num(f[3], c.delta)); }
  if (f[0] == "instance" && (f.size() == 2 || f.size() == 3)) { c.instance = true; return num(f[1], c.row) && (f.size() == 2 || num(f[2], c.delta)); }
  return false;
}

int main(int argc, char **argv) {
  std::string protocol_path, out_dir;
  int threads = 8; uint64_t seed = 1; double fill = 0.9; bool builder_only = false, prove = false, no_dump = false; uint32_t cap = 16;
  std::vector<Corruption> corrupt;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto nexts = [&]() -> std::string { return i + 1 < argc ? std::string(argv[++i]) : std::string(); };
    if (a == "--protocol") protocol_path = nexts(); else if (a == "--out") out_dir = nexts(); else if (a == "--threads") threads = std::atoi(nexts().c_str());
    else if (a == "--seed") seed = (uint64_t)std::atoll(nexts().c_str()); else if (a == "--fill") fill = std::atof(nexts().c_str()); else if (a == "--cap") cap = (uint32_t)std::atoi(nexts().c_str());
    else if (a == "--builder-only") builder_only = true; else if (a == "--prove") prove = true; else if (a == "--no-dump") no_dump = true;
    else if (a == "--corrupt") { Corruption c; if (!parse_spec(nexts(), c)) { std::printf("--corrupt advice:<col>:<row>[:<delta>] | instance:<i>[:<delta>]\n"); return 1; } corrupt.push_back(c); }
    else { std::printf("usage: %s --protocol FILE --out DIR [--seed S] [--fill F] [--corrupt SPEC]... [--builder-only] [--no-dump] [--prove] [--cap N] [--threads T]\n", argv[0]); return 1; }
  }
  if (protocol_path.empty() || out_dir.empty()) { std::printf("--protocol and --out are required\n"); return 1; }
  threads = std::max(1, std::min(16, threads));
  Protocol P;
  try { P.load(protocol_path); } catch (const std::exception &e) { std::printf("cannot load the protocol: %s\n", e.what()); return 1; }
  const uint32_t k = P.k, Q = P.Q; const uint64_t n = P.n;
  const TranscriptKind transcript = reference_transcript(P);
  const Fr tau = fr_u64(0x5343524F4C4C0001ull + (uint64_t)(P.layer < 0 ? 0 : P.layer));   // the key test_plonk_replay.cpp uses: the tests verify with the same tau
  std::unique_ptr<Circuit> C;
  try {
    CircuitOptions co; co.seed = seed; co.threads = threads; co.fill = fill;
    C = build_circuit(P, co);
    for (const auto &c : corrupt) {
      if (c.instance) { if (c.row >= C->instances.size()) throw std::invalid_argument("--corrupt: instance " + std::to_string(c.row) + " does not exist"); C->instances[c.row] = fr_add(C->instances[c.row], fr_u64(c.delta)); }
      else { if (c.col >= C->advice.size() || c.row >= n) throw std::invalid_argument("--corrupt: advice cell outside the circuit"); C->advice[c.col][c.row] = fr_add(C->advice[c.col][c.row], fr_u64(c.delta)); }
    }
    if (!no_dump) dump_circuit(*C, out_dir, tau, protocol_path);
  } catch (const std::exception &e) { std::printf("FAILED with exception: %s\n", e.what()); return 1; }
  if (builder_only) { std::printf("{\"builder_only\": true, \"layer\": %d, \"k\": %u, \"copy_pairs\": %zu, \"corruptions\": %zu}\n", P.layer, k, C->pairs.size(), corrupt.size()); return 0; }
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
    // the check reads Lagrange values and coefficients only: the coset parts are kept for --prove, when they fit (test_plonk_replay.cpp's `--pk-cosets auto`)
    const bool resident = prove && sz.base_bytes + sz.coset_bytes + sz.working_bytes <= 0.94 * (double)hbm_free;
    auto pk = keygen(P, *C, hl, resident, 1);
    check(mi355_synchronize());
    CheckOptions ck; ck.threads = threads; ck.cap = cap;
    const auto t0 = Clock::now();
    const std::vector<VerifyFailure> bad = check_witness(*pk, *C, ck);
    const double check_ms = ms_since(t0);
    std::string js = "{\"check_ms\": " + std::to_string(check_ms) + ", \"failures\": [";
    for (size_t i = 0; i < bad.size(); i++) {
      const VerifyFailure &f = bad[i]; char buf[320];
      std::snprintf(buf, sizeof buf, "%s{\"kind\": \"%s\", \"index\": %u, \"row\": %llu, \"count\": %llu, \"col_a\": %u, \"col_b\": %u, \"row_b\": %llu}", i ? ", " : "", failure_kind_name(f.kind), f.index,
                    (unsigned long long)f.row, (unsigned long long)f.count, f.col_a, f.col_b, (unsigned long long)f.row_b);
      js += buf;
    }
    js += "]}\n";
    write_file(out_dir + "/check.json", js.data(), js.size());
    bool threw = false, proof_written = false, proofs_equal = false; std::string message; double proof_ms = 0;
    if (prove) {
      ProofOptions opt; opt.threads = threads; opt.packed_multiplicities = true; opt.transcript = transcript;   // test_plonk_replay.cpp's defaults
      write_file(out_dir + "/vk.bin", pk->vk.data(), pk->vk.size());
      write_file(out_dir + "/instances.bin", C->instances.data(), C->instances.size() * 32);
      try {
        opt.check_witness = true;
        const ProofResult R = create_proof(hg, hl, *pk, *C, opt);
        write_file(out_dir + "/proof.bin", R.proof.data(), R.proof.size()); proof_written = true;
        opt.check_witness = false;
        const ProofResult R0 = create_proof(hg, hl, *pk, *C, opt);
        write_file(out_dir + "/proof_plain.bin", R0.proof.data(), R0.proof.size());
        proofs_equal = R.proof == R0.proof; proof_ms = R0.total_ms;
      } catch (const WitnessError &e) { threw = true; message = e.what(); }
      const std::string pj = std::string("{\"threw\": ") + (threw ? "true" : "false") + ", \"message\": \"" + json_escape(message) + "\", \"proof_written\": " + (proof_written ? "true" : "false") + "}\n";
      write_file(out_dir + "/prove.json", pj.data(), pj.size());
    }
    char line[1024];
    std::snprintf(line, sizeof line,
      "{\"layer\": %d, \"k\": %u, \"gates\": %zu, \"lookups\": %zu, \"perm_columns\": %zu, \"copy_pairs\": %zu, \"corruptions\": %zu, \"cap\": %u, \"failures\": %zu, \"check_ms\": %.3f, \"transcript\": \"%s\", "
      "\"pk_cosets\": \"%s\", \"prove\": %s, \"threw\": %s, \"proof_written\": %s, \"proofs_equal\": %s, \"proof_ms\": %.3f, \"ok\": true}",
      P.layer, k, P.gates.size(), P.lookups.size(), C->pcols.size(), C->pairs.size(), corrupt.size(), cap, bad.size(), check_ms, transcript_name(transcript),
      resident ? "resident" : "on-the-fly", prove ? "true" : "false", threw ? "true" : "false", proof_written ? "true" : "false", proofs_equal ? "true" : "false", proof_ms);
    std::printf("%s\n", line);
    write_file(out_dir + "/result.json", line, std::strlen(line));
    rc_main = 0;
    pk.reset();
    check(mi355_srs_release(hg)); check(mi355_srs_release(hl));
  } catch (const std::exception &e) { std::printf("FAILED with exception: %s\n", e.what()); rc_main = 1; }
  (void)mi355_shutdown();
  std::fflush(stdout);
  return rc_main;
}
