// test_lookup_multiplicities.cpp -- a COMPILED caller of create_proof (include/mi355zk_plonk.hpp) that checks the device route of the lookup multiplicities
// (ProofOptions::device_multiplicities: step 3 counts m on the device after theta, as the scroll fork's mv_lookup prover does on the CPU) against the default route,
// where the caller hands in the m columns the circuit builder counted.
//
// One layer: synthetic SRS, the builder's circuit instance, keygen; then create_proof by the default route, then -- on the same witness with its m columns EMPTIED
// (the device route must not read them) -- by the device route.  With the first-occurrence rule both routes must give the same bytes (the builder gives the counts of
// the all-zero tuple to table row 0, which is where the first rule puts them).
//
//   --protocol FILE     a PlonkProtocol JSON (scroll-prover_amd/protocols.py or tests/golden/)
//   --out DIR           proof.bin (device route), proof_default.bin, vk.bin, instances.bin -- the layout oracle/plonk.py reads -- and result.json
//   --rule first|last   the duplicate rule of the device route (last: the proof differs from the default route's and must still verify)
//   --corrupt-lookup    one input cell of lookup 0 set to a value outside its table; the device route must refuse with the lookup and the row named, and emit no proof
//   --devices D         as tests/cpp/test_plonk_replay.cpp (MI355_ALLOW_DUP_DEVICES=1: one device bound D times)
// Prints one JSON line; exit code 0 = the run did what it was asked (proofs written, or the corrupt lookup refused), 1 = it did not, 2 = no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mi355zk_plonk.hpp"

using namespace mi355zk::plonk;
using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
static void write_file(const std::string &path, const void *p, size_t bytes) { std::ofstream f(path, std::ios::binary); if (!f) throw std::invalid_argument("cannot write " + path); f.write(static_cast<const char *>(p), (std::streamsize)bytes); }
static std::string steps_json(const ProofResult &R) {
  char b[512];
  std::snprintf(b, sizeof b, "{\"1_instance\": %.2f, \"2_3_advice_lookup_commits\": %.2f, \"4_products\": %.2f, \"5_random\": %.2f, \"6_to_coeff\": %.2f, \"7_quotient\": %.2f, \"8_commit_h\": %.2f, \"9_evals\": %.2f, \"10_shplonk\": %.2f}",
                R.step_ms[1], R.step_ms[2], R.step_ms[4], R.step_ms[5], R.step_ms[6], R.step_ms[7], R.step_ms[8], R.step_ms[9], R.step_ms[10]);
  return b;
}

int main(int argc, char **argv) {
  std::string protocol_path, out_dir, rule = "first";
  int devices = 1, threads = 8; bool corrupt_lookup = false; uint64_t seed = 1;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto nexts = [&]() -> std::string { return i + 1 < argc ? std::string(argv[++i]) : std::string(); };
    if (a == "--protocol") protocol_path = nexts(); else if (a == "--out") out_dir = nexts(); else if (a == "--rule") rule = nexts();
    else if (a == "--devices") devices = std::atoi(nexts().c_str()); else if (a == "--threads") threads = std::atoi(nexts().c_str());
    else if (a == "--seed") seed = (uint64_t)std::atoll(nexts().c_str()); else if (a == "--corrupt-lookup") corrupt_lookup = true;
    else { std::printf("usage: %s --protocol FILE --out DIR [--rule first|last] [--corrupt-lookup] [--devices D] [--threads T] [--seed S]\n", argv[0]); return 1; }
  }
  if (protocol_path.empty() || out_dir.empty() || (rule != "first" && rule != "last")) { std::printf("--protocol and --out are required; --rule is first or last\n"); return 1; }
  threads = std::max(1, std::min(16, threads)); devices = std::max(1, devices);
  Protocol P;
  try { P.load(protocol_path); } catch (const std::exception &e) { std::printf("cannot load the protocol: %s\n", e.what()); return 1; }
  if (P.lookups.empty()) { std::printf("the protocol has no lookup\n"); return 1; }
  const uint32_t k = P.k, Q = P.Q; const uint64_t n = P.n;
  const TranscriptKind transcript = reference_transcript(P);
  const Fr tau = fr_u64(0x5343524F4C4C0001ull + (uint64_t)(P.layer < 0 ? 0 : P.layer));   // the key test_plonk_replay.cpp uses: the tests verify with the same tau
  {
    std::vector<int> ids(devices); for (int d = 0; d < devices; d++) ids[d] = d;
    if (std::getenv("MI355_ALLOW_DUP_DEVICES")) for (auto &d : ids) d = 0;
    const int rc = devices == 1 ? mi355_init(0) : mi355_init_multi(ids.data(), devices);
    if (rc != MI355_OK) { std::printf("mi355_init failed (%d): %s\n", rc, mi355_last_error()); return 2; }
  }
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
    auto pk = keygen(P, *C, hl, resident, devices);
    for (auto &c : C->pre) { Column().swap(c); }
    std::vector<Fr>().swap(C->omega_pow);
    check(mi355_buf_trim());
    ProofOptions base; base.devices = devices; base.threads = threads; base.packed_multiplicities = true; base.transcript = transcript;   // test_plonk_replay.cpp's defaults
    ProofOptions dev = base; dev.device_multiplicities = true; dev.multiplicity_rule_last = rule == "last";
    char line[4096];
    if (corrupt_lookup) {
      // lookup 0 reads an advice column at rotation 0 (under a selector, which is on at row 1 for the builder's in-place lookups: block 0's middle input)
      std::vector<std::pair<int32_t, int32_t>> reads; collect_polys(*P.lookups[0].input, reads);
      int adv = -1; for (const auto &r : reads) if (!P.is_pre((uint32_t)r.first) && !P.is_instance((uint32_t)r.first) && r.second == 0) { adv = (int)((uint32_t)r.first - P.phase0[0]); break; }
      if (adv < 0) throw std::invalid_argument("lookup 0 reads no advice column at rotation 0");
      const uint64_t row = 1;
      C->advice[(size_t)adv][row] = fr_u64(0x8000000000000000ull + 12345);   // above every table of the builder (range tables of at most 2^26 rows, tuples i (j + 1))
      for (auto &c : C->m) Column().swap(c);
      C->m_counts.clear();
      std::string err; int code = 0; bool emitted = false;
      try { const ProofResult R = create_proof(hg, hl, *pk, *C, dev); emitted = !R.proof.empty(); }
      catch (const mi355zk::halo2::Error &e) { err = e.what(); code = e.code; }
      const std::string want = "lookup 0: input row " + std::to_string(row) + " is not in the table";
      const bool ok = !emitted && code == MI355_EBADARG && err.find(want) != std::string::npos;
      std::string esc; for (char c : err) { if (c == '"' || c == '\\') esc += '\\'; esc += c; }
      std::snprintf(line, sizeof line, "{\"layer\": %d, \"k\": %u, \"corrupt_lookup\": {\"lookup\": 0, \"row\": %llu, \"advice_column\": %d}, \"error_code\": %d, \"error\": \"%s\", \"proof_emitted\": %s, \"ok\": %s}",
                    P.layer, k, (unsigned long long)row, adv, code, esc.c_str(), emitted ? "true" : "false", ok ? "true" : "false");
      rc_main = ok ? 0 : 1;
    } else {
      const ProofResult A = create_proof(hg, hl, *pk, *C, base);
      for (auto &c : C->m) Column().swap(c);   // the device route reads m_blind only
      C->m_counts.clear();
      const ProofResult B = create_proof(hg, hl, *pk, *C, dev);
      write_file(out_dir + "/proof.bin", B.proof.data(), B.proof.size());
      write_file(out_dir + "/proof_default.bin", A.proof.data(), A.proof.size());
      write_file(out_dir + "/vk.bin", pk->vk.data(), pk->vk.size());
      write_file(out_dir + "/instances.bin", C->instances.data(), C->instances.size() * 32);
      uint64_t live = 0, pooled = 0, ws = 0; check(mi355_mem_info(0, nullptr, nullptr, &live, &pooled, &ws));
      const double GiB = 1024.0 * 1024 * 1024;
      std::snprintf(line, sizeof line,
        "{\"layer\": %d, \"k\": %u, \"devices\": %d, \"lookups\": %zu, \"rule\": \"%s\", \"transcript\": \"%s\", \"pk_cosets\": \"%s\", \"proof_bytes\": %zu, \"bytes_equal\": %s, "
        "\"default_ms\": %.2f, \"device_ms\": %.2f, \"multiplicity_ms\": %.3f, \"step_ms_default\": %s, \"step_ms_device\": %s, \"hbm\": {\"live_gib\": %.2f, \"pooled_gib\": %.2f, \"workspace_gib\": %.2f}, \"ok\": true}",
        P.layer, k, devices, P.lookups.size(), rule.c_str(), transcript_name(transcript), resident ? "resident" : "on-the-fly", B.proof.size(), A.proof == B.proof ? "true" : "false",
        A.total_ms, B.total_ms, B.multiplicity_ms, steps_json(A).c_str(), steps_json(B).c_str(), live / GiB, pooled / GiB, ws / GiB);
      rc_main = 0;
    }
    std::printf("%s\n", line);
    write_file(out_dir + "/result.json", line, std::strlen(line));
    pk.reset();
    check(mi355_srs_release(hg)); check(mi355_srs_release(hl));
  } catch (const std::exception &e) { std::printf("FAILED with exception: %s\n", e.what()); rc_main = 1; }
  (void)mi355_shutdown();
  std::fflush(stdout);
  return rc_main;
}
