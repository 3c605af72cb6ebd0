// test_hbm_budget.cpp -- a COMPILED caller of the memory limit (mi355_mem_set_limit / _usage / _reset_peak, csrc/mem_budget.hpp) and of the quotient in coset groups
// (ProofOptions::coset_group_polys, include/mi355zk_plonk.hpp): ONE process proves the same instance of a layer's PlonkProtocol by the ungrouped and by the grouped route and
// writes both proofs.  Set-up as test_plonk_replay.cpp: synthetic SRS with a known tau, the builder's circuit instance, keygen.  The reference runs create_proof once per layer
// in one prover process [REF integration/src/prove.rs:30-43,67,95-97]; what this program measures is what such a process must hold in HBM while it does.
//
//   --protocol FILE --out DIR      as test_plonk_replay
//   --group G | all                ProofOptions::coset_group_polys of the grouped route (default 24)
//   --pk-cosets resident|on-the-fly   the proving key keeps its coset parts, or is lean (default resident)
//   --devices D, --device-multiplicities, --threads T
//   --fit                          the limit between the two routes' peaks: both high-water marks are measured (mi355_mem_reset_peak and mi355_buf_trim between), the limit is
//                                  set midway; then the grouped proof must succeed below it, the ungrouped one must be refused with MI355_EOOM naming the limit, and a grouped
//                                  proof after that must still succeed
//   --bench N --groups a,b,..      no proof files: per entry of the list (0 = ungrouped, all, or G) one warm-up proof and N timed ones; medians per entry
// Writes proof_ungrouped.bin, proof_grouped.bin, vk.bin, instances.bin and prints one JSON line (also result.json); exit code 0 = the record was written, 2 = no GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mi355zk_plonk.hpp"

using namespace mi355zk::plonk;
namespace h2 = mi355zk::halo2;
static void write_file(const std::string &path, const void *p, size_t bytes) { std::ofstream f(path, std::ios::binary); if (!f) throw std::invalid_argument("cannot write " + path); f.write(static_cast<const char *>(p), (std::streamsize)bytes); }
static std::string json_escape(const std::string &s) { std::string o; for (char c : s) { if (c == '"' || c == '\\') o += '\\'; o += c == '\n' ? ' ' : c; } return o; }
static uint32_t parse_group(const std::string &s) { return s == "all" ? detail::COSET_GROUP_ALL : (uint32_t)std::atol(s.c_str()); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0 : v[v.size() / 2]; }

struct Run { ProofResult R; uint64_t peak = 0; };
// one proof between two trims, its high-water mark on slot 0 read from the ledger
static Run prove(uint64_t hg, uint64_t hl, const ProvingKey &pk, const Circuit &C, const ProofOptions &opt) {
  h2::check(mi355_buf_trim()); h2::mem_reset_peak(0);
  Run r; r.R = create_proof(hg, hl, pk, C, opt);
  r.peak = h2::mem_usage(0).high_water;
  return r;
}
static std::string run_json(const Run &r) {
  char b[512];
  std::snprintf(b, sizeof b, "{\"coset_ntt\": %u, \"coset_groups\": %u, \"coset_retransforms\": %u, \"gate_launches\": %u, \"high_water\": %llu, \"step7_ms\": %.3f, \"total_ms\": %.3f, \"proof_bytes\": %zu}",
                r.R.coset_ntt, r.R.coset_groups, r.R.coset_retransforms, r.R.gate_launches, (unsigned long long)r.peak, r.R.step_ms[7], r.R.total_ms, r.R.proof.size());
  return b;
}

int main(int argc, char **argv) {
  std::string protocol_path, out_dir, pk_mode = "resident", groups_list = "0";
  int devices = 1, threads = 8, bench = 0; uint32_t G = 24; bool dev_m = false, fit = false;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto nexts = [&]() -> std::string { return i + 1 < argc ? std::string(argv[++i]) : std::string(); };
    if (a == "--protocol") protocol_path = nexts(); else if (a == "--out") out_dir = nexts(); else if (a == "--devices") devices = std::atoi(nexts().c_str()); else if (a == "--threads") threads = std::atoi(nexts().c_str());
    else if (a == "--group") G = parse_group(nexts()); else if (a == "--pk-cosets") pk_mode = nexts(); else if (a == "--device-multiplicities") dev_m = true; else if (a == "--fit") fit = true;
    else if (a == "--bench") bench = std::atoi(nexts().c_str()); else if (a == "--groups") groups_list = nexts();
    else { std::printf("usage: %s --protocol FILE --out DIR [--group G|all] [--pk-cosets resident|on-the-fly] [--devices D] [--device-multiplicities] [--threads T] [--fit] [--bench N --groups 0,all,64,24]\n", argv[0]); return 1; }
  }
  if (protocol_path.empty() || out_dir.empty()) { std::printf("--protocol and --out are required\n"); return 1; }
  threads = std::max(1, std::min(16, threads));
  Protocol P;
  try { P.load(protocol_path); } catch (const std::exception &e) { std::printf("cannot load the protocol: %s\n", e.what()); return 1; }
  const uint32_t k = P.k, Q = P.Q; const uint64_t n = P.n;
  const Fr tau = fr_u64(0x5343524F4C4C0001ull + (uint64_t)(P.layer < 0 ? 0 : P.layer));
  {
    std::vector<int> ids(devices); for (int d = 0; d < devices; d++) ids[d] = d;
    if (std::getenv("MI355_ALLOW_DUP_DEVICES")) for (auto &d : ids) d = 0;
    const int rc = devices == 1 ? mi355_init(0) : mi355_init_multi(ids.data(), devices);
    if (rc != MI355_OK) { std::printf("mi355_init failed (%d): %s\n", rc, mi355_last_error()); return 2; }
  }
  int rc_main = 0;
  try {
    const h2::EvaluationDomain dom(Q + 1, k);
    uint64_t hg = 0, hl = 0;
    {
      DevicePoly g(2 * n, 0), gl(2 * n, 0);   // 64 bytes per point
      check(mi355_srs_setup_dev(g.p, gl.p, k, tau.data(), dom.omega.data()));
      check(mi355_srs_register_dev(g.p, n, 1, &hg)); check(mi355_srs_register_dev(gl.p, n, 1, &hl));
      check(mi355_synchronize());
    }
    CircuitOptions co; co.seed = 1; co.threads = threads;
    auto C = build_circuit(P, co);
    const bool resident = pk_mode != "on-the-fly";
    auto pk = keygen(P, *C, hl, resident, devices);
    for (auto &c : C->pre) { Column().swap(c); }
    ProofOptions plain; plain.devices = devices; plain.threads = threads; plain.device_multiplicities = dev_m; plain.transcript = reference_transcript(P);
    ProofOptions grouped = plain; grouped.coset_group_polys = G;
    std::string line;
    if (bench > 0) {
      line = "{\"bench\": true, \"layer\": " + std::to_string(P.layer) + ", \"k\": " + std::to_string(k) + ", \"pk_cosets\": \"" + (resident ? "resident" : "on-the-fly") + "\", \"proofs\": " + std::to_string(bench) + ", \"runs\": [";
      size_t at = 0; bool firstg = true;
      while (at <= groups_list.size()) {
        const size_t c = groups_list.find(',', at); const std::string tok = groups_list.substr(at, c == std::string::npos ? std::string::npos : c - at); at = c == std::string::npos ? groups_list.size() + 1 : c + 1;
        if (tok.empty()) continue;
        ProofOptions o = plain; o.coset_group_polys = parse_group(tok);
        Run last = prove(hg, hl, *pk, *C, o);   // warm-up: grows the workspace and the pool
        std::vector<double> s7, tot; uint64_t peak = 0;
        for (int it = 0; it < bench; it++) { last = prove(hg, hl, *pk, *C, o); s7.push_back(last.R.step_ms[7]); tot.push_back(last.R.total_ms); peak = std::max(peak, last.peak); }
        char b[512]; std::snprintf(b, sizeof b, "%s{\"group\": \"%s\", \"coset_groups\": %u, \"coset_ntt\": %u, \"coset_retransforms\": %u, \"high_water\": %llu, \"step7_ms_median\": %.3f, \"step7_ms_min\": %.3f, \"step7_ms_max\": %.3f, \"total_ms_median\": %.3f, \"total_ms_min\": %.3f, \"total_ms_max\": %.3f}",
                                    firstg ? "" : ", ", tok.c_str(), last.R.coset_groups, last.R.coset_ntt, last.R.coset_retransforms, (unsigned long long)peak, median(s7), *std::min_element(s7.begin(), s7.end()), *std::max_element(s7.begin(), s7.end()), median(tot), *std::min_element(tot.begin(), tot.end()), *std::max_element(tot.begin(), tot.end()));
        line += b; firstg = false;
      }
      line += "], \"ok\": true}";
    } else {
      const Run a = prove(hg, hl, *pk, *C, plain);
      const Run b = prove(hg, hl, *pk, *C, grouped);
      write_file(out_dir + "/proof_ungrouped.bin", a.R.proof.data(), a.R.proof.size());
      write_file(out_dir + "/proof_grouped.bin", b.R.proof.data(), b.R.proof.size());
      write_file(out_dir + "/vk.bin", pk->vk.data(), pk->vk.size());
      write_file(out_dir + "/instances.bin", C->instances.data(), C->instances.size() * 32);
      line = "{\"layer\": " + std::to_string(P.layer) + ", \"k\": " + std::to_string(k) + ", \"devices\": " + std::to_string(devices) + ", \"pk_cosets\": \"" + (resident ? "resident" : "on-the-fly") + "\", \"group\": " + std::to_string(G) +
             ", \"transcript\": \"" + transcript_name(plain.transcript) + "\", \"ungrouped\": " + run_json(a) + ", \"grouped\": " + run_json(b) + ", \"equal\": " + (a.R.proof == b.R.proof ? "true" : "false");
      if (fit) {
        // the limit midway between the two peaks; held now (keys, SRS, workspace) is below both
        const uint64_t limit = b.peak + (a.peak - std::min(a.peak, b.peak)) / 2;
        h2::check(mi355_buf_trim()); h2::mem_set_limit(0, limit);
        std::string g1_err, u_err, g2_err; int u_code = 0; Run g1, g2; uint64_t refused0 = h2::mem_usage(0).refused;
        try { g1 = prove(hg, hl, *pk, *C, grouped); } catch (const std::exception &e) { g1_err = e.what(); }
        try { (void)prove(hg, hl, *pk, *C, plain); } catch (const h2::Error &e) { u_err = e.what(); u_code = e.code; } catch (const std::exception &e) { u_err = e.what(); u_code = -1; }
        try { g2 = prove(hg, hl, *pk, *C, grouped); } catch (const std::exception &e) { g2_err = e.what(); }
        const h2::MemUsage u = h2::mem_usage(0);
        h2::mem_set_limit(0, 0);
        line += ", \"fit\": {\"limit\": " + std::to_string(limit) + ", \"grouped_ok\": " + (g1_err.empty() ? "true" : "false") + ", \"grouped_equal\": " + (g1.R.proof == a.R.proof ? "true" : "false") + ", \"grouped_high_water\": " + std::to_string(g1.peak) +
                ", \"grouped_error\": \"" + json_escape(g1_err) + "\", \"ungrouped_code\": " + std::to_string(u_code) + ", \"ungrouped_error\": \"" + json_escape(u_err) + "\", \"refused_grew\": " + (u.refused > refused0 ? "true" : "false") +
                ", \"grouped_again_ok\": " + (g2_err.empty() ? "true" : "false") + ", \"grouped_again_equal\": " + (g2.R.proof == a.R.proof ? "true" : "false") + ", \"grouped_again_error\": \"" + json_escape(g2_err) + "\", \"held_after\": " + std::to_string(u.held) + "}";
      }
      const h2::MemUsage u = h2::mem_usage(0);
      line += ", \"usage\": {\"held\": " + std::to_string(u.held) + ", \"buffers\": " + std::to_string(u.buffers()) + ", \"workspace\": " + std::to_string(u.workspace()) + ", \"ntt_required\": " + std::to_string(u.ntt_required()) + ", \"ntt_optional\": " + std::to_string(u.ntt_optional()) +
              ", \"srs\": " + std::to_string(u.srs()) + ", \"reclaims\": " + std::to_string(u.reclaims) + ", \"refused\": " + std::to_string(u.refused) + "}, \"ok\": true}";
    }
    std::printf("%s\n", line.c_str());
    write_file(out_dir + "/result.json", line.data(), line.size());
    pk.reset();
    check(mi355_srs_release(hg)); check(mi355_srs_release(hl));
  } catch (const std::exception &e) { std::printf("FAILED with exception: %s\n", e.what()); rc_main = 1; }
  (void)mi355_shutdown();
  std::fflush(stdout);
  return rc_main;
}
