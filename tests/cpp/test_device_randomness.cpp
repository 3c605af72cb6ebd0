// test_device_randomness.cpp -- a COMPILED caller of create_proof (include/mi355zk_plonk.hpp) that proves one layer with the prover's randomness drawn on the device
// (ProofOptions::device_randomness: ChaCha20 blocks reduced to Fr, the stream table of mi355zk_plonk.hpp) and writes what a CPU restatement needs to redo the proof.
//
// One layer: synthetic SRS, the builder's circuit instance (as tests/cpp/test_plonk_replay.cpp builds it), keygen; the instance is dumped; create_proof by the default
// route (the builder's randomness, uploaded); then the witness's random fields are EMPTIED -- random_poly, m_blind, z_blind, phi_blind gone, the blinding rows of every
// advice and multiplicity column zeroed: the device route must not read them -- and create_proof runs with device_randomness under the given key.  tests/ recompute every
// drawn value from the key (tests/frrand_common.py), put them into the dumped inputs and hold oracle/plonk.py's proof to these bytes.
//
//   --protocol FILE           a PlonkProtocol JSON (scroll-prover_amd/protocols.py or tests/golden/)
//   --out DIR                 the dump_circuit files, proof.bin (device randomness, --key), proof_again.bin (the same key once more), proof_off.bin (default route),
//                             proof_key2.bin (--key2), proof_os1.bin / proof_os2.bin (--os-key: rng_key_from_os, twice), vk.bin, instances.bin, result.json
//   --key HEX / --key2 HEX    64 hex digits: the 32 key bytes in order
//   --device-multiplicities   both routes count the multiplicities on the device; for the device-randomness proofs the m columns are emptied as well
//   --sparse-uploads, --check-witness, --upload-threads U, --devices D (MI355_ALLOW_DUP_DEVICES=1: one device bound D times), --proofs N (timed repeats of both routes)
//   --builder-key             the builder assigns its gates against the advice blinding rows the device will draw under --key (CircuitOptions::device_rng_key: layer 0)
// Prints one JSON line; exit code 0 = the proofs were written, 1 = they were not, 2 = no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "mi355zk_plonk.hpp"

using namespace mi355zk::plonk;
using Clock = std::chrono::steady_clock;
static void write_file(const std::string &path, const void *p, size_t bytes) { std::ofstream f(path, std::ios::binary); if (!f) throw std::invalid_argument("cannot write " + path); f.write(static_cast<const char *>(p), (std::streamsize)bytes); }
static bool parse_key(const std::string &hex, uint8_t out[32]) {
  if (hex.size() != 64) return false;
  for (int i = 0; i < 32; i++) { char *end = nullptr; const std::string b = hex.substr(2 * i, 2); out[i] = (uint8_t)std::strtoul(b.c_str(), &end, 16); if (*end) return false; }
  return true;
}
static std::string steps_json(const ProofResult &R) {
  char b[640];
  std::snprintf(b, sizeof b, "{\"total_ms\": %.2f, \"random_ms\": %.3f, \"witness_link_bytes\": %llu, \"2_3_advice_lookup_commits\": %.2f, \"4_products\": %.2f, \"5_random\": %.2f, \"6_to_coeff\": %.2f, \"7_quotient\": %.2f}",
                R.total_ms, R.random_ms, (unsigned long long)R.witness_link_bytes, R.step_ms[2], R.step_ms[4], R.step_ms[5], R.step_ms[6], R.step_ms[7]);
  return b;
}

int main(int argc, char **argv) {
  std::string protocol_path, out_dir, key_hex, key2_hex;
  int devices = 1, threads = 8, upload_threads = 1, proofs = 1; bool dev_m = false, sparse = false, check_w = false, os_key = false, builder_key = false; uint64_t seed = 1;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto nexts = [&]() -> std::string { return i + 1 < argc ? std::string(argv[++i]) : std::string(); };
    if (a == "--protocol") protocol_path = nexts(); else if (a == "--out") out_dir = nexts(); else if (a == "--key") key_hex = nexts(); else if (a == "--key2") key2_hex = nexts();
    else if (a == "--devices") devices = std::atoi(nexts().c_str()); else if (a == "--threads") threads = std::atoi(nexts().c_str()); else if (a == "--upload-threads") upload_threads = std::atoi(nexts().c_str());
    else if (a == "--proofs") proofs = std::atoi(nexts().c_str()); else if (a == "--seed") seed = (uint64_t)std::atoll(nexts().c_str());
    else if (a == "--device-multiplicities") dev_m = true; else if (a == "--sparse-uploads") sparse = true; else if (a == "--check-witness") check_w = true; else if (a == "--os-key") os_key = true;
    else if (a == "--builder-key") builder_key = true;
    else { std::printf("usage: %s --protocol FILE --out DIR --key HEX64 [--key2 HEX64] [--os-key] [--device-multiplicities] [--sparse-uploads] [--check-witness] [--builder-key] [--devices D] [--threads T] [--upload-threads U] [--proofs N] [--seed S]\n", argv[0]); return 1; }
  }
  uint8_t key[32], key2[32];
  if (protocol_path.empty() || out_dir.empty() || !parse_key(key_hex, key) || (!key2_hex.empty() && !parse_key(key2_hex, key2))) { std::printf("--protocol, --out and --key (64 hex digits) are required\n"); return 1; }
  threads = std::max(1, std::min(16, threads)); devices = std::max(1, devices); proofs = std::max(1, proofs);
  Protocol P;
  try { P.load(protocol_path); } catch (const std::exception &e) { std::printf("cannot load the protocol: %s\n", e.what()); return 1; }
  const uint32_t k = P.k, Q = P.Q; const uint64_t n = P.n, u = P.usable;
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
    CircuitOptions co; co.seed = seed; co.threads = threads; if (builder_key) co.device_rng_key = key;
    auto C = build_circuit(P, co);
    dump_circuit(*C, out_dir, tau, protocol_path);
    auto pk = keygen(P, *C, hl, resident, devices);
    for (auto &c : C->pre) { Column().swap(c); }
    std::vector<Fr>().swap(C->omega_pow);
    check(mi355_buf_trim());
    ProofOptions off; off.devices = devices; off.threads = threads; off.upload_threads = upload_threads; off.packed_multiplicities = true; off.transcript = transcript;   // test_plonk_replay.cpp's defaults
    off.device_multiplicities = dev_m; off.sparse_uploads = sparse;
    ProofResult A;
    for (int it = 0; it < proofs; it++) A = create_proof(hg, hl, *pk, *C, off);
    // ---- the randomness leaves the witness
    Column().swap(C->random_poly); C->m_blind.clear(); C->z_blind.clear(); C->phi_blind.clear();
    for (auto &c : C->advice) for (uint64_t r = u + 1; r < n; r++) c[r] = fr_zero();
    for (auto &c : C->m) for (uint64_t r = u + 1; r < n; r++) c[r] = fr_zero();
    if (dev_m) { for (auto &c : C->m) Column().swap(c); C->m_counts.clear(); }
    ProofOptions on = off; on.device_randomness = true; on.check_witness = check_w; std::memcpy(on.rng_key, key, 32);
    ProofResult B;
    for (int it = 0; it < proofs; it++) B = create_proof(hg, hl, *pk, *C, on);
    const ProofResult B2 = create_proof(hg, hl, *pk, *C, on);
    write_file(out_dir + "/proof.bin", B.proof.data(), B.proof.size());
    write_file(out_dir + "/proof_again.bin", B2.proof.data(), B2.proof.size());
    write_file(out_dir + "/proof_off.bin", A.proof.data(), A.proof.size());
    if (!key2_hex.empty()) { ProofOptions o2 = on; std::memcpy(o2.rng_key, key2, 32); const ProofResult K = create_proof(hg, hl, *pk, *C, o2); write_file(out_dir + "/proof_key2.bin", K.proof.data(), K.proof.size()); }
    if (os_key) {
      ProofOptions o3 = on; o3.rng_key_from_os = true;
      const ProofResult O1 = create_proof(hg, hl, *pk, *C, o3), O2 = create_proof(hg, hl, *pk, *C, o3);
      write_file(out_dir + "/proof_os1.bin", O1.proof.data(), O1.proof.size()); write_file(out_dir + "/proof_os2.bin", O2.proof.data(), O2.proof.size());
    }
    write_file(out_dir + "/vk.bin", pk->vk.data(), pk->vk.size());
    write_file(out_dir + "/instances.bin", C->instances.data(), C->instances.size() * 32);
    char line[4096];
    std::snprintf(line, sizeof line,
      "{\"layer\": %d, \"k\": %u, \"devices\": %d, \"advice\": %u, \"lookups\": %zu, \"permutation_chunks\": %zu, \"blind\": %u, \"transcript\": \"%s\", \"pk_cosets\": \"%s\", \"device_multiplicities\": %s, \"sparse_uploads\": %s, "
      "\"check_witness\": %s, \"proofs\": %d, \"proof_bytes\": %zu, \"same_key_same_bytes\": %s, \"off\": %s, \"on\": %s, \"ok\": true}",
      P.layer, k, devices, P.num_advice(), P.lookups.size(), P.perm.size(), P.blind, transcript_name(transcript), resident ? "resident" : "on-the-fly", dev_m ? "true" : "false", sparse ? "true" : "false",
      check_w ? "true" : "false", proofs, B.proof.size(), B.proof == B2.proof ? "true" : "false", steps_json(A).c_str(), steps_json(B).c_str());
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
