// test_verify_proof.cpp -- the driver of plonk::verify_proof (include/mi355zk_plonk_verify.hpp): reads a protocol JSON, key material, instances and a proof from files and
// prints the VerifyResult as one JSON line (field elements and coordinates as canonical hexadecimal integers).  scroll-prover_amd/halo2.py verify_proof runs it as a process.
//   --protocol FILE  --proof FILE  --instances FILE (32-byte big-endian words)  --transcript blake2b|poseidon|evm (default: by the protocol's layer)
//   --vk FILE (.vkey bytes) | --preprocessed FILE (64-byte G1Affine records, Montgomery limbs) | neither: the protocol file's own commitments
//   --initial-state HEX (canonical integer)      --g2 FILE --neg-s-g2 FILE | --s-g2 FILE (128-byte G2Affine records; negated on the host)
//   --no-accumulator | --accumulator (force the check of the first twelve instances for a protocol that does not declare one)
//   --check-g2 PARAMS_FILE   instead of a proof: load a RawBytes params file and print {"check_g2": ParamsKZG::check_g2()}; --swap-g2 replaces s_g2 by g2 first
//   --host-only  stop after the (scalars, points) list: no device is touched (the points are decompressed on the host)
#include <cstdio>
#include <fstream>
#include <iterator>
#include "mi355zk_plonk.hpp"

using namespace mi355zk;
using namespace mi355zk::plonk;

static std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary); if (!f) throw std::invalid_argument("cannot open " + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::string hex_of(const zk::fe_t &canonical) { char b[65]; for (int i = 0; i < 8; i++) std::snprintf(b + 8 * i, 9, "%08x", canonical.l[7 - i]); return std::string(b, 64); }
static std::string fr_hex(const Fr &a) { return "\"" + hex_of(zk::Fr::to_canonical(halo2::detail::to_fe(a))) + "\""; }
static std::string pt_hex(const halo2::G1Affine &a) { zk::fe_t x, y; std::memcpy(&x, a.data(), 32); std::memcpy(&y, a.data() + 4, 32); return "[\"" + hex_of(zk::Fq::to_canonical(x)) + "\",\"" + hex_of(zk::Fq::to_canonical(y)) + "\"]"; }
static zk::fe_t be_word(const uint8_t *p) { zk::fe_t c; uint8_t *le = reinterpret_cast<uint8_t *>(&c); for (int i = 0; i < 32; i++) le[i] = p[31 - i]; return c; }
static Fr fr_from_be(const uint8_t *p) {   // any 256-bit word, reduced mod r (the transcript absorbs instance values mod r)
  zk::fe_t c = be_word(p); uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = zk::FrP::mod(i);
  while (zk::Fr::w_geq(c.l, m)) zk::Fr::w_sub(c.l, m);
  return halo2::detail::from_fe(zk::Fr::from_canonical(c));
}

int main(int argc, char **argv) {
  try {
    std::string protocol, proof_f, inst_f, vk_f, pre_f, g2_f, neg_f, sg2_f, state_hex, params_f; bool swap_g2 = false; VerifyOptions opt;
    for (int i = 1; i < argc; i++) {
      const std::string a = argv[i]; auto next = [&]() { if (i + 1 >= argc) throw std::invalid_argument(a + " needs a value"); return std::string(argv[++i]); };
      if (a == "--protocol") protocol = next(); else if (a == "--proof") proof_f = next(); else if (a == "--instances") inst_f = next(); else if (a == "--vk") vk_f = next();
      else if (a == "--preprocessed") pre_f = next(); else if (a == "--g2") g2_f = next(); else if (a == "--neg-s-g2") neg_f = next(); else if (a == "--s-g2") sg2_f = next();
      else if (a == "--initial-state") state_hex = next(); else if (a == "--transcript") opt.transcript = transcript_kind_from_name(next());
      else if (a == "--check-g2") params_f = next(); else if (a == "--swap-g2") swap_g2 = true;
      else if (a == "--no-accumulator") opt.check_accumulator = false; else if (a == "--accumulator") opt.accumulator = 1; else if (a == "--host-only") opt.host_only = true;
      else throw std::invalid_argument("unknown argument " + a);
    }
    if (!params_f.empty()) {
      halo2::init(0);
      auto params = halo2::ParamsKZG::read(params_f);
      if (swap_g2) params->s_g2 = params->g2;
      std::printf("{\"check_g2\":%s,\"k\":%u}\n", params->check_g2() ? "true" : "false", params->k);
      return 0;
    }
    if (protocol.empty() || proof_f.empty() || inst_f.empty()) throw std::invalid_argument("--protocol, --proof and --instances are required");
    Protocol P; P.load(protocol);
    VerifyingKeyRef vk;
    if (!vk_f.empty()) vk.vk_bytes = slurp(vk_f);
    if (!pre_f.empty()) { const auto b = slurp(pre_f); if (b.size() % 64) throw std::invalid_argument("--preprocessed: 64-byte records expected"); vk.preprocessed.resize(b.size() / 64); std::memcpy(vk.preprocessed.data(), b.data(), b.size()); }
    if (!state_hex.empty()) {
      if (state_hex.size() > 64) throw std::invalid_argument("--initial-state: at most 64 hexadecimal digits");
      const std::string h = std::string(64 - state_hex.size(), '0') + state_hex; uint8_t w[32];
      for (int i = 0; i < 32; i++) w[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
      vk.initial_state = fr_from_be(w); vk.has_initial_state = true;
    }
    const auto ib = slurp(inst_f); if (ib.size() % 32) throw std::invalid_argument("--instances: 32-byte words expected");
    std::vector<Fr> instances; for (size_t i = 0; i < ib.size(); i += 32) instances.push_back(fr_from_be(ib.data() + i));
    const auto proof = slurp(proof_f);
    G2Pair srs;
    auto g2rec = [&](const std::string &f) { const auto b = slurp(f); if (b.size() != 128) throw std::invalid_argument(f + ": one 128-byte G2Affine expected"); std::array<uint8_t, 128> r; std::memcpy(r.data(), b.data(), 128); return r; };
    if (!opt.host_only) {
      if (g2_f.empty() || (neg_f.empty() == sg2_f.empty())) throw std::invalid_argument("--g2 and one of --neg-s-g2 / --s-g2 are required");
      srs = neg_f.empty() ? G2Pair::from_params(g2rec(g2_f), g2rec(sg2_f)) : G2Pair::from_negated(g2rec(g2_f), g2rec(neg_f));
      halo2::init(0);
    }
    const VerifyResult r = verify_proof(P, vk, instances, proof, srs, opt);
    std::string o = "{\"ok\":" + std::string(r.ok ? "true" : "false") + ",\"error\":\"" + r.error + "\",\"detail\":\"" + r.detail + "\",\"host_only\":" + (opt.host_only ? "true" : "false");
    o += ",\"challenges\":{\"theta\":" + fr_hex(r.theta) + ",\"beta\":" + fr_hex(r.beta) + ",\"gamma\":" + fr_hex(r.gamma) + ",\"y\":" + fr_hex(r.y) + ",\"x\":" + fr_hex(r.x) +
         ",\"shplonk_y\":" + fr_hex(r.shplonk_y) + ",\"shplonk_v\":" + fr_hex(r.shplonk_v) + ",\"shplonk_u\":" + fr_hex(r.shplonk_u) + "}";
    o += ",\"numerator_at_x\":" + fr_hex(r.numerator_at_x) + ",\"msm\":{\"scalars\":[";
    for (size_t i = 0; i < r.msm_scalars.size(); i++) o += (i ? "," : "") + fr_hex(r.msm_scalars[i]);
    o += "],\"points\":[";
    for (size_t i = 0; i < r.msm_points.size(); i++) o += (i ? "," : "") + pt_hex(r.msm_points[i]);
    o += "],\"result\":" + pt_hex(r.msm_result) + ",\"w_prime\":" + pt_hex(r.w_prime) + "},\"has_accumulator\":" + (r.has_accumulator ? "true" : "false") + ",\"pairing\":[";
    for (size_t i = 0; i < r.pairing.size(); i++) o += (i ? "," : "") + std::to_string(r.pairing[i]);
    o += "]}";
    std::printf("%s\n", o.c_str());
    return 0;
  } catch (const std::exception &e) { std::fprintf(stderr, "test_verify_proof: %s\n", e.what()); return 2; }
}
