// scalar_side_main.cpp -- the scalar-side compiler of include/mi355zk_plonk_scalar.hpp on the CPU: for a protocol, the program compile_scalar_program records is interpreted
// by the code the kernel runs (csrc/frprog.hpp frprog_run_host) and held, word for word, to the same walk over Fr itself (scalar_side<FrArith>, what every host verification
// runs).  No device is used.  tests/test_scalar_side_on_host.py builds and runs it.
//   --protocol FILE [--jobs N]   N random input sets (challenges, evaluations, instances: any words below r) for the protocol; then the crafted ones: x = omega^0 (flag bit 1,
//                                x_in_domain), u = x omega^rot for a rotation outside the first set (flag bit 2, shplonk_degenerate), x = 0 (bit 0 alone: no failure on the
//                                host), each also through vdetail::host_finish, whose VerifyResult must equal the host's field for field
//   --manifest FILE              the proofs of a verify_proofs manifest (protocol, proof, instances, transcript, preprocessed, initial_state): the inputs are what
//                                vdetail::host_part hands over for each proof (points decoded on the host), grouped by protocol as plonk::verify_proofs groups them
// Every program must hold exactly one INV, at most 2^16 registers, and pass frprog_check.  Prints one line per program and "all passed", or the first FAIL.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <random>
#include "mi355zk_plonk.hpp"

using namespace mi355zk;
using namespace mi355zk::plonk;

static int fails = 0;
static void expect(bool ok, const std::string &what) { if (!ok) { std::printf("FAIL %s\n", what.c_str()); fails++; } }
static std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary); if (!f) throw std::invalid_argument("cannot open " + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static Fr fr_from_be(const uint8_t *p) {
  zk::fe_t c; uint8_t *le = reinterpret_cast<uint8_t *>(&c); for (int i = 0; i < 32; i++) le[i] = p[31 - i];
  uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = zk::FrP::mod(i);
  while (zk::Fr::w_geq(c.l, m)) zk::Fr::w_sub(c.l, m);
  return halo2::detail::from_fe(zk::Fr::from_canonical(c));
}

// the program over `jobs` input sets, through the argument checks and the interpreter in the kernel's layout
static bool run_program(const sdetail::ScalarProgram &prog, const std::vector<Fr> &inputs, uint32_t jobs, std::vector<Fr> &out, std::vector<uint32_t> &flags, const std::string &what) {
  out.assign((size_t)jobs * prog.out_regs.size(), Fr{}); flags.assign(jobs, 0xdeadbeefu);
  std::string why;
  const bool ok = zk::frprog_check(prog.code.data(), prog.n_instr, prog.n_regs, prog.consts.data(), (uint32_t)prog.consts.size(), inputs.data(), prog.n_inputs, jobs, prog.out_regs.data(),
                                   (uint32_t)prog.out_regs.size(), out.data(), flags.data(), why);
  expect(ok, what + ": frprog_check refuses the compiled program: " + why);
  if (!ok) return false;
  zk::frprog_run_host(prog.code.data(), prog.n_instr, prog.n_regs, (const zk::fe_t *)prog.consts.data(), (uint32_t)prog.consts.size(), (const zk::fe_t *)inputs.data(), prog.n_inputs, jobs,
                      prog.out_regs.data(), (uint32_t)prog.out_regs.size(), (zk::fe_t *)out.data(), flags.data());
  return true;
}
static bool same_result(const VerifyResult &a, const VerifyResult &b) {
  return a.ok == b.ok && a.error == b.error && a.detail == b.detail && a.numerator_at_x == b.numerator_at_x && a.msm_scalars == b.msm_scalars && a.msm_points == b.msm_points &&
         a.has_accumulator == b.has_accumulator && a.acc_lhs == b.acc_lhs && a.acc_rhs == b.acc_rhs;
}
static void describe(const Protocol &P, size_t n_inst, const sdetail::ScalarProgram &prog, size_t jobs) {
  std::printf("{\"layer\":%d,\"k\":%u,\"instances\":%zu,\"jobs\":%zu,\"instructions\":%u,\"registers\":%u,\"constants\":%zu,\"inputs\":%u,\"outputs\":%zu,\"inversions\":%u}\n", P.layer, P.k, n_inst, jobs,
              prog.n_instr, prog.n_regs, prog.consts.size(), prog.n_inputs, prog.out_regs.size(), prog.n_inv);
}
static bool sound(const sdetail::ScalarProgram &prog, const std::string &what) {
  expect(prog.usable, what + ": no program: " + (prog.why.name ? std::string(prog.why.name) + ": " + prog.why.detail : std::string()));
  if (!prog.usable) return false;
  expect(prog.n_inv == 1, what + ": " + std::to_string(prog.n_inv) + " INV instructions, one expected");
  uint32_t inv = 0; for (uint32_t i = 0; i < prog.n_instr; i++) inv += prog.code[4 * i] == zk::FRP_INV;
  expect(inv == 1, what + ": the code holds " + std::to_string(inv) + " INV instructions");
  expect(prog.n_regs <= (1u << 16) && prog.n_instr <= (1u << 20), what + ": the program exceeds the caps");
  expect(prog.n_inputs == sdetail::N_CHALLENGE_INPUTS + prog.n_evals + prog.n_instances && prog.out_regs.size() == 1 + prog.sources.size(), what + ": input / output counts");
  return true;
}
// a job's outputs and flag word against the host walk over the same inputs, and host_finish against the host's VerifyResult
static void hold_to_host(const Protocol &P, const sdetail::ScalarProgram &prog, const vdetail::ScalarWork &work, size_t n_inst, const Fr *out, uint32_t flags, uint32_t want_flags, const char *want_error,
                         const std::string &what) {
  VerifyResult host; const bool ok = vdetail::scalar_side_on_host(P, n_inst, work, host);
  expect(flags == want_flags, what + ": flag word " + std::to_string(flags) + ", expected " + std::to_string(want_flags));
  expect(host.error == want_error && ok == (want_error[0] == 0), what + ": the host says '" + host.error + "', expected '" + want_error + "'");
  if (ok) {
    expect(flags != 0 || out[0] == host.numerator_at_x, what + ": numerator_at_x differs");
    expect(flags != 0 || (host.msm_scalars.size() == prog.sources.size() && std::equal(host.msm_scalars.begin(), host.msm_scalars.end(), out + 1)), what + ": an msm scalar differs");
  }
  VerifyOptions opt; opt.check_accumulator = false;
  std::vector<Fr> instances(work.inputs.end() - (ptrdiff_t)n_inst, work.inputs.end());
  VerifyResult fin; const bool fin_ok = vdetail::host_finish(P, instances, opt, prog, work, out, flags, fin);
  if (ok) host.ok = false;   // neither path sets ok: that is the pairing's word
  expect(fin_ok == ok && same_result(fin, host), what + ": host_finish gives '" + fin.error + "' / another record than the host ('" + host.error + "')");
}

static std::mt19937_64 rng(0x5ca1a5);
static Fr random_fr() { Fr a; for (auto &w : a) w = rng(); a[3] &= 0x0fffffffffffffffull; return a; }   // below 2^252 < r: any such word is a Montgomery word of some element

static void random_and_crafted(const Protocol &P, uint32_t jobs) {
  const size_t n_inst = P.num_instance.at(0);
  const std::string what = "layer " + std::to_string(P.layer);
  const sdetail::ScalarProgram prog = sdetail::compile_scalar_program(P, n_inst);
  if (!sound(prog, what)) return;
  describe(P, n_inst, prog, jobs);
  std::vector<vdetail::ScalarWork> work(jobs + 3);
  uint32_t n_wit = 0; for (auto w : P.num_witness) n_wit += w;
  for (auto &w : work) {
    for (uint32_t i = 0; i < prog.n_inputs; i++) w.inputs.push_back(random_fr());
    w.pieces.assign(P.Q, halo2::G1Affine{}); for (uint32_t p = 0; p < P.num_pre; p++) w.com[p] = halo2::G1Affine{}; for (uint32_t p = 0; p < n_wit; p++) w.com[P.wit0 + p] = halo2::G1Affine{};
    for (uint32_t j = 0; j < P.Q; j++) w.pieces[j][0] = 100 + j;   // the points are labels here: which one lands where is what is compared
    for (auto &kv : w.com) kv.second[0] = 1000 + kv.first;
    w.c_h[0] = 7; w.c_w[0] = 8;
  }
  // crafted: x = omega^0; u = x omega^rot, rot outside the first rotation set; x = 0
  const std::vector<RotationSet> sets = rotation_sets(P.queries);
  int32_t outside = 0; bool have_outside = false;
  for (const auto &s : sets) for (int32_t r : s.rots) if (!have_outside && std::find(sets[0].rots.begin(), sets[0].rots.end(), r) == sets[0].rots.end()) { outside = r; have_outside = true; }
  work[jobs].inputs[4] = fr_one();
  if (have_outside) work[jobs + 1].inputs[7] = fr_mul(work[jobs + 1].inputs[4], rot_power(P.omega, P.omega_inv, outside));
  work[jobs + 2].inputs[4] = fr_zero();
  std::vector<Fr> inputs; for (const auto &w : work) inputs.insert(inputs.end(), w.inputs.begin(), w.inputs.end());
  std::vector<Fr> out; std::vector<uint32_t> flags;
  if (!run_program(prog, inputs, jobs + 3, out, flags, what)) return;
  const size_t no = prog.out_regs.size();
  for (uint32_t j = 0; j < jobs; j++) hold_to_host(P, prog, work[j], n_inst, out.data() + j * no, flags[j], 0, "", what + " job " + std::to_string(j));
  const uint32_t b1 = 1u << sdetail::FLAG_BIT_X_IN_DOMAIN, b2 = 1u << sdetail::FLAG_BIT_DEGENERATE;
  expect((flags[jobs] & b1) != 0, what + ": x = omega^0 does not set the x_in_domain bit");
  hold_to_host(P, prog, work[jobs], n_inst, out.data() + jobs * no, flags[jobs], flags[jobs], "x_in_domain", what + " x = omega^0");
  if (have_outside) hold_to_host(P, prog, work[jobs + 1], n_inst, out.data() + (jobs + 1) * no, flags[jobs + 1], b2 | zk::FRP_FLAG_INV_OF_ZERO, "shplonk_degenerate", what + " u = x omega^" + std::to_string(outside));
  // (no rotation outside the first set: Z_T\S0 is the empty product and the failure cannot occur)
  bool shared_points = false; for (const auto &s : sets) shared_points = shared_points || s.rots.size() > 1;   // x = 0: the points of such a set coincide, a basis denominator is zero
  hold_to_host(P, prog, work[jobs + 2], n_inst, out.data() + (jobs + 2) * no, flags[jobs + 2], shared_points ? zk::FRP_FLAG_INV_OF_ZERO : 0u, "", what + " x = 0");
}

static void released(const std::string &manifest) {
  std::string text; { const auto b = slurp(manifest); text.assign(b.begin(), b.end()); }
  const json::Value M = json::Parser(text).parse();
  const auto &arr = M.at("proofs").arr;
  std::map<std::string, Protocol> protocols;
  for (const auto &e : arr) { const std::string p = e.at("protocol").s; if (!protocols.count(p)) protocols[p].load(p); }
  struct Group { sdetail::ScalarProgram prog; std::vector<size_t> members; };
  std::map<std::pair<const Protocol *, size_t>, Group> groups; std::vector<vdetail::ScalarWork> work(arr.size()); std::vector<std::vector<Fr>> insts(arr.size());
  for (size_t i = 0; i < arr.size(); i++) {
    const json::Value &e = arr[i]; const Protocol &P = protocols.at(e.at("protocol").s); VerifyingKeyRef vk; VerifyOptions opt;
    auto str = [&](const char *k) { const json::Value *v = e.find(k); return v && v->type == json::Value::STR ? v->s : std::string(); };
    if (!str("preprocessed").empty()) { const auto b = slurp(str("preprocessed")); vk.preprocessed.resize(b.size() / 64); std::memcpy(vk.preprocessed.data(), b.data(), b.size()); }
    if (!str("initial_state").empty()) { const std::string h = std::string(64 - str("initial_state").size(), '0') + str("initial_state"); uint8_t w[32]; for (int k = 0; k < 32; k++) w[k] = (uint8_t)std::stoul(h.substr(2 * k, 2), nullptr, 16); vk.initial_state = fr_from_be(w); vk.has_initial_state = true; }
    const auto ib = slurp(e.at("instances").s); for (size_t k = 0; k < ib.size(); k += 32) insts[i].push_back(fr_from_be(ib.data() + k));
    const auto proof = slurp(e.at("proof").s);
    if (!str("transcript").empty()) opt.transcript = transcript_kind_from_name(str("transcript"));
    VerifyResult res; vdetail::Layout L; std::vector<halo2::G1Affine> decoded;
    const std::string what = "proof " + std::to_string(i);
    if (!vdetail::layout_of(P, vk, proof, opt, L, res)) { expect(false, what + ": " + res.error); continue; }
    vdetail::decode_words(L.words, decoded, true);
    if (!vdetail::host_part(P, vk, insts[i], proof, opt, L, decoded.data(), res, nullptr, vdetail::HostPass::Whole, &work[i])) { expect(false, what + ": " + res.error + ": " + res.detail); continue; }
    Group &g = groups[{&P, insts[i].size()}];
    if (g.members.empty()) g.prog = sdetail::compile_scalar_program(P, insts[i].size());
    g.members.push_back(i);
  }
  for (auto &kv : groups) {
    const Protocol &P = *kv.first.first; const Group &g = kv.second; const std::string what = "released, layer " + std::to_string(P.layer);
    if (!sound(g.prog, what)) continue;
    describe(P, kv.first.second, g.prog, g.members.size());
    std::vector<Fr> inputs, out; std::vector<uint32_t> flags;
    for (size_t i : g.members) inputs.insert(inputs.end(), work[i].inputs.begin(), work[i].inputs.end());
    if (!run_program(g.prog, inputs, (uint32_t)g.members.size(), out, flags, what)) continue;
    for (size_t j = 0; j < g.members.size(); j++)
      hold_to_host(P, g.prog, work[g.members[j]], kv.first.second, out.data() + j * g.prog.out_regs.size(), flags[j], 0, "", what + ", proof " + std::to_string(g.members[j]));
  }
  std::printf("{\"released\":%zu,\"programs\":%zu}\n", arr.size(), groups.size());
}

int main(int argc, char **argv) {
  try {
    std::string manifest, protocol; uint32_t jobs = 3;
    for (int i = 1; i < argc; i++) {
      const std::string a = argv[i]; auto next = [&]() { if (i + 1 >= argc) throw std::invalid_argument(a + " needs a value"); return std::string(argv[++i]); };
      if (a == "--manifest") manifest = next(); else if (a == "--protocol") protocol = next(); else if (a == "--jobs") jobs = (uint32_t)std::stoul(next());
      else throw std::invalid_argument("unknown argument " + a);
    }
    if (manifest.empty() == protocol.empty()) throw std::invalid_argument("give --manifest or --protocol");
    if (!protocol.empty()) { Protocol P; P.load(protocol); random_and_crafted(P, jobs); } else released(manifest);
    if (fails) { std::printf("%d FAILED\n", fails); return 1; }
    std::printf("all passed\n");
    return 0;
  } catch (const std::exception &e) { std::fprintf(stderr, "scalar_side_main: %s\n", e.what()); return 2; }
}
