// frprog_main.cpp -- the interpreter of csrc/frprog.hpp (frprog_job: the code k_fr_program runs for one lane; frprog_run_host: the same call in the kernel's register layout;
// frprog_check: every argument check of mi355_fr_program_host) on the CPU, against a plain big-integer interpreter written here: canonical 256-bit integers, addition and
// subtraction with a conditional correction, products by double-and-add, inverses by Fermat.  Nothing of the field layer under test is used by the reference.
// A stand-alone program: tests/test_fr_program_on_host.py builds it with -fsanitize=address,undefined and runs it.  Prints "all passed" or the first FAIL.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../scroll-prover_amd/csrc/frprog.hpp"

using namespace zk;

struct U { uint64_t w[4]; };
static const U R_MOD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
static bool geq(const U &a, const U &b) { for (int i = 3; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i]; return true; }
static bool is0(const U &a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) == 0; }
static bool same(const U &a, const U &b) { return !std::memcmp(&a, &b, 32); }
static uint64_t add_raw(U &a, const U &b) { unsigned __int128 c = 0; for (int i = 0; i < 4; i++) { c += (unsigned __int128)a.w[i] + b.w[i]; a.w[i] = (uint64_t)c; c >>= 64; } return (uint64_t)c; }
static void sub_raw(U &a, const U &b) { uint64_t br = 0; for (int i = 0; i < 4; i++) { const unsigned __int128 t = (unsigned __int128)a.w[i] - b.w[i] - br; a.w[i] = (uint64_t)t; br = (uint64_t)(t >> 64) & 1; } }
static U addm(U a, const U &b) { const uint64_t c = add_raw(a, b); if (c || geq(a, R_MOD)) sub_raw(a, R_MOD); return a; }   // r < 2^254: no carry for reduced operands
static U subm(U a, const U &b) { if (geq(a, b)) { sub_raw(a, b); return a; } U t = R_MOD; sub_raw(t, b); add_raw(a, t); return a; }
static U mulm(const U &a, const U &b) { U acc = {{0, 0, 0, 0}}; for (int i = 255; i >= 0; i--) { acc = addm(acc, acc); if ((b.w[i >> 6] >> (i & 63)) & 1) acc = addm(acc, a); } return acc; }
static U powm(const U &a, const U &e) { U acc = {{1, 0, 0, 0}}; for (int i = 255; i >= 0; i--) { acc = mulm(acc, acc); if ((e.w[i >> 6] >> (i & 63)) & 1) acc = mulm(acc, a); } return acc; }
static U invm(const U &a) { U e = R_MOD; e.w[0] -= 2; return powm(a, e); }
static U small(uint64_t v) { return U{{v, 0, 0, 0}}; }
static U MONT_R, MONT_RINV;   // 2^256 mod r and its inverse
static fe_t to_mont(const U &a) { const U m = mulm(a, MONT_R); fe_t r; std::memcpy(&r, &m, 32); return r; }
static U from_mont(const fe_t &a) { U m; std::memcpy(&m, &a, 32); return mulm(m, MONT_RINV); }

struct Prog { std::vector<uint32_t> code; uint32_t n_regs = 0; std::vector<U> consts; uint32_t n_inputs = 0; std::vector<uint32_t> out_regs;
  void ins(uint32_t op, uint32_t d, uint32_t a, uint32_t b) { code.push_back(op); code.push_back(d); code.push_back(a); code.push_back(b); }
  uint32_t n_instr() const { return (uint32_t)(code.size() / 4); } };

// the reference: registers as canonical integers, one job at a time
static void ref_run(const Prog &P, const std::vector<U> &inputs, uint32_t jobs, std::vector<U> &outputs, std::vector<uint32_t> &flags) {
  outputs.clear(); flags.assign(jobs, 0);
  for (uint32_t j = 0; j < jobs; j++) {
    std::vector<U> reg(P.n_regs, U{{~0ull, ~0ull, ~0ull, ~0ull}});
    for (size_t i = 0; i < P.consts.size(); i++) reg[i] = P.consts[i];
    for (uint32_t t = 0; t < P.n_inputs; t++) reg[P.consts.size() + t] = inputs[(size_t)j * P.n_inputs + t];
    for (uint32_t i = 0; i < P.n_instr(); i++) {
      const uint32_t op = P.code[4 * i], d = P.code[4 * i + 1], a = P.code[4 * i + 2], b = P.code[4 * i + 3];
      if (op == FRP_ADD) reg[d] = addm(reg[a], reg[b]);
      else if (op == FRP_SUB) reg[d] = subm(reg[a], reg[b]);
      else if (op == FRP_MUL) reg[d] = mulm(reg[a], reg[b]);
      else if (op == FRP_SQRN) { U r = reg[a]; for (uint32_t k = 0; k < b; k++) r = mulm(r, r); reg[d] = r; }
      else if (op == FRP_INV) { if (is0(reg[a])) flags[j] |= 1; reg[d] = invm(reg[a]); }
      else if (is0(reg[a])) flags[j] |= 1u << b;
    }
    for (uint32_t r : P.out_regs) outputs.push_back(reg[r]);
  }
}
// the code under test, through the same arguments the entry point takes
static bool dev_run(const Prog &P, const std::vector<U> &inputs, uint32_t jobs, std::vector<U> &outputs, std::vector<uint32_t> &flags, std::string &why) {
  std::vector<fe_t> consts, in, out((size_t)jobs * P.out_regs.size() + 1);
  for (const U &c : P.consts) consts.push_back(to_mont(c));
  for (const U &v : inputs) in.push_back(to_mont(v));
  flags.assign(jobs + 1, 0xdeadbeefu); std::memset(&out.back(), 0x5a, 32);
  if (!frprog_check(P.code.data(), P.n_instr(), P.n_regs, consts.data(), (uint32_t)consts.size(), in.data(), P.n_inputs, jobs, P.out_regs.data(), (uint32_t)P.out_regs.size(), out.data(), flags.data(), why)) return false;
  frprog_run_host(P.code.data(), P.n_instr(), P.n_regs, consts.data(), (uint32_t)consts.size(), in.data(), P.n_inputs, jobs, P.out_regs.data(), (uint32_t)P.out_regs.size(), out.data(), flags.data());
  fe_t guard; std::memset(&guard, 0x5a, 32);
  if (std::memcmp(&out.back(), &guard, 32) || flags.back() != 0xdeadbeefu) { why = "wrote behind its outputs"; return false; }
  uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = FrP::mod(i);
  outputs.clear(); for (size_t i = 0; i + 1 < out.size(); i++) { if (Fr::w_geq(out[i].l, m)) { why = "an output is not fully reduced"; return false; } outputs.push_back(from_mont(out[i])); }
  flags.pop_back();
  return true;
}
static int fails = 0;
static void expect(bool ok, const std::string &what) { if (!ok) { std::printf("FAIL %s\n", what.c_str()); fails++; } }
static void compare(const Prog &P, const std::vector<U> &inputs, uint32_t jobs, const std::string &what) {
  std::vector<U> want, got; std::vector<uint32_t> wf, gf; std::string why;
  ref_run(P, inputs, jobs, want, wf);
  if (!dev_run(P, inputs, jobs, got, gf, why)) { expect(false, what + ": " + why); return; }
  bool ok = want.size() == got.size() && wf == gf;
  for (size_t i = 0; ok && i < want.size(); i++) ok = same(want[i], got[i]);
  expect(ok, what);
}

// the call of mi355_fr_program_host on the CPU, for tests/test_fr_program_on_host.py (this file built as a shared object): the checks, then the interpreter; 0 = ran
extern "C" int frp_host_run(const uint32_t *code, uint32_t n_instr, uint32_t n_regs, const void *consts, uint32_t n_consts, const void *inputs, uint32_t n_inputs, uint32_t jobs,
                            const uint32_t *out_regs, uint32_t n_outputs, void *outputs, uint32_t *flags) {
  std::string why;
  if (!frprog_check(code, n_instr, n_regs, consts, n_consts, inputs, n_inputs, jobs, out_regs, n_outputs, outputs, flags, why)) { std::fprintf(stderr, "frp_host_run: %s\n", why.c_str()); return 1; }
  frprog_run_host(code, n_instr, n_regs, (const fe_t *)consts, n_consts, (const fe_t *)inputs, n_inputs, jobs, out_regs, n_outputs, (fe_t *)outputs, flags);
  return 0;
}

int main() {
  { U one = small(1); MONT_R = one; for (int i = 0; i < 256; i++) MONT_R = addm(MONT_R, MONT_R); MONT_RINV = invm(MONT_R); }
  U rm1 = R_MOD; rm1.w[0] -= 1;
  U two255 = small(1); for (int i = 0; i < 255; i++) two255 = addm(two255, two255);
  const std::vector<U> edges = {small(0), small(1), rm1, two255, MONT_R};

  // ---- every op on every pair of the edge operands, with the destination apart from, and aliasing, its operands
  std::vector<U> pairs; for (const U &a : edges) for (const U &b : edges) { pairs.push_back(a); pairs.push_back(b); }
  const uint32_t jobs25 = (uint32_t)(edges.size() * edges.size());
  for (uint32_t op : {FRP_ADD, FRP_SUB, FRP_MUL}) for (int alias = 0; alias < 4; alias++) {
    Prog P; P.consts = {small(0)}; P.n_inputs = 2; P.n_regs = 6;          // r0 = 0 | r1, r2 inputs | r3, r4 copies | r5
    P.ins(FRP_ADD, 3, 1, 0); P.ins(FRP_ADD, 4, 2, 0);
    if (alias == 0) P.ins(op, 5, 3, 4); else if (alias == 1) P.ins(op, 3, 3, 4); else if (alias == 2) P.ins(op, 4, 3, 4); else P.ins(op, 3, 3, 3);
    P.out_regs = {3, 4, (uint32_t)(alias == 0 ? 5 : 3)};
    compare(P, pairs, jobs25, "op " + std::to_string(op) + " alias mode " + std::to_string(alias));
  }
  for (uint32_t n : {0u, 1u, 64u}) for (int alias = 0; alias < 2; alias++) {
    Prog P; P.consts = {small(0)}; P.n_inputs = 1; P.n_regs = 4;
    P.ins(FRP_ADD, 2, 1, 0); P.ins(FRP_SQRN, alias ? 2 : 3, 2, n); P.out_regs = {(uint32_t)(alias ? 2 : 3)};
    compare(P, edges, (uint32_t)edges.size(), "SQRN by " + std::to_string(n) + (alias ? " in place" : ""));
  }
  for (int alias = 0; alias < 2; alias++) {
    Prog P; P.consts = {small(0)}; P.n_inputs = 1; P.n_regs = 4;
    P.ins(FRP_ADD, 2, 1, 0); P.ins(FRP_INV, alias ? 2 : 3, 2, 0); P.ins(FRP_NZ, 0, 1, 7); P.ins(FRP_NZ, 0, 0, 31); P.out_regs = {(uint32_t)(alias ? 2 : 3), 1, 0};   // an input and a constant as outputs
    compare(P, edges, (uint32_t)edges.size(), std::string("INV and NZ") + (alias ? " in place" : ""));
  }

  // ---- INV of zero in one job among 65: zero out, bit 0 in that job's word alone
  {
    Prog P; P.n_inputs = 1; P.n_regs = 2; P.ins(FRP_INV, 1, 0, 0); P.out_regs = {1};
    std::vector<U> in; for (uint32_t j = 0; j < 65; j++) in.push_back(small(j == 40 ? 0 : j + 2));
    std::vector<U> got; std::vector<uint32_t> gf; std::string why;
    expect(dev_run(P, in, 65, got, gf, why), "INV of zero among 65: " + why);
    bool ok = got.size() == 65; for (uint32_t j = 0; ok && j < 65; j++) ok = gf[j] == (j == 40 ? 1u : 0u) && (j == 40 ? is0(got[j]) : same(mulm(got[j], in[j]), small(1)));
    expect(ok, "INV of zero among 65 jobs");
    compare(P, in, 65, "INV of zero among 65 jobs against the reference");
  }

  // ---- random programs
  std::mt19937_64 rng(20241);
  auto rnd = [&]() { U a; for (auto &w : a.w) w = rng(); a.w[3] &= 0x3fffffffffffffffull; while (geq(a, R_MOD)) sub_raw(a, R_MOD); return a; };
  for (int round = 0; round < 6; round++) {
    const uint32_t nc = 3, ni = 4, nt = round < 3 ? 5 : 40, n_instr = round == 0 ? 1 : round == 1 ? 2 : 300, jobs = round % 2 ? 66 : 3;
    Prog P; P.consts = {small(0), small(1), rnd()}; P.n_inputs = ni; P.n_regs = nc + ni + nt;
    std::vector<uint32_t> written; for (uint32_t r = 0; r < nc + ni; r++) written.push_back(r);
    auto src = [&]() { return written[rng() % written.size()]; };
    for (uint32_t i = 0; i < n_instr; i++) {
      const uint32_t pick = (uint32_t)(rng() % 40), d = nc + ni + (uint32_t)(rng() % nt);
      if (pick < 10) P.ins(FRP_ADD, d, src(), src()); else if (pick < 18) P.ins(FRP_SUB, d, src(), src()); else if (pick < 32) P.ins(FRP_MUL, d, src(), src());
      else if (pick < 36) P.ins(FRP_SQRN, d, src(), (uint32_t)(rng() % 8 == 0 ? 64 : rng() % 5)); else if (pick == 36) P.ins(FRP_INV, d, src(), 0);
      else { P.ins(FRP_NZ, 0, src(), 1 + (uint32_t)(rng() % 31)); continue; }
      if (std::find(written.begin(), written.end(), d) == written.end()) written.push_back(d);
    }
    for (uint32_t r : written) P.out_regs.push_back(r);
    P.out_regs.push_back(written.back());                                  // one register named twice
    std::vector<U> in; for (uint32_t i = 0; i < jobs * ni; i++) in.push_back(i % 7 == 3 ? edges[i % edges.size()] : rnd());
    compare(P, in, jobs, "random program " + std::to_string(round));
  }

  // ---- every rejection of the argument checks, each by its message
  {
    const fe_t zero = Fr::zero(); fe_t big; for (int i = 0; i < 8; i++) big.l[i] = FrP::mod(i);   // the word r itself
    const std::vector<uint32_t> good = {FRP_ADD, 3, 0, 1, FRP_MUL, 3, 3, 2};
    const std::vector<fe_t> consts = {zero}, inputs = {zero, zero, zero, zero};   // 1 constant, 2 inputs, 2 jobs, registers 0 .. 3
    const std::vector<uint32_t> outs = {3}; std::vector<fe_t> out(2); std::vector<uint32_t> fl(2);
    struct Args { const uint32_t *code; uint32_t n_instr, n_regs; const void *consts; uint32_t n_consts; const void *inputs; uint32_t n_inputs, jobs; const uint32_t *out_regs; uint32_t n_outputs; void *outputs; uint32_t *flags; };
    const Args ok = {good.data(), 2, 4, consts.data(), 1, inputs.data(), 2, 2, outs.data(), 1, out.data(), fl.data()};
    auto check = [&](const Args &a, std::string &why) { return frprog_check(a.code, a.n_instr, a.n_regs, a.consts, a.n_consts, a.inputs, a.n_inputs, a.jobs, a.out_regs, a.n_outputs, a.outputs, a.flags, why); };
    auto refused = [&](Args a, const char *needle) { std::string why; const bool r = check(a, why); expect(!r && why.find(needle) != std::string::npos, std::string("rejection: ") + needle + " (got: " + why + ")"); };
    { std::string why; expect(check(ok, why), "the good call is accepted: " + why); }
    { Args a = ok; a.code = nullptr; refused(a, "null pointer"); }
    { Args a = ok; a.consts = nullptr; refused(a, "null pointer"); }
    { Args a = ok; a.inputs = nullptr; refused(a, "null pointer"); }
    { Args a = ok; a.out_regs = nullptr; refused(a, "null pointer"); }
    { Args a = ok; a.outputs = nullptr; refused(a, "null pointer"); }
    { Args a = ok; a.flags = nullptr; refused(a, "null pointer"); }
    { Args a = ok; a.n_regs = (1u << 16) + 1; refused(a, "more than 2^16 registers"); }
    { Args a = ok; a.n_instr = (1u << 20) + 1; refused(a, "more than 2^20 instructions"); }
    { Args a = ok; a.jobs = (1u << 20) + 1; refused(a, "more than 2^20 jobs"); }
    { Args a = ok; a.n_regs = 2; refused(a, "exceeds n_regs"); }
    auto with_code = [&](std::vector<uint32_t> &c, const char *needle) { Args a = ok; a.code = c.data(); a.n_instr = (uint32_t)(c.size() / 4); refused(a, needle); };
    { std::vector<uint32_t> c = good; c[4] = FRP_OPS; with_code(c, "instruction 1: unknown op 6"); }
    { std::vector<uint32_t> c = good; c[2] = 4; with_code(c, "instruction 0: operand register 4 is not below n_regs"); }
    { std::vector<uint32_t> c = good; c[7] = 9; with_code(c, "instruction 1: operand register 9 is not below n_regs"); }
    { std::vector<uint32_t> c = good; c[5] = 4; with_code(c, "instruction 1: destination register 4 is not below n_regs"); }
    { std::vector<uint32_t> c = good; c[1] = 2; with_code(c, "instruction 0: destination register 2 is a constant or an input"); }
    { std::vector<uint32_t> c = good; c[1] = 0; with_code(c, "instruction 0: destination register 0 is a constant or an input"); }
    { std::vector<uint32_t> c = {FRP_SQRN, 3, 1, 65}; with_code(c, "instruction 0: SQRN by 65"); }
    { std::vector<uint32_t> c = {FRP_NZ, 0, 1, 0}; with_code(c, "instruction 0: NZ names flag bit 0"); }
    { std::vector<uint32_t> c = {FRP_NZ, 0, 1, 32}; with_code(c, "instruction 0: NZ names flag bit 32"); }
    { std::vector<uint32_t> c = {FRP_SQRN, 3, 1, 64, FRP_NZ, 99, 1, 31, FRP_INV, 3, 3, 99}; Args a = ok; a.code = c.data(); a.n_instr = 3; std::string why; expect(check(a, why), "immediates at their limits and ignored fields are accepted: " + why); }
    { Args a = ok; const std::vector<uint32_t> o = {4}; a.out_regs = o.data(); refused(a, "output 0 names register 4"); }
    { Args a = ok; const std::vector<fe_t> c = {big}; a.consts = c.data(); refused(a, "constant 0 is not below r"); }
    { Args a = ok; std::vector<fe_t> in = inputs; in[3] = big; a.inputs = in.data(); refused(a, "input 1 of job 1 is not below r"); }
    { Args a = ok; a.jobs = 0; a.inputs = nullptr; a.outputs = nullptr; a.flags = nullptr; std::string why; expect(check(a, why), "jobs == 0 needs no per-job arrays: " + why); }
  }
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("all passed\n");
  return 0;
}
