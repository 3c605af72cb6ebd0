// mi355zk_plonk.hpp -- halo2_proofs::plonk::create_proof for a PlonkProtocol, over resident polynomials on the MI355X, through the C-ABI (include/mi355zk.h).
//
// What the reference reaches: gen_halo2_chunk_proof / gen_batch_proof / gen_bundle_proof [REF integration/src/prove.rs:37,67,95-97] run create_proof once per
// layer; the constraint system of a layer is the PlonkProtocol the proof carries ([REF release-v0.13.1/chunk.protocol],
// [REF integration/tests/test_data/full_proof_batch_agg_1.json]; mi355zk_plonk_protocol.hpp).  This header is the prover for ANY such protocol:
//
//   keygen          commit_lagrange of every fixed / sigma column (= the verifying key, serialised like [REF release-v0.13.1/vk_chunk.vkey]); coefficient and
//                   extended-coset forms of the proving key resident in HBM (Q coset parts of 2^k, the scroll fork's coeff_to_extended_part), plus the
//                   common polynomials the numerator names (l_0, l_last = Lagrange(-7), l_active = 1 - l_last - sum Lagrange(-6..-1), X)
//   compile         quotient.numerator -> launches of mi355_fr_gate_eval_dev (sums of products of rotated polynomials).  A cost model decides per Product node
//                   whether to distribute it or to materialise a factor as a temporary (one extra pass over HBM against re-evaluating its factors in every
//                   term); challenges are scalars by then.  Nothing in the plan comes from the recognised argument structure -- the tree is compiled as it
//                   stands, so the quotient the device computes is the fixture's numerator and not a re-derivation of it.
//   create_proof    SURVEY 3.2's steps with halo2's transcript: instance values and advice commitments in, theta out; m commitments in, beta / gamma out; grand
//                   products z (chunks linked through z_(c-1)(w^last X)), running sums phi, the RANDOM polynomial of the vanishing argument (step 5) in, y out;
//                   the quotient part by part, its Q pieces in, x out; the evaluations in the protocol's order; SHPLONK over the rotation sets the protocol's
//                   `queries` imply (per set: interpolated remainders, division by the set's vanishing polynomial; one combined quotient commitment, the
//                   linearised polynomial at u, its kate_division) -- two closing commitments, as the fixtures' two trailing G1 words.
//   check_witness   MockProver::verify on the device: every gate on every row, every copy constraint, every lookup input, reported as (constraint, row) failures
//                   (csrc/check.hpp); ProofOptions::check_witness runs it ahead of the proof
//   the proof       bytes in the reference's layout: 32-byte compressed G1 commitments in transcript order, canonical little-endian
//                   Fr evaluations, two compressed SHPLONK points: 896 B for layer 2 ([1,1,3] witness polynomials, Q = 4, 17 evaluations), 1 312 B for layer 4.
//
// Checked by oracle/plonk.py (tests only): a verifier that walks the JSON tree itself, and a CPU restatement of this prover whose proof bytes must be IDENTICAL.
// The Rust twin of the flow is rust_shim/create_proof_resident.rs.  Host code here is the transcript, the plan compiler and a few field operations per rotation
// set; everything proportional to 2^k runs on the device.
#pragma once
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <sys/random.h>   // getrandom(2): ProofOptions::rng_key_from_os

#include "mi355zk_plonk_circuit.hpp"
#include "mi355zk_transcript.hpp"
#include "mi355zk_plonk_verify.hpp"   // plonk::verify_proof

namespace mi355zk {
namespace plonk {

using halo2::check;
using halo2::DevicePoly;
using halo2::Error;
using halo2::EvaluationDomain;
using halo2::G1;

// ------------------------------------------------------------------------------------------------ the plan
enum AtomKind : uint8_t { A_POLY = 0, A_COMMON, A_TMP };
struct Atom { AtomKind kind; uint32_t idx; int32_t rot; bool operator<(const Atom &o) const { return kind != o.kind ? kind < o.kind : idx != o.idx ? idx < o.idx : rot < o.rot; } };
struct Term { Fr coeff; std::vector<Atom> f; };
using SoP = std::vector<Term>;
struct Launch { int dst; bool accumulate; std::vector<Term> terms; };     // dst >= 0: TMP[dst]; dst == -1: the quotient accumulator of the part
constexpr uint32_t PLAN_MAX_TERMS = 16, PLAN_MAX_FACTORS = 48, PLAN_MAX_POLYS = 24, PLAN_MAX_TERM_LEN = 16;   // per launch (mi355_fr_gate_eval_dev)

struct CommonRegistry {   // the fixed polynomials the numerator names through CommonPolynomial leaves, deduplicated by subtree
  std::vector<CommonLinear> defs; std::map<std::string, uint32_t> by_key;
  uint32_t id_of(const Expr &e, bool create) {
    std::string key; expr_key(e, key);
    auto it = by_key.find(key);
    if (it != by_key.end()) return it->second;
    if (!create) throw std::invalid_argument("plan compiler: common polynomial " + key + " is not in the proving key");
    CommonLinear d; common_linear_terms(e, fr_one(), d);
    defs.push_back(d); by_key.emplace(key, (uint32_t)defs.size() - 1);
    return (uint32_t)defs.size() - 1;
  }
};

struct Compiler {
  CommonRegistry &reg; bool create_commons; std::vector<Fr> ch;
  std::vector<Launch> out; uint32_t tmp_base = 0, tmp_next = 0, tmp_max = 0;
  uint32_t constraints = 0, terms_total = 0;
  static constexpr double PASS = 3.0;       // one more pass over HBM (write + read 32 B per row), in units of one factor of the ALU-bound fused kernel
  Compiler(CommonRegistry &r, bool create, std::vector<Fr> challenges) : reg(r), create_commons(create), ch(std::move(challenges)) {}

  static double F(const SoP &S) { double f = 0; for (const auto &t : S) f += (double)t.f.size() + 0.5; return f; }
  static bool is_unit(const SoP &S) { return S.size() == 1 && S[0].f.size() == 1 && S[0].coeff == fr_one(); }
  static size_t maxlen(const SoP &S) { size_t m = 0; for (const auto &t : S) m = std::max(m, t.f.size()); return m; }
  static SoP scaled(SoP S, const Fr &c) { for (auto &t : S) t.coeff = fr_mul(t.coeff, c); return S; }
  static void merge_scalars(SoP &S) {   // one constant term per sum
    int first = -1;
    for (size_t i = 0; i < S.size();) { if (!S[i].f.empty()) { i++; continue; } if (first < 0) { first = (int)i++; continue; } S[first].coeff = fr_add(S[first].coeff, S[i].coeff); S.erase(S.begin() + (long)i); }
    if (first >= 0 && fr_is_zero(S[first].coeff) && S.size() > 1) S.erase(S.begin() + first);
  }
  // TMP[t] = S, split to the launch limits
  void emit(int dst, const SoP &S, bool accumulate_first = false) {
    Launch cur{dst, accumulate_first, {}}; std::set<Atom> polys; uint32_t nf = 0; bool any = false;
    auto key = [](const Atom &a) { return Atom{a.kind, a.idx, 0}; };
    for (const auto &t : S) {
      if (t.f.size() > PLAN_MAX_TERM_LEN) throw std::invalid_argument("plan compiler: a term exceeds 16 factors");
      std::set<Atom> np = polys; for (const auto &a : t.f) np.insert(key(a));
      if (cur.terms.size() + 1 > PLAN_MAX_TERMS || nf + t.f.size() > PLAN_MAX_FACTORS || np.size() > PLAN_MAX_POLYS) {
        out.push_back(cur); any = true; cur = Launch{dst, true, {}}; polys.clear(); nf = 0; np.clear(); for (const auto &a : t.f) np.insert(key(a));
      }
      cur.terms.push_back(t); polys = np; nf += (uint32_t)t.f.size();
    }
    if (!cur.terms.empty() || !any) out.push_back(cur);
  }
  SoP materialize(const SoP &S) {
    if (is_unit(S)) return S;
    const uint32_t t = tmp_base + tmp_next++; tmp_max = std::max(tmp_max, t + 1);
    emit((int)t, S);
    return SoP{Term{fr_one(), {Atom{A_TMP, t, 0}}}};
  }
  SoP expand(const SoP &A, const SoP &B) {
    SoP R; R.reserve(A.size() * B.size());
    for (const auto &a : A) for (const auto &b : B) { Term t{fr_mul(a.coeff, b.coeff), a.f}; t.f.insert(t.f.end(), b.f.begin(), b.f.end()); R.push_back(std::move(t)); }
    return R;
  }
  SoP product(SoP A, SoP B) {
    for (;;) {
      const double nA = (double)A.size(), nB = (double)B.size(), inf = 1e30;
      const bool fits = maxlen(A) + maxlen(B) <= PLAN_MAX_TERM_LEN;
      const double c_expand = fits ? nB * F(A) + nA * F(B) : inf;
      const double c_matA = is_unit(A) ? inf : F(A) + PASS + F(B) + nB;
      const double c_matB = is_unit(B) ? inf : F(B) + PASS + F(A) + nA;
      if (c_expand <= c_matA && c_expand <= c_matB) return expand(A, B);
      if (c_matA <= c_matB) A = materialize(A); else B = materialize(B);
    }
  }
  Fr scalar_of(const SoP &S) const { if (S.size() != 1 || !S[0].f.empty()) throw std::invalid_argument("plan compiler: the base of DistributePowers must be a scalar"); return S[0].coeff; }
  SoP compile(const Expr &e) {
    bool common = false;
    if ((e.kind == Expr::IDENTITY || e.kind == Expr::LAGRANGE || e.kind == Expr::SUM || e.kind == Expr::NEG) && is_common_linear(e, &common) && common)
      return SoP{Term{fr_one(), {Atom{A_COMMON, reg.id_of(e, create_commons), 0}}}};
    switch (e.kind) {
      case Expr::CONSTANT: return SoP{Term{e.c, {}}};
      case Expr::CHALLENGE: return SoP{Term{ch.at((size_t)e.i), {}}};
      case Expr::POLY: return SoP{Term{fr_one(), {Atom{A_POLY, (uint32_t)e.i, e.rot}}}};
      case Expr::NEG: return scaled(compile(e.kids[0]), fr_neg(fr_one()));
      case Expr::SCALED: return scaled(compile(e.kids[0]), e.c);
      case Expr::SUM: { SoP a = compile(e.kids[0]), b = compile(e.kids[1]); a.insert(a.end(), b.begin(), b.end()); merge_scalars(a); return a; }
      case Expr::PROD: return product(compile(e.kids[0]), compile(e.kids[1]));
      case Expr::DPOW: {   // Horner in the base: ((e_0 b + e_1) b + e_2) ...
        const Fr b = scalar_of(compile(e.kids.back()));
        SoP acc = compile(e.kids[0]);
        for (size_t i = 1; i + 1 < e.kids.size(); i++) { acc = scaled(std::move(acc), b); SoP x = compile(e.kids[i]); acc.insert(acc.end(), x.begin(), x.end()); merge_scalars(acc); }
        return acc;
      }
      default: throw std::invalid_argument("plan compiler: unexpected node");
    }
  }
  // the whole numerator: constraint i of DistributePowers(constraints, y) carries y^(m - 1 - i); constraints that needed temporaries are flushed at once so that the
  // next one may reuse them
  // Constraints that needed temporaries share an accumulate launch while their temporaries fit TMP_GROUP blocks: each constraint is compiled with ids from 0 and
  // RELOCATED behind the ids of the constraints already waiting; everything waiting is flushed (its terms emitted) before ids are reused.
  // COMMON PREFIXES.  Many constraints are  p * (...)  with the same leading polynomial p -- every assigned gate of the inner circuit carries the one selector, every
  // permutation chunk and lookup carries l_active.  Distributed, p is loaded, re-sliced and multiplied into every term; instead the bracketed parts of such a group
  // (>= 16 constraints) accumulate, with their powers of y, into ONE long-lived temporary G_p, and the quotient receives the single term p * G_p at the end:
  // one factor fewer in every term of the group for one more pass over HBM per group.
  static constexpr uint32_t TMP_GROUP = 12, GROUP_BASE = 32;   // waiting constraints share up to TMP_GROUP local temporaries (ids < GROUP_BASE); the long-lived G_p live at GROUP_BASE + g
  static uint32_t prefix_min() { const char *e = std::getenv("MI355_PLAN_PREFIX_MIN"); const long v = e ? std::atol(e) : 16; return v <= 0 ? 0xffffffffu : (uint32_t)v; }   // 0: never group (A/B, profiles/r05_gate_eval.md)
  uint32_t prefix_groups = 0;
  uint32_t tmps_used() const { std::set<int> u; for (const auto &L : out) if (L.dst >= 0) u.insert(L.dst); return (uint32_t)u.size(); }
  void compile_numerator(const Expr &num) {
    const size_t m = num.kids.size() - 1; const Fr y = scalar_of(compile(num.kids.back()));
    std::vector<Fr> ypow(m, fr_one()); for (size_t i = 1; i < m; i++) ypow[i] = fr_mul(ypow[i - 1], y);
    // pass 0: which constraints share a leading polynomial
    auto prefix_of = [&](const Expr &c, Atom &a) -> bool {
      if (c.kind != Expr::PROD) return false;
      const Expr &p = c.kids[0]; bool common = false;
      if (p.kind == Expr::POLY) { a = Atom{A_POLY, (uint32_t)p.i, p.rot}; return true; }
      if (is_common_linear(p, &common) && common) { a = Atom{A_COMMON, reg.id_of(p, create_commons), 0}; return true; }
      return false;
    };
    std::map<Atom, uint32_t> count; std::map<Atom, int> group_tmp;
    for (size_t i = 0; i < m; i++) { Atom a; if (prefix_of(num.kids[i], a)) count[a]++; }
    for (const auto &kv : count) if (kv.second >= prefix_min()) { group_tmp[kv.first] = (int)(GROUP_BASE + prefix_groups++); tmp_max = std::max(tmp_max, GROUP_BASE + prefix_groups); }
    // pass 1
    std::map<int, SoP> pending; std::set<int> started; uint32_t waiting_tmps = 0;
    auto relocate = [](std::vector<Term> &ts, uint32_t off) { for (auto &t : ts) for (auto &a : t.f) if (a.kind == A_TMP && a.idx < GROUP_BASE) a.idx += off; };
    auto flush = [&]() {
      for (auto &kv : pending) { if (kv.second.empty()) continue; emit(kv.first, kv.second, kv.first < 0 || started.count(kv.first) > 0); started.insert(kv.first); kv.second.clear(); }
      waiting_tmps = 0;
    };
    for (size_t i = 0; i < m; i++) {
      Atom pa; const bool grouped = prefix_of(num.kids[i], pa) && group_tmp.count(pa);
      const size_t first_launch = out.size();
      tmp_base = 0; tmp_next = 0;
      SoP s = scaled(compile(grouped ? num.kids[i].kids[1] : num.kids[i]), ypow[m - 1 - i]);
      constraints++; terms_total += (uint32_t)s.size();
      const uint32_t used = tmp_next;
      if (used > GROUP_BASE) throw std::invalid_argument("plan compiler: one constraint needs more than 32 temporaries");
      std::vector<Launch> mine(out.begin() + (long)first_launch, out.end()); out.resize(first_launch);   // this constraint's temporaries
      if (used > 0 && waiting_tmps > 0 && waiting_tmps + used > TMP_GROUP) flush();
      if (used > 0) {
        if (waiting_tmps > 0) { for (auto &L : mine) { L.dst += (int)waiting_tmps; relocate(L.terms, waiting_tmps); } relocate(s, waiting_tmps); }
        waiting_tmps += used; tmp_max = std::max(tmp_max, waiting_tmps);
      }
      out.insert(out.end(), mine.begin(), mine.end());
      SoP &dst = pending[grouped ? group_tmp[pa] : -1];
      dst.insert(dst.end(), s.begin(), s.end());
    }
    flush();                                                                                                    // every G_p is complete ...
    for (const auto &kv : group_tmp) pending[-1].push_back(Term{fr_one(), {kv.first, Atom{A_TMP, (uint32_t)kv.second, 0}}});
    flush();                                                                                                    // ... before the quotient reads p * G_p
  }
};

// what the fused kernel was asked to do, summed over every launch of this process: the ALGORITHMIC side of its roofline (profiles/r05_gate_eval.md compares it with
// the FETCH_SIZE / WRITE_SIZE and SQ counters of the same run).  bytes = 32 B x rows x (distinct operand polynomials + dst written + dst read when accumulating)
// distinct_rows: (polynomial, rotation) pairs a launch names, times its rows -- what a launch would load if every operand were re-sliced ONCE and kept in registers across its
// terms; hot_repeat_rows: the loads beyond the first of operands that appear in >= 4 terms of one launch (selectors, l_active, a prefix polynomial): what a register cache of a
// few hot operands could save (measure the operand cache instead of arguing it away -- profiles/r06_gate_operand_reuse.md)
struct GateStats { std::atomic<uint64_t> launches{0}, bytes{0}, factor_rows{0}, term_rows{0}, distinct_rows{0}, hot_repeat_rows{0}; };
inline GateStats &gate_stats() { static GateStats g; return g; }
inline void gate_eval(void *dst, const void *const *polys, uint32_t n_polys, const Fr *coeffs, const uint32_t *term_len, uint32_t n_terms, const uint32_t *factor_poly, const int32_t *factor_rot, uint64_t n, int accumulate) {
  check(mi355_fr_gate_eval_dev(dst, polys, n_polys, coeffs, term_len, n_terms, factor_poly, factor_rot, n, accumulate));
  uint64_t nf = 0; for (uint32_t j = 0; j < n_terms; j++) nf += term_len[j];
  GateStats &g = gate_stats(); g.launches++; g.bytes += 32 * n * (uint64_t)(n_polys + 1 + (accumulate ? 1 : 0)); g.factor_rows += nf * n; g.term_rows += (uint64_t)n_terms * n;
  { std::map<std::pair<uint32_t, int32_t>, uint32_t> uses; uint32_t f = 0;
    for (uint32_t j = 0; j < n_terms; j++) { std::set<std::pair<uint32_t, int32_t>> in_term; for (uint32_t q = 0; q < term_len[j]; q++, f++) if (in_term.insert({factor_poly[f], factor_rot[f]}).second) uses[{factor_poly[f], factor_rot[f]}]++; }
    uint64_t hot = 0; for (const auto &kv : uses) if (kv.second >= 4) hot += kv.second - 1;
    g.distinct_rows += (uint64_t)uses.size() * n; g.hot_repeat_rows += hot * n; }
}
// one Launch through mi355_fr_gate_eval_dev; resolve(Atom) -> device pointer of the operand on the domain the launch runs on
template <class Resolve> inline void run_launch(const Launch &L, void *dst, uint64_t n, const Fr &scale, bool accumulate, Resolve resolve) {
  std::vector<const void *> polys; std::map<Atom, uint32_t> slot;
  std::vector<Fr> coeffs; std::vector<uint32_t> tl, fp; std::vector<int32_t> fr;
  for (const auto &t : L.terms) {
    coeffs.push_back(fr_mul(t.coeff, scale)); tl.push_back((uint32_t)t.f.size());
    for (const auto &f : t.f) {
      const Atom key{f.kind, f.idx, 0};
      auto it = slot.find(key);
      if (it == slot.end()) { it = slot.emplace(key, (uint32_t)polys.size()).first; polys.push_back(resolve(key)); }
      fp.push_back(it->second); fr.push_back(f.rot);
    }
  }
  if (L.terms.empty()) { if (!accumulate) check(mi355_buf_zero(dst, n * 32)); return; }
  gate_eval(dst, polys.empty() ? nullptr : polys.data(), (uint32_t)polys.size(), coeffs.data(), tl.data(), (uint32_t)tl.size(), fp.empty() ? nullptr : fp.data(), fr.empty() ? nullptr : fr.data(), n, accumulate ? 1 : 0);
}
inline DevicePoly clone(const DevicePoly &s, int slot) { DevicePoly d(s.n, slot); check(mi355_buf_copy(d.p, s.p, s.n * 32)); return d; }
inline Fr part_factor(const EvaluationDomain &dom, uint32_t q) { return fr_mul(dom.g_coset, fr_pow(dom.extended_omega, q)); }

// ------------------------------------------------------------------------------------------------ the proving key, resident
struct ProvingKey {
  const Protocol *P = nullptr; std::unique_ptr<EvaluationDomain> dom; bool resident_cosets = true; int devices = 1;
  std::vector<DevicePoly> pre_lagrange, pre_coeff; std::vector<std::vector<DevicePoly>> pre_cosets;          // [polynomial][part]; Lagrange values only where step 4 reads them
  CommonRegistry commons; std::vector<DevicePoly> common_lagrange, common_coeff; std::vector<std::vector<DevicePoly>> common_cosets;
  uint32_t identity_common = 0;
  std::vector<uint8_t> vk;                                                                                  // u32 BE k | u32 BE fixed columns | compressed commitments
  uint64_t bytes = 0;
  double sigma_ms = 0, sigma_host_prep_ms = 0;   // keygen's sigma stage, wall time: default route = sigma_column + upload of every sigma column; device_sigma = the one call (host_prep: PermutationAssembly + overrides before it)
  const DevicePoly &coeff(const Atom &a) const { return a.kind == A_COMMON ? common_coeff.at(a.idx) : pre_coeff.at(a.idx); }
  const DevicePoly *coset(const Atom &a, uint32_t q) const { if (!resident_cosets) return nullptr; return a.kind == A_COMMON ? &common_cosets.at(a.idx)[q] : &pre_cosets.at(a.idx)[q]; }
};
// which preprocessed polynomials step 4 reads as Lagrange values: permuted fixed columns, every sigma, whatever the lookups' table / input expressions name
inline std::set<uint32_t> lagrange_needed(const Protocol &P) {
  std::set<uint32_t> s;
  for (const auto &c : P.perm) for (const auto &col : c.columns) { s.insert(col.sigma); if (P.is_pre(col.column)) s.insert(col.column); }
  for (const auto &l : P.lookups) { std::vector<std::pair<int32_t, int32_t>> r; collect_polys(*l.table, r); collect_polys(*l.input, r); for (const auto &x : r) if (P.is_pre((uint32_t)x.first)) s.insert((uint32_t)x.first); }
  return s;
}
// HBM a layer's prover needs, from the protocol alone: a dry compile gives the plan's temporaries and the common polynomials
// coset_group: ProofOptions::coset_group_polys of the proofs to come (0: step 7 holds one coset part of every witness polynomial, and a lean key one of every key polynomial;
// G: of the G operands of one group of launches)
struct PkSizes { uint32_t polys, lagrange, commons, plan_tmps; double base_bytes, coset_bytes, lean_tmp_bytes, working_bytes; };
inline PkSizes pk_sizes(const Protocol &P, uint32_t coset_group = 0) {
  const double per = (double)P.n * 32; PkSizes s;
  CommonRegistry reg; { Expr id; id.kind = Expr::IDENTITY; reg.id_of(id, true); }
  Compiler cmp(reg, true, std::vector<Fr>(4, fr_one())); cmp.compile_numerator(P.numerator);
  s.commons = (uint32_t)reg.defs.size(); s.plan_tmps = cmp.tmps_used();
  s.polys = P.num_pre + s.commons; s.lagrange = (uint32_t)lagrange_needed(P).size() + 1;
  s.base_bytes = per * (s.polys + s.lagrange); s.coset_bytes = per * s.polys * P.Q; s.lean_tmp_bytes = coset_group ? 0.0 : per * s.polys;   // grouped: the key's operands share the G part buffers of step 7
  uint32_t NW = 1; for (auto w : P.num_witness) NW += w;                     // instance + witness polynomials
  uint32_t max_chunk = 0; for (const auto &c : P.perm) max_chunk = std::max<uint32_t>(max_chunk, (uint32_t)c.columns.size());
  // the peak is step 7: every polynomial's coefficients + one coset part of each (the random polynomial has none), the plan's temporaries, h as Q parts and as one
  // vector; step 4 (Lagrange values + 2 + 2 chunk temporaries) and step 10 (one combination per rotation set + H, L, work, the combined quotient) stay below it when
  // the early coefficient copies of a many-column layer are counted (one more copy of every advice column).  Plus the scratch of the 2^(k + e) inverse transform,
  // the MSM workspace (~22 B per entry, up to 13 windows) and fixed overheads.
  const double parts7 = coset_group ? (double)std::min<uint32_t>(coset_group, NW - 1 + s.polys) : (double)(NW - 1);
  const double step7 = per * (NW + parts7 + s.plan_tmps + 2.0 * P.Q), step4 = per * (NW + (P.num_advice() >= 8 ? P.num_advice() : 0) + 3.0 + 2.0 * max_chunk), step10 = per * (NW + P.Q + 10.0);
  s.working_bytes = std::max(step7, std::max(step4, step10)) + per * P.Q + (double)P.n * 13 * 22 + 0.5 * 1024.0 * 1024 * 1024;
  return s;
}


// ------------------------------------------------------------------------------------------------ what stays resident
// A prover process holds several layers at once (a chunk prover the degrees {20, 24, 25}, a batch prover {21, 26} [REF bin/src/trace_prover.rs:35-36]): the
// SRS of every degree, every layer's proving key, and the working set of the ONE proof that runs.  Everything resident does not fit 288 GiB; this is the
// rule of section 7c as code.  What each optional resident buys per proof: window tables of a basis ~8 % of every commitment on it (W x the basis of HBM);
// the Q coset parts of a proving key one coset transform per polynomial and part.  So cosets are kept before tables, the subset of keys that saves the most proof time and fits (round 6; round 5: smaller keys first, so that more layers stay
// fully resident), then tables go to the Lagrange bases (they carry most commitments), the largest degree first.
// one coset transform of 2^k on an MI355X, batched (0.109 ms at 2^20, 0.228 at 2^21, 0.479 at 2^22, 2.03 at 2^24, 4.3 at 2^25, 9.0 at 2^26)
inline double coset_transform_ms(uint32_t k) {
  static const double t[7] = {0.109, 0.228, 0.479, 1.0, 2.03, 4.3, 9.0};
  return k < 20 ? 0.109 / (double)(1u << (20 - k)) : k <= 26 ? t[k - 20] : 9.0 * (double)(1u << (k - 26));
}
struct LayerResidency { const Protocol *P; PkSizes sz; bool cosets_resident = false, table_lagrange = false, table_coeff = false; };
struct ResidencyPlan { std::vector<LayerResidency> layers; double srs_gib = 0, keys_gib = 0, tables_gib = 0, working_gib = 0, total_gib = 0, budget_gib = 0; bool fits = false; };
inline ResidencyPlan plan_residency(const std::vector<const Protocol *> &protos, double hbm_gib, double reserve_fraction = 0.08, uint32_t coset_group = 0) {
  const double GiB = 1024.0 * 1024 * 1024;
  ResidencyPlan R; R.budget_gib = hbm_gib * (1.0 - reserve_fraction);
  std::set<uint32_t> degrees;
  for (const Protocol *p : protos) { LayerResidency L{p, pk_sizes(*p, coset_group)}; R.working_gib = std::max(R.working_gib, L.sz.working_bytes / GiB); degrees.insert(p->k); R.keys_gib += L.sz.base_bytes / GiB; R.layers.push_back(L); }
  for (uint32_t k : degrees) R.srs_gib += 2.0 * (double)(uint64_t(64) << k) / GiB;                       // two bases of 64-byte points
  // Which keys keep their coset parts (round 6): the subset that SAVES THE MOST PROOF TIME and fits -- a resident key saves one coset transform per polynomial, part and proof
  // (coset_transform_ms: measured, section 5).  Round 5 took "smaller keys first"; by value a chunk prover would rather keep layer 1's 80 GiB (160 transforms of 2^24 = 0.33 s)
  // than layer 0's 68.5 GiB (2 192 transforms of 2^20 = 0.24 s) -- but that plan ran OUT OF MEMORY inside layer 0's quotient on the device (288 GiB), because a lean layer 0
  // adds its recomputed part (8.6 GiB) to the LARGEST working set of the process.  So the accounting of a multi-layer process is the measured one (chunk prover: 276 GiB real):
  //   * the buffer pool keeps the high-water mark of the largest per-layer demand = that layer's blocks + (if ITS key is lean) one part's cosets, plus ~10 % that another
  //     layer's block sizes cannot reuse;
  //   * the MSM workspace and the transform scratch are sized by the LARGEST degree / extended domain of the process, whichever layer has the largest working set;
  //   * the folded coset shift keeps one table per coset factor for degrees up to 2^24 (bigger ones are only built into spare memory: lib_ntt.hip).
  // At most 7 layers: all subsets are tried.
  const size_t NL = R.layers.size();
  std::vector<double> core(NL), msm_ws(NL), ntt_scr(NL);
  double max_msm = 0, max_scr = 0, fold_tables = 0;
  for (size_t i = 0; i < NL; i++) {
    const Protocol &P = *R.layers[i].P;
    msm_ws[i] = (double)P.n * 13 * 22 / GiB; ntt_scr[i] = (double)P.n * 32 * P.Q / GiB;
    core[i] = R.layers[i].sz.working_bytes / GiB - msm_ws[i] - ntt_scr[i];
    max_msm = std::max(max_msm, msm_ws[i]); max_scr = std::max(max_scr, ntt_scr[i]);
  }
  if (NL > 1) for (uint32_t k : degrees) if (k <= 24) { uint32_t q = 0; for (const auto &L : R.layers) if (L.P->k == k) q = std::max(q, L.P->Q); fold_tables += (double)q * 36 * (double)(uint64_t(1) << k) / GiB; }
  auto demand = [&](uint32_t mask, double &mem, double &val) {          // GiB a process needs with the keys of `mask` resident; val = ms of transforms saved per round
    mem = 0; val = 0; double pool = 0;
    for (size_t i = 0; i < NL; i++) {
      const LayerResidency &L = R.layers[i];
      const bool res = mask >> i & 1;
      if (res) { mem += L.sz.coset_bytes / GiB; val += (double)L.sz.polys * L.P->Q * coset_transform_ms(L.P->k); }
      pool = std::max(pool, core[i] + (res ? 0.0 : L.sz.lean_tmp_bytes / GiB));
    }
    return (NL > 1 ? 1.10 : 1.0) * pool + max_msm + max_scr + fold_tables;
  };
  uint32_t best_mask = 0; double best_val = -1, best_mem = 0, best_work = 0;
  for (uint32_t mask = 0; mask < (1u << NL); mask++) {
    double mem, val; const double work = demand(mask, mem, val);
    if (R.srs_gib + R.keys_gib + mem + work > R.budget_gib) continue;
    if (val > best_val + 1e-9 || (val > best_val - 1e-9 && mem + work < best_mem + best_work)) { best_val = val; best_mask = mask; best_mem = mem; best_work = work; }
  }
  if (best_val < 0) { double mem, val; best_work = demand(0, mem, val); best_mem = 0; best_mask = 0; }   // not even every key lean fits: the caller sees fits == false
  for (size_t i = 0; i < NL; i++) if (best_mask >> i & 1) R.layers[i].cosets_resident = true;
  R.working_gib = best_work; R.keys_gib += best_mem;
  double used = R.srs_gib + R.keys_gib + R.working_gib;
  std::vector<uint32_t> ks(degrees.rbegin(), degrees.rend());
  for (int pass = 0; pass < 2; pass++) for (uint32_t k : ks) {
    const double t = (double)(uint64_t(64) << k) * (k >= 24 ? 12 : 15) / GiB;                               // W x 64 bytes per point
    if (used + t > R.budget_gib) continue;
    used += t; R.tables_gib += t;
    for (auto &L : R.layers) if (L.P->k == k) (pass == 0 ? L.table_lagrange : L.table_coeff) = true;
  }
  R.total_gib = used; R.fits = used <= R.budget_gib;
  return R;
}

// device_sigma: every sigma column is produced on the device by ONE mi355_fr_permutation_sigma_dev call from the copy mapping (Circuit::pairs fed through
// halo2::PermutationAssembly): no sigma column is computed or uploaded by the host.  The key (vk bytes included) is the default route's, bit for bit.
inline std::unique_ptr<ProvingKey> keygen(const Protocol &P, const Circuit &C, uint64_t h_g_lagrange, bool resident_cosets, int devices, bool device_sigma = false) {
  auto pk = std::make_unique<ProvingKey>(); pk->P = &P; pk->resident_cosets = resident_cosets; pk->devices = std::max(1, devices);
  pk->dom = std::make_unique<EvaluationDomain>(P.Q + 1, P.k);
  const EvaluationDomain &dom = *pk->dom;
  if (dom.extended_k != P.extended_k) throw std::invalid_argument("keygen: extended domain mismatch");
  const uint64_t n = P.n; const uint32_t Q = P.Q;
  auto to_coeff = [&](const DevicePoly &lag) { DevicePoly c = clone(lag, 0); check(mi355_intt_fr_dev(c.p, dom.k, dom.omega_inv.data(), dom.ifft_divisor.data())); return c; };
  auto cosets_of = [&](const DevicePoly &coeff) {
    std::vector<DevicePoly> parts;
    if (!resident_cosets) return parts;
    for (uint32_t q = 0; q < Q; q++) {
      const int slot = (int)(q % (uint32_t)pk->devices);
      DevicePoly part(n, slot); const Fr f = part_factor(dom, q);
      if (slot == 0) check(mi355_coset_ntt_fr_dev(part.p, coeff.p, dom.k, f.data(), dom.omega.data()));
      else { check(mi355_buf_copy(part.p, coeff.p, n * 32)); check(mi355_coset_ntt_fr_dev(part.p, part.p, dom.k, f.data(), dom.omega.data())); }
      parts.push_back(std::move(part));
    }
    return parts;
  };
  const std::set<uint32_t> keep = lagrange_needed(P);
  pk->pre_lagrange.resize(P.num_pre); pk->pre_coeff.resize(P.num_pre); pk->pre_cosets.resize(P.num_pre);
  pk->vk.resize(8 + 32 * (size_t)P.num_pre);
  { const uint32_t nf = P.num_pre - P.num_sigma(); for (int i = 0; i < 4; i++) { pk->vk[i] = (uint8_t)(P.k >> (24 - 8 * i)); pk->vk[4 + i] = (uint8_t)(nf >> (24 - 8 * i)); } }
  std::vector<Fr> sig;
  std::vector<DevicePoly> sig_dev;   // device_sigma: the sigma column of every permutation position
  using SigmaClock = std::chrono::steady_clock;
  auto ms_since = [](SigmaClock::time_point t0) { return std::chrono::duration<double, std::milli>(SigmaClock::now() - t0).count(); };
  if (device_sigma) {
    const uint32_t NP = (uint32_t)C.pcols.size();
    const Fr delta = NP > 1 ? C.pcols[1].delta_pow : fr_one();
    { Fr dp = fr_one(); for (uint32_t j = 0; j < NP; j++) { if (!(C.pcols[j].delta_pow == dp)) throw std::invalid_argument("keygen: the permutation's constants are not the powers of one delta"); dp = fr_mul(dp, delta); } }
    const auto t0 = SigmaClock::now();
    std::vector<uint64_t> cells, images;
    { halo2::PermutationAssembly as(NP, n); for (const auto &cp : C.pairs) as.copy(cp.ja, cp.ra, cp.jb, cp.rb); as.overrides(cells, images); }
    pk->sigma_host_prep_ms = ms_since(t0);
    std::vector<void *> ptrs;
    for (uint32_t j = 0; j < NP; j++) { sig_dev.emplace_back(n, 0); ptrs.push_back(sig_dev.back().p); }
    check(mi355_synchronize());
    const auto t1 = SigmaClock::now();
    check(mi355_fr_permutation_sigma_dev(ptrs.data(), NP, P.k, delta.data(), P.omega.data(), cells.data(), images.data(), cells.size(), 0));
    pk->sigma_ms = ms_since(t1);
  }
  for (uint32_t p = 0; p < P.num_pre; p++) {
    int j = -1; for (size_t t = 0; t < C.pcols.size(); t++) if (C.pcols[t].sigma == p) j = (int)t;
    DevicePoly lag = j >= 0 && device_sigma ? std::move(sig_dev[(size_t)j]) : DevicePoly(n, 0);
    if (j >= 0 && !device_sigma) { const auto t0 = SigmaClock::now(); C.sigma_column((uint32_t)j, sig); check(mi355_buf_upload(lag.p, sig.data(), n * 32)); pk->sigma_ms += ms_since(t0); }
    else if (j < 0) check(mi355_buf_upload(lag.p, C.pre[p].data(), n * 32));
    G1 c; check(mi355_msm_g1_dev(h_g_lagrange, 0, lag.p, n, c.data()));
    halo2::G1Affine a; std::memcpy(a.data(), c.data(), 64); const halo2::G1Bytes b = halo2::g1_to_bytes(a);
    std::memcpy(pk->vk.data() + 8 + 32 * (size_t)p, b.data(), 32);
    pk->pre_coeff[p] = to_coeff(lag);
    pk->pre_cosets[p] = cosets_of(pk->pre_coeff[p]);
    if (keep.count(p)) pk->pre_lagrange[p] = std::move(lag);
  }
  // the common polynomials: enumerate them with a structure-only compile (dummy challenges), then build each from its definition on the Lagrange domain
  { Expr id; id.kind = Expr::IDENTITY; pk->identity_common = pk->commons.id_of(id, true); }
  { Compiler cmp(pk->commons, true, std::vector<Fr>(4, fr_one())); cmp.compile_numerator(P.numerator); }
  const Fr one = fr_one();
  for (const auto &d : pk->commons.defs) {
    DevicePoly lag(n, 0); check(mi355_buf_zero(lag.p, n * 32));
    if (!fr_is_zero(d.x_coeff)) { check(mi355_synchronize()); check(mi355_buf_upload(lag.at(1), d.x_coeff.data(), 32)); check(mi355_ntt_fr_dev(lag.p, dom.k, dom.omega.data())); }   // x_coeff X -> x_coeff omega^row
    if (!fr_is_zero(d.constant)) {
      const void *pp[1] = {lag.p}; const Fr cs[2] = {one, d.constant}; const uint32_t tl[2] = {1, 0}, fp[1] = {0}; const int32_t fr_[1] = {0};
      gate_eval(lag.p, pp, 1, cs, tl, 2, fp, fr_, n, 0);
    }
    for (const auto &sp : d.lagrange) {
      const uint64_t row = (uint64_t)(((int64_t)sp.first % (int64_t)n + (int64_t)n) % (int64_t)n);
      Fr cur; check(mi355_buf_download(cur.data(), lag.at(row), 32)); cur = fr_add(cur, sp.second); check(mi355_buf_upload(lag.at(row), cur.data(), 32));
    }
    pk->common_coeff.push_back(to_coeff(lag));
    pk->common_cosets.push_back(cosets_of(pk->common_coeff.back()));
    pk->common_lagrange.push_back(std::move(lag));
  }
  for (size_t i = 0; i < pk->common_lagrange.size(); i++) if (i != pk->identity_common) pk->common_lagrange[i].release();   // step 4 reads X only
  check(mi355_synchronize());
  const PkSizes sz = pk_sizes(P);
  pk->bytes = (uint64_t)(sz.base_bytes + (resident_cosets ? sz.coset_bytes : 0));
  return pk;
}

// ------------------------------------------------------------------------------------------------ what check_witness and create_proof share
namespace detail {
struct Joiner { std::vector<std::thread> th; void join() { for (auto &t : th) if (t.joinable()) t.join(); } ~Joiner() { join(); } };   // every thread is joined on every path

// Items 0 .. items - 1 on `stripes` host threads, worker w taking w, w + stripes, ...: how witness columns cross the link.  Every worker runs ITS OWN COPY of `item`, so what
// `item` captures by value is that worker's scratch.  A worker stops at its first exception; the first one of all is kept in `error`, and `failed()` runs under `mu` right
// after it is stored.  With `caller_works`, stripe 0 runs on the calling thread before start() returns.
struct StripedUploader {
  std::mutex mu; std::string error; Joiner workers;
  template <class Item, class Failed> void start(size_t items, size_t stripes, bool caller_works, Item item, Failed failed) {
    auto worker = [this, items, stripes, item, failed](size_t w) mutable {
      try { for (size_t i = w; i < items; i += stripes) item(i); }
      catch (const std::exception &e) { std::lock_guard<std::mutex> lk(mu); if (error.empty()) error = e.what(); failed(); }
    };
    for (size_t w = caller_works ? 1 : 0; w < stripes; w++) workers.th.emplace_back(worker, w);
    if (caller_works) worker(0);
  }
  void join() { workers.join(); }
};

// dst = (accumulate ? dst : 0) + sum_i coeffs[i] ptrs[i], one launch of the fused kernel (at most PLAN_MAX_TERMS polynomials)
inline void linear_combination(void *dst, const std::vector<const void *> &ptrs, const std::vector<Fr> &coeffs, uint64_t n, bool accumulate) {
  const uint32_t m = (uint32_t)ptrs.size(); std::vector<uint32_t> tl(m, 1), fp(m); std::vector<int32_t> rot(m, 0);
  for (uint32_t i = 0; i < m; i++) fp[i] = i;
  gate_eval(dst, ptrs.data(), m, coeffs.data(), tl.data(), m, fp.data(), rot.data(), n, accumulate ? 1 : 0);
}

// Plans that run on the Lagrange domain, rotations in rows: step 3's device route and step 4 of create_proof, and check_witness.  Owns the compiler, the pool of
// temporaries and the launch loop.  `column` gives the witness and instance polynomials; the key's own come from its kept Lagrange values.  Where the key kept none, a
// prover step fails under its name (`step`); with step == nullptr (check_witness) they come back from the coefficients by a forward transform into scratch, once.
struct LagrangePlan {
  static constexpr uint32_t RESULT_BASE = 1u << 20;   // ids of result temporaries (check_witness judges a batch of them in one call), above every id the compiler hands out
  const ProvingKey &pk; const uint64_t n; const char *step; std::function<const void *(uint32_t)> column;
  Compiler cmp; std::vector<DevicePoly> tmp, result; std::map<Atom, DevicePoly> scratch; uint32_t launches = 0;
  LagrangePlan(const ProvingKey &pk_, const char *step_, std::vector<Fr> challenges, std::function<const void *(uint32_t)> column_)
      : pk(pk_), n(pk_.P->n), step(step_), column(std::move(column_)), cmp(const_cast<CommonRegistry &>(pk_.commons), false, std::move(challenges)) {}
  DevicePoly &tmp_at(uint32_t i) { while (tmp.size() <= i) tmp.emplace_back(n, 0); return tmp[i]; }
  void *dst(uint32_t id) { return id >= RESULT_BASE ? result.at(id - RESULT_BASE).p : tmp_at(id).p; }
  const void *key_lagrange(const Atom &a) {
    if (step && a.kind == A_COMMON && a.idx != pk.identity_common) throw std::invalid_argument(std::string(step) + " reads no common polynomial but X");
    const DevicePoly &kept = a.kind == A_COMMON ? pk.common_lagrange[a.idx] : pk.pre_lagrange[a.idx];
    if (kept.p) return kept.p;
    if (step) throw std::invalid_argument(std::string(step) + (a.kind == A_COMMON ? ": Lagrange values of X were not kept" : ": Lagrange values of a preprocessed polynomial were not kept"));
    auto it = scratch.find(a);
    if (it == scratch.end()) { DevicePoly c = clone(pk.coeff(a), 0); check(mi355_ntt_fr_dev(c.p, pk.dom->k, pk.dom->omega.data())); it = scratch.emplace(a, std::move(c)).first; }
    return it->second.p;
  }
  const void *resolve(const Atom &a) { return a.kind == A_TMP ? dst(a.idx) : a.kind == A_COMMON || pk.P->is_pre(a.idx) ? key_lagrange(a) : column(a.idx); }
  void run() {   // everything compiled so far, in order
    for (const auto &L : cmp.out) { run_launch(L, dst((uint32_t)L.dst), n, fr_one(), L.accumulate, [this](const Atom &a) { return resolve(a); }); launches++; }
    cmp.out.clear();
  }
  // The challenges later compiles read.  The compiler keeps nothing of a compile but its pending launches, and run() has drained those: the only state to replace is the list
  void set_challenges(std::vector<Fr> challenges) { if (!cmp.out.empty()) throw std::logic_error("LagrangePlan: challenges changed with launches pending"); cmp.ch = std::move(challenges); }
  // TMP 0 = the lookup's table, TMP 1 = its input, both compressed with theta (challenge 0)
  void compress_lookup(const Lookup &lk) { cmp.tmp_base = 2; cmp.tmp_next = 0; cmp.emit(0, cmp.compile(*lk.table)); cmp.emit(1, cmp.compile(*lk.input)); run(); }
  // m = how often each of TMP 0's usable rows is looked up by TMP 1's; an input cell that is not in the table comes back as (any, input, row), the smallest one
  struct Missing { bool any; uint32_t input; uint64_t row; };
  Missing multiplicities(void *m, uint64_t usable, uint32_t rule) {
    const void *inputs[1] = {tmp_at(1).p}; uint64_t missing = ~uint64_t(0);
    const int rc = mi355_fr_lookup_multiplicities_dev(m, n, tmp_at(0).p, usable, inputs, 1, usable, rule, &missing);
    if (rc == MI355_EBADARG && missing != ~uint64_t(0)) return {true, (uint32_t)(missing >> 40), missing & ((uint64_t(1) << 40) - 1)};
    check(rc); return {false, 0, 0};
  }
};
}  // namespace detail

// ------------------------------------------------------------------------------------------------ check_witness
// halo2_proofs::dev::MockProver::verify for a PlonkProtocol, on the device [EXT-recalled halo2_proofs src/dev.rs, MockProver::verify: gate, lookup and permutation
// failures]; the reference runs it on every trace before proving [REF integration/src/mock.rs:16-24], [REF bin/src/prove_utils.rs:54-55,81-88].  create_proof takes any
// witness and a wrong cell only shows as a proof the verifier rejects; this names the constraint and the row.
//   gates     every constraint i of the numerator the recogniser classifies as a gate (Protocol::gates), compiled ON ITS OWN, without powers of y, into a temporary on
//             the Lagrange domain (rotations in rows, as step 4 runs the plan), and held to zero on ALL n rows -- what divisibility by X^n - 1 needs; a superset of
//             MockProver's usable rows (selectors are zero on the blinding rows).  Temporaries are judged a batch at a time by one mi355_fr_nonzero_rows_dev call.
//             Fixed / common polynomials whose Lagrange values the key does not keep (lagrange_needed) come back from their coefficients by a forward transform into
//             scratch, lazily and only those.  index = the constraint's position in the numerator's list (the protocol file's numbering).
//   copies    Circuit::pairs through halo2::PermutationAssembly, as keygen(..., device_sigma = true) feeds them; the columns in permutation position order (advice,
//             instance, fixed: Lagrange values); one mi355_fr_copy_check_dev call.  index = t in the override lists; both cells decoded.
//   lookups   table and input compressed with a theta drawn from theta_seed (the builder's splitmix stream, nonzero), then mi355_fr_lookup_multiplicities_dev into a
//             scratch m over the usable rows, as step 3's device_multiplicities route.  Two different tuples compress to one value for at most (columns - 1) of the r
//             choices of theta: a tuple mismatch escapes with probability at most (columns - 1) / r.  The entry point reports only the SMALLEST missing (input, row),
//             so a lookup yields at most one failure (count = 1, col_a = the input index the entry point names: 0, the one compressed column).
// The argument polynomials' own constraints (z, phi) are not checked: they hold by construction once copies and lookups do.  The check uploads the advice and instance
// columns itself and frees everything it allocated before it returns.
struct VerifyFailure { enum Kind { Gate, Copy, Lookup } kind; uint32_t index; uint64_t row; uint64_t count; uint32_t col_a, col_b; uint64_t row_b; };
struct CheckOptions { int threads = 8 /* host threads; one upload thread per four */; uint32_t cap = 16 /* failures reported per gate / for the copies; counts stay full */; uint64_t theta_seed = 1; };
inline const char *failure_kind_name(VerifyFailure::Kind k) { return k == VerifyFailure::Gate ? "gate" : k == VerifyFailure::Copy ? "copy" : "lookup"; }
inline std::string describe(const VerifyFailure &f) {
  if (f.kind == VerifyFailure::Gate) return "gate constraint " + std::to_string(f.index) + " fails at row " + std::to_string(f.row) + " (" + std::to_string(f.count) + " rows in all)";
  if (f.kind == VerifyFailure::Copy) return "copy constraint " + std::to_string(f.index) + " fails: permutation column " + std::to_string(f.col_a) + " row " + std::to_string(f.row) + " differs from column " +
                                            std::to_string(f.col_b) + " row " + std::to_string(f.row_b) + " (" + std::to_string(f.count) + " pairs in all)";
  return "lookup " + std::to_string(f.index) + ": input row " + std::to_string(f.row) + " is not in the table";
}
struct WitnessError : std::runtime_error {
  std::vector<VerifyFailure> failures;
  explicit WitnessError(std::vector<VerifyFailure> f) : std::runtime_error("witness check: " + describe(f.at(0)) + (f.size() > 1 ? "; " + std::to_string(f.size()) + " failures reported" : std::string())), failures(std::move(f)) {}
};
inline std::vector<VerifyFailure> check_witness(const ProvingKey &pk, const Circuit &wit, const CheckOptions &opt) {
  const Protocol &P = *pk.P;
  const uint64_t n = P.n, u = P.usable; const uint32_t A = P.num_advice(), NL = (uint32_t)P.lookups.size();
  if (wit.advice.size() != A) throw std::invalid_argument("check_witness: the witness has " + std::to_string(wit.advice.size()) + " advice columns, the protocol " + std::to_string(A));
  if (wit.instances.size() > n) throw std::invalid_argument("check_witness: more instance values than rows");
  std::vector<VerifyFailure> out;
  // ---- the witness crosses the link
  std::vector<DevicePoly> adv(A); DevicePoly inst(n, 0);
  check(mi355_buf_zero(inst.p, n * 32));
  if (!wit.instances.empty()) check(mi355_buf_upload(inst.p, wit.instances.data(), wit.instances.size() * 32));
  {
    const size_t UT = (size_t)std::max(1, std::min<int>(std::min(3, opt.threads / 4), (int)A));
    detail::StripedUploader up;
    up.start(A, UT, true, [&](size_t i) {
      if (wit.advice[i].size() != n) throw std::invalid_argument("advice column " + std::to_string(i) + " is not n rows");
      DevicePoly d(n, 0); check(mi355_buf_upload(d.p, wit.advice[i].data(), n * 32)); adv[i] = std::move(d);
    }, [] {});
    up.join();
    if (!up.error.empty()) throw Error(MI355_EHIP, "check_witness: witness upload: " + up.error);
  }
  // ---- operands: Lagrange values; what the key holds as coefficients only comes back by a forward transform, once, when first named (LagrangePlan::key_lagrange)
  detail::LagrangePlan plan(pk, nullptr, {}, [&](uint32_t poly) -> const void * {   // no challenge is drawn before the gates: one that names a challenge is no gate of a one-phase circuit
    if (P.is_instance(poly)) return inst.p;
    if (poly >= P.phase0[0] && poly < P.phase0[0] + A) return adv[poly - P.phase0[0]].p;
    throw std::invalid_argument("check_witness: polynomial " + std::to_string(poly) + " is neither fixed, instance nor advice");
  });
  Compiler &cmp = plan.cmp;
  // ---- gates: batches of temporaries, one synchronisation per batch
  {
    const uint32_t B = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, (uint64_t(1) << 28) / n));   // 8 GiB of temporaries at most
    const size_t NG = P.gates.size();
    for (size_t g0 = 0; g0 < NG; g0 += B) {
      const uint32_t nb = (uint32_t)std::min<size_t>(B, NG - g0);
      while (plan.result.size() < nb) plan.result.emplace_back(n, 0);
      std::vector<const void *> ptrs(nb);
      for (uint32_t b = 0; b < nb; b++) {
        cmp.tmp_base = 0; cmp.tmp_next = 0;
        cmp.emit((int)(detail::LagrangePlan::RESULT_BASE + b), cmp.compile(*P.gates[g0 + b].expr));
        plan.run();
        ptrs[b] = plan.result[b].p;
      }
      const halo2::NonzeroRows r = halo2::nonzero_rows(ptrs, n, opt.cap);
      for (uint32_t b = 0; b < nb; b++) {
        const uint32_t index = (uint32_t)(P.gates[g0 + b].expr - P.numerator.kids.data());
        for (uint32_t s = 0; s < opt.cap && r.rows_of(b)[s] != ~uint64_t(0); s++) out.push_back({VerifyFailure::Gate, index, r.rows_of(b)[s], r.counts[b], 0, 0, 0});
        if (opt.cap == 0 && r.counts[b]) out.push_back({VerifyFailure::Gate, index, ~uint64_t(0), r.counts[b], 0, 0, 0});   // counts only: the row is not known
      }
    }
    plan.result.clear(); plan.tmp.clear();
  }
  // ---- copy constraints
  {
    const uint32_t NP = (uint32_t)wit.pcols.size();
    std::vector<uint64_t> cells, images;
    { halo2::PermutationAssembly as(NP, n); for (const auto &cp : wit.pairs) as.copy(cp.ja, cp.ra, cp.jb, cp.rb); as.overrides(cells, images); }
    std::vector<const void *> cols(NP); for (uint32_t j = 0; j < NP; j++) cols[j] = plan.resolve(Atom{A_POLY, wit.pcols[j].column, 0});
    if (NP) {
      const halo2::CopyCheck r = halo2::copy_check(cols, P.k, cells, images, opt.cap);
      const uint64_t mask = n - 1;
      for (uint32_t s = 0; s < opt.cap && r.failed_t[s] != ~uint64_t(0); s++) {
        const uint64_t t = r.failed_t[s], c = cells[t], im = images[t];
        out.push_back({VerifyFailure::Copy, (uint32_t)t, c & mask, r.n_failed, (uint32_t)(c >> P.k), (uint32_t)(im >> P.k), im & mask});
      }
      if (opt.cap == 0 && r.n_failed) out.push_back({VerifyFailure::Copy, ~0u, ~uint64_t(0), r.n_failed, 0, 0, 0});
    }
  }
  // ---- lookups, under a theta of the check's own
  if (NL) {
    detail::Rng rng(opt.theta_seed); Fr theta = rng.uniform(); while (fr_is_zero(theta)) theta = rng.uniform();
    plan.set_challenges({theta});
    DevicePoly m(n, 0);
    for (uint32_t l = 0; l < NL; l++) {
      plan.compress_lookup(P.lookups[l]);
      const auto miss = plan.multiplicities(m.p, u, 0);
      if (miss.any) out.push_back({VerifyFailure::Lookup, l, miss.row, 1, miss.input, 0, 0});
    }
  }
  check(mi355_synchronize());
  return out;
}

// ------------------------------------------------------------------------------------------------ create_proof
struct ProofOptions { int devices = 1; int threads = 8; uint32_t commit_batch = 0 /* 0: by column count */; int upload_threads = 1; int early_intt = -1 /* -1: by column count */;
                      bool sparse_uploads = false /* columns that are at least half zeros cross PCIe as (index, value) pairs */;
                      bool packed_multiplicities = false /* the lookup multiplicities cross PCIe as the 4-byte counts they are (mi355_buf_upload_packed); their blinding rows follow as 32-byte words */;
                      bool device_multiplicities = false /* step 3 computes the multiplicity columns on the device after theta (mi355_fr_lookup_multiplicities_dev), as the scroll fork's
                                                            mv_lookup prover does on the CPU: the caller's `m` columns are not read (they may be empty), only Circuit::m_blind */;
                      bool multiplicity_rule_last = false /* with device_multiplicities: a repeated table value's count goes to its LAST usable row (default: the first) */;
                      bool check_witness = false /* run plonk::check_witness on the witness first and throw WitnessError (the failures, the first one named in the message) before anything is written to the
                                                    transcript.  The check does its own upload, so the witness crosses the link twice; sharing the prover's uploads is not done */;
                      bool device_randomness = false /* the prover's randomness is drawn on the device from rng_key (mi355_fr_random_dev / _rows_dev, the stream table below): the random
                                                        polynomial is not uploaded and Circuit::random_poly, m_blind, z_blind, phi_blind and the blinding rows of Circuit::advice / m are not read */;
                      uint8_t rng_key[32] = {0} /* the ChaCha20 key of this proof's draws.  One key per proof: a (key, stream, counter) triple must never serve two proofs */;
                      bool rng_key_from_os = false /* with device_randomness: the key is filled from getrandom(2) inside create_proof (rng_key is not read); a failure throws */;
                      uint32_t coset_group_polys = 0 /* 0: step 7 transforms one coset part of EVERY polynomial the plan reads before it runs the part's launches.  G >= PLAN_MAX_POLYS: the
                                                        launches run in consecutive groups whose operands number at most G (detail::coset_groups), each group behind ONE batched transform of its
                                                        operands into a pool of G part buffers; an operand a later group needs again is transformed again (ProofResult::coset_retransforms).  Same proof bytes */;
                      TranscriptKind transcript = TranscriptKind::ByLayer /* the reference's choice for the protocol's layer (reference_transcript below): Poseidon for 0-5, Evm for 6; or name one */; };
// the transcript the reference proves a layer with: Poseidon for every proof the next layer verifies in-circuit (layers 0-5, [REF integration/src/prove.rs:30-43,67,95-97] -> snark-verifier-sdk
// gen_snark_shplonk), Keccak in the EVM layout for layer 6 (gen_evm_proof_shplonk: what the released verifier contract reads).  Files without a layer number are the reference's fixtures (layers 2, 4).
inline TranscriptKind reference_transcript(const Protocol &P) { return P.layer == 6 ? TranscriptKind::Evm : TranscriptKind::Poseidon; }
// The first scalar of the transcript.  A verifier built from a PlonkProtocol (snark-verifier's PlonkVerifier, the next layer's in-circuit verifier, the EVM contract) absorbs the
// protocol's `transcript_initial_state`, never the key's bytes -- so when the protocol file carries one (the reference's own files do) the prover MUST start from it, or its
// proof cannot pass that verifier whatever else is right.  Protocols generated here carry none (halo2 derives it by hashing a Rust Debug string of the
// pinned key, which does not exist outside Rust): for those keys the scalar is a convention of this repository, the Blake2b hash of the .vkey bytes (vk_transcript_repr).
inline Fr vk_transcript_scalar(const Protocol &P, const std::vector<uint8_t> &vk_bytes) { return P.has_initial_state ? P.initial_state : vk_transcript_repr(vk_bytes); }
inline const char *transcript_name(TranscriptKind k) { return k == TranscriptKind::Poseidon ? "poseidon" : k == TranscriptKind::Evm ? "evm" : "blake2b"; }
// The streams ProofOptions::device_randomness draws from.  Element (stream, block index) = halo2::fr_random_reference(rng_key, stream, block index); blind = Protocol::blind,
// the rows u + 1 .. n - 1 of a column (j = row - u - 1).  A caller -- and every test -- can recompute each value on the CPU from the key alone.
//   stream                     what                                                    block index
//   RNG_STREAM_RANDOM_POLY  0  random polynomial of step 5, coefficient i              i
//   RNG_STREAM_ADVICE_BLIND 1  advice column a (protocol order), blinding row j        a * blind + j
//   RNG_STREAM_M_BLIND      2  multiplicity column of lookup l, blinding row j         l * blind + j
//   RNG_STREAM_Z_BLIND      3  permutation product z of chunk c, blinding value j      c * blind + j
//   RNG_STREAM_PHI_BLIND    4  lookup sum phi of lookup l, blinding value j            l * blind + j
constexpr uint64_t RNG_STREAM_RANDOM_POLY = 0, RNG_STREAM_ADVICE_BLIND = 1, RNG_STREAM_M_BLIND = 2, RNG_STREAM_Z_BLIND = 3, RNG_STREAM_PHI_BLIND = 4;
struct ProofResult {
  std::vector<uint8_t> proof;
  double step_ms[11] = {0}; double total_ms = 0;
  uint64_t peak_hbm_bytes = 0, hbm_total_bytes = 0;
  uint64_t sparse_columns = 0, packed_columns = 0, witness_link_bytes = 0;
  double random_ms = 0;         // device_randomness: the random polynomial's block, its draw and the wait for it (an upper bound of the draw's device time), plus the host time of the blinding-row launches
  double multiplicity_ms = 0;   // device_multiplicities: compression, counting and blinding rows of every lookup (host wall time, the commitments excluded)
  uint32_t coset_groups = 0 /* groups of launches per coset part (0: the ungrouped route) */, coset_retransforms = 0 /* coset transforms beyond one per operand and part; counted in coset_ntt too */;
  uint32_t msm = 0, intt = 0, coset_ntt = 0, gate_launches = 0, evals = 0, plan_launches = 0, plan_terms = 0, plan_tmps = 0, plan_constraints = 0, plan_prefix_groups = 0, rotation_sets = 0;
};

namespace detail {
// coefficients (low first) of the polynomial of degree < m through (points[i], values[i]); m <= 8, host arithmetic
inline std::vector<Fr> interpolate(const std::vector<Fr> &pts, const std::vector<Fr> &vals) {
  const size_t m = pts.size(); std::vector<Fr> out(m, fr_zero());
  for (size_t i = 0; i < m; i++) {
    std::vector<Fr> num{fr_one()}; Fr den = fr_one();
    for (size_t j = 0; j < m; j++) {
      if (j == i) continue;
      std::vector<Fr> nx(num.size() + 1, fr_zero());
      for (size_t t = 0; t < num.size(); t++) { nx[t + 1] = fr_add(nx[t + 1], num[t]); nx[t] = fr_sub(nx[t], fr_mul(pts[j], num[t])); }
      num.swap(nx); den = fr_mul(den, fr_sub(pts[i], pts[j]));
    }
    const Fr s = fr_mul(vals[i], fr_inv(den));
    for (size_t t = 0; t < num.size(); t++) out[t] = fr_add(out[t], fr_mul(s, num[t]));
  }
  return out;
}
inline Fr horner(const std::vector<Fr> &c, const Fr &x) { Fr acc = fr_zero(); for (size_t i = c.size(); i-- > 0;) acc = fr_add(fr_mul(acc, x), c[i]); return acc; }
inline std::vector<Fr> powers(const Fr &b, size_t m) { std::vector<Fr> p(m, fr_one()); for (size_t i = 1; i < m; i++) p[i] = fr_mul(p[i - 1], b); return p; }

// SHPLONK's scalar side: host arithmetic, no device call.  points[i] = the opening points of rotation set i, in the order of its rotations.  It comes in two parts because
// the transcript sits between them (u is drawn after the commitment to H, and H needs the remainders), and the first runs set by set, under the device's work on that set.
//   remainder      of one set: R = sum_j ys^j r_j, r_j = the polynomial of degree < |rots| through the evaluations of the set's j-th polynomial (coefficients, low first)
//   linearisation  L = sum_i v^i zd_i (A_i - R_i(u)) - Z_T(u) H, scaled by 1 / zd_0, with zd_i = prod (u - point) over the points set i does not open at and Z_T over
//                  every point: the coefficient of each A_i, the one of H, and the constant that is subtracted.  L(u) = 0
inline std::vector<Fr> shplonk_remainder(const RotationSet &s, const std::vector<Fr> &points, const std::map<PolyRot, Fr> &evals, const Fr &ys) {
  std::vector<Fr> sum(s.rots.size(), fr_zero()); Fr yp = fr_one();
  for (uint32_t p : s.polys) {
    std::vector<Fr> vals; for (int32_t r : s.rots) vals.push_back(evals.at({p, r}));
    const std::vector<Fr> rj = interpolate(points, vals);
    for (size_t t = 0; t < sum.size(); t++) sum[t] = fr_add(sum[t], fr_mul(yp, rj[t]));
    yp = fr_mul(yp, ys);
  }
  return sum;
}
struct ShplonkLinearisation { std::vector<Fr> a; Fr h, constant; };
inline ShplonkLinearisation shplonk_linearisation(const std::vector<std::vector<Fr>> &points, const std::vector<std::vector<Fr>> &rem, const Fr &v, const Fr &u) {
  const size_t M = points.size();
  std::vector<Fr> super; for (size_t i = 0; i < M; i++) for (const auto &pt : points[i]) if (std::find(super.begin(), super.end(), pt) == super.end()) super.push_back(pt);
  Fr zt = fr_one(); for (const auto &pt : super) zt = fr_mul(zt, fr_sub(u, pt));
  const std::vector<Fr> vpow = powers(v, M);
  std::vector<Fr> lc(M); Fr zd0 = fr_one(), cst = fr_zero();
  for (size_t i = 0; i < M; i++) {
    Fr zd = fr_one(); for (const auto &pt : super) if (std::find(points[i].begin(), points[i].end(), pt) == points[i].end()) zd = fr_mul(zd, fr_sub(u, pt));
    if (i == 0) zd0 = zd;
    lc[i] = fr_mul(vpow[i], zd); cst = fr_add(cst, fr_mul(lc[i], horner(rem[i], u)));
  }
  const Fr zi = fr_inv(zd0);
  ShplonkLinearisation out; for (size_t i = 0; i < M; i++) out.a.push_back(fr_mul(lc[i], zi));
  out.h = fr_neg(fr_mul(zt, zi)); out.constant = fr_mul(cst, zi);
  return out;
}

// Commitments into the transcript.  One rule for a group of finished polynomials (steps 4 and 8): on small domains one batched pass whatever the count (one reduction tail
// per batch); big ones keep one commitment per pass -- a batch of two at 2^24 doubles the sorter's workspace (8.8 GB) for no gain, and a multi-layer prover process has no
// HBM to spare.
struct Committer {
  Transcript &T; uint32_t &msm; const uint64_t n;
  static bool small_domain(uint64_t n) { return n <= (uint64_t(1) << 22); }
  void commit_one(uint64_t basis, const void *ptr) { G1 out; check(mi355_msm_g1_dev(basis, 0, ptr, n, out.data())); msm++; T.write_point(out); }
  void commit_many(uint64_t basis, const std::vector<const void *> &ptrs, uint32_t cap) {   // batched passes of at most `cap`
    for (size_t base = 0; base < ptrs.size(); base += cap) {
      const uint32_t cnt = (uint32_t)std::min<size_t>(cap, ptrs.size() - base); std::vector<G1> outs(cnt);
      check(mi355_msm_g1_batch_dev(basis, 0, ptrs.data() + base, cnt, n, outs.data())); msm += cnt;
      for (const auto &o : outs) T.write_point(o);
    }
  }
  void commit_group(uint64_t basis, const std::vector<const void *> &ptrs, bool batched, uint32_t cap) { if (batched) commit_many(basis, ptrs, cap); else for (const void *p : ptrs) commit_one(basis, p); }
  // columns of `poly` committed in the order of `refs`, at most `cap` per pass (cap 1: single commitments): wait(i) returns once refs[i] is on the device, done(pass) runs
  // after each pass with the columns it committed
  template <class Wait, class Done> void commit_in_batches(uint64_t basis, const std::map<uint32_t, DevicePoly> &poly, const std::vector<uint32_t> &refs, uint32_t cap, Wait wait, Done done) {
    std::vector<uint32_t> pass;
    for (size_t i = 0; i < refs.size(); i++) {
      wait(i); pass.push_back(refs[i]);
      if (pass.size() < cap && i + 1 < refs.size()) continue;
      if (cap == 1) commit_one(basis, poly.at(pass[0]).p);
      else { std::vector<const void *> ptrs; for (uint32_t r : pass) ptrs.push_back(poly.at(r).p); commit_many(basis, ptrs, cap); }
      done(pass); pass.clear();
    }
  }
};

// ProofOptions::coset_group_polys: the compiled quotient plan cut into consecutive runs of launches.  Walking the plan in order, a run is closed as soon as the next launch would
// take the union of the run's non-temporary operands past G -- witness polynomials and, with a lean key (`lean`: the key's coset parts are not resident), the key's and the common
// polynomials.  Temporaries live across groups and do not count.  One launch names at most PLAN_MAX_POLYS operands, so any G >= PLAN_MAX_POLYS cuts any plan; a smaller G is
// refused.  Greedy and order-preserving on purpose: the plan's order is what makes temporaries valid, and the arithmetic is exact, so any cut gives the same quotient.
constexpr uint32_t COSET_GROUP_ALL = 0xffffffffu;
struct CosetGroup { size_t first, last; std::vector<uint32_t> witness; std::vector<Atom> key; };   // launches [first, last) of the plan; the operands to transform, ascending
struct CosetGrouping { std::vector<CosetGroup> groups; uint32_t distinct = 0 /* operands of the whole plan */, retransforms = 0 /* members of all groups beyond `distinct`, per coset part */, max_witness = 0, max_key = 0; };
inline CosetGrouping coset_groups(const Protocol &P, const std::vector<Launch> &plan, uint32_t G, bool lean) {
  if (G < PLAN_MAX_POLYS) throw std::invalid_argument("coset_group_polys must be 0 or at least " + std::to_string(PLAN_MAX_POLYS) + " (one launch may name that many operands)");
  CosetGrouping R; std::set<Atom> all, cur; size_t first = 0;
  auto close = [&](size_t last) {
    CosetGroup g{first, last, {}, {}};
    for (const auto &a : cur) { if (a.kind == A_POLY && !P.is_pre(a.idx)) g.witness.push_back(a.idx); else g.key.push_back(a); }
    R.max_witness = std::max<uint32_t>(R.max_witness, (uint32_t)g.witness.size()); R.max_key = std::max<uint32_t>(R.max_key, (uint32_t)g.key.size());
    R.retransforms += (uint32_t)cur.size(); R.groups.push_back(std::move(g)); cur.clear(); first = last;
  };
  for (size_t l = 0; l < plan.size(); l++) {
    std::set<Atom> next = cur;
    for (const auto &t : plan[l].terms) for (const auto &f : t.f) {
      if (f.kind == A_TMP) continue;
      const bool key = f.kind == A_COMMON || P.is_pre(f.idx);
      if (!key || lean) { next.insert(Atom{f.kind, f.idx, 0}); all.insert(Atom{f.kind, f.idx, 0}); }
    }
    if (next.size() > G && l > first) { close(l); l--; continue; }   // the launch opens the next group
    cur.swap(next);
  }
  if (first < plan.size() || R.groups.empty()) close(plan.size());
  R.distinct = (uint32_t)all.size(); R.retransforms -= R.distinct;
  return R;
}
// the largest G whose part buffers fit `bytes_for_parts` (what the caller can spare for step 7's coset parts): 0 = no grouping needed, everything fits; never below PLAN_MAX_POLYS
inline uint32_t suggest_coset_group(const Protocol &P, bool lean, double bytes_for_parts) {
  const PkSizes sz = pk_sizes(P); uint32_t NW = 1; for (auto w : P.num_witness) NW += w;
  const double per = (double)P.n * 32; const uint32_t all = NW - 1 + (lean ? sz.polys : 0);
  if (bytes_for_parts >= per * all) return 0;
  return std::max<uint32_t>(PLAN_MAX_POLYS, (uint32_t)std::max(0.0, bytes_for_parts / per));
}

// The state of one proof; the steps are SURVEY 3.2's, numbered as the replay record's step_ms and rust_shim/create_proof_resident.rs number them.
struct ProofRun {
  using Clock = std::chrono::steady_clock;
  static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
  const uint64_t h_g, h_g_lagrange; const ProvingKey &pk; const Circuit &wit; const ProofOptions &opt; const Protocol &P; const EvaluationDomain &dom;
  const uint32_t k, Q; const uint64_t n, u; const uint32_t A, NL, NZ; const int D; const bool permuted /* the classic lookup argument: steps 3 and 4 make A', S' and the lookups' z */, dev_m, dev_rng;
  const uint32_t batch_cap; const bool batch_cols, early_intt;   // steps 2 and 3: commitments per pass as the columns arrive; their coefficient copies made pass by pass
  ProofResult R; const Clock::time_point t_start; Clock::time_point tl; Transcript T; Committer C;
  halo2::RngKey rng_key; std::vector<Fr> ch; Fr x;
  std::map<uint32_t, DevicePoly> poly;          // protocol index -> Lagrange values until step 6, coefficients afterwards
  std::map<uint32_t, DevicePoly> coeff_early;   // coefficient copies made while the witness still arrives; step 6 moves them into `poly`
  DevicePoly inst_lagrange;                     // the instance column's Lagrange values, from step 1's transform until step 4 has read them
  DevicePoly h;                                 // the quotient: Q pieces of n coefficients, from step 7 on
  std::map<PolyRot, Fr> evals;
  // the witness crosses PCIe on other host threads (rayon workers in the real caller): arrived[i] is set, under up.mu, when uploads[i] is in `poly`
  std::vector<std::pair<uint32_t, const Column *>> uploads; std::vector<char> arrived; std::condition_variable cv; size_t UT = 1;
  std::atomic<uint64_t> sparse_cols{0}, packed_cols{0}, link_bytes{0};
  StripedUploader up;                           // declared last: its threads are joined before anything they touch goes away

  ProofRun(uint64_t h_g_, uint64_t h_g_lagrange_, const ProvingKey &pk_, const Circuit &wit_, const ProofOptions &opt_)
      : h_g(h_g_), h_g_lagrange(h_g_lagrange_), pk(pk_), wit(wit_), opt(opt_), P(*pk_.P), dom(*pk_.dom), k(P.k), Q(P.Q), n(P.n), u(P.usable), A(P.num_advice()), NL((uint32_t)P.lookups.size()),
        NZ((uint32_t)P.perm.size()), D(std::max(1, std::min<int>(opt_.devices, (int)Q))), permuted(P.permuted_lookups()), dev_m(opt_.device_multiplicities && NL > 0 && !permuted), dev_rng(opt_.device_randomness),
        batch_cap(opt_.commit_batch ? opt_.commit_batch : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(32, (uint64_t(1) << 25) / n))), batch_cols(A >= 16 && batch_cap > 1),
        early_intt(opt_.early_intt < 0 ? A >= 8 : opt_.early_intt != 0), t_start(Clock::now()), tl(t_start),
        T(opt_.transcript == TranscriptKind::ByLayer ? reference_transcript(P) : opt_.transcript), C{T, R.msm, n} {
    T.common_scalar(vk_transcript_scalar(P, pk.vk));
    for (const auto &v : wit.instances) T.common_scalar(v);
    std::memcpy(rng_key.data(), opt.rng_key, 32);
    if (dev_rng && opt.rng_key_from_os) {
      for (size_t got = 0; got < 32;) { const ssize_t r = getrandom(rng_key.data() + got, 32 - got, 0); if (r < 0) { if (errno == EINTR) continue; throw Error(MI355_EHIP, "create_proof: getrandom failed (errno " + std::to_string(errno) + "): no key for the device randomness"); } got += (size_t)r; }
    }
  }
  void lap(int step) { R.step_ms[step] += ms_since(tl); tl = Clock::now(); }
  void squeeze_challenges(uint32_t count) { for (uint32_t i = 0; i < count; i++) ch.push_back(T.squeeze_challenge()); }
  const void *coeff_ptr(uint32_t p) const { return P.is_pre(p) ? pk.pre_coeff.at(p).p : poly.at(p).p; }
  Fr rot_point(int32_t rot) const { return fr_mul(x, rot_power(dom.omega, dom.omega_inv, rot)); }
  uint32_t commit_pass() const { return opt.commit_batch ? opt.commit_batch : 32; }   // commitments per batched pass of a finished group
  // rows [u + 1, n) of a group of resident columns (all on one device) in ONE launch; column i of the group draws the blocks i * blind + j of `stream`
  void draw_blinding(const std::vector<uint32_t> &refs, uint64_t stream) {
    if (!P.blind || refs.empty()) return;
    const auto t0 = Clock::now();
    std::vector<void *> cols; for (uint32_t r : refs) cols.push_back(poly.at(r).p);
    halo2::fr_random_rows(cols, u + 1, P.blind, rng_key, stream, 0);
    R.random_ms += ms_since(t0);
  }
  void wait_for(size_t i) { std::unique_lock<std::mutex> lk(up.mu); cv.wait(lk, [&] { return arrived[i] != 0; }); if (!up.error.empty()) throw Error(MI355_EHIP, "witness upload: " + up.error); }
  void to_coeff_early(const std::vector<uint32_t> &refs) {
    if (!early_intt) return;
    std::vector<void *> ptrs;
    for (uint32_t r : refs) { DevicePoly c = clone(poly.at(r), 0); ptrs.push_back(c.p); coeff_early[r] = std::move(c); }
    check(mi355_ntt_fr_batch_dev(ptrs.data(), (uint32_t)ptrs.size(), k, dom.omega_inv.data(), dom.ifft_divisor.data())); R.intt += (uint32_t)ptrs.size();
  }
  // one phase's columns, committed in order: uploads[lo, hi) as they arrive, or columns made on the device
  template <class Wait> void commit_columns(const std::vector<uint32_t> &refs, Wait wait) {
    C.commit_in_batches(h_g_lagrange, poly, refs, batch_cols ? batch_cap : 1, wait, [this](const std::vector<uint32_t> &pass) { to_coeff_early(pass); });
  }
  void commit_uploaded(size_t lo, size_t hi) { std::vector<uint32_t> refs; for (size_t i = lo; i < hi; i++) refs.push_back(uploads[i].first); commit_columns(refs, [this, lo](size_t i) { wait_for(lo + i); }); }

  // uploads[i] crosses the link in the cheapest form its content allows; sidx / svals: the calling worker's scratch for the sparse form
  void upload_column(size_t i, std::vector<uint32_t> &sidx, std::vector<Fr> &svals) {
    // device_randomness: the block exists already and its rows [u + 1, n) are being drawn; rows [0, u + 1) cross the link.  The two regions are disjoint
    const uint64_t len = dev_rng ? u + 1 : uploads[i].second->size();
    if (uploads[i].second->size() < len) throw std::invalid_argument("create_proof: a witness column has fewer than the usable rows + 1");
    DevicePoly d = dev_rng ? std::move(poly.at(uploads[i].first)) : DevicePoly(len, 0);
    uint64_t nz = len;
    if (opt.sparse_uploads && len >= (1u << 12) && uploads[i].first != P.random_poly) {
      sidx.resize(len); svals.resize(len);
      check(mi355_host_compact_nonzero(uploads[i].second->data(), len, sidx.data(), svals.data(), &nz, std::max(1, opt.threads / (int)UT)));
    }
    const bool is_m = uploads[i].first >= P.phase0[1] && uploads[i].first < P.phase0[1] + NL;
    if (opt.packed_multiplicities && is_m && wit.m_counts.size() == NL) {
      // a column whose KIND bounds its cells: counts below 2^32 on the rows up to l_last, then the prover's blinding values
      check(mi355_buf_upload_packed(d.p, wit.m_counts[uploads[i].first - P.phase0[1]].data(), len, 4));
      if (P.blind && !dev_rng) check(mi355_buf_upload(d.at(u + 1), uploads[i].second->data() + (u + 1), P.blind * 32));
      packed_cols++; link_bytes += len * 4 + (dev_rng ? 0 : P.blind * 32);
    }
    else if (2 * nz <= len) { check(mi355_buf_upload_sparse(d.p, len, sidx.data(), svals.data(), nz)); sparse_cols++; link_bytes += nz * 36; }
    else { check(mi355_buf_upload(d.p, uploads[i].second->data(), len * 32)); link_bytes += len * 32; }
    { std::lock_guard<std::mutex> lk(up.mu); poly.at(uploads[i].first) = std::move(d); arrived[i] = 1; }
    cv.notify_all();
  }

  // ---- steps 1-3: the uploads start; commitments as the columns arrive; theta; the multiplicities; beta, gamma
  void witness_commits() {
    for (uint32_t i = 0; i < A; i++) uploads.push_back({P.phase0[0] + i, &wit.advice[i]});
    if (!dev_m && !permuted) for (uint32_t l = 0; l < NL; l++) uploads.push_back({P.phase0[1] + l, &wit.m[l]});
    if (!dev_rng) uploads.push_back({P.random_poly, &wit.random_poly});                   // step 5's polynomial (coefficients): needed last, crosses last
    for (const auto &up_ : uploads) poly[up_.first];
    poly[P.random_poly];
    poly[P.inst0];
    for (uint32_t l = 0; l < P.num_witness[1]; l++) poly[P.phase0[1] + l];
    for (const auto &c : P.perm) poly[c.z];                                               // every entry exists before the uploaders start: the map's structure does not change under them
    for (const auto &l : P.lookups) poly[l.permuted ? l.z : l.phi];
    {                                                                                     // step 1's input, made NOW: the instance column (public values, zero below).  Its few words must
      // cross PCIe before the uploader threads fill the copy stream: that stream is first-in first-out, and queued behind the witness this 1 KiB upload waited for the random polynomial
      // of step 5 (2 GiB at k = 26) -- 33 ms of host time in step 1 of every k = 26 proof until round 6 (17 ms at k = 25).  No device-wide synchronisation either: mi355_buf_upload
      // orders itself behind the zeroing of its block, and the compute stream behind the copy.
      DevicePoly inst(n, 0); check(mi355_buf_zero(inst.p, n * 32));
      if (!wit.instances.empty()) check(mi355_buf_upload(inst.p, wit.instances.data(), wit.instances.size() * 32));
      poly.at(P.inst0) = std::move(inst);
    }
    if (dev_rng) {                                                                        // the blocks of every uploaded column, their blinding rows drawn: one launch per kind of column
      std::vector<uint32_t> adv, ms;
      for (size_t i = 0; i < uploads.size(); i++) { poly.at(uploads[i].first) = DevicePoly(n, 0); (i < A ? adv : ms).push_back(uploads[i].first); }
      draw_blinding(adv, RNG_STREAM_ADVICE_BLIND); draw_blinding(ms, RNG_STREAM_M_BLIND);
    }
    arrived.assign(uploads.size(), 0);
    UT = (size_t)std::max(1, std::min<int>(opt.upload_threads, (int)uploads.size()));
    up.start(uploads.size(), UT, false, [this, sidx = std::vector<uint32_t>(), svals = std::vector<Fr>()](size_t i) mutable { upload_column(i, sidx, svals); },
             [this] { std::fill(arrived.begin(), arrived.end(), 1); cv.notify_all(); });
    commit_uploaded(0, A);                                                                // step 2
    squeeze_challenges(P.num_challenge[0]);                                               // theta
    if (permuted) device_permuted_columns();                                              // step 3 of the classic lookup argument: A' and S' exist only on the device
    else if (!dev_m) commit_uploaded(A, A + NL);                                          // step 3 (the multiplicities are the caller's: they do not depend on theta for the lookups halo2 compresses)
    else device_multiplicities();
    squeeze_challenges(P.num_challenge[1]);                                               // beta, gamma
  }
  // step 3 as the scroll fork's mv_lookup prover runs it [EXT-recalled halo2_proofs src/plonk/mv_lookup/prover.rs, `prepare`]: table and input compressed with theta (the
  // expressions of step 4 without the beta term, into TMP 0 / 1), every input cell of the usable rows looked up in the table's usable rows on the device, the rng's blinding
  // values into the last rows.  The instance column still holds its Lagrange values here (step 1's inverse transform comes after step 3).  Commitments as step 2 makes them.
  void device_multiplicities() {
    const auto t_m = Clock::now();
    std::vector<uint32_t> made;
    {
      LagrangePlan plan(pk, "step 3", ch, [this](uint32_t p) { return poly.at(p).p; });   // advice (committed in step 2) or the instance column (Lagrange values)
      for (uint32_t l = 0; l < NL; l++) {
        plan.compress_lookup(P.lookups[l]);
        DevicePoly m(n, 0);
        const auto miss = plan.multiplicities(m.p, u, opt.multiplicity_rule_last ? 1u : 0u);
        if (miss.any) throw Error(MI355_EBADARG, describe(VerifyFailure{VerifyFailure::Lookup, l, miss.row, 1, miss.input, 0, 0}));
        if (P.blind && !dev_rng) check(mi355_buf_upload(m.at(u + 1), wit.m_blind[l].data(), P.blind * 32));
        { std::lock_guard<std::mutex> lk(up.mu); poly.at(P.phase0[1] + l) = std::move(m); }
        made.push_back(P.phase0[1] + l);
      }
      if (dev_rng) draw_blinding(made, RNG_STREAM_M_BLIND);
      R.gate_launches += plan.launches;
    }                                                                                     // the temporaries go before the commitments
    R.multiplicity_ms = ms_since(t_m);
    commit_columns(made, [](size_t) {});
  }
  // step 3 of upstream halo2's classic lookup argument [EXT-recalled halo2_proofs src/plonk/lookup/prover.rs, `commit_permuted`]: input and table compressed with theta as above,
  // the permuted columns A' and S' built on the device over the usable rows (mi355_fr_lookup_permute_dev), the rng's blinding values into the rows from the l_last row on
  // (blind + 1 per column: unlike a grand product, the l_last row is random too), A' then S' committed per lookup.  There is no host route and the circuit carries no column.
  void device_permuted_columns() {
    const auto t_m = Clock::now();
    std::vector<uint32_t> made;
    {
      LagrangePlan plan(pk, "step 3", ch, [this](uint32_t p) { return poly.at(p).p; });
      const uint64_t tail = (uint64_t)P.blind + 1;
      for (uint32_t l = 0; l < NL; l++) {
        const Lookup &lk = P.lookups[l];
        plan.compress_lookup(lk);
        DevicePoly a(n, 0), s(n, 0);
        uint64_t missing = ~uint64_t(0);
        const int rc = mi355_fr_lookup_permute_dev(a.p, s.p, plan.tmp_at(1).p, plan.tmp_at(0).p, u, &missing);
        if (rc == MI355_EBADARG && missing != ~uint64_t(0)) throw Error(MI355_EBADARG, describe(VerifyFailure{VerifyFailure::Lookup, l, missing, 1, 0, 0, 0}));
        check(rc);
        check(mi355_buf_upload(a.at(u), wit.perm_blind.at(l).data(), tail * 32));
        check(mi355_buf_upload(s.at(u), wit.perm_blind.at(l).data() + tail, tail * 32));
        { std::lock_guard<std::mutex> lk_(up.mu); poly.at(lk.perm_input) = std::move(a); poly.at(lk.perm_table) = std::move(s); }
        made.push_back(lk.perm_input); made.push_back(lk.perm_table);
      }
      R.gate_launches += plan.launches;
    }                                                                                     // the temporaries go before the commitments
    R.multiplicity_ms = ms_since(t_m);
    commit_columns(made, [](size_t) {});
  }
  // ---- step 1's transform: the instance column to coefficients; step 4 still reads its Lagrange values
  void instance_to_coefficients() {
    inst_lagrange = clone(poly.at(P.inst0), 0);
    check(mi355_intt_fr_dev(poly.at(P.inst0).p, k, dom.omega_inv.data(), dom.ifft_divisor.data())); R.intt++;
  }
  // ---- step 4: grand products and running sums, built on the device from the Lagrange values
  void products_and_sums() {
    const Fr beta = ch.at(1), gamma = ch.at(2);
    std::vector<uint32_t> made;
    {
      LagrangePlan plan(pk, "step 4", ch, [this](uint32_t p) { return P.is_instance(p) ? inst_lagrange.p : poly.at(p).p; });
      Compiler &cmp = plan.cmp;
      Fr carry = fr_one();
      for (uint32_t c = 0; c < NZ; c++) {
        const PermChunk &chunk = P.perm[c]; const uint32_t cl = (uint32_t)chunk.columns.size();
        SoP us{Term{fr_one(), {}}}, vs{Term{fr_one(), {}}};
        cmp.tmp_base = 2; cmp.tmp_next = 0;
        for (uint32_t j = 0; j < cl; j++) {
          const PermColumn &pc = chunk.columns[j];
          SoP uj{Term{fr_one(), {Atom{A_POLY, pc.column, 0}}}, Term{fr_mul(beta, pc.delta_pow), {Atom{A_COMMON, pk.identity_common, 0}}}, Term{gamma, {}}};
          SoP vj{Term{fr_one(), {Atom{A_POLY, pc.column, 0}}}, Term{beta, {Atom{A_POLY, pc.sigma, 0}}}, Term{gamma, {}}};
          us = cmp.product(std::move(us), cmp.materialize(uj)); vs = cmp.product(std::move(vs), cmp.materialize(vj));
        }
        cmp.emit(0, us); cmp.emit(1, vs);                                                  // TMP[0] = prod_j u_j, TMP[1] = prod_j v_j
        plan.run();
        check(mi355_fr_batch_invert_dev(plan.tmp_at(1).p, n));
        check(mi355_fr_vec_op_dev(2, plan.tmp_at(0).p, plan.tmp_at(0).p, plan.tmp_at(1).p, n));
        DevicePoly z(n, 0);
        check(mi355_fr_prefix_product_dev(z.p, plan.tmp_at(0).p, n, nullptr));             // z[0] = 1, z[i + 1] = z[i] prod u / prod v
        if (c > 0) check(mi355_fr_vec_axpy_dev(z.p, nullptr, z.p, carry.data(), n));       // chunk c starts where chunk c - 1 ended: z_c(1) = z_(c-1)(w^last)
        if (c + 1 < NZ) check(mi355_buf_download(carry.data(), z.at(u), 32));
        if (P.blind && !dev_rng) check(mi355_buf_upload(z.at(u + 1), wit.z_blind.at(c).data(), P.blind * 32));
        poly.at(chunk.z) = std::move(z); made.push_back(chunk.z);
      }
      if (dev_rng) draw_blinding(made, RNG_STREAM_Z_BLIND);
      for (uint32_t l = 0; l < NL; l++) {                                                 // phi[i + 1] = phi[i] + 1 / (I + beta) - m / (T + beta)
        const Lookup &lk = P.lookups[l];
        cmp.tmp_base = 4; cmp.tmp_next = 0;
        if (lk.permuted) {                                                                // z[0] = 1, z[i + 1] = z[i] (A + beta)(S + gamma) / ((A' + beta)(S' + gamma))
          SoP ab = cmp.compile(*lk.input); ab.push_back(Term{beta, {}}); Compiler::merge_scalars(ab);
          SoP sb = cmp.compile(*lk.table); sb.push_back(Term{gamma, {}}); Compiler::merge_scalars(sb);
          cmp.emit(0, ab); cmp.emit(1, sb);
          const Atom t0{A_TMP, 0, 0}, t1{A_TMP, 1, 0}, ap{A_POLY, lk.perm_input, 0}, sp{A_POLY, lk.perm_table, 0};
          cmp.emit(2, SoP{Term{fr_one(), {t0, t1}}});
          cmp.emit(3, SoP{Term{fr_one(), {ap, sp}}, Term{gamma, {ap}}, Term{beta, {sp}}, Term{fr_mul(beta, gamma), {}}});
          plan.run();
          check(mi355_fr_batch_invert_dev(plan.tmp_at(3).p, n));
          check(mi355_fr_vec_op_dev(2, plan.tmp_at(2).p, plan.tmp_at(2).p, plan.tmp_at(3).p, n));
          DevicePoly z(n, 0);
          check(mi355_fr_prefix_product_dev(z.p, plan.tmp_at(2).p, n, nullptr));
          Fr end{}; check(mi355_buf_download(end.data(), z.at(u), 32));                   // the product over the usable rows: one for columns that are permutations of the input and the table
          if (!(end == fr_one())) throw Error(MI355_EBADARG, "create_proof: lookup " + std::to_string(l) + ": the grand product of the permuted columns does not return to one");
          if (P.blind) check(mi355_buf_upload(z.at(u + 1), wit.lz_blind.at(l).data(), P.blind * 32));
          poly.at(lk.z) = std::move(z); made.push_back(lk.z);
          continue;
        }
        SoP tb = cmp.compile(*lk.table); tb.push_back(Term{beta, {}}); Compiler::merge_scalars(tb);
        SoP ib = cmp.compile(*lk.input); ib.push_back(Term{beta, {}}); Compiler::merge_scalars(ib);
        cmp.emit(0, tb); cmp.emit(1, ib);
        const Atom t0{A_TMP, 0, 0}, t1{A_TMP, 1, 0}, mm{A_POLY, lk.m, 0};
        cmp.emit(2, SoP{Term{fr_one(), {t0, t1}}});
        cmp.emit(3, SoP{Term{fr_one(), {t0}}, Term{fr_neg(fr_one()), {mm, t1}}});
        plan.run();
        check(mi355_fr_batch_invert_dev(plan.tmp_at(2).p, n));
        check(mi355_fr_vec_op_dev(2, plan.tmp_at(3).p, plan.tmp_at(3).p, plan.tmp_at(2).p, n));
        DevicePoly phi(n, 0);
        check(mi355_fr_prefix_sum_dev(phi.p, plan.tmp_at(3).p, n, nullptr));
        if (P.blind && !dev_rng) check(mi355_buf_upload(phi.at(u + 1), wit.phi_blind.at(l).data(), P.blind * 32));
        poly.at(lk.phi) = std::move(phi); made.push_back(lk.phi);
      }
      if (dev_rng) draw_blinding(std::vector<uint32_t>(made.begin() + NZ, made.end()), RNG_STREAM_PHI_BLIND);
      std::vector<const void *> ptrs; for (uint32_t r : made) ptrs.push_back(poly.at(r).p);
      C.commit_group(h_g_lagrange, ptrs, made.size() >= 8 || Committer::small_domain(n), commit_pass());
      R.gate_launches += plan.launches;
      inst_lagrange.release();
    }                                                                                     // step 4's temporaries go before step 5
  }
  // ---- step 5: the random polynomial of the vanishing argument: one commitment on the coefficient basis, one evaluation later, no transform
  void random_polynomial() {
    if (!uploads.empty()) wait_for(uploads.size() - 1);
    up.join();
    if (dev_rng) {                                                                        // drawn where it lives: nothing crosses the link.  Waited for, so that random_ms holds the draw
      const auto t0 = Clock::now();                                                         // (with the block's allocation and whatever the stream still held; the commitment below waits anyway)
      DevicePoly rp(n, 0); rp.random(rng_key, RNG_STREAM_RANDOM_POLY, 0); check(mi355_synchronize());
      poly.at(P.random_poly) = std::move(rp);
      R.random_ms += ms_since(t0);
    }
    C.commit_one(h_g, poly.at(P.random_poly).p);
    squeeze_challenges(P.num_challenge[2]);                                               // y
  }
  // ---- step 6: every witness polynomial to coefficients, one batched call
  void to_coefficients() {
    std::vector<void *> ptrs;
    for (auto &kv : poly) if (kv.first != P.inst0 && kv.first != P.random_poly && !coeff_early.count(kv.first)) ptrs.push_back(kv.second.p);
    if (!ptrs.empty()) check(mi355_ntt_fr_batch_dev(ptrs.data(), (uint32_t)ptrs.size(), k, dom.omega_inv.data(), dom.ifft_divisor.data()));
    R.intt += (uint32_t)ptrs.size();
    for (auto &kv : coeff_early) poly.at(kv.first) = std::move(kv.second);
    coeff_early.clear();
  }
  // ---- step 7: the quotient, coset part by coset part; part q on device q % D (the proving key's cosets of that part live there).  Everything but h goes before step 8.
  // ProofOptions::coset_group_polys = G runs a part's launches in the groups of detail::coset_groups: G part buffers instead of one per polynomial the plan reads
  void quotient() {
    h = DevicePoly(Q * n, 0);
    Compiler cmp(const_cast<CommonRegistry &>(pk.commons), false, ch);
    cmp.compile_numerator(P.numerator);
    R.plan_launches = (uint32_t)cmp.out.size(); R.plan_terms = cmp.terms_total; R.plan_tmps = cmp.tmps_used(); R.plan_constraints = cmp.constraints; R.plan_prefix_groups = cmp.prefix_groups;
    std::set<uint32_t> wset; std::set<Atom> pkset;
    for (const auto &L : cmp.out) for (const auto &t : L.terms) for (const auto &f : t.f) { if (f.kind == A_POLY && !P.is_pre(f.idx)) wset.insert(f.idx); else if (f.kind != A_TMP) pkset.insert(Atom{f.kind, f.idx, 0}); }
    const std::vector<uint32_t> wrefs(wset.begin(), wset.end()); const uint32_t NP = (uint32_t)wrefs.size();
    std::vector<std::map<uint32_t, DevicePoly>> part_on(D), coeff_on(D); std::vector<std::map<Atom, DevicePoly>> pkpart_on(D);
    std::vector<std::vector<DevicePoly>> tmp_on(D); std::vector<DevicePoly> hq_on(D);
    std::vector<DevicePoly> hpart; for (uint32_t q = 0; q < Q; q++) hpart.emplace_back(n, 0);
    // coset_group_polys: the part buffers are a pool per device, as many as the largest group needs (at most G in all); no per-polynomial part, no coefficient copies on the other devices
    const bool grouped = opt.coset_group_polys != 0;
    CosetGrouping CG; std::vector<std::vector<DevicePoly>> wpool(D), kpool(D);
    if (grouped) { CG = coset_groups(P, cmp.out, opt.coset_group_polys, !pk.resident_cosets); R.coset_groups = (uint32_t)CG.groups.size(); R.coset_retransforms = CG.retransforms * Q; }
    for (int d = 0; d < D; d++) {
      if (!grouped) for (uint32_t r : wrefs) part_on[d][r] = DevicePoly(n, d);
      else { for (uint32_t i = 0; i < CG.max_witness; i++) wpool[d].emplace_back(n, d); for (uint32_t i = 0; i < CG.max_key; i++) kpool[d].emplace_back(n, d); }
      tmp_on[d].resize(cmp.tmp_max);
      for (const auto &L : cmp.out) if (L.dst >= 0 && !tmp_on[d][(size_t)L.dst].p) tmp_on[d][(size_t)L.dst] = DevicePoly(n, d);   // only the ids the plan writes
      if (d > 0) { hq_on[d] = DevicePoly(n, d); if (!grouped) for (uint32_t r : wrefs) { coeff_on[d][r] = DevicePoly(n, d); check(mi355_buf_copy(coeff_on[d][r].p, poly.at(r).p, n * 32)); } }
    }
    std::vector<std::string> errs(D); std::vector<int> codes(D, MI355_EHIP); std::vector<uint32_t> launches(D, 0), cosets(D, 0);
    // one coset part by groups: per group ONE batched transform of its operands (witness and, lean, key) into the pool, then its launches; the temporaries and the part's
    // accumulator carry over from group to group.  Everything of a device runs on its compute stream, which orders the reuse of a pool buffer behind the launches that read it
    auto grouped_part = [&](int d, uint32_t q) {
      const Fr factor = part_factor(dom, q);
      const Fr tq_inv = fr_inv(fr_sub(fr_pow(factor, n), fr_one()));
      void *hq = d == 0 ? hpart[q].p : hq_on[d].p;
      bool first = true;
      for (const CosetGroup &grp : CG.groups) {
        std::map<uint32_t, const void *> wat; std::map<Atom, const void *> kat;
        std::vector<void *> dst; std::vector<const void *> src;
        auto stage = [&](void *buf, const void *coeff) {   // another device: the coefficients are copied into the part buffer first, then transformed in place
          if (d != 0) { check(mi355_buf_copy(buf, coeff, n * 32)); coeff = buf; }
          dst.push_back(buf); src.push_back(coeff);
        };
        for (size_t i = 0; i < grp.witness.size(); i++) { void *b = wpool[d].at(i).p; stage(b, poly.at(grp.witness[i]).p); wat[grp.witness[i]] = b; }
        for (size_t i = 0; i < grp.key.size(); i++) { void *b = kpool[d].at(i).p; stage(b, pk.coeff(grp.key[i]).p); kat[grp.key[i]] = b; }
        if (!dst.empty()) check(mi355_coset_ntt_fr_batch_dev(dst.data(), src.data(), (uint32_t)dst.size(), k, factor.data(), dom.omega.data()));
        cosets[d] += (uint32_t)dst.size();
        auto resolve = [&](const Atom &a) -> const void * {
          if (a.kind == A_TMP) return tmp_on[d].at(a.idx).p;
          if (a.kind == A_COMMON || P.is_pre(a.idx)) { const DevicePoly *c = pk.coset(a, q); return c ? c->p : kat.at(a); }
          return wat.at(a.idx);
        };
        for (size_t l = grp.first; l < grp.last; l++) {
          const Launch &L = cmp.out[l];
          if (L.dst >= 0) run_launch(L, tmp_on[d].at((size_t)L.dst).p, n, fr_one(), L.accumulate, resolve);
          else { run_launch(L, hq, n, tq_inv, !first, resolve); first = false; }
          launches[d]++;
        }
      }
      if (d != 0) check(mi355_buf_copy(hpart[q].p, hq, n * 32));
    };
    auto do_parts = [&](int d) {
      try {
        for (uint32_t q = (uint32_t)d; q < Q; q += (uint32_t)D) {
          if (grouped) { grouped_part(d, q); continue; }
          const Fr factor = part_factor(dom, q);
          std::vector<void *> dst(NP); std::vector<const void *> src(NP);
          for (uint32_t i = 0; i < NP; i++) { dst[i] = part_on[d].at(wrefs[i]).p; src[i] = d == 0 ? poly.at(wrefs[i]).p : coeff_on[d].at(wrefs[i]).p; }
          check(mi355_coset_ntt_fr_batch_dev(dst.data(), src.data(), NP, k, factor.data(), dom.omega.data())); cosets[d] += NP;
          if (!pk.resident_cosets) {   // the HBM-lean proving key: this part's cosets are recomputed from the coefficients, in ONE batched call (round 6: a lean many-column key
            std::vector<void *> kd; std::vector<const void *> ks;   // used to issue one transform per polynomial -- 2 192 single 2^20 launches per layer-0 proof)
            for (const auto &a : pkset) {
              auto it = pkpart_on[d].find(a); if (it == pkpart_on[d].end()) it = pkpart_on[d].emplace(a, DevicePoly(n, d)).first;
              if (d != 0) check(mi355_buf_copy(it->second.p, pk.coeff(a).p, n * 32));   // another device: copy first, then in place
              kd.push_back(it->second.p); ks.push_back(d == 0 ? pk.coeff(a).p : it->second.p);
            }
            if (!kd.empty()) check(mi355_coset_ntt_fr_batch_dev(kd.data(), ks.data(), (uint32_t)kd.size(), k, factor.data(), dom.omega.data()));
            cosets[d] += (uint32_t)kd.size();
          }
          auto resolve = [&](const Atom &a) -> const void * {
            if (a.kind == A_TMP) return tmp_on[d].at(a.idx).p;
            if (a.kind == A_COMMON || P.is_pre(a.idx)) { const DevicePoly *c = pk.coset(a, q); return c ? c->p : pkpart_on[d].at(a).p; }
            return part_on[d].at(a.idx).p;
          };
          // 1 / ((zeta w_ext^q)^n - 1): the vanishing polynomial is constant on a coset part; it rides on the coefficients
          const Fr tq_inv = fr_inv(fr_sub(fr_pow(factor, n), fr_one()));
          void *hq = d == 0 ? hpart[q].p : hq_on[d].p;
          bool first = true;
          for (const auto &L : cmp.out) {
            if (L.dst >= 0) run_launch(L, tmp_on[d].at((size_t)L.dst).p, n, fr_one(), L.accumulate, resolve);
            else { run_launch(L, hq, n, tq_inv, !first, resolve); first = false; }
            launches[d]++;
          }
          if (d != 0) check(mi355_buf_copy(hpart[q].p, hq, n * 32));
        }
      } catch (const Error &e) { errs[d] = e.what(); codes[d] = e.code; }   // the library's own code travels on: MI355_EOOM under a memory limit stays MI355_EOOM
      catch (const std::exception &e) { errs[d] = e.what(); }
    };
    { Joiner others; for (int d = 1; d < D; d++) others.th.emplace_back(do_parts, d); do_parts(0); others.join(); }
    for (int d = 0; d < D; d++) { if (!errs[d].empty()) throw Error(codes[d], "quotient part on device slot " + std::to_string(d) + ": " + errs[d]); R.gate_launches += launches[d]; R.coset_ntt += cosets[d]; }
    { std::vector<const void *> pp(Q); for (uint32_t q = 0; q < Q; q++) pp[q] = hpart[q].p; check(mi355_fr_interleave_dev(h.p, pp.data(), Q, n)); }
    check(mi355_extended_to_coeff_dev(h.p, dom.extended_k, dom.g_coset.data(), dom.g_coset_inv.data(), dom.extended_omega_inv.data(), dom.extended_ifft_divisor.data()));
  }
  // ---- step 8: the Q pieces of h, on small domains in one batched pass (at k = 20 / 21 one reduction tail instead of Q); x
  void commit_quotient() {
    std::vector<const void *> ptrs(Q); for (uint32_t q = 0; q < Q; q++) ptrs[q] = h.at((uint64_t)q * n);
    C.commit_group(h_g, ptrs, Committer::small_domain(n), Q);
    x = T.squeeze_challenge();
  }
  // ---- step 9: the evaluations, in the protocol's order; plus the Q pieces at x (for the combined quotient's value)
  void evaluations() {
    std::vector<const void *> ptrs; std::vector<Fr> pts;
    for (const auto &e : P.evaluations) { ptrs.push_back(coeff_ptr(e.poly)); pts.push_back(rot_point(e.rot)); }
    for (uint32_t q = 0; q < Q; q++) { ptrs.push_back(h.at((uint64_t)q * n)); pts.push_back(x); }
    std::vector<Fr> ev(ptrs.size());
    check(mi355_eval_polynomial_batch_dev(ptrs.data(), (uint32_t)ptrs.size(), n, pts.data(), ev.data()));
    for (size_t i = 0; i < P.evaluations.size(); i++) { evals[P.evaluations[i]] = ev[i]; T.write_scalar(ev[i]); }
    R.evals = (uint32_t)P.evaluations.size();
    const std::vector<Fr> xnpow = powers(fr_pow(x, n), Q); Fr hx = fr_zero();
    for (uint32_t q = 0; q < Q; q++) hx = fr_add(hx, fr_mul(xnpow[q], ev[P.evaluations.size() + q]));
    evals[{P.quotient_poly, 0}] = hx;
  }
  // ---- step 10: SHPLONK
  void shplonk() {
    // the vanishing argument opens ONE combined quotient polynomial h_0 + x^n h_1 + ...
    DevicePoly hcomb(n, 0);
    { std::vector<const void *> pp(Q); for (uint32_t q = 0; q < Q; q++) pp[q] = h.at((uint64_t)q * n); linear_combination(hcomb.p, pp, powers(fr_pow(x, n), Q), n, false); R.gate_launches++; }
    const Fr ys = T.squeeze_challenge(), v = T.squeeze_challenge();
    const std::vector<RotationSet> sets = rotation_sets(P.queries); const size_t M = sets.size(); R.rotation_sets = (uint32_t)M;
    std::vector<std::vector<Fr>> points(M);
    for (size_t i = 0; i < M; i++) for (int32_t r : sets[i].rots) points[i].push_back(rot_point(r));
    std::vector<std::vector<Fr>> rem; std::vector<DevicePoly> Acomb;
    DevicePoly H(n, 0), work(n, 0); check(mi355_buf_zero(H.p, n * 32));
    Fr vpow_i = fr_one();
    for (size_t i = 0; i < M; i++) {
      const RotationSet &s = sets[i]; const size_t np = s.polys.size(), m = s.rots.size();
      // A_i = sum_j y^j P_ij (the j-th polynomial of a set carries y^j: what the reference's released proofs satisfy, tests/test_plonk_protocol.py::test_reference_released_proofs_verify),
      // and the same combination of the interpolated remainders (m coefficients, on the host, while the device works on A_i)
      const std::vector<Fr> ypow = powers(ys, np);
      DevicePoly Ai(n, 0);
      for (size_t base = 0; base < np; base += 16) {
        const size_t cnt = std::min<size_t>(16, np - base);
        std::vector<const void *> pp(cnt); for (size_t j = 0; j < cnt; j++) pp[j] = s.polys[base + j] == P.quotient_poly ? hcomb.p : coeff_ptr(s.polys[base + j]);
        linear_combination(Ai.p, pp, std::vector<Fr>(ypow.begin() + (long)base, ypow.begin() + (long)(base + cnt)), n, base != 0); R.gate_launches++;
      }
      rem.push_back(shplonk_remainder(s, points[i], evals, ys));
      // N_i = A_i - R_i: only the lowest m coefficients change; then N_i / prod (X - point), one kate_division per point, in place (shifting up by one each time)
      check(mi355_buf_copy(work.p, Ai.p, n * 32));
      { std::vector<Fr> low(m); check(mi355_buf_download(low.data(), work.p, m * 32)); for (size_t t = 0; t < m; t++) low[t] = fr_sub(low[t], rem[i][t]); check(mi355_buf_upload(work.p, low.data(), m * 32)); }
      for (size_t t = 0; t < m; t++) check(mi355_fr_kate_division_dev(work.at(t + 1), work.at(t), n - t, points[i][t].data()));
      // H += v^i Q_i (the i-th rotation set carries v^i); Q_i has n - m coefficients at work[m ..]
      check(mi355_fr_vec_axpy_dev(H.p, H.p, work.at(m), vpow_i.data(), n - m));
      vpow_i = fr_mul(vpow_i, v);
      Acomb.push_back(std::move(Ai));
    }
    C.commit_one(h_g, H.p);
    const Fr uu = T.squeeze_challenge();
    const ShplonkLinearisation lin = shplonk_linearisation(points, rem, v, uu);
    DevicePoly Lx(n, 0);
    {
      if (M + 1 > PLAN_MAX_TERMS) throw std::invalid_argument("SHPLONK: more than 15 rotation sets");
      std::vector<const void *> pp; for (size_t i = 0; i < M; i++) pp.push_back(Acomb[i].p);
      pp.push_back(H.p); std::vector<Fr> cs = lin.a; cs.push_back(lin.h);
      linear_combination(Lx.p, pp, cs, n, false); R.gate_launches++;
      Fr l0; check(mi355_buf_download(l0.data(), Lx.p, 32)); l0 = fr_sub(l0, lin.constant); check(mi355_buf_upload(Lx.p, l0.data(), 32));
    }
    check(mi355_buf_zero(work.p, n * 32));
    check(mi355_fr_kate_division_dev(work.p, Lx.p, n, uu.data()));                       // n - 1 coefficients, the top one stays zero
    C.commit_one(h_g, work.p);
  }
  ProofResult result() {
    R.total_ms = ms_since(t_start);
    R.proof = std::move(T.proof); R.sparse_columns = sparse_cols.load(); R.packed_columns = packed_cols.load(); R.witness_link_bytes = link_bytes.load();
    { uint64_t fr_ = 0, tot = 0; check(mi355_mem_info(0, &fr_, &tot, nullptr, nullptr, nullptr)); R.peak_hbm_bytes = tot - fr_; R.hbm_total_bytes = tot; }
    return std::move(R);
  }
};
}  // namespace detail

inline ProofResult create_proof(uint64_t h_g, uint64_t h_g_lagrange, const ProvingKey &pk, const Circuit &wit, const ProofOptions &opt) {
  const Protocol &P = *pk.P;
  // resident coset parts were placed by keygen at q % pk.devices: the gate kernel on device d must find part q on d, so the proof runs on the key's device count
  // (a differing opt.devices would read a coset that sits on another device)
  if (pk.resident_cosets && pk.devices != std::max(1, opt.devices)) throw std::invalid_argument("create_proof: ProofOptions::devices (" + std::to_string(opt.devices) + ") differs from the proving key's (" + std::to_string(pk.devices) + ") while its coset parts are resident");
  if (opt.coset_group_polys != 0 && opt.coset_group_polys < PLAN_MAX_POLYS) throw std::invalid_argument("create_proof: ProofOptions::coset_group_polys must be 0 or at least " + std::to_string(PLAN_MAX_POLYS));
  if (P.permuted_lookups()) {   // the classic lookup argument: A', S' and the lookups' z are made on the device; what the circuit carries is their blinding values
    if (opt.device_randomness) throw std::invalid_argument("create_proof: ProofOptions::device_randomness is not available for a protocol with the classic (permuted) lookup argument");
    if (std::max(1, opt.devices) > 1) throw std::invalid_argument("create_proof: ProofOptions::devices > 1 is not available for a protocol with the classic (permuted) lookup argument");
    if (wit.perm_blind.size() != P.lookups.size() || wit.lz_blind.size() != P.lookups.size()) throw std::invalid_argument("create_proof: the classic lookup argument needs the blinding values of every lookup (Circuit::perm_blind, Circuit::lz_blind)");
    for (size_t l = 0; l < P.lookups.size(); l++) if (wit.perm_blind[l].size() != 2 * ((size_t)P.blind + 1) || wit.lz_blind[l].size() != P.blind) throw std::invalid_argument("create_proof: Circuit::perm_blind holds 2 x (blind + 1) words per lookup and Circuit::lz_blind blind words");
  }
  if (opt.check_witness) { CheckOptions co; co.threads = opt.threads; std::vector<VerifyFailure> bad = check_witness(pk, wit, co); if (!bad.empty()) throw WitnessError(std::move(bad)); }
  detail::ProofRun run(h_g, h_g_lagrange, pk, wit, opt);                                // the clock starts; the transcript takes the key's scalar and the instance values
  if (run.dev_rng) for (uint32_t i = 0; i < run.A; i++) if (wit.advice.at(i).size() < P.usable + 1) throw std::invalid_argument("create_proof: advice column " + std::to_string(i) + " has fewer than the usable rows + 1");
  if (run.dev_m && !run.dev_rng && wit.m_blind.size() != run.NL) throw std::invalid_argument("create_proof: device_multiplicities needs the blinding values of every multiplicity column (Circuit::m_blind)");
  run.witness_commits(); run.lap(2);            // steps 1-3; step 3 on the device: device_multiplicities()
  run.instance_to_coefficients(); run.lap(1);
  run.products_and_sums(); run.lap(4);
  run.random_polynomial(); run.lap(5);
  run.to_coefficients(); run.lap(6);
  run.quotient(); run.lap(7);
  run.commit_quotient(); run.lap(8);
  run.evaluations(); run.lap(9);
  run.shplonk(); check(mi355_synchronize()); run.lap(10);
  return run.result();
}

}  // namespace plonk
}  // namespace mi355zk
