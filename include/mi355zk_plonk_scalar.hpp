// mi355zk_plonk_scalar.hpp -- the SCALAR SIDE of plonk::verify_proof as one function template over the scalar type: x^n, the Lagrange values at x, the instance evaluation,
// the numerator tree at x, h(x) and the SHPLONK scalars over the rotation sets.  Included from mi355zk_plonk_verify.hpp.
//   scalar_side<FrArith>    the arithmetic itself: what vdetail::host_part runs for every proof verified on the host
//   scalar_side<Recorder>   the same walk over the protocol with a type that WRITES DOWN each operation: the program mi355_fr_program_host runs for every proof of that protocol
//                           in a batch (VerifyOptions::device_scalars), compiled once per (protocol, number of instances) by compile_scalar_program
// Given a protocol the scalar side is straight-line arithmetic in Fr: its inputs are the eight challenges, the proof's evaluations and the instances, and nothing in it branches on
// their values.  What looked at values before is structural or a flag here:
//   opening points      x omega^rot is one point per ROTATION (two rotations give the same point only for x = 0, which is flagged, see below): sets are compared by rotation
//   x_in_domain         is_zero(x^n - 1): the host type answers, the recorder emits NZ -> flag bit FLAG_BIT_X_IN_DOMAIN
//   shplonk_degenerate  is_zero(Z_T\S0(u)): likewise -> flag bit FLAG_BIT_DEGENERATE
//   inverses            every denominator depends on challenges only and is known before the evaluations are touched: invert_all takes them together.  The host type inverts
//                       each (today's values, today's cost); the recorder emits Montgomery's trick around ONE INV.  A zero among them (x = 0, or a flagged failure) makes that
//                       INV set flag bit 0: a job with bit 0 alone is verified again on the host, so every result equals the host's.
// A protocol that names evaluations or commitments the proof does not carry fails under the name "protocol" whatever the proof says: compile_scalar_program reports it as
// unusable and its proofs take the host path, where that failure is produced as always.
// Registers are reused by liveness (linear scan over the recorded code), constants are shared by value.
#pragma once
#include <map>
#include <queue>
#include "mi355zk_plonk_protocol.hpp"
#include "../scroll-prover_amd/csrc/frprog.hpp"

namespace mi355zk {
namespace plonk {
namespace sdetail {

constexpr uint32_t FLAG_BIT_X_IN_DOMAIN = 1, FLAG_BIT_DEGENERATE = 2;
constexpr uint32_t N_CHALLENGE_INPUTS = 8;   // theta, beta, gamma, y, x, SHPLONK's y, v, u: the first inputs of a program, then the evaluations in proof order, then the instances
inline const char *x_in_domain_text() { return "the evaluation point lies in the domain"; }
inline const char *degenerate_text() { return "u coincides with an opening point"; }

struct MsmSource { enum Kind : uint8_t { Piece, Commitment, Generator, H, W } kind; uint32_t index; };   // where the point of an MSM term comes from: quotient piece j, commitment of polynomial p, ...
struct Failure { const char *name = nullptr; std::string detail; };

// ---- the two scalar types
struct FrArith {
  using T = Fr;
  T constant(const Fr &c) { return c; }
  T add(const T &a, const T &b) { return fr_add(a, b); }
  T sub(const T &a, const T &b) { return fr_sub(a, b); }
  T mul(const T &a, const T &b) { return fr_mul(a, b); }
  T neg(const T &a) { return fr_neg(a); }
  T sqrn(T a, uint32_t n) { for (uint32_t i = 0; i < n; i++) a = fr_mul(a, a); return a; }
  bool is_zero(const T &a, uint32_t /* flag bit */) { return fr_is_zero(a); }
  void invert_all(std::vector<T> &v) { for (auto &a : v) a = fr_inv(a); }
};

struct ScalarProgram {
  bool usable = false; Failure why;                 // not usable: the protocol fails structurally; its proofs go to the host
  std::vector<uint32_t> code; uint32_t n_instr = 0, n_regs = 0, n_inputs = 0, n_inv = 0; std::vector<Fr> consts; std::vector<uint32_t> out_regs;   // outputs: numerator_at_x, then the MSM scalars
  std::vector<MsmSource> sources; size_t n_evals = 0, n_instances = 0;
};

struct Recorder {
  struct T { uint32_t id = ~0u; };
  enum : uint32_t { CONST = 0u, INPUT = 1u << 30, TEMP = 2u << 30, KIND = 3u << 30, INDEX = ~KIND };
  struct Ins { uint32_t op, d, a, b; };
  std::vector<Fr> consts; std::map<Fr, uint32_t> const_at; uint32_t n_inputs = 0, n_temps = 0; std::vector<Ins> code;
  const Fr one_ = fr_one(), zero_ = fr_zero();

  T input() { return T{INPUT | n_inputs++}; }
  T constant(const Fr &c) { auto it = const_at.find(c); if (it == const_at.end()) { it = const_at.emplace(c, (uint32_t)consts.size()).first; consts.push_back(c); } return T{CONST | it->second}; }
  bool is_const(const T &a, const Fr &c) const { return (a.id & KIND) == CONST && consts[a.id & INDEX] == c; }
  T emit(uint32_t op, uint32_t a, uint32_t b) { const T d{TEMP | n_temps++}; code.push_back({op, d.id, a, b}); return d; }
  T add(const T &a, const T &b) { if (is_const(a, zero_)) return b; if (is_const(b, zero_)) return a; return emit(zk::FRP_ADD, a.id, b.id); }
  T sub(const T &a, const T &b) { if (is_const(b, zero_)) return a; return emit(zk::FRP_SUB, a.id, b.id); }
  T mul(const T &a, const T &b) { if (is_const(a, one_)) return b; if (is_const(b, one_)) return a; return emit(zk::FRP_MUL, a.id, b.id); }
  T neg(const T &a) { return emit(zk::FRP_SUB, constant(zero_).id, a.id); }
  T sqrn(const T &a, uint32_t n) { T r = a; while (n) { const uint32_t step = std::min(n, zk::FRP_MAX_SQRN); r = emit(zk::FRP_SQRN, r.id, step); n -= step; } return r; }
  bool is_zero(const T &a, uint32_t bit) { code.push_back({zk::FRP_NZ, 0, a.id, bit}); return false; }
  void invert_all(std::vector<T> &v) {   // Montgomery's trick: prefix products, ONE inverse, back-substitution
    if (v.empty()) return;
    std::vector<T> prefix(v.size()); prefix[0] = v[0];
    for (size_t i = 1; i < v.size(); i++) prefix[i] = mul(prefix[i - 1], v[i]);
    T inv = emit(zk::FRP_INV, prefix.back().id, 0);
    for (size_t i = v.size(); i-- > 1;) { const T vi = v[i]; v[i] = mul(inv, prefix[i - 1]); inv = mul(inv, vi); }
    v[0] = inv;
  }

  // physical registers: constants, inputs, then the temporaries by linear scan -- a temporary's register is free again behind its last use, and an instruction's destination
  // may take the register of an operand that dies in it
  void finish(const std::vector<T> &outputs, ScalarProgram &out) const {
    const uint32_t nc = (uint32_t)consts.size(), first_temp = nc + n_inputs;
    constexpr int64_t NEVER = -1, KEEP = INT64_MAX;
    std::vector<int64_t> last(n_temps, NEVER);
    auto touch = [&](uint32_t id, int64_t at) { if ((id & KIND) == TEMP && last[id & INDEX] != KEEP) last[id & INDEX] = at; };
    for (size_t i = 0; i < code.size(); i++) { touch(code[i].a, (int64_t)i); if (code[i].op <= zk::FRP_MUL) touch(code[i].b, (int64_t)i); }
    for (const T &o : outputs) if ((o.id & KIND) == TEMP) last[o.id & INDEX] = KEEP;
    std::vector<uint32_t> where(n_temps, ~0u); std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> free_regs; uint32_t used = 0;
    auto phys = [&](uint32_t id) { return (id & KIND) == CONST ? id & INDEX : (id & KIND) == INPUT ? nc + (id & INDEX) : where[id & INDEX]; };
    auto release = [&](uint32_t id, int64_t at) { if ((id & KIND) == TEMP && last[id & INDEX] == at) { free_regs.push(where[id & INDEX]); last[id & INDEX] = NEVER - 1; } };   // marked: a == b releases once
    out.code.clear(); out.code.reserve(4 * code.size()); out.n_inv = 0;
    for (size_t i = 0; i < code.size(); i++) {
      const Ins &c = code[i]; const bool binary = c.op <= zk::FRP_MUL;
      const uint32_t pa = phys(c.a), pb = binary ? phys(c.b) : c.b;
      release(c.a, (int64_t)i); if (binary) release(c.b, (int64_t)i);
      uint32_t pd = 0;
      if (c.op != zk::FRP_NZ) {
        if (free_regs.empty()) pd = first_temp + used++; else { pd = free_regs.top(); free_regs.pop(); }
        where[c.d & INDEX] = pd;
        if (last[c.d & INDEX] == NEVER) free_regs.push(pd);   // never read: the register is free again at once
      }
      if (c.op == zk::FRP_INV) out.n_inv++;
      out.code.push_back(c.op); out.code.push_back(pd); out.code.push_back(pa); out.code.push_back(pb);
    }
    out.n_instr = (uint32_t)code.size(); out.n_regs = first_temp + used; out.n_inputs = n_inputs; out.consts = consts;
    out.out_regs.clear(); for (const T &o : outputs) out.out_regs.push_back(phys(o.id));
  }
};

// ---- the walk
template <class A> struct ScalarInputs { typename A::T ch[4], x, ys, v, u; std::vector<typename A::T> evals /* in the order of Protocol::evaluations */, instances; };
template <class A> struct ScalarSide { bool numerator_set = false; typename A::T numerator{}; std::vector<typename A::T> scalars; std::vector<MsmSource> sources; Failure failure; };

template <class A> typename A::T eval_expr(A &ar, const Expr &e, const std::map<PolyRot, typename A::T> &evals, const typename A::T *ch, const typename A::T &x,
                                           const std::map<int32_t, typename A::T> &lag) {
  using T = typename A::T;
  auto ev = [&](const Expr &k) { return eval_expr(ar, k, evals, ch, x, lag); };
  switch (e.kind) {
    case Expr::CONSTANT: return ar.constant(e.c);
    case Expr::IDENTITY: return x;
    case Expr::LAGRANGE: return lag.at(e.i);
    case Expr::POLY: { auto it = evals.find({(uint32_t)e.i, e.rot}); if (it == evals.end()) throw std::invalid_argument("verify: the numerator names an evaluation the proof does not carry"); return it->second; }
    case Expr::CHALLENGE: return ch[e.i];
    case Expr::NEG: return ar.neg(ev(e.kids[0]));
    case Expr::SUM: { const T a = ev(e.kids[0]); return ar.add(a, ev(e.kids[1])); }
    case Expr::PROD: { const T a = ev(e.kids[0]); return ar.mul(a, ev(e.kids[1])); }
    case Expr::SCALED: return ar.mul(ev(e.kids[0]), ar.constant(e.c));
    case Expr::DPOW: { const T b = ev(e.kids.back()); T acc = ev(e.kids[0]); for (size_t i = 1; i + 1 < e.kids.size(); i++) acc = ar.add(ar.mul(acc, b), ev(e.kids[i])); return acc; }   // Horner, the first expression at the highest power
  }
  throw std::invalid_argument("verify: unknown expression node");
}

// false with out.failure set; what was computed before the failure stays in `out` (numerator_at_x survives a later failure, as the terms pushed before a missing commitment do)
template <class A> bool scalar_side(A &ar, const Protocol &P, const ScalarInputs<A> &in, ScalarSide<A> &out) {
  using T = typename A::T;
  auto failed = [&](const char *name, const std::string &why) { out.failure.name = name; out.failure.detail = why; return false; };
  const T one = ar.constant(fr_one()), zero = ar.constant(fr_zero());
  const T &x = in.x, &uu = in.u;
  const T xn = ar.sqrn(x, P.k);
  const T xn_minus_1 = ar.sub(xn, one);
  if (ar.is_zero(xn_minus_1, FLAG_BIT_X_IN_DOMAIN)) return failed("x_in_domain", x_in_domain_text());

  // ---- every denominator, then their inverses together: x - omega^i of the Lagrange values, x^n - 1, the basis denominators of the rotation sets, Z_T\S0(u)
  std::vector<int32_t> lag_idx;
  { std::vector<int32_t> need; collect_lagrange(P.numerator, need); for (size_t i = 0; i < in.instances.size(); i++) need.push_back((int32_t)i);
    for (int32_t i : need) if (std::find(lag_idx.begin(), lag_idx.end(), i) == lag_idx.end()) lag_idx.push_back(i); }
  const std::vector<RotationSet> sets = rotation_sets(P.queries);
  std::vector<int32_t> super_rots;   // the opening points, one per rotation, by first appearance
  for (const auto &s : sets) for (int32_t r : s.rots) if (std::find(super_rots.begin(), super_rots.end(), r) == super_rots.end()) super_rots.push_back(r);
  std::map<int32_t, T> pt, diff;     // x omega^r and u - x omega^r
  for (int32_t r : super_rots) { pt[r] = ar.mul(x, ar.constant(rot_power(P.omega, P.omega_inv, r))); diff[r] = ar.sub(uu, pt[r]); }
  auto in_set = [](const RotationSet &s, int32_t r) { return std::find(s.rots.begin(), s.rots.end(), r) != s.rots.end(); };
  auto zd_of = [&](const RotationSet &s) { T zd = one; for (int32_t r : super_rots) if (!in_set(s, r)) zd = ar.mul(zd, diff[r]); return zd; };
  std::vector<T> dens;
  for (int32_t i : lag_idx) dens.push_back(ar.sub(x, ar.constant(rot_power(P.omega, P.omega_inv, i))));
  const size_t at_xn = dens.size(); dens.push_back(xn_minus_1);
  std::vector<size_t> at_set(sets.size());
  for (size_t k = 0; k < sets.size(); k++) {
    at_set[k] = dens.size();
    const auto &rots = sets[k].rots;
    if (rots.size() > 1) for (size_t a = 0; a < rots.size(); a++) { T den = one; for (size_t b = 0; b < rots.size(); b++) if (b != a) den = ar.mul(den, ar.sub(pt[rots[a]], pt[rots[b]])); dens.push_back(den); }
  }
  const T zd0 = sets.empty() ? zero : zd_of(sets[0]);
  const size_t at_zd0 = dens.size(); dens.push_back(zd0);
  ar.invert_all(dens);

  std::map<int32_t, T> lag;          // omega^i (x^n - 1) / (n (x - omega^i))
  for (size_t j = 0; j < lag_idx.size(); j++) lag[lag_idx[j]] = ar.mul(ar.mul(ar.mul(ar.constant(rot_power(P.omega, P.omega_inv, lag_idx[j])), xn_minus_1), ar.constant(P.n_inv)), dens[j]);
  std::map<PolyRot, T> evals;
  for (size_t i = 0; i < P.evaluations.size(); i++) evals[P.evaluations[i]] = in.evals[i];
  { T acc = zero; for (size_t i = 0; i < in.instances.size(); i++) acc = ar.add(acc, ar.mul(in.instances[i], lag.at((int32_t)i))); for (size_t j = 0; j < P.num_instance.size(); j++) evals[{P.inst0 + (uint32_t)j, 0}] = acc; }
  { std::vector<std::pair<int32_t, int32_t>> named; collect_polys(P.numerator, named);   // an inconsistent protocol is a named failure here as in the SHPLONK part, never an exception
    for (const auto &pr : named) if (!evals.count({(uint32_t)pr.first, pr.second})) return failed("protocol", "the numerator names polynomial " + std::to_string(pr.first) + " at rotation " + std::to_string(pr.second) + ", which the proof carries no evaluation for"); }
  const T numer = eval_expr(ar, P.numerator, evals, in.ch, x, lag);
  out.numerator = numer; out.numerator_set = true;
  evals[{P.quotient_poly, 0}] = ar.mul(numer, dens[at_xn]);

  // ---- SHPLONK: the scalars of the (scalars, points) list
  T zt = one; for (int32_t r : super_rots) zt = ar.mul(zt, diff[r]);
  std::vector<uint32_t> term_order; std::map<uint32_t, T> terms;
  T r_acc = zero, vp = one;
  for (size_t k = 0; k < sets.size(); k++) {
    const RotationSet &s = sets[k];
    const T zd = k == 0 ? zd0 : zd_of(s);
    std::vector<T> basis(s.rots.size());   // the Lagrange basis of the set's points at u: r_ij(u) = sum_k eval_k basis_k
    if (s.rots.size() == 1) basis[0] = one;
    else for (size_t a = 0; a < s.rots.size(); a++) { T num = one; for (size_t b = 0; b < s.rots.size(); b++) if (b != a) num = ar.mul(num, diff[s.rots[b]]); basis[a] = ar.mul(num, dens[at_set[k] + a]); }
    const T w = ar.mul(vp, zd);
    T inner_r = zero, yp = one;
    for (uint32_t p : s.polys) {
      T r_u = zero;
      for (size_t a = 0; a < s.rots.size(); a++) { auto it = evals.find({p, s.rots[a]}); if (it == evals.end()) return failed("protocol", "polynomial " + std::to_string(p) + " is queried at a rotation the proof carries no evaluation for"); r_u = ar.add(r_u, ar.mul(it->second, basis[a])); }
      inner_r = ar.add(inner_r, ar.mul(yp, r_u));
      const T wy = ar.mul(w, yp);
      auto it = terms.find(p);
      if (it == terms.end()) { terms.emplace(p, wy); term_order.push_back(p); } else it->second = ar.add(it->second, wy);
      yp = ar.mul(yp, in.ys);
    }
    r_acc = ar.add(r_acc, ar.mul(w, inner_r));
    vp = ar.mul(vp, in.v);
  }
  if (ar.is_zero(zd0, FLAG_BIT_DEGENERATE)) return failed("shplonk_degenerate", degenerate_text());
  const T zi = dens[at_zd0];
  uint32_t n_wit = 0; for (auto w : P.num_witness) n_wit += w;
  for (uint32_t p : term_order) {
    const T c = ar.mul(terms.at(p), zi);
    if (p == P.quotient_poly) { T f = one; for (uint32_t j = 0; j < P.Q; j++) { out.scalars.push_back(ar.mul(c, f)); out.sources.push_back({MsmSource::Piece, j}); f = ar.mul(f, xn); } }
    else { if (!(p < P.num_pre || (p >= P.wit0 && p < P.wit0 + n_wit))) return failed("protocol", "no commitment for queried polynomial " + std::to_string(p)); out.scalars.push_back(c); out.sources.push_back({MsmSource::Commitment, p}); }
  }
  out.scalars.push_back(ar.neg(ar.mul(r_acc, zi))); out.sources.push_back({MsmSource::Generator, 0});
  out.scalars.push_back(ar.neg(ar.mul(zt, zi))); out.sources.push_back({MsmSource::H, 0});
  out.scalars.push_back(uu); out.sources.push_back({MsmSource::W, 0});
  return true;
}

// the program of protocol P for proofs with n_instances instance values
inline ScalarProgram compile_scalar_program(const Protocol &P, size_t n_instances) {
  Recorder rec; ScalarInputs<Recorder> in; ScalarSide<Recorder> side; ScalarProgram prog;
  for (auto &c : in.ch) c = rec.input();
  in.x = rec.input(); in.ys = rec.input(); in.v = rec.input(); in.u = rec.input();
  for (size_t i = 0; i < P.evaluations.size(); i++) in.evals.push_back(rec.input());
  for (size_t i = 0; i < n_instances; i++) in.instances.push_back(rec.input());
  prog.n_evals = P.evaluations.size(); prog.n_instances = n_instances;
  if (!scalar_side(rec, P, in, side)) { prog.why = side.failure; return prog; }
  std::vector<Recorder::T> outputs = {side.numerator}; outputs.insert(outputs.end(), side.scalars.begin(), side.scalars.end());
  rec.finish(outputs, prog);
  prog.sources = side.sources;
  if (prog.n_regs > zk::FRP_MAX_REGS || prog.n_instr > zk::FRP_MAX_INSTR) { prog.why.name = "program_size"; prog.why.detail = "the scalar side needs " + std::to_string(prog.n_instr) + " instructions and " + std::to_string(prog.n_regs) + " registers"; return prog; }
  prog.usable = true;
  return prog;
}

}  // namespace sdetail
}  // namespace plonk
}  // namespace mi355zk
