// plan_interp_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around mi355zk::plonk::Compiler (include/mi355zk_plonk.hpp), the code that turns a protocol's numerator
// tree into Launch lists for mi355_fr_gate_eval_dev.  It compiles the numerator of the PlonkProtocol file it is given with the challenges (2, 3, 5, 7) and INTERPRETS the
// launch list, in order, on the Lagrange domain over the column values of a second file (32-byte Montgomery words, n rows per polynomial index, indices 0 .. quotient - 1),
// rotations in rows modulo n:
//     dst[r] (+)= sum_j coeff_j prod_f operand_f[(r + rot_f) mod n]
// operands being columns, earlier temporaries, or common polynomials evaluated from their CommonLinear as  constant + x_coeff omega^r + sum_i lagrange[i] [r == i mod n];
// the quotient's accumulator (dst == -1) starts at zero.  It prints the accumulator's n words ("row r <canonical hex>") and what the plan looked like ("fact name value");
// tests/test_plan_compiler_on_host.py compares the rows with oracle.plonk.evaluate of the whole numerator in Python integers and holds every gate family of
// tests/plan_common.py to the fact that shows its path was reached.  It fails on its own account ("WRONG ...", exit code 1) when a launch exceeds a limit of the kernel, reads a
// temporary nothing has written, or accumulates into one.  A compile the compiler refuses prints "refused <what()>" and exits 0.  Built with -fsanitize=address,undefined.
// No device call is made.  Never shipped.
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "mi355zk_plonk.hpp"

using namespace mi355zk::plonk;

static int g_wrong = 0;
static void wrong(const std::string &what) { std::printf("WRONG %s\n", what.c_str()); g_wrong++; }

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: plan_interp_main protocol.json columns.bin\n"); return 2; }
  Protocol P; P.load(argv[1]);
  const uint64_t n = P.n; const uint32_t NP = P.quotient_poly;
  std::vector<std::vector<Fr>> col(NP, std::vector<Fr>(n));
  { std::ifstream f(argv[2], std::ios::binary);
    for (auto &c : col) f.read(reinterpret_cast<char *>(c.data()), (std::streamsize)(n * 32));
    if (!f || f.peek() != std::ifstream::traits_type::eof()) { std::fprintf(stderr, "columns: %u polynomials of %llu rows expected\n", NP, (unsigned long long)n); return 2; } }
  CommonRegistry reg; { Expr id; id.kind = Expr::IDENTITY; reg.id_of(id, true); }
  const std::vector<Fr> ch{fr_u64(2), fr_u64(3), fr_u64(5), fr_u64(7)};
  Compiler cmp(reg, true, ch);
  try { cmp.compile_numerator(P.numerator); }
  catch (const std::invalid_argument &e) { std::printf("refused %s\n", e.what()); return 0; }

  // ---- the temporaries each constraint needs on its own: what compile_numerator compiles for it (the bracket alone where the leading polynomial has a G_p), from id 0
  uint32_t constraint_tmps_max = 0;
  { const size_t m = P.numerator.kids.size() - 1;
    auto prefix_of = [&](const Expr &c, Atom &a) -> bool {
      if (c.kind != Expr::PROD) return false;
      const Expr &p = c.kids[0]; bool common = false;
      if (p.kind == Expr::POLY) { a = Atom{A_POLY, (uint32_t)p.i, p.rot}; return true; }
      if (is_common_linear(p, &common) && common) { a = Atom{A_COMMON, reg.id_of(p, true), 0}; return true; }
      return false;
    };
    std::map<Atom, uint32_t> count;
    for (size_t i = 0; i < m; i++) { Atom a; if (prefix_of(P.numerator.kids[i], a)) count[a]++; }
    Compiler one(reg, true, ch);
    for (size_t i = 0; i < m; i++) {
      Atom a; const bool grouped = prefix_of(P.numerator.kids[i], a) && count[a] >= Compiler::prefix_min();
      one.tmp_base = 0; one.tmp_next = 0; one.out.clear();
      (void)one.compile(grouped ? P.numerator.kids[i].kids[1] : P.numerator.kids[i]);
      constraint_tmps_max = std::max(constraint_tmps_max, one.tmp_next);
    } }

  // ---- the common polynomials on the Lagrange domain
  std::vector<std::vector<Fr>> common;
  for (const auto &d : reg.defs) {
    std::vector<Fr> v(n); Fr w = fr_one();
    for (uint64_t r = 0; r < n; r++) { v[r] = fr_add(d.constant, fr_mul(d.x_coeff, w)); w = fr_mul(w, P.omega); }
    for (const auto &sp : d.lagrange) { const uint64_t row = (uint64_t)(((int64_t)sp.first % (int64_t)n + (int64_t)n) % (int64_t)n); v[row] = fr_add(v[row], sp.second); }
    common.push_back(std::move(v));
  }

  // ---- the launches, in order
  std::map<int, std::vector<Fr>> tmp;          // the temporaries something has written
  std::vector<Fr> acc(n, fr_zero());
  size_t max_terms = 0, max_factors = 0, max_polys = 0, max_term_len = 0, accumulate_into_tmp = 0;
  for (size_t li = 0; li < cmp.out.size(); li++) {
    const Launch &L = cmp.out[li];
    const std::string at = "launch " + std::to_string(li);
    std::set<Atom> polys; size_t nf = 0;
    for (const auto &t : L.terms) { nf += t.f.size(); max_term_len = std::max(max_term_len, t.f.size()); for (const auto &a : t.f) polys.insert(Atom{a.kind, a.idx, 0}); }
    max_terms = std::max(max_terms, L.terms.size()); max_factors = std::max(max_factors, nf); max_polys = std::max(max_polys, polys.size());
    if (L.terms.size() > PLAN_MAX_TERMS) wrong(at + " has " + std::to_string(L.terms.size()) + " terms");
    if (nf > PLAN_MAX_FACTORS) wrong(at + " has " + std::to_string(nf) + " factors");
    if (polys.size() > PLAN_MAX_POLYS) wrong(at + " names " + std::to_string(polys.size()) + " polynomials");
    for (const auto &t : L.terms) if (t.f.size() > PLAN_MAX_TERM_LEN) wrong(at + " has a term of " + std::to_string(t.f.size()) + " factors");
    if (L.dst < -1) { wrong(at + " writes destination " + std::to_string(L.dst)); continue; }
    if (L.dst >= 0 && (uint32_t)L.dst >= cmp.tmp_max) wrong(at + " writes temporary " + std::to_string(L.dst) + " beyond tmp_max");
    bool readable = true;
    for (const auto &t : L.terms) for (const auto &a : t.f) {
      if (a.kind == A_TMP && !tmp.count((int)a.idx)) { wrong(at + " reads temporary " + std::to_string(a.idx) + ", which nothing has written"); readable = false; }
      if (a.kind == A_TMP && (int)a.idx == L.dst) { wrong(at + " reads the temporary it writes"); readable = false; }
      if (a.kind == A_POLY && a.idx >= NP) { wrong(at + " reads polynomial " + std::to_string(a.idx)); readable = false; }
      if (a.kind == A_COMMON && a.idx >= common.size()) { wrong(at + " reads common polynomial " + std::to_string(a.idx)); readable = false; }
    }
    if (L.dst >= 0 && L.accumulate) { accumulate_into_tmp++; if (!tmp.count(L.dst)) { wrong(at + " accumulates into temporary " + std::to_string(L.dst) + ", which nothing has written"); readable = false; } }
    if (!readable) continue;
    std::vector<Fr> sum(n, fr_zero());
    for (const auto &t : L.terms)
      for (uint64_t r = 0; r < n; r++) {
        Fr v = t.coeff;
        for (const auto &a : t.f) {
          const std::vector<Fr> &src = a.kind == A_TMP ? tmp.at((int)a.idx) : a.kind == A_COMMON ? common[a.idx] : col[a.idx];
          v = fr_mul(v, src[(uint64_t)(((int64_t)r + a.rot) % (int64_t)n + (int64_t)n) % n]);
        }
        sum[r] = fr_add(sum[r], v);
      }
    std::vector<Fr> &dst = L.dst < 0 ? acc : tmp[L.dst];
    if (L.dst >= 0 && !L.accumulate) dst.assign(n, fr_zero());
    for (uint64_t r = 0; r < n; r++) dst[r] = fr_add(dst[r], sum[r]);
  }

  std::printf("fact launches %zu\nfact tmps_used %u\nfact tmp_max %u\nfact prefix_groups %u\nfact constraints %u\nfact terms %u\n", cmp.out.size(), cmp.tmps_used(), cmp.tmp_max, cmp.prefix_groups, cmp.constraints, cmp.terms_total);
  std::printf("fact max_terms %zu\nfact max_factors %zu\nfact max_polys %zu\nfact max_term_len %zu\nfact accumulate_into_tmp %zu\nfact constraint_tmps_max %u\n",
              max_terms, max_factors, max_polys, max_term_len, accumulate_into_tmp, constraint_tmps_max);
  for (uint64_t r = 0; r < n; r++) {
    const Fr c = fr_to_canonical(acc[r]);
    std::printf("row %llu %016llx%016llx%016llx%016llx\n", (unsigned long long)r, (unsigned long long)c[3], (unsigned long long)c[2], (unsigned long long)c[1], (unsigned long long)c[0]);
  }
  return g_wrong ? 1 : 0;
}
