// coset_groups_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around mi355zk::plonk::detail::coset_groups (include/mi355zk_plonk.hpp), the cut of a compiled quotient plan
// into consecutive groups of launches that ProofOptions::coset_group_polys runs one coset transform batch at a time.  tests/test_coset_groups_on_host.py builds it with
// -fsanitize=address,undefined and runs it on the PlonkProtocol files it is given (the seven layers scroll-prover_amd/protocols.py writes and the reference's two fixtures);
// every property prints one line "name ok|WRONG ..." and the exit code is the number of properties that went wrong.  No device call is made.  Never shipped.
#include <cstdio>
#include <map>
#include <set>
#include <string>

#include "mi355zk_plonk.hpp"

using namespace mi355zk::plonk;

static std::map<std::string, int> g_fail;
static void expect(const char *prop, bool ok) { g_fail[prop] += ok ? 0 : 1; }

int main(int argc, char **argv) {
  for (const char *p : {"groups_are_consecutive_in_order_and_cover_every_launch_once", "every_launch_operand_lies_in_its_group", "no_group_exceeds_G", "all_gives_one_group_and_no_retransform",
                        "more_than_G_operands_give_two_groups_or_more", "G_23_is_refused", "retransforms_are_the_repeated_members", "groups_are_greedy", "resident_key_counts_witness_only",
                        "seven_layers_and_two_fixtures"}) g_fail[p] = 0;
  int files = 0, cut = 0;
  for (int a = 1; a < argc; a++) {
    Protocol P; P.load(argv[a]); files++;
    CommonRegistry reg; { Expr id; id.kind = Expr::IDENTITY; reg.id_of(id, true); }
    Compiler cmp(reg, true, {fr_u64(2), fr_u64(3), fr_u64(5), fr_u64(7)});
    cmp.compile_numerator(P.numerator);
    auto operands = [&](const Launch &L, bool lean) {   // the launch's non-temporary operands, as the grouping must count them
      std::set<Atom> s;
      for (const auto &t : L.terms) for (const auto &f : t.f) { if (f.kind == A_TMP) continue; const bool key = f.kind == A_COMMON || P.is_pre(f.idx); if (!key || lean) s.insert(Atom{f.kind, f.idx, 0}); }
      return s;
    };
    for (int lean = 0; lean < 2; lean++) {
      std::set<Atom> distinct; for (const auto &L : cmp.out) for (const auto &x : operands(L, lean != 0)) distinct.insert(x);
      bool refused = false; try { (void)detail::coset_groups(P, cmp.out, 23, lean != 0); } catch (const std::invalid_argument &) { refused = true; }
      expect("G_23_is_refused", refused);
      for (uint32_t G : {24u, 25u, 40u, 64u, detail::COSET_GROUP_ALL}) {
        const detail::CosetGrouping R = detail::coset_groups(P, cmp.out, G, lean != 0);
        size_t at = 0; uint64_t members = 0; bool order = !R.groups.empty() || cmp.out.empty();
        for (size_t gi = 0; gi < R.groups.size(); gi++) {
          const detail::CosetGroup &g = R.groups[gi];
          order = order && g.first == at && g.last > g.first && g.last <= cmp.out.size(); at = g.last;
          std::set<Atom> have; for (uint32_t w : g.witness) have.insert(Atom{A_POLY, w, 0}); for (const auto &k : g.key) have.insert(k);
          expect("no_group_exceeds_G", have.size() <= G && have.size() == g.witness.size() + g.key.size());
          if (!lean) expect("resident_key_counts_witness_only", g.key.empty());
          std::set<Atom> need;
          for (size_t l = g.first; l < g.last && l < cmp.out.size(); l++) for (const auto &x : operands(cmp.out[l], lean != 0)) { need.insert(x); expect("every_launch_operand_lies_in_its_group", have.count(x) == 1); }
          expect("every_launch_operand_lies_in_its_group", need.size() == have.size());   // (need is a subset of have by the line above) and nothing is transformed that no launch of the group reads
          for (uint32_t w : g.witness) expect("every_launch_operand_lies_in_its_group", !P.is_pre(w));
          // greedy: the next launch did not fit any more
          if (g.last < cmp.out.size()) { std::set<Atom> more = have; for (const auto &x : operands(cmp.out[g.last], lean != 0)) more.insert(x); expect("groups_are_greedy", more.size() > G); }
          members += have.size();
        }
        expect("groups_are_consecutive_in_order_and_cover_every_launch_once", order && at == cmp.out.size());
        expect("retransforms_are_the_repeated_members", R.retransforms == members - distinct.size() && R.distinct == distinct.size());
        if (G == detail::COSET_GROUP_ALL) expect("all_gives_one_group_and_no_retransform", R.groups.size() == 1 && R.retransforms == 0);
        if (distinct.size() > G) { expect("more_than_G_operands_give_two_groups_or_more", R.groups.size() >= 2); cut++; }
        std::printf("# %s lean=%d G=%u: launches %zu, distinct %zu, groups %zu, retransforms %u\n", argv[a], lean, G, cmp.out.size(), distinct.size(), R.groups.size(), R.retransforms);
      }
    }
  }
  expect("seven_layers_and_two_fixtures", files == 9 && cut > 0);
  expect("more_than_G_operands_give_two_groups_or_more", cut > 0);
  int wrong = 0;
  for (auto &kv : g_fail) { if (kv.second) { std::printf("%s WRONG %d violations\n", kv.first.c_str(), kv.second); wrong++; } else std::printf("%s ok\n", kv.first.c_str()); }
  return wrong;
}
