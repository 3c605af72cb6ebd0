// plonk_capi_main.cpp -- csrc/plonk_capi.hpp (the handle table, the option parser and the JSON writer behind the mi355_plonk_* entry points) as a program of its own, built
// under -fsanitize=address,undefined by tests/test_plonk_capi_on_host.py.  Prints "<property> ok|FAILED" lines and "json <name> <text>" lines the test parses strictly.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <iterator>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../scroll-prover_amd/csrc/plonk_capi.hpp"

using namespace mi355zk::capi;

static std::map<std::string, bool> g_props;
static void prop(const char *name, bool ok) { auto it = g_props.find(name); if (it == g_props.end()) g_props[name] = ok; else it->second = it->second && ok; }
template <class F> static bool throws_bad_handle(F f, const char *needle) {
  try { f(); } catch (const BadHandle &e) { return std::string(e.what()).find(needle) != std::string::npos; } catch (...) { return false; }
  return false;
}
template <class F> static bool throws_naming(F f, const char *needle) {
  try { f(); } catch (const std::invalid_argument &e) { return std::string(e.what()).find(needle) != std::string::npos; } catch (...) { return false; }
  return false;
}

struct Payload { uint64_t tag; int *alive; explicit Payload(uint64_t t, int *a) : tag(t), alive(a) { ++*alive; } ~Payload() { --*alive; } };

int main() {
  // ---- random issue / free / lookup sequences against a model
  {
    HandleTable T; std::mt19937_64 rng(12345); int alive = 0;
    std::map<uint64_t, std::pair<Kind, uint64_t>> model; std::vector<uint64_t> freed; uint64_t last = 0;
    const Kind kinds[5] = {Kind::Protocol, Kind::Circuit, Kind::Key, Kind::Options, Kind::Record};
    for (int step = 0; step < 20000; step++) {
      const uint64_t r = rng() % 10;
      if (r < 4 || model.empty()) {
        const Kind k = kinds[rng() % 5]; const uint64_t tag = rng();
        const uint64_t h = T.issue(k, std::make_shared<Payload>(tag, &alive));
        prop("handles_are_issued_in_increasing_order", h > last); last = h;
        prop("a_handle_value_is_never_issued_twice", !model.count(h) && std::find(freed.begin(), freed.end(), h) == freed.end());
        model[h] = {k, tag};
      } else if (r < 7) {
        auto it = model.begin(); std::advance(it, (long)(rng() % model.size()));
        auto obj = std::static_pointer_cast<Payload>(T.get(it->first, it->second.first));
        prop("lookup_returns_the_issued_object", obj && obj->tag == it->second.second);
        const Kind other = kinds[((int)it->second.first) % 5];   // Kind values are 1..5: this is always another kind
        prop("wrong_kind_is_refused_and_names_the_expected_kind", throws_bad_handle([&] { T.get(it->first, other); }, kind_name(other)));
        prop("kind_of_a_live_handle", T.kind_of(it->first) == it->second.first);
      } else if (r < 9) {
        auto it = model.begin(); std::advance(it, (long)(rng() % model.size()));
        const uint64_t h = it->first; const Kind k = it->second.first;
        { auto held = T.get(h, k); const int before = alive; T.release(h).reset(); prop("a_held_object_outlives_its_handle", alive == before); }
        model.erase(it); freed.push_back(h);
        prop("a_freed_handle_is_refused", throws_bad_handle([&] { T.get(h, k); }, "already freed"));
        prop("a_second_free_is_refused", throws_bad_handle([&] { T.release(h); }, "already freed"));
        prop("kind_of_a_freed_handle_is_none", T.kind_of(h) == Kind::None);
      } else if (!freed.empty()) {
        const uint64_t h = freed[rng() % freed.size()];
        prop("a_stale_handle_stays_refused", throws_bad_handle([&] { T.get(h, Kind::Key); }, "proving key"));
      }
      prop("live_count_follows_the_model", T.live() == model.size() && (size_t)alive == model.size());
    }
    prop("a_never_issued_handle_is_refused", throws_bad_handle([&] { T.get(last + 1000, Kind::Protocol); }, "never issued") && throws_bad_handle([&] { T.release(last + 1000); }, "never issued"));
    prop("handle_zero_is_refused", throws_bad_handle([&] { T.get(0, Kind::Options); }, "never issued") && throws_bad_handle([&] { T.release(0); }, "never issued"));
    prop("issued_counts_every_handle", T.issued() == last);
    for (const auto &kv : model) T.release(kv.first);
    prop("everything_freed_nothing_alive", T.live() == 0 && alive == 0);
    prop("nothing_to_issue_is_refused", throws_naming([&] { T.issue(Kind::None, std::make_shared<int>(1)); }, "nothing to issue") && throws_naming([&] { T.issue(Kind::Key, nullptr); }, "nothing to issue"));
  }
  // ---- every option name: a good value is stored, bad ones are refused with the name in the message
  {
    for (const auto &s : option_specs()) {
      Options o; const std::string name = s.name;
      switch (s.type) {
        case OptType::Bool:
          o.set(s.name, "1"); prop("bool_options_parse", o.find(s.name) && o.find(s.name)->i == 1);
          o.set(s.name, "false"); prop("bool_options_parse", o.find(s.name)->i == 0);
          prop("bad_bool_is_refused_by_name", throws_naming([&] { o.set(s.name, "yes"); }, s.name) && throws_naming([&] { o.set(s.name, ""); }, s.name) && throws_naming([&] { o.set(s.name, "2"); }, s.name));
          break;
        case OptType::Int: {
          o.set(s.name, std::to_string(s.lo).c_str()); prop("int_options_parse", o.find(s.name)->i == s.lo);
          o.set(s.name, std::to_string(s.hi).c_str()); prop("int_options_parse", o.find(s.name)->i == (int64_t)s.hi);
          prop("out_of_range_int_is_refused_by_name", throws_naming([&] { o.set(s.name, std::to_string(s.lo - 1).c_str()); }, s.name) && throws_naming([&] { o.set(s.name, std::to_string(s.hi + 1).c_str()); }, s.name));
          prop("bad_int_is_refused_by_name", throws_naming([&] { o.set(s.name, "1x"); }, s.name) && throws_naming([&] { o.set(s.name, " 1"); }, s.name) && throws_naming([&] { o.set(s.name, "-"); }, s.name) &&
                                                 throws_naming([&] { o.set(s.name, "99999999999999999999999"); }, s.name));
          break; }
        case OptType::Uint: {
          o.set(s.name, std::to_string(s.hi).c_str()); prop("uint_options_parse", o.find(s.name)->u == s.hi);
          o.set(s.name, "0"); prop("uint_options_parse", o.find(s.name)->u == 0);
          if (s.hi != ~uint64_t(0)) prop("out_of_range_uint_is_refused_by_name", throws_naming([&] { o.set(s.name, std::to_string(s.hi + 1).c_str()); }, s.name));
          prop("bad_uint_is_refused_by_name", throws_naming([&] { o.set(s.name, "-1"); }, s.name) && throws_naming([&] { o.set(s.name, "18446744073709551616"); }, s.name) && throws_naming([&] { o.set(s.name, "0x10"); }, s.name));
          break; }
        case OptType::Hex32: {
          std::string hex; for (int i = 0; i < 32; i++) { char b[3]; std::snprintf(b, sizeof b, "%02x", (i * 37 + 5) & 255); hex += b; }
          o.set(s.name, hex.c_str()); bool same = true; for (int i = 0; i < 32; i++) same = same && o.find(s.name)->bytes[i] == (uint8_t)((i * 37 + 5) & 255);
          prop("hex_options_parse_in_byte_order", same);
          std::string upper = hex; for (auto &c : upper) c = (char)std::toupper((unsigned char)c);
          o.set(s.name, upper.c_str()); same = true; for (int i = 0; i < 32; i++) same = same && o.find(s.name)->bytes[i] == (uint8_t)((i * 37 + 5) & 255);
          prop("hex_options_accept_upper_case", same);
          std::string bad = hex; bad[17] = 'g';
          prop("bad_hex_is_refused_by_name", throws_naming([&] { o.set(s.name, bad.c_str()); }, s.name) && throws_naming([&] { o.set(s.name, hex.substr(1).c_str()); }, s.name) &&
                                                 throws_naming([&] { o.set(s.name, (hex + "00").c_str()); }, s.name) && throws_naming([&] { o.set(s.name, ""); }, s.name));
          break; }
        case OptType::Transcript:
          o.set(s.name, "poseidon"); prop("transcript_names_parse", o.find(s.name)->i == TRANSCRIPT_POSEIDON);
          o.set(s.name, "evm"); prop("transcript_names_parse", o.find(s.name)->i == TRANSCRIPT_EVM);
          o.set(s.name, "blake2b"); prop("transcript_names_parse", o.find(s.name)->i == TRANSCRIPT_BLAKE2B);
          o.set(s.name, "by_layer"); prop("transcript_names_parse", o.find(s.name)->i == TRANSCRIPT_BY_LAYER);
          prop("bad_transcript_is_refused_by_name", throws_naming([&] { o.set(s.name, "sha256"); }, s.name));
          break;
      }
      prop("a_refused_value_leaves_the_option_as_it_was", o.values.size() == 1);
    }
    Options o;
    prop("unknown_option_is_named", throws_naming([&] { o.set("no_such_option", "1"); }, "no_such_option") && o.values.empty());
    prop("unprintable_names_are_masked", throws_naming([&] { o.set("bad\x01name\xff", "1"); }, "bad?name?"));
    prop("null_name_or_value_is_refused", throws_naming([&] { o.set(nullptr, "1"); }, "null") && throws_naming([&] { o.set("threads", nullptr); }, "null"));
    prop("unset_options_are_absent", o.find("threads") == nullptr);
  }
  // ---- copy_out: the size-query convention
  {
    const char src[5] = {1, 2, 3, 4, 5}; char dst[8] = {0}; uint64_t n = 0;
    copy_out(src, 5, nullptr, 0, &n, "t"); prop("cap_zero_asks_for_the_size", n == 5);
    copy_out(src, 5, dst, 8, &n, "t"); prop("copy_out_copies", n == 5 && dst[4] == 5 && dst[5] == 0);
    prop("a_small_buffer_is_refused_and_untouched", throws_naming([&] { char small[4] = {9, 9, 9, 9}; copy_out(src, 5, small, 4, &n, "t"); }, "do not fit"));
    prop("null_outputs_are_refused", throws_naming([&] { copy_out(src, 5, dst, 8, nullptr, "t"); }, "null") && throws_naming([&] { copy_out(src, 5, nullptr, 8, &n, "t"); }, "null"));
  }
  // ---- the JSON writer on extreme values: the test holds every line to json.loads
  {
    JsonWriter w;
    w.begin_object().key("u64_max").value(~uint64_t(0)).key("i64_min").value(std::numeric_limits<int64_t>::min()).key("zero").value((uint64_t)0);
    w.key("nan").value(std::nan("")).key("inf").value(std::numeric_limits<double>::infinity()).key("ninf").value(-std::numeric_limits<double>::infinity());
    w.key("dbl_max").value(std::numeric_limits<double>::max()).key("dbl_min").value(std::numeric_limits<double>::denorm_min()).key("neg_zero").value(-0.0).key("three").value(3.0).key("tenth").value(0.1);
    std::string all; for (int c = 1; c < 256; c++) all.push_back((char)c);
    w.key("every_byte").value(all).key("quote\"back\\slash\nnewline").value("\"\\\n\t\r\b\f").key("empty").value("").key("nul_inside").value(std::string("a\0b", 3));
    w.key("t").value(true).key("f").value(false).key("null").null().key("hex").hex("\x00\xff\x10", 3);
    w.key("nested").begin_array().begin_array().end_array().begin_object().end_object().begin_array().value((uint32_t)1).value(-2).begin_object().key("k").begin_array().end_array().end_object().end_array().end_array();
    w.end_object();
    std::printf("json extremes %s\n", w.str().c_str());
    prop("writer_is_complete_after_the_last_close", w.complete());
    JsonWriter deep; for (int i = 0; i < 200; i++) deep.begin_array(); deep.value((uint64_t)7); for (int i = 0; i < 200; i++) deep.end_array();
    std::printf("json deep %s\n", deep.str().c_str());
    JsonWriter scalar; scalar.value("alone"); std::printf("json scalar %s\n", scalar.str().c_str());
    auto logic = [](auto f) { try { f(); } catch (const std::logic_error &) { return true; } catch (...) { return false; } return false; };
    prop("writer_refuses_a_value_without_a_key", logic([] { JsonWriter x; x.begin_object().value(true); }));
    prop("writer_refuses_a_key_in_an_array", logic([] { JsonWriter x; x.begin_array().key("k"); }));
    prop("writer_refuses_a_mismatched_close", logic([] { JsonWriter x; x.begin_array().end_object(); }) && logic([] { JsonWriter x; x.begin_object().key("k").end_object(); }) && logic([] { JsonWriter x; x.end_array(); }));
    prop("writer_refuses_two_top_level_values", logic([] { JsonWriter x; x.value(true).value(false); }));
    prop("writer_refuses_to_print_an_unclosed_document", logic([] { JsonWriter x; x.begin_array(); (void)x.str(); }));
  }
  bool all_ok = true;
  for (const auto &kv : g_props) { std::printf("%s %s\n", kv.first.c_str(), kv.second ? "ok" : "FAILED"); all_ok = all_ok && kv.second; }
  return all_ok ? 0 : 1;
}
