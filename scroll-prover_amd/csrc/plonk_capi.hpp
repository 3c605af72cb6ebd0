// plonk_capi.hpp -- the bookkeeping of the mi355_plonk_* entry points (csrc/lib_plonk.cpp; include/mi355zk.h "the prover and the verifier behind the C-ABI"): the handle
// table, the parser of the option objects and the writer of the JSON records.  Plain C++: neither HIP nor the library nor the prover's headers, so that
// tests/hostcheck/plonk_capi_main.cpp checks it on the host under the sanitizers, the way knobs.hpp, buf_registry.hpp and ws_layout.hpp are checked.
//
//   HandleTable   objects are uint64_t handles issued from ONE counter that starts at 1 and never goes back: a value is issued once per process, so a stale handle can
//                 never name a newer object.  An entry holds a shared_ptr: an entry point that looked its object up keeps it alive until it returns, and an object that
//                 refers to another (a circuit or a key to its protocol) holds that one's shared_ptr -- freeing the protocol's handle first is allowed, the memory goes
//                 when the last user does.  A freed, never-issued or wrong-kind handle is BadHandle (-> MI355_EBADARG) with the expected kind in the message.
//   Options       name = value pairs as text, checked against ONE table of (name, type, range).  Only what was set is stored: the defaults stay where they are defined,
//                 in ProofOptions / VerifyOptions / CheckOptions, and lib_plonk.cpp overrides just the named fields.
//   JsonWriter    strict JSON (RFC 8259): escaped strings, no NaN / Infinity (null instead), 64-bit integers exact.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace mi355zk {
namespace capi {

// ------------------------------------------------------------------------------------------------ handles
enum class Kind : uint32_t { None = 0, Protocol, Circuit, Key, Options, Record };
inline const char *kind_name(Kind k) {
  switch (k) {
    case Kind::Protocol: return "protocol";
    case Kind::Circuit: return "circuit";
    case Kind::Key: return "proving key";
    case Kind::Options: return "options";
    case Kind::Record: return "record";
    default: return "none";
  }
}
struct BadHandle : std::invalid_argument { using std::invalid_argument::invalid_argument; };

class HandleTable {
 public:
  uint64_t issue(Kind kind, std::shared_ptr<void> obj) {
    if (kind == Kind::None || !obj) throw std::invalid_argument("handle table: nothing to issue");
    std::lock_guard<std::mutex> lk(mu_);
    const uint64_t h = next_++;
    live_.emplace(h, Entry{kind, std::move(obj)});
    return h;
  }
  // the object behind `h` when it is live and of kind `want`; BadHandle otherwise (the object is never touched)
  std::shared_ptr<void> get(uint64_t h, Kind want) const {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = live_.find(h);
    if (it == live_.end()) throw BadHandle(std::string("handle ") + std::to_string(h) + " is no live " + kind_name(want) + " handle (" + (h != 0 && h < next_ ? "already freed" : "never issued") + ")");
    if (it->second.kind != want) throw BadHandle(std::string("handle ") + std::to_string(h) + " is a " + kind_name(it->second.kind) + " handle, a " + kind_name(want) + " handle is expected");
    return it->second.obj;
  }
  Kind kind_of(uint64_t h) const { std::lock_guard<std::mutex> lk(mu_); auto it = live_.find(h); return it == live_.end() ? Kind::None : it->second.kind; }
  // take the entry out; the caller drops the returned pointer OUTSIDE the table's lock (a key's destructor calls back into the library)
  std::shared_ptr<void> release(uint64_t h) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = live_.find(h);
    if (it == live_.end()) throw BadHandle(std::string("handle ") + std::to_string(h) + " is no live handle (" + (h != 0 && h < next_ ? "already freed" : "never issued") + ")");
    std::shared_ptr<void> obj = std::move(it->second.obj);
    live_.erase(it);
    return obj;
  }
  size_t live() const { std::lock_guard<std::mutex> lk(mu_); return live_.size(); }
  uint64_t issued() const { std::lock_guard<std::mutex> lk(mu_); return next_ - 1; }

 private:
  struct Entry { Kind kind; std::shared_ptr<void> obj; };
  mutable std::mutex mu_;
  uint64_t next_ = 1;
  std::unordered_map<uint64_t, Entry> live_;
};

// ------------------------------------------------------------------------------------------------ options
// transcript codes follow mi355zk::plonk::TranscriptKind (lib_plonk.cpp static_asserts the order)
enum : int64_t { TRANSCRIPT_BLAKE2B = 0, TRANSCRIPT_POSEIDON = 1, TRANSCRIPT_EVM = 2, TRANSCRIPT_BY_LAYER = 3 };
enum class OptType : uint8_t { Bool, Int, Uint, Hex32, Transcript };
struct OptSpec { const char *name; OptType type; int64_t lo; uint64_t hi; const char *of; };
// the field names of ProofOptions, VerifyOptions (plus VerifyingKeyRef's initial_state) and CheckOptions; `threads` and `transcript` are shared by the structs that have them
inline const std::vector<OptSpec> &option_specs() {
  static const std::vector<OptSpec> t = {
      {"devices", OptType::Int, 1, 16, "ProofOptions"},
      {"threads", OptType::Int, 1, 1024, "ProofOptions, CheckOptions"},
      {"commit_batch", OptType::Uint, 0, 1u << 20, "ProofOptions"},
      {"upload_threads", OptType::Int, 1, 256, "ProofOptions"},
      {"early_intt", OptType::Int, -1, 1, "ProofOptions"},
      {"sparse_uploads", OptType::Bool, 0, 1, "ProofOptions"},
      {"packed_multiplicities", OptType::Bool, 0, 1, "ProofOptions"},
      {"device_multiplicities", OptType::Bool, 0, 1, "ProofOptions"},
      {"multiplicity_rule_last", OptType::Bool, 0, 1, "ProofOptions"},
      {"check_witness", OptType::Bool, 0, 1, "ProofOptions"},
      {"device_randomness", OptType::Bool, 0, 1, "ProofOptions"},
      {"rng_key", OptType::Hex32, 0, 0, "ProofOptions"},
      {"rng_key_from_os", OptType::Bool, 0, 1, "ProofOptions"},
      {"coset_group_polys", OptType::Uint, 0, 0xffffffffull, "ProofOptions"},
      {"transcript", OptType::Transcript, 0, 3, "ProofOptions, VerifyOptions"},
      {"check_accumulator", OptType::Bool, 0, 1, "VerifyOptions"},
      {"accumulator", OptType::Int, -1, 1, "VerifyOptions"},
      {"host_only", OptType::Bool, 0, 1, "VerifyOptions"},
      {"device_transcript", OptType::Bool, 0, 1, "VerifyOptions"},
      {"device_scalars", OptType::Bool, 0, 1, "VerifyOptions"},
      {"initial_state", OptType::Hex32, 0, 0, "VerifyingKeyRef"},
      {"cap", OptType::Uint, 0, 65536, "CheckOptions"},
      {"theta_seed", OptType::Uint, 0, ~uint64_t(0), "CheckOptions"},
  };
  return t;
}
struct OptValue { int64_t i = 0; uint64_t u = 0; std::array<uint8_t, 32> bytes{}; };

namespace detail {
inline int hex_digit(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
// decimal, optional sign; false on anything else (empty, spaces, trailing text, overflow)
inline bool parse_u64(const std::string &s, uint64_t &out) {
  if (s.empty() || s.size() > 20) return false;
  uint64_t v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return false;
    const uint64_t d = (uint64_t)(c - '0');
    if (v > (~uint64_t(0) - d) / 10) return false;
    v = v * 10 + d;
  }
  out = v; return true;
}
inline bool parse_i64(const std::string &s, int64_t &out) {
  const bool neg = !s.empty() && s[0] == '-';
  uint64_t m = 0;
  if (!parse_u64(neg ? s.substr(1) : s, m)) return false;
  if (m > (uint64_t)INT64_MAX) return false;
  out = neg ? -(int64_t)m : (int64_t)m; return true;
}
}  // namespace detail

struct Options {
  std::map<std::string, OptValue> values;   // only what was set

  const OptValue *find(const char *name) const { auto it = values.find(name); return it == values.end() ? nullptr : &it->second; }
  // name = value, both as text; std::invalid_argument naming the option for an unknown name or a value that does not parse or lies outside the range
  void set(const char *name, const char *value) {
    if (!name || !value) throw std::invalid_argument("options: null name or value");
    const OptSpec *spec = nullptr;
    for (const auto &s : option_specs()) if (std::strcmp(s.name, name) == 0) spec = &s;
    if (!spec) throw std::invalid_argument(std::string("options: unknown option '") + printable(name) + "'");
    const std::string v = value;
    auto bad = [&](const char *want) -> std::invalid_argument { return std::invalid_argument(std::string("options: ") + name + " = '" + printable(value) + "' is not " + want); };
    OptValue o;
    switch (spec->type) {
      case OptType::Bool:
        if (v == "1" || v == "true") o.i = 1; else if (v == "0" || v == "false") o.i = 0; else throw bad("a boolean (0, 1, true, false)");
        o.u = (uint64_t)o.i; break;
      case OptType::Int:
        if (!detail::parse_i64(v, o.i) || o.i < spec->lo || o.i > (int64_t)spec->hi) throw bad(("an integer in [" + std::to_string(spec->lo) + ", " + std::to_string(spec->hi) + "]").c_str());
        o.u = (uint64_t)o.i; break;
      case OptType::Uint:
        if (!detail::parse_u64(v, o.u) || o.u < (uint64_t)spec->lo || o.u > spec->hi) throw bad(("an integer in [" + std::to_string(spec->lo) + ", " + std::to_string(spec->hi) + "]").c_str());
        o.i = (int64_t)o.u; break;
      case OptType::Hex32:
        if (v.size() != 64) throw bad("64 hexadecimal digits");
        for (size_t k = 0; k < 32; k++) {
          const int hi = detail::hex_digit(v[2 * k]), lo = detail::hex_digit(v[2 * k + 1]);
          if (hi < 0 || lo < 0) throw bad("64 hexadecimal digits");
          o.bytes[k] = (uint8_t)(hi * 16 + lo);
        }
        break;
      case OptType::Transcript:
        if (v == "blake2b") o.i = TRANSCRIPT_BLAKE2B; else if (v == "poseidon") o.i = TRANSCRIPT_POSEIDON; else if (v == "evm") o.i = TRANSCRIPT_EVM;
        else if (v == "by_layer" || v == "auto") o.i = TRANSCRIPT_BY_LAYER; else throw bad("one of blake2b, poseidon, evm, by_layer");
        o.u = (uint64_t)o.i; break;
    }
    values[name] = o;
  }
  // what goes into an error message of a caller's text: printable ASCII only, cut at 64 characters
  static std::string printable(const char *s) {
    std::string o;
    for (size_t i = 0; s[i] && i < 64; i++) o.push_back(s[i] >= 0x20 && s[i] < 0x7f ? s[i] : '?');
    return o;
  }
};

// ------------------------------------------------------------------------------------------------ records
class JsonWriter {
 public:
  JsonWriter &begin_object() { open('{'); return *this; }
  JsonWriter &end_object() { close('}'); return *this; }
  JsonWriter &begin_array() { open('['); return *this; }
  JsonWriter &end_array() { close(']'); return *this; }
  JsonWriter &key(const std::string &k) {
    if (stack_.empty() || stack_.back().array || stack_.back().after_key) throw std::logic_error("json writer: a key outside an object");
    comma(); string_(k); out_ += ':'; stack_.back().after_key = true; return *this;
  }
  JsonWriter &value(const std::string &s) { before_value(); string_(s); return *this; }
  JsonWriter &value(const char *s) { return value(std::string(s ? s : "")); }
  JsonWriter &value(bool b) { before_value(); out_ += b ? "true" : "false"; return *this; }
  JsonWriter &value(uint64_t v) { before_value(); out_ += std::to_string(v); return *this; }
  JsonWriter &value(int64_t v) { before_value(); out_ += std::to_string(v); return *this; }
  JsonWriter &value(uint32_t v) { return value((uint64_t)v); }
  JsonWriter &value(int v) { return value((int64_t)v); }
  JsonWriter &value(double d) {
    before_value();
    if (!std::isfinite(d)) { out_ += "null"; return *this; }
    char b[40]; std::snprintf(b, sizeof b, "%.17g", d);
    out_ += b;
    if (!std::strpbrk(b, ".eE")) out_ += ".0";   // a double stays a JSON number with a fraction: 3 -> 3.0
    return *this;
  }
  JsonWriter &null() { before_value(); out_ += "null"; return *this; }
  // bytes as lower-case hexadecimal text
  JsonWriter &hex(const void *p, size_t n) {
    static const char *d = "0123456789abcdef"; std::string s; s.reserve(2 * n);
    for (size_t i = 0; i < n; i++) { const uint8_t b = static_cast<const uint8_t *>(p)[i]; s.push_back(d[b >> 4]); s.push_back(d[b & 15]); }
    return value(s);
  }
  bool complete() const { return stack_.empty() && !out_.empty(); }
  const std::string &str() const { if (!stack_.empty()) throw std::logic_error("json writer: unclosed container"); return out_; }

 private:
  struct Level { bool array; bool any = false; bool after_key = false; };
  std::string out_; std::vector<Level> stack_;
  void comma() { if (stack_.back().any) out_ += ','; stack_.back().any = true; }
  void before_value() {
    if (stack_.empty()) { if (!out_.empty()) throw std::logic_error("json writer: two top-level values"); return; }
    Level &l = stack_.back();
    if (l.array) comma(); else { if (!l.after_key) throw std::logic_error("json writer: a value without a key"); l.after_key = false; }
  }
  void open(char c) { before_value(); out_ += c; stack_.push_back(Level{c == '['}); }
  void close(char c) {
    if (stack_.empty() || stack_.back().array != (c == ']') || stack_.back().after_key) throw std::logic_error("json writer: mismatched close");
    stack_.pop_back(); out_ += c;
  }
  // every byte outside printable ASCII goes out as \u00XX: the text stays valid JSON (and ASCII) whatever an error message carries
  void string_(const std::string &s) {
    out_ += '"';
    for (unsigned char c : s) {
      if (c == '"') out_ += "\\\""; else if (c == '\\') out_ += "\\\\"; else if (c == '\n') out_ += "\\n"; else if (c == '\t') out_ += "\\t"; else if (c == '\r') out_ += "\\r";
      else if (c < 0x20 || c >= 0x7f) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", (unsigned)c); out_ += b; }
      else out_ += (char)c;
    }
    out_ += '"';
  }
};
struct Record { std::string json; };

// the size-query convention of every mi355_plonk_* call that returns bytes: *bytes_out = the size; cap == 0 asks for it alone; a cap that is too small is an error
inline void copy_out(const void *src, uint64_t bytes, void *out, uint64_t cap, uint64_t *bytes_out, const char *what) {
  if (!bytes_out) throw std::invalid_argument(std::string(what) + ": bytes_out is null");
  *bytes_out = bytes;
  if (cap == 0) return;
  if (!out) throw std::invalid_argument(std::string(what) + ": the output pointer is null");
  if (cap < bytes) throw std::invalid_argument(std::string(what) + ": " + std::to_string(bytes) + " bytes do not fit a buffer of " + std::to_string(cap));
  if (bytes) std::memcpy(out, src, bytes);
}

}  // namespace capi
}  // namespace mi355zk
