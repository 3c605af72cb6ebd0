// lib_plonk.cpp -- the sixth translation unit of libmi355zk.so: the mi355_plonk_* entry points of include/mi355zk.h, i.e. plonk::keygen / create_proof / check_witness /
// verify_proof / verify_proofs / aggregate (include/mi355zk_plonk*.hpp, mi355zk_transcript.hpp, mi355zk_plonk_verify.hpp) behind extern "C".  HOST CODE ONLY: no kernel is
// declared or launched here; the headers reach the device through the library's own C-ABI, exactly as a program under tests/cpp/ does, so a proof made through this unit issues
// the launches of that program and writes its bytes.
//
//   exception barrier   every entry point runs inside barrier(): halo2::Error keeps its code, std::bad_alloc is MI355_EOOM, every other std::exception (invalid_argument and the
//                       protocol / layout complaints of the headers) and anything else is MI355_EBADARG; the text goes to the calling thread's mi355_last_error() slot
//   symbol visibility   build.py compiles this unit with -fvisibility=hidden: the inline functions of the headers and their function statics (vdetail::phase_times(),
//                       device_calls(), detail::small_table(), gate_stats()) are PRIVATE copies of the library.  The programs under tests/cpp/ compile the same inline functions
//                       and link the library; exported copies would interpose and the two would share those statics.  Only the mi355_plonk_* functions below are exported
//   handles, options, records   csrc/plonk_capi.hpp (plain C++, checked on the host under the sanitizers)
//   threading           see include/mi355zk.h: one thread per object at a time; the verify family serialises on g_verify_mu
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mi355zk_plonk.hpp"
#include "../../include/mi355zk_transcript.hpp"
#include "../../include/mi355zk_plonk_verify.hpp"
#include "plonk_capi.hpp"

namespace mi355 {
int fail(int code, const std::string &msg);   // lib_core.hip: stores the message in the thread's mi355_last_error() slot and returns the code
}

namespace {
using namespace mi355zk;
using namespace mi355zk::plonk;
using capi::Kind;

static_assert((int)TranscriptKind::Blake2b == capi::TRANSCRIPT_BLAKE2B && (int)TranscriptKind::Poseidon == capi::TRANSCRIPT_POSEIDON && (int)TranscriptKind::Evm == capi::TRANSCRIPT_EVM &&
              (int)TranscriptKind::ByLayer == capi::TRANSCRIPT_BY_LAYER, "csrc/plonk_capi.hpp numbers the transcripts as TranscriptKind does");

struct ProtocolObj { Protocol P; };
struct CircuitObj { std::shared_ptr<ProtocolObj> proto; std::unique_ptr<Circuit> C; };
struct KeyObj { std::shared_ptr<ProtocolObj> proto; std::unique_ptr<ProvingKey> pk; };   // the key's device blocks go back to the pool with the last reference

capi::HandleTable &table() { static capi::HandleTable &t = *new capi::HandleTable(); return t; }   // never destroyed: a key freed by a late destructor still finds it
std::mutex g_verify_mu;

template <class T> std::shared_ptr<T> object(uint64_t h, Kind k) { return std::static_pointer_cast<T>(table().get(h, k)); }
std::shared_ptr<capi::Options> options_or_default(uint64_t h) { return h ? object<capi::Options>(h, Kind::Options) : std::make_shared<capi::Options>(); }

template <class F> int barrier(const char *fn, F &&body) noexcept {
  try { return body(); }
  catch (const halo2::Error &e) { return mi355::fail(e.code, std::string(fn) + ": " + e.what()); }
  catch (const std::bad_alloc &) { return mi355::fail(MI355_EOOM, std::string(fn) + ": out of host memory"); }
  catch (const std::exception &e) { return mi355::fail(MI355_EBADARG, std::string(fn) + ": " + e.what()); }
  catch (...) { return mi355::fail(MI355_EBADARG, std::string(fn) + ": unknown exception"); }
}
void need(const void *p, const char *what) { if (!p) throw std::invalid_argument(std::string(what) + " is null"); }
// "the device is looked up first": MI355_ENODEVICE before any other argument is judged
void need_device() { halo2::check(mi355_mem_info(0, nullptr, nullptr, nullptr, nullptr, nullptr)); }

// ---- options -> the structs of the headers: only what was set overrides a default
TranscriptKind transcript_of(int64_t code) { return (TranscriptKind)code; }
ProofOptions proof_options(const capi::Options &o) {
  ProofOptions p;
  if (auto v = o.find("devices")) p.devices = (int)v->i;
  if (auto v = o.find("threads")) p.threads = (int)v->i;
  if (auto v = o.find("commit_batch")) p.commit_batch = (uint32_t)v->u;
  if (auto v = o.find("upload_threads")) p.upload_threads = (int)v->i;
  if (auto v = o.find("early_intt")) p.early_intt = (int)v->i;
  if (auto v = o.find("sparse_uploads")) p.sparse_uploads = v->i != 0;
  if (auto v = o.find("packed_multiplicities")) p.packed_multiplicities = v->i != 0;
  if (auto v = o.find("device_multiplicities")) p.device_multiplicities = v->i != 0;
  if (auto v = o.find("multiplicity_rule_last")) p.multiplicity_rule_last = v->i != 0;
  if (auto v = o.find("check_witness")) p.check_witness = v->i != 0;
  if (auto v = o.find("device_randomness")) p.device_randomness = v->i != 0;
  if (auto v = o.find("rng_key")) std::memcpy(p.rng_key, v->bytes.data(), 32);
  if (auto v = o.find("rng_key_from_os")) p.rng_key_from_os = v->i != 0;
  if (auto v = o.find("coset_group_polys")) p.coset_group_polys = (uint32_t)v->u;
  if (auto v = o.find("transcript")) p.transcript = transcript_of(v->i);
  return p;
}
VerifyOptions verify_options(const capi::Options &o) {
  VerifyOptions p;
  if (auto v = o.find("transcript")) p.transcript = transcript_of(v->i);
  if (auto v = o.find("check_accumulator")) p.check_accumulator = v->i != 0;
  if (auto v = o.find("accumulator")) p.accumulator = (int)v->i;
  if (auto v = o.find("host_only")) p.host_only = v->i != 0;
  if (auto v = o.find("device_transcript")) p.device_transcript = v->i != 0;
  if (auto v = o.find("device_scalars")) p.device_scalars = v->i != 0;
  return p;
}
CheckOptions check_options(const capi::Options &o) {
  CheckOptions p;
  if (auto v = o.find("threads")) p.threads = (int)v->i;
  if (auto v = o.find("cap")) p.cap = (uint32_t)v->u;
  if (auto v = o.find("theta_seed")) p.theta_seed = v->u;
  return p;
}
Fr fr_from_be(const uint8_t *p) {   // any 256-bit big-endian word, reduced mod r
  zk::fe_t c; uint8_t *le = reinterpret_cast<uint8_t *>(&c); for (int i = 0; i < 32; i++) le[i] = p[31 - i];
  uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = zk::FrP::mod(i);
  while (zk::Fr::w_geq(c.l, m)) zk::Fr::w_sub(c.l, m);
  return halo2::detail::from_fe(zk::Fr::from_canonical(c));
}

// ---- records
std::string hex_of(const zk::fe_t &canonical) { char b[65]; for (int i = 0; i < 8; i++) std::snprintf(b + 8 * i, 9, "%08x", canonical.l[7 - i]); return std::string(b, 64); }
std::string fr_hex(const Fr &a) { return hex_of(zk::Fr::to_canonical(halo2::detail::to_fe(a))); }
void put_point(capi::JsonWriter &w, const halo2::G1Affine &a) {
  zk::fe_t x, y; std::memcpy(&x, a.data(), 32); std::memcpy(&y, a.data() + 4, 32);
  w.begin_array().value(hex_of(zk::Fq::to_canonical(x))).value(hex_of(zk::Fq::to_canonical(y))).end_array();
}
uint64_t issue_record(const capi::JsonWriter &w) { auto r = std::make_shared<capi::Record>(); r->json = w.str(); return table().issue(Kind::Record, r); }

void put_failures(capi::JsonWriter &w, const std::vector<VerifyFailure> &fs) {
  w.key("n_failures").value((uint64_t)fs.size()).key("failures").begin_array();
  for (const auto &f : fs)
    w.begin_object().key("kind").value(failure_kind_name(f.kind)).key("index").value(f.index).key("row").value(f.row).key("count").value(f.count).key("col_a").value(f.col_a)
        .key("col_b").value(f.col_b).key("row_b").value(f.row_b).key("message").value(describe(f)).end_object();
  w.end_array();
}
void put_proof_result(capi::JsonWriter &w, const ProofResult &R, TranscriptKind kind) {
  static const char *steps[11] = {nullptr, "1_instance", "2_3_advice_lookup_commits", nullptr, "4_products", "5_random", "6_to_coeff", "7_quotient", "8_commit_h", "9_evals", "10_shplonk"};
  w.key("ok").value(true).key("proof_bytes").value((uint64_t)R.proof.size()).key("transcript").value(transcript_name(kind)).key("total_ms").value(R.total_ms).key("step_ms").begin_object();
  for (int i = 0; i < 11; i++) if (steps[i]) w.key(steps[i]).value(R.step_ms[i]);
  w.end_object();
  w.key("msm").value(R.msm).key("intt").value(R.intt).key("coset_ntt").value(R.coset_ntt).key("gate_launches").value(R.gate_launches).key("evals").value(R.evals).key("rotation_sets").value(R.rotation_sets);
  w.key("plan_launches").value(R.plan_launches).key("plan_terms").value(R.plan_terms).key("plan_tmps").value(R.plan_tmps).key("plan_constraints").value(R.plan_constraints).key("plan_prefix_groups").value(R.plan_prefix_groups);
  w.key("peak_hbm_bytes").value(R.peak_hbm_bytes).key("hbm_total_bytes").value(R.hbm_total_bytes).key("sparse_columns").value(R.sparse_columns).key("packed_columns").value(R.packed_columns)
      .key("witness_link_bytes").value(R.witness_link_bytes).key("coset_groups").value(R.coset_groups).key("coset_retransforms").value(R.coset_retransforms)
      .key("random_ms").value(R.random_ms).key("multiplicity_ms").value(R.multiplicity_ms);
}
// the record of tests/cpp/test_verify_proofs.cpp, key for key
void put_verify_result(capi::JsonWriter &w, const VerifyResult &r, bool host_only) {
  w.begin_object().key("ok").value(r.ok).key("error").value(r.error).key("detail").value(r.detail).key("host_only").value(host_only);
  w.key("challenges").begin_object().key("theta").value(fr_hex(r.theta)).key("beta").value(fr_hex(r.beta)).key("gamma").value(fr_hex(r.gamma)).key("y").value(fr_hex(r.y)).key("x").value(fr_hex(r.x))
      .key("shplonk_y").value(fr_hex(r.shplonk_y)).key("shplonk_v").value(fr_hex(r.shplonk_v)).key("shplonk_u").value(fr_hex(r.shplonk_u)).end_object();
  w.key("numerator_at_x").value(fr_hex(r.numerator_at_x)).key("msm").begin_object().key("scalars").begin_array();
  for (const auto &s : r.msm_scalars) w.value(fr_hex(s));
  w.end_array().key("points").begin_array();
  for (const auto &p : r.msm_points) put_point(w, p);
  w.end_array().key("result"); put_point(w, r.msm_result); w.key("w_prime"); put_point(w, r.w_prime);
  w.end_object().key("has_accumulator").value(r.has_accumulator).key("pairing").begin_array();
  for (uint32_t f : r.pairing) w.value(f);
  w.end_array().end_object();
}

// ---- the parts of a circuit by name
uint32_t sigma_position(const Circuit &C, uint32_t p) { for (size_t t = 0; t < C.pcols.size(); t++) if (C.pcols[t].sigma == p) return (uint32_t)t; return ~0u; }
void index_below(uint32_t index, size_t count, const char *what) { if (index >= count) throw std::invalid_argument(std::string("circuit: ") + what + " index " + std::to_string(index) + " is out of range (the protocol has " + std::to_string(count) + ")"); }
void size_is(uint64_t bytes, uint64_t want, const char *what) { if (bytes != want) throw std::invalid_argument(std::string("circuit: ") + what + " takes " + std::to_string(want) + " bytes for this protocol, " + std::to_string(bytes) + " given"); }
// destination of a fixed-size part: pointer and size in bytes (the containers are sized at construction and never resized by _set)
struct Span { void *p; uint64_t bytes; };
bool fixed_part(Circuit &C, const std::string &what, uint32_t index, Span &out) {
  const Protocol &P = *C.pr; const uint64_t col = P.n * 32, bl = (uint64_t)P.blind * 32;
  if (what == "advice") { index_below(index, C.advice.size(), "advice"); out = {C.advice[index].data(), col}; return true; }
  if (what == "m") { index_below(index, C.m.size(), "m"); out = {C.m[index].data(), col}; return true; }
  if (what == "m_counts") { index_below(index, C.m_counts.size(), "m_counts"); out = {C.m_counts[index].data(), P.n * 4}; return true; }
  if (what == "m_blind") { index_below(index, C.m_blind.size(), "m_blind"); out = {C.m_blind[index].data(), bl}; return true; }
  if (what == "z_blind") { index_below(index, C.z_blind.size(), "z_blind"); out = {C.z_blind[index].data(), bl}; return true; }
  if (what == "phi_blind") { index_below(index, C.phi_blind.size(), "phi_blind"); out = {C.phi_blind[index].data(), bl}; return true; }
  if (what == "perm_blind") { index_below(index, C.perm_blind.size(), "perm_blind"); out = {C.perm_blind[index].data(), 2 * (bl + 32)}; return true; }
  if (what == "lz_blind") { index_below(index, C.lz_blind.size(), "lz_blind"); out = {C.lz_blind[index].data(), bl}; return true; }
  if (what == "random_poly") { index_below(index, 1, "random_poly"); out = {C.random_poly.data(), col}; return true; }
  return false;
}
// every container at the size the protocol gives it (a circuit built by build_circuit already is; the check keeps keygen and create_proof from reading past a column)
void check_shape(const Circuit &C) {
  const Protocol &P = *C.pr; const uint64_t n = P.n; const size_t L = P.lookups.size();
  auto bad = [](const char *w) { throw std::invalid_argument(std::string("circuit: ") + w + " does not have the protocol's shape"); };
  if (C.pre.size() != P.num_pre) bad("preprocessed");
  for (uint32_t p = 0; p < P.num_pre; p++) if (!C.is_sigma(p) && C.pre[p].size() != n) bad("preprocessed");
  if (C.advice.size() != P.num_advice()) bad("advice");
  for (const auto &c : C.advice) if (c.size() != n) bad("advice");
  if (P.permuted_lookups()) {   // no m and no phi: the blinding values of A', S' and the lookups' z
    if (C.perm_blind.size() != L || C.lz_blind.size() != L || C.z_blind.size() != P.perm.size()) bad("the lookup / permutation parts");
    for (size_t l = 0; l < L; l++) if (C.perm_blind[l].size() != 2 * ((size_t)P.blind + 1) || C.lz_blind[l].size() != P.blind) bad("a lookup part");
  }
  else if (C.m.size() != L || C.m_counts.size() != L || C.m_blind.size() != L || C.phi_blind.size() != L || C.z_blind.size() != P.perm.size()) bad("the lookup / permutation parts");
  for (size_t l = 0; l < L && !P.permuted_lookups(); l++) if (C.m[l].size() != n || C.m_counts[l].size() != n || C.m_blind[l].size() != P.blind || C.phi_blind[l].size() != P.blind) bad("a lookup part");
  for (const auto &z : C.z_blind) if (z.size() != P.blind) bad("z_blind");
  if (C.random_poly.size() != n || C.omega_pow.size() != n || C.instances.size() > n) bad("random_poly / instances");
}
std::unique_ptr<Circuit> empty_circuit(const Protocol &P) {
  auto C = std::make_unique<Circuit>(); C->pr = &P;
  const uint64_t n = P.n; const size_t L = P.permuted_lookups() ? 0 : P.lookups.size();
  if (P.permuted_lookups()) { C->perm_blind.assign(P.lookups.size(), std::vector<Fr>(2 * ((size_t)P.blind + 1), fr_zero())); C->lz_blind.assign(P.lookups.size(), std::vector<Fr>(P.blind, fr_zero())); }
  for (const auto &ch : P.perm) for (const auto &c : ch.columns) C->pcols.push_back(c);
  C->pre.resize(P.num_pre);
  for (uint32_t p = 0; p < P.num_pre; p++) if (!C->is_sigma(p)) C->pre[p].assign(n, fr_zero());
  C->advice.resize(P.num_advice()); for (auto &c : C->advice) c.assign(n, fr_zero());
  C->m.resize(L); for (auto &c : C->m) c.assign(n, fr_zero());
  C->m_counts.assign(L, std::vector<uint32_t>(n, 0));
  C->m_blind.assign(L, std::vector<Fr>(P.blind, fr_zero()));
  C->phi_blind.assign(L, std::vector<Fr>(P.blind, fr_zero()));
  C->z_blind.assign(P.perm.size(), std::vector<Fr>(P.blind, fr_zero()));
  C->random_poly.assign(n, fr_zero());
  C->omega_pow.resize(n); { Fr w = fr_one(); for (uint64_t i = 0; i < n; i++) { C->omega_pow[i] = w; w = fr_mul(w, P.omega); } }
  return C;
}

uint64_t protocol_field(const Protocol &P, const std::string &f) {
  uint32_t nw = 0; for (auto w : P.num_witness) nw += w;
  const uint64_t points = (uint64_t)nw + P.Q + 2, ev = P.evaluations.size();
  if (f == "k") return P.k;
  if (f == "n") return P.n;
  if (f == "layer") return (uint64_t)(int64_t)P.layer;
  if (f == "num_preprocessed") return P.num_pre;
  if (f == "num_instance") return P.num_instance.at(0);
  if (f == "num_advice") return P.num_advice();
  if (f == "num_lookups") return P.lookups.size();
  if (f == "num_perm_columns") return P.num_sigma();
  if (f == "num_perm_chunks") return P.perm.size();
  if (f == "num_gates") return P.gates.size();
  if (f == "num_witness") return nw;
  if (f == "num_commitments") return P.commitments();
  if (f == "blind") return P.blind;
  if (f == "usable") return P.usable;
  if (f == "quotient_pieces") return P.Q;
  if (f == "extended_k") return P.extended_k;
  if (f == "num_evaluations") return ev;
  if (f == "num_queries") return P.queries.size();
  if (f == "lookup_bits") return P.lookup_bits;
  if (f == "proof_bytes_poseidon") return points * 32 + ev * 32;
  if (f == "proof_bytes_evm") return points * 64 + ev * 32;
  if (f == "has_initial_state") return P.has_initial_state ? 1 : 0;
  if (f == "has_accumulator") return P.has_accumulator ? 1 : 0;
  if (f == "lookup_permuted") return P.permuted_lookups() ? 1 : 0;
  throw std::invalid_argument("unknown protocol field '" + capi::Options::printable(f.c_str()) + "'");
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int mi355_plonk_protocol_from_json(const char *json, uint64_t len, uint64_t *protocol_out) {
  return barrier("mi355_plonk_protocol_from_json", [&]() -> int {
    need(json, "json"); need(protocol_out, "protocol_out");
    auto obj = std::make_shared<ProtocolObj>(); obj->P.load_text(std::string(json, (size_t)len));
    *protocol_out = table().issue(Kind::Protocol, obj); return MI355_OK;
  });
}
int mi355_plonk_protocol_from_file(const char *path, uint64_t *protocol_out) {
  return barrier("mi355_plonk_protocol_from_file", [&]() -> int {
    need(path, "path"); need(protocol_out, "protocol_out");
    auto obj = std::make_shared<ProtocolObj>(); obj->P.load(path);
    *protocol_out = table().issue(Kind::Protocol, obj); return MI355_OK;
  });
}
int mi355_plonk_protocol_info(uint64_t protocol, const char *field, uint64_t *value_out) {
  return barrier("mi355_plonk_protocol_info", [&]() -> int {
    need(field, "field"); need(value_out, "value_out");
    *value_out = protocol_field(object<ProtocolObj>(protocol, Kind::Protocol)->P, field); return MI355_OK;
  });
}
int mi355_plonk_free(uint64_t handle) {
  return barrier("mi355_plonk_free", [&]() -> int { std::shared_ptr<void> gone = table().release(handle); gone.reset(); return MI355_OK; });
}

int mi355_plonk_circuit_new(uint64_t protocol, uint64_t *circuit_out) {
  return barrier("mi355_plonk_circuit_new", [&]() -> int {
    need(circuit_out, "circuit_out");
    auto obj = std::make_shared<CircuitObj>(); obj->proto = object<ProtocolObj>(protocol, Kind::Protocol);
    obj->C = empty_circuit(obj->proto->P);
    *circuit_out = table().issue(Kind::Circuit, obj); return MI355_OK;
  });
}
int mi355_plonk_circuit_synthetic(uint64_t protocol, uint64_t seed, uint64_t blind_seed, double fill, double assign_density, uint32_t flags, uint64_t *circuit_out) {
  return barrier("mi355_plonk_circuit_synthetic", [&]() -> int {
    need(circuit_out, "circuit_out");
    if (flags & ~3u) throw std::invalid_argument("flags: bit 0 (pinned) and bit 1 (zero_blinding) are defined");
    if (!(fill > 0.0 && fill <= 1.0) || !(assign_density >= 0.0 && assign_density <= 1.0)) throw std::invalid_argument("fill must lie in (0, 1] and assign_density in [0, 1]");
    auto obj = std::make_shared<CircuitObj>(); obj->proto = object<ProtocolObj>(protocol, Kind::Protocol);
    CircuitOptions co; co.seed = seed; co.blind_seed = blind_seed; co.fill = fill; co.assign_density = assign_density; co.pinned = flags & 1; co.zero_blinding = (flags & 2) != 0;
    obj->C = build_circuit(obj->proto->P, co);
    *circuit_out = table().issue(Kind::Circuit, obj); return MI355_OK;
  });
}
int mi355_plonk_circuit_set(uint64_t circuit, const char *what, uint32_t index, const void *data, uint64_t bytes) {
  return barrier("mi355_plonk_circuit_set", [&]() -> int {
    need(what, "what"); if (bytes) need(data, "data");
    auto obj = object<CircuitObj>(circuit, Kind::Circuit); Circuit &C = *obj->C; const Protocol &P = *C.pr; const std::string w = what;
    Span s;
    if (w == "preprocessed") {
      index_below(index, P.num_pre, "preprocessed");
      if (C.is_sigma(index)) throw std::invalid_argument("circuit: preprocessed column " + std::to_string(index) + " is a sigma column: it follows from the copies");
      size_is(bytes, P.n * 32, "preprocessed"); std::memcpy(C.pre[index].data(), data, bytes);
    } else if (fixed_part(C, w, index, s)) { size_is(bytes, s.bytes, what); std::memcpy(s.p, data, bytes); }
    else if (w == "instances") {
      index_below(index, 1, "instances");
      if (bytes % 32 || bytes / 32 > P.num_instance.at(0) || bytes / 32 > P.n) throw std::invalid_argument("circuit: instances takes at most " + std::to_string(P.num_instance.at(0)) + " words of 32 bytes, " + std::to_string(bytes) + " bytes given");
      std::vector<Fr> v(bytes / 32); if (bytes) std::memcpy(v.data(), data, bytes); C.instances.swap(v);
    } else if (w == "copies") {
      index_below(index, 1, "copies");
      if (bytes % 32) throw std::invalid_argument("circuit: copies takes records of four 64-bit words, " + std::to_string(bytes) + " bytes given");
      std::vector<CopyPair> v(bytes / 32); const size_t NP = C.pcols.size();
      for (size_t i = 0; i < v.size(); i++) {
        uint64_t r[4]; std::memcpy(r, static_cast<const char *>(data) + 32 * i, 32);
        if (r[0] >= NP || r[2] >= NP || r[1] >= P.n || r[3] >= P.n) throw std::invalid_argument("circuit: copy " + std::to_string(i) + " names a cell outside the permutation (" + std::to_string(NP) + " columns of " + std::to_string(P.n) + " rows)");
        v[i] = {(uint32_t)r[0], r[1], (uint32_t)r[2], r[3]};
      }
      C.pairs.swap(v);
    } else throw std::invalid_argument("circuit: unknown part '" + capi::Options::printable(what) + "'");
    return MI355_OK;
  });
}
int mi355_plonk_circuit_get(uint64_t circuit, const char *what, uint32_t index, void *out, uint64_t cap, uint64_t *bytes_out) {
  return barrier("mi355_plonk_circuit_get", [&]() -> int {
    need(what, "what");
    auto obj = object<CircuitObj>(circuit, Kind::Circuit); Circuit &C = *obj->C; const Protocol &P = *C.pr; const std::string w = what;
    Span s;
    if (w == "preprocessed") {
      index_below(index, P.num_pre, "preprocessed");
      const uint32_t j = sigma_position(C, index);
      if (j == ~0u) capi::copy_out(C.pre[index].data(), P.n * 32, out, cap, bytes_out, what);
      else if (cap == 0) capi::copy_out(nullptr, P.n * 32, out, cap, bytes_out, what);
      else { std::vector<Fr> sig; C.sigma_column(j, sig); capi::copy_out(sig.data(), P.n * 32, out, cap, bytes_out, what); }
    } else if (fixed_part(C, w, index, s)) capi::copy_out(s.p, s.bytes, out, cap, bytes_out, what);
    else if (w == "instances") { index_below(index, 1, "instances"); capi::copy_out(C.instances.data(), C.instances.size() * 32, out, cap, bytes_out, what); }
    else if (w == "copies") {
      index_below(index, 1, "copies");
      std::vector<uint64_t> v; v.reserve(4 * C.pairs.size());
      for (const auto &p : C.pairs) { v.push_back(p.ja); v.push_back(p.ra); v.push_back(p.jb); v.push_back(p.rb); }
      capi::copy_out(v.data(), v.size() * 8, out, cap, bytes_out, what);
    } else throw std::invalid_argument("circuit: unknown part '" + capi::Options::printable(what) + "'");
    return MI355_OK;
  });
}

int mi355_plonk_keygen(uint64_t protocol, uint64_t circuit, uint64_t srs_g_lagrange, uint32_t flags, int devices, uint64_t *pk_out) {
  return barrier("mi355_plonk_keygen", [&]() -> int {
    need_device();
    need(pk_out, "pk_out");
    if (flags & ~3u) throw std::invalid_argument("flags: bit 0 (resident cosets) and bit 1 (device_sigma) are defined");
    if (devices < 1 || devices > 16) throw std::invalid_argument("devices must lie in [1, 16]");
    auto proto = object<ProtocolObj>(protocol, Kind::Protocol); auto circ = object<CircuitObj>(circuit, Kind::Circuit);
    if (circ->proto.get() != proto.get()) throw std::invalid_argument("the circuit was made for another protocol handle");
    check_shape(*circ->C);
    uint64_t srs_n = 0; halo2::check(mi355_srs_len(srs_g_lagrange, &srs_n));
    if (srs_n < proto->P.n) throw std::invalid_argument("srs_g_lagrange holds " + std::to_string(srs_n) + " points, the protocol needs " + std::to_string(proto->P.n));
    auto obj = std::make_shared<KeyObj>(); obj->proto = proto;
    obj->pk = keygen(proto->P, *circ->C, srs_g_lagrange, (flags & 1) != 0, devices, (flags & 2) != 0);
    *pk_out = table().issue(Kind::Key, obj); return MI355_OK;
  });
}
int mi355_plonk_pk_vk(uint64_t pk, void *out, uint64_t cap, uint64_t *bytes_out) {
  return barrier("mi355_plonk_pk_vk", [&]() -> int {
    auto key = object<KeyObj>(pk, Kind::Key);
    capi::copy_out(key->pk->vk.data(), key->pk->vk.size(), out, cap, bytes_out, "vk"); return MI355_OK;
  });
}

int mi355_plonk_options_new(uint64_t *opts_out) {
  return barrier("mi355_plonk_options_new", [&]() -> int { need(opts_out, "opts_out"); *opts_out = table().issue(Kind::Options, std::make_shared<capi::Options>()); return MI355_OK; });
}
int mi355_plonk_options_set(uint64_t opts, const char *name, const char *value) {
  return barrier("mi355_plonk_options_set", [&]() -> int { object<capi::Options>(opts, Kind::Options)->set(name, value); return MI355_OK; });
}

int mi355_plonk_create_proof(uint64_t srs_g, uint64_t srs_g_lagrange, uint64_t pk, uint64_t circuit, uint64_t opts, void *proof_out, uint64_t cap, uint64_t *bytes_out, uint64_t *record_out) {
  return barrier("mi355_plonk_create_proof", [&]() -> int {
    need_device();
    need(proof_out, "proof_out"); need(bytes_out, "bytes_out");
    if (record_out) *record_out = 0;
    auto key = object<KeyObj>(pk, Kind::Key); auto circ = object<CircuitObj>(circuit, Kind::Circuit);
    if (circ->proto.get() != key->proto.get()) throw std::invalid_argument("the circuit and the proving key were made for different protocol handles");
    const ProofOptions po = proof_options(*options_or_default(opts)); const Protocol &P = key->proto->P;
    check_shape(*circ->C);
    const TranscriptKind kind = po.transcript == TranscriptKind::ByLayer ? reference_transcript(P) : po.transcript;
    const uint64_t size = protocol_field(P, kind == TranscriptKind::Evm ? "proof_bytes_evm" : "proof_bytes_poseidon");
    *bytes_out = size;
    if (cap < size) throw std::invalid_argument("the proof has " + std::to_string(size) + " bytes, the buffer " + std::to_string(cap));
    try {
      const ProofResult R = create_proof(srs_g, srs_g_lagrange, *key->pk, *circ->C, po);
      if (R.proof.size() != size) throw std::logic_error("the proof has " + std::to_string(R.proof.size()) + " bytes, the protocol says " + std::to_string(size));
      std::memcpy(proof_out, R.proof.data(), R.proof.size());
      if (record_out) { capi::JsonWriter w; w.begin_object().key("kind").value("proof"); put_proof_result(w, R, kind); w.end_object(); *record_out = issue_record(w); }
    } catch (const WitnessError &e) {   // check_witness refused the witness: nothing was written to the transcript, nothing goes to proof_out
      if (record_out) { capi::JsonWriter w; w.begin_object().key("kind").value("proof").key("ok").value(false).key("error").value(e.what()); put_failures(w, e.failures); w.end_object(); *record_out = issue_record(w); }
      throw;
    }
    return MI355_OK;
  });
}
int mi355_plonk_check_witness(uint64_t pk, uint64_t circuit, uint64_t opts, uint64_t *n_failures_out, uint64_t *record_out) {
  return barrier("mi355_plonk_check_witness", [&]() -> int {
    need_device();
    need(n_failures_out, "n_failures_out");
    if (record_out) *record_out = 0;
    auto key = object<KeyObj>(pk, Kind::Key); auto circ = object<CircuitObj>(circuit, Kind::Circuit);
    if (circ->proto.get() != key->proto.get()) throw std::invalid_argument("the circuit and the proving key were made for different protocol handles");
    check_shape(*circ->C);
    const std::vector<VerifyFailure> fs = check_witness(*key->pk, *circ->C, check_options(*options_or_default(opts)));
    *n_failures_out = fs.size();
    if (record_out) { capi::JsonWriter w; w.begin_object().key("kind").value("check"); put_failures(w, fs); w.end_object(); *record_out = issue_record(w); }
    return MI355_OK;
  });
}

int mi355_plonk_verify_proofs(uint32_t n, const uint64_t *protocols, const void *const *vk_bytes, const uint64_t *vk_len, const void *const *instances, const uint64_t *n_instances,
                              const void *const *proofs, const uint64_t *proof_len, const void *g2, const void *s_g2, uint32_t s_g2_is_negated, uint64_t opts, uint32_t mode,
                              uint8_t *ok_out, uint64_t *record_out) {
  return barrier("mi355_plonk_verify_proofs", [&]() -> int {
    if (mode > 3) throw std::invalid_argument("mode must be 0 (batched), 1 (one by one), 2 (aggregate) or 3 (aggregate, fold only)");
    const auto o = options_or_default(opts); const VerifyOptions vo = verify_options(*o);
    const bool agg = mode >= 2, need_srs = !vo.host_only && mode != 3;
    if (agg && vo.host_only) throw std::invalid_argument("host_only stops before the sums an aggregation folds: modes 2 and 3 need the device");
    if (!vo.host_only) need_device();
    if (record_out) *record_out = 0;
    if (n) { need(protocols, "protocols"); need(instances, "instances"); need(n_instances, "n_instances"); need(proofs, "proofs"); need(proof_len, "proof_len"); need(ok_out, "ok_out"); }
    if (n > (1u << 20)) throw std::invalid_argument("more than 2^20 proofs in one call");
    if (vk_bytes && !vk_len) throw std::invalid_argument("vk_len is null");
    G2Pair srs;
    if (need_srs) {
      need(g2, "g2"); need(s_g2, "s_g2");
      std::array<uint8_t, 128> a, b; std::memcpy(a.data(), g2, 128); std::memcpy(b.data(), s_g2, 128);
      srs = s_g2_is_negated ? G2Pair::from_negated(a, b) : G2Pair::from_params(a, b);
    }
    std::vector<std::shared_ptr<ProtocolObj>> held(n); std::vector<VerifyingKeyRef> keys(n); std::vector<ProofInput> in(n);
    for (uint32_t i = 0; i < n; i++) {
      held[i] = object<ProtocolObj>(protocols[i], Kind::Protocol);
      if (n_instances[i] && !instances[i]) throw std::invalid_argument("instances[" + std::to_string(i) + "] is null");
      if (proof_len[i] && !proofs[i]) throw std::invalid_argument("proofs[" + std::to_string(i) + "] is null");
      if (n_instances[i] > (1u << 24) || proof_len[i] > (1u << 24)) throw std::invalid_argument("proof " + std::to_string(i) + ": more than 2^24 instance values or proof bytes");
      if (vk_bytes && vk_bytes[i]) { if (!vk_len[i] || vk_len[i] > (1u << 24)) throw std::invalid_argument("vk_len[" + std::to_string(i) + "] is out of range"); keys[i].vk_bytes.assign(static_cast<const uint8_t *>(vk_bytes[i]), static_cast<const uint8_t *>(vk_bytes[i]) + vk_len[i]); }
      if (auto v = o->find("initial_state")) { keys[i].initial_state = fr_from_be(v->bytes.data()); keys[i].has_initial_state = true; }
      in[i].protocol = &held[i]->P; in[i].vk = &keys[i]; in[i].opt = vo;
      in[i].instances.resize(n_instances[i]); if (n_instances[i]) std::memcpy(in[i].instances.data(), instances[i], 32 * n_instances[i]);
      in[i].proof.assign(static_cast<const uint8_t *>(proofs[i]), static_cast<const uint8_t *>(proofs[i]) + proof_len[i]);
    }
    std::lock_guard<std::mutex> lk(g_verify_mu);   // the verifier's phase clocks and its device-call counter are function statics of the headers
    const uint64_t calls0 = vdetail::device_calls();
    capi::JsonWriter w; w.begin_object().key("kind").value("verify").key("mode").value(mode);
    std::vector<VerifyResult> res; AggregateResult A;
    if (mode == 0) res = verify_proofs(in, srs);
    else if (mode == 1) for (const auto &p : in) res.push_back(verify_proof(*p.protocol, *p.vk, p.instances, p.proof, srs, p.opt));
    else { A = aggregate(in, mode == 2 ? &srs : nullptr); res = A.proofs; }
    for (uint32_t i = 0; i < n; i++) ok_out[i] = i < res.size() && res[i].ok && (!agg || A.ok) ? 1 : 0;
    w.key("device_calls").value(vdetail::device_calls() - calls0).key("proofs").begin_array();
    for (const auto &r : res) put_verify_result(w, r, vo.host_only);
    w.end_array();
    if (agg) {
      w.key("aggregate").begin_object().key("ok").value(A.ok).key("error").value(A.error).key("detail").value(A.detail).key("accumulators").begin_array();
      for (const auto &a : A.accumulators) { w.begin_array(); put_point(w, a.first); put_point(w, a.second); w.end_array(); }
      w.end_array().key("r").value(fr_hex(A.r)).key("lhs"); put_point(w, A.lhs); w.key("rhs"); put_point(w, A.rhs);
      w.key("limbs").begin_array(); for (const auto &l : A.limbs) w.value(fr_hex(l)); w.end_array().key("pairing").value(A.pairing).end_object();
    }
    w.end_object();
    if (record_out) *record_out = issue_record(w);
    return MI355_OK;
  });
}

int mi355_plonk_record_json(uint64_t record, char *out, uint64_t cap, uint64_t *bytes_out) {
  return barrier("mi355_plonk_record_json", [&]() -> int {
    auto r = object<capi::Record>(record, Kind::Record);
    capi::copy_out(r->json.data(), r->json.size(), out, cap, bytes_out, "record"); return MI355_OK;
  });
}

}  // extern "C"
#pragma GCC visibility pop
