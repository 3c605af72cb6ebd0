// mi355zk_plonk_verify.hpp -- plonk::verify_proof: the verifier of a SHPLONK halo2 proof for any snark-verifier PlonkProtocol, a port of oracle/plonk.py verify()
// [EXT-recalled snark-verifier verifier/plonk.rs, pcs/kzg/multiopen/bdfg21.rs].  Included from mi355zk_plonk.hpp.
//   key         the .vkey bytes | the protocol file's own `preprocessed` and `transcript_initial_state` (the route of the released proofs) | an explicit list and state
//   transcript  the read side of mi355zk_transcript.hpp; a non-canonical scalar, a word that is no curve point, leftover or missing bytes are NAMED failures
//   points      the compressed layouts: ONE mi355_g1_decompress_host call over every point word of the proof (positions follow from the protocol) and of the .vkey;
//               the Evm layout: uncompressed, checked on the curve by the transcript
//   scalars     instance evaluations by Lagrange, the numerator tree at x, h(x) = numerator / (x^n - 1)
//   SHPLONK     rotation sets by first appearance in `queries`, the i-th set at v^i, its j-th polynomial at y^j; everything collapses to ONE (scalars, points) list, summed by
//               mi355_msm_g1_adhoc_host
//   pairing     ONE mi355_pairing_products_host call: group 0 = e(lhs, g2) e(W', -s_g2); group 1 = the carried accumulator when the protocol has one
// Failures of the INPUT (proof, key, instances, protocol) are statuses in VerifyResult::error; only a failing device call throws (halo2::Error, as everywhere in these headers).
// VerifyOptions::host_only stops after the list is built (points decompressed on the host): the verifier's own logic runs without a device.
// plonk::verify_proofs runs the same host part for N proofs and ONE decompression, ONE segmented MSM and ONE pairing call for all of them; plonk::aggregate folds their
// KZG accumulators into the one the next layer's first twelve instances carry (KzgAs).  Both stand further down, behind verify_proof.
// VerifyOptions::device_transcript (off by default) moves the Poseidon transcripts of such a batch onto the device: the transcript section of every Poseidon proof is RECORDED
// (its words and squeeze positions, nothing hashed), ONE mi355_poseidon_transcripts_host call hashes all of them, and the rest of the host part REPLAYS the challenges.
// VerifyOptions::device_scalars (off by default) moves the scalar side of such a batch onto the device: the proofs that ask for it are grouped by protocol, each group's scalar
// side is compiled ONCE into a straight-line Fr program (mi355zk_plonk_scalar.hpp) and ONE mi355_fr_program_host call per group runs it for all of the group's proofs.
#pragma once
#include <chrono>
#include "mi355zk_plonk_protocol.hpp"
#include "mi355zk_transcript.hpp"
#include "mi355zk_plonk_scalar.hpp"

namespace mi355zk {
namespace plonk {

struct G2Pair {   // the two G2 points of the final check, as the pairing takes them: g2 and -[s]g2 (128-byte G2Affine)
  std::array<uint8_t, 128> g2{}, neg_s_g2{};
  static std::array<uint8_t, 128> negate(const std::array<uint8_t, 128> &q) {
    std::array<uint8_t, 128> r = q; zk::fe_t y[2]; std::memcpy(y, q.data() + 64, 64);
    for (auto &c : y) c = zk::Fq::neg(c);   // neg(0) = 0 keeps the identity
    std::memcpy(r.data() + 64, y, 64); return r;
  }
  static G2Pair from_params(const std::array<uint8_t, 128> &g2, const std::array<uint8_t, 128> &s_g2) { G2Pair p; p.g2 = g2; p.neg_s_g2 = negate(s_g2); return p; }   // ParamsKZG's g2 / s_g2
  static G2Pair from_negated(const std::array<uint8_t, 128> &g2, const std::array<uint8_t, 128> &neg_s_g2) { G2Pair p; p.g2 = g2; p.neg_s_g2 = neg_s_g2; return p; }
};
struct VerifyingKeyRef {   // vk_bytes when not empty; else `preprocessed` when not empty; else the protocol file's own.  initial_state overrides the transcript's first scalar
  std::vector<uint8_t> vk_bytes; std::vector<halo2::G1Affine> preprocessed; bool has_initial_state = false; Fr initial_state{};
};
struct VerifyOptions {
  TranscriptKind transcript = TranscriptKind::ByLayer; bool check_accumulator = true; int accumulator = -1 /* -1: as the protocol says; 0 / 1: no / yes */; bool host_only = false;
  // verify_proofs / aggregate: hash this proof's Poseidon transcript on the device, together with every other proof of the batch that asks for it (one more device call per
  // batch).  Proofs read with the EVM or Blake2b transcript, and host_only ones, take the host path inside the same batch.  Every VerifyResult equals the one with the option off.
  // verify_proof (one proof) IGNORES it: one sponge is a serial chain, and the host is the faster place for it.
  bool device_transcript = false;
  // verify_proofs / aggregate: run this proof's scalar side (x^n, the Lagrange values, the numerator at x, the SHPLONK scalars) on the device, together with every other proof
  // of the batch that asks for it and has the same protocol: one more device call per distinct protocol.  host_only proofs take the host path inside the same batch; composes
  // with device_transcript.  Every VerifyResult equals the one with the option off, failures included.  verify_proof (one proof) IGNORES it, as it ignores device_transcript.
  bool device_scalars = false;
};
struct VerifyResult {
  bool ok = false; std::string error;                       // the name of the first failed check ("" when none); `detail` says more
  std::string detail;
  Fr theta{}, beta{}, gamma{}, y{}, x{}, shplonk_y{}, shplonk_v{}, shplonk_u{};
  Fr numerator_at_x{};
  std::vector<Fr> msm_scalars; std::vector<halo2::G1Affine> msm_points; halo2::G1Affine msm_result{}, w_prime{};
  bool has_accumulator = false; halo2::G1Affine acc_lhs{}, acc_rhs{};
  std::vector<uint32_t> pairing;                            // per group: 1 where the product is 1
};

namespace vdetail {
inline bool fq_on_curve(const halo2::G1Affine &a) {
  zk::fe_t x, y; std::memcpy(&x, a.data(), 32); std::memcpy(&y, a.data() + 4, 32);
  zk::fe_t three = zk::Fq::zero(); three.l[0] = 3; three = zk::Fq::from_canonical(three);
  return zk::Fq::eq(zk::Fq::sqr(y), zk::Fq::add(zk::Fq::mul(zk::Fq::sqr(x), x), three));
}

// ---- the HOST PART of one verification, in three steps that plonk::verify_proof runs for one proof and plonk::verify_proofs / plonk::aggregate for many:
//   layout_of     what the proof's length and the key decide before any point is looked at: the transcript, the word counts, every compressed point word
//   decode_words  the words -> affine points (all-zero for a rejected word): one mi355_g1_decompress_host call, or the host decoder
//   host_part     the transcript, the scalar side, the SHPLONK list and the carried accumulator; what VerifyOptions::host_only stops after
// Each returns false after it has written the named failure into `res`.
inline bool failed(VerifyResult &res, const char *name, const std::string &why) { res.ok = false; res.error = name; res.detail = why; return false; }
inline uint64_t &device_calls() { static uint64_t n = 0; return n; }   // how many C-ABI calls that need a device the verifiers of this header have made (the drivers print it)
// where the wall time of verify_proofs / aggregate went, in milliseconds, summed over the calls since the caller last cleared it (the drivers' --bench prints it):
// decode = layouts + the decompression call; record = the recording pass of device_transcript; transcript_call = mi355_poseidon_transcripts_host; host_part = the pass over
// host_part (the scalar side, the SHPLONK list, the accumulator; with the transcript on the host its hashing as well; with device_scalars the compilation of the programs and
// what is left of the host part around them); scalar_call = packing the inputs and mi355_fr_program_host, summed over the groups; msm and pairing = those calls with their packing
struct PhaseTimes { double decode = 0, record = 0, transcript_call = 0, host_part = 0, msm = 0, pairing = 0, scalar_call = 0; };
inline PhaseTimes &phase_times() { static PhaseTimes t; return t; }
struct PhaseClock {
  double &into; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit PhaseClock(double &d) : into(d) {}
  ~PhaseClock() { into += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
struct Layout { TranscriptKind kind = TranscriptKind::Poseidon; size_t nb = 32, n_com = 0, n_ev = 0, vk0 = 0; bool use_vk = false; std::vector<halo2::G1Bytes> words; };
inline bool layout_of(const Protocol &P, const VerifyingKeyRef &vk, const std::vector<uint8_t> &proof, const VerifyOptions &opt, Layout &L, VerifyResult &res) {
  L.kind = opt.transcript == TranscriptKind::ByLayer ? (P.layer == 6 ? TranscriptKind::Evm : TranscriptKind::Poseidon) : opt.transcript;
  L.nb = Transcript(L.kind).point_bytes();
  uint32_t nw = 0; for (auto w : P.num_witness) nw += w;
  L.n_com = nw + P.Q; L.n_ev = P.evaluations.size();
  const size_t expect = (L.n_com + 2) * L.nb + L.n_ev * 32;
  if (proof.size() != expect) return failed(res, "proof_length", "proof has " + std::to_string(proof.size()) + " bytes, the protocol reads " + std::to_string(expect));

  // ---- every compressed point word of the proof (and of the .vkey) through one decompression
  L.use_vk = !vk.vk_bytes.empty();
  if (L.use_vk && vk.vk_bytes.size() != 8 + 32 * (size_t)P.num_pre) return failed(res, "vk_length", "the .vkey has " + std::to_string(vk.vk_bytes.size()) + " bytes, the protocol has " + std::to_string(P.num_pre) + " preprocessed polynomials");
  std::vector<halo2::G1Bytes> &words = L.words;
  if (L.kind != TranscriptKind::Evm) {
    words.resize(L.n_com + 2);
    for (size_t i = 0; i < L.n_com; i++) std::memcpy(words[i].data(), proof.data() + 32 * i, 32);
    for (size_t i = 0; i < 2; i++) std::memcpy(words[L.n_com + i].data(), proof.data() + 32 * (L.n_com + L.n_ev) + (i ? 32 : 0), 32);
  }
  L.vk0 = words.size();
  if (L.use_vk) { words.resize(L.vk0 + P.num_pre); for (uint32_t i = 0; i < P.num_pre; i++) std::memcpy(words[L.vk0 + i].data(), vk.vk_bytes.data() + 8 + 32 * i, 32); }
  return true;
}
inline void decode_words(const std::vector<halo2::G1Bytes> &words, std::vector<halo2::G1Affine> &decoded, bool on_host) {
  using halo2::G1Affine;
  decoded.assign(words.size(), G1Affine{});
  if (!words.empty()) {
    if (on_host) { for (size_t i = 0; i < words.size(); i++) if (!halo2::g1_from_bytes(words[i], decoded[i])) decoded[i].fill(0); }
    else {
      uint64_t bad = ~0ull; device_calls()++; const int rc = mi355_g1_decompress_host(words.data(), decoded.data(), words.size(), &bad);
      if (rc == MI355_EBADARG && bad != ~0ull) {   // a rejected word: name it below, where the transcript reaches it; the words behind it are decoded on the host
        for (size_t i = 0; i < words.size(); i++) if (!halo2::g1_from_bytes(words[i], decoded[i])) decoded[i].fill(0);
      } else halo2::check(rc);
    }
  }
}
// decoded: the L.words.size() points of THIS proof (its slice of a batch's decompression)
// tape (Poseidon only): null = the transcript hashes on the host.  Otherwise pass = HostPass::Record runs the transcript section alone -- every absorbed word and every squeeze
// position goes onto the tape, nothing is hashed, the section's named failures are reported as always -- and stops; pass = HostPass::Replay runs everything with the tape's
// challenges in place of the sponge's.
// defer (verify_proofs / aggregate with device_scalars): not null = stop where the scalar side begins and hand over what it and the rest need; the caller runs the protocol's
// program for the whole group and finishes each proof with host_finish.
enum class HostPass { Whole, Record, Replay };
// what stands between the transcript section and the scalar side: the program's inputs for this proof (the eight challenges, the evaluations in proof order, the instances) and
// the points the MSM list takes
struct ScalarWork { std::vector<Fr> inputs; std::vector<halo2::G1Affine> pieces; std::map<uint32_t, halo2::G1Affine> com; halo2::G1Affine c_h{}, c_w{}; };
inline void points_of(const std::vector<sdetail::MsmSource> &src, const ScalarWork &w, std::vector<halo2::G1Affine> &out) {
  using sdetail::MsmSource;
  halo2::G1Affine gen{}; { zk::fe_t c = zk::Fq::zero(); c.l[0] = 1; const zk::fe_t gx = zk::Fq::from_canonical(c); c.l[0] = 2; const zk::fe_t gy = zk::Fq::from_canonical(c); std::memcpy(gen.data(), &gx, 32); std::memcpy(gen.data() + 4, &gy, 32); }
  for (const MsmSource &s : src) out.push_back(s.kind == MsmSource::Piece ? w.pieces[s.index] : s.kind == MsmSource::Commitment ? w.com.at(s.index) : s.kind == MsmSource::Generator ? gen : s.kind == MsmSource::H ? w.c_h : w.c_w);
}
// the scalar side in Fr itself (sdetail::scalar_side<FrArith>): numerator_at_x and the (scalars, points) list into res
inline bool scalar_side_on_host(const Protocol &P, size_t n_instances, const ScalarWork &w, VerifyResult &res) {
  using A = sdetail::FrArith;
  A ar; sdetail::ScalarInputs<A> in; sdetail::ScalarSide<A> side;
  const Fr *p = w.inputs.data();
  for (auto &c : in.ch) c = *p++;
  in.x = *p++; in.ys = *p++; in.v = *p++; in.u = *p++;
  in.evals.assign(p, p + P.evaluations.size()); p += P.evaluations.size();
  in.instances.assign(p, p + n_instances);
  const bool ok = sdetail::scalar_side(ar, P, in, side);
  if (side.numerator_set) res.numerator_at_x = side.numerator;
  res.msm_scalars.insert(res.msm_scalars.end(), side.scalars.begin(), side.scalars.end());
  points_of(side.sources, w, res.msm_points);
  return ok || failed(res, side.failure.name, side.failure.detail);
}
// the carried accumulator: limbs of 88 bits, three per coordinate, (lhs.x, lhs.y, rhs.x, rhs.y) in the first twelve instances
inline bool accumulator_part(const std::vector<Fr> &instances, const VerifyOptions &opt, const Protocol &P, VerifyResult &res) {
  auto failed = [&](const char *name, const std::string &why) { return vdetail::failed(res, name, why); };
  res.has_accumulator = opt.check_accumulator && (opt.accumulator < 0 ? P.has_accumulator : opt.accumulator != 0);
  if (res.has_accumulator) {
    if (instances.size() < 12) return failed("accumulator_limb", "an accumulator needs twelve instance values");
    uint32_t q[8]; for (int i = 0; i < 8; i++) q[i] = zk::FqP::mod(i);
    zk::fe_t co[4];
    for (int cidx = 0; cidx < 4; cidx++) {
      uint64_t wds[5] = {0, 0, 0, 0, 0};
      for (int l = 0; l < 3; l++) {
        const Fr cv = fr_to_canonical(instances[3 * cidx + l]);
        if (cv[2] || cv[3] || (cv[1] >> 24)) return failed("accumulator_limb", "instance " + std::to_string(3 * cidx + l) + " is an accumulator limb of 2^88 or more");
        const int bit = 88 * l, wi = bit / 64, sh = bit % 64;
        wds[wi] |= cv[0] << sh; if (sh) { wds[wi + 1] |= cv[0] >> (64 - sh); } wds[wi + 1] |= cv[1] << sh; if (sh && wi + 2 < 5) wds[wi + 2] |= cv[1] >> (64 - sh);
      }
      std::memcpy(&co[cidx], wds, 32);
      if (wds[4] || zk::Fq::w_geq(co[cidx].l, q)) return failed("accumulator_point", "accumulator coordinate " + std::to_string(cidx) + " is not below q");
      co[cidx] = zk::Fq::from_canonical(co[cidx]);
    }
    std::memcpy(res.acc_lhs.data(), &co[0], 32); std::memcpy(res.acc_lhs.data() + 4, &co[1], 32); std::memcpy(res.acc_rhs.data(), &co[2], 32); std::memcpy(res.acc_rhs.data() + 4, &co[3], 32);
    if (!vdetail::fq_on_curve(res.acc_lhs) || !vdetail::fq_on_curve(res.acc_rhs)) return failed("accumulator_point", "a point of the carried accumulator is not on the curve");
  }
  return true;
}
inline bool host_part(const Protocol &P, const VerifyingKeyRef &vk, const std::vector<Fr> &instances, const std::vector<uint8_t> &proof, const VerifyOptions &opt, const Layout &L,
                      const halo2::G1Affine *decoded, VerifyResult &res, TranscriptTape *tape = nullptr, HostPass pass = HostPass::Whole, ScalarWork *defer = nullptr) {
  using halo2::G1Affine;
  auto failed = [&](const char *name, const std::string &why) { return vdetail::failed(res, name, why); };
  const TranscriptKind kind = L.kind; const bool use_vk = L.use_vk; const size_t nb = L.nb, n_ev = L.n_ev, vk0 = L.vk0;
  Transcript T(kind);
  if (pass != HostPass::Whole) T.use_tape(pass == HostPass::Record ? Transcript::Mode::Record : Transcript::Mode::Replay, tape);
  std::vector<G1Affine> pre;
  if (use_vk) { for (uint32_t i = 0; i < P.num_pre; i++) { pre.push_back(decoded[vk0 + i]); bool z = true; for (auto w : pre.back()) z = z && w == 0; if (z) return failed("invalid_point", ".vkey commitment " + std::to_string(i) + " is no curve point"); } }
  else pre = vk.preprocessed.empty() ? P.preprocessed : vk.preprocessed;
  if (pre.size() != P.num_pre) return failed("preprocessed", std::to_string(pre.size()) + " preprocessed commitments given, the protocol has " + std::to_string(P.num_pre));
  for (size_t i = 0; i < pre.size(); i++) if (!vdetail::fq_on_curve(pre[i])) return failed("invalid_point", "preprocessed commitment " + std::to_string(i) + " is not on the curve");

  // ---- transcript: key scalar, instances, commitments by phase with their challenges, quotient pieces, x, evaluations, y, v, H, u, W'
  if (vk.has_initial_state) T.common_scalar(vk.initial_state);
  else if (P.has_initial_state) T.common_scalar(P.initial_state);
  else if (use_vk) T.common_scalar(vk_transcript_repr(vk.vk_bytes));
  else return failed("initial_state", "no transcript initial state: give the .vkey, a protocol file that carries one, or an explicit value");
  for (const Fr &v : instances) T.common_scalar(v);
  size_t pos = 0, word = 0;
  std::map<uint32_t, G1Affine> com; for (uint32_t i = 0; i < P.num_pre; i++) com[i] = pre[i];
  auto read_point = [&](G1Affine &out, std::string &err) {
    const Transcript::Read st = T.read_point(proof, pos, kind == TranscriptKind::Evm ? nullptr : &decoded[word], out);
    if (st != Transcript::Read::Ok) err = "point " + std::to_string(word) + " of the proof (byte " + std::to_string(pos - nb) + ") is no curve point";
    word++;
    return st == Transcript::Read::Ok;
  };
  std::string err; Fr ch[4]; uint32_t idx = P.wit0, nch = 0;
  for (size_t ph = 0; ph < P.num_witness.size(); ph++) {
    for (uint32_t j = 0; j < P.num_witness[ph]; j++) if (!read_point(com[idx++], err)) return failed("invalid_point", err);
    for (uint32_t j = 0; j < P.num_challenge[ph]; j++) ch[nch++] = T.squeeze_challenge();
  }
  std::vector<G1Affine> pieces(P.Q);
  for (auto &pc : pieces) if (!read_point(pc, err)) return failed("invalid_point", err);
  const Fr x = T.squeeze_challenge();
  std::vector<Fr> evals(n_ev);   // in the order of P.evaluations
  for (size_t i = 0; i < n_ev; i++) {
    Fr v; const Transcript::Read st = T.read_scalar(proof, pos, v);
    if (st == Transcript::Read::NonCanonical) return failed("non_canonical_scalar", "evaluation " + std::to_string(i) + " of the proof is not below r");
    if (st != Transcript::Read::Ok) return failed("proof_length", "the proof ends inside evaluation " + std::to_string(i));
    evals[i] = v;
  }
  const Fr ys = T.squeeze_challenge(), v = T.squeeze_challenge();
  G1Affine c_h, c_w;
  if (!read_point(c_h, err)) return failed("invalid_point", err);
  const Fr uu = T.squeeze_challenge();
  if (!read_point(c_w, err)) return failed("invalid_point", err);
  if (pos != proof.size()) return failed("proof_length", "proof has " + std::to_string(proof.size()) + " bytes, the protocol reads " + std::to_string(pos));
  res.theta = ch[0]; res.beta = ch[1]; res.gamma = ch[2]; res.y = ch[3]; res.x = x; res.shplonk_y = ys; res.shplonk_v = v; res.shplonk_u = uu; res.w_prime = c_w;
  if (pass == HostPass::Record) return true;   // the script is on the tape; the challenges above are placeholders until the replay

  // ---- scalar side: its inputs in the order a program takes them, then either handed over (device_scalars: the caller runs the program and calls host_finish) or run here
  ScalarWork work;
  work.inputs = {ch[0], ch[1], ch[2], ch[3], x, ys, v, uu};
  work.inputs.insert(work.inputs.end(), evals.begin(), evals.end()); work.inputs.insert(work.inputs.end(), instances.begin(), instances.end());
  work.pieces = std::move(pieces); work.com = std::move(com); work.c_h = c_h; work.c_w = c_w;
  if (defer) { *defer = std::move(work); return true; }
  if (!scalar_side_on_host(P, instances.size(), work, res)) return false;
  return accumulator_part(instances, opt, P, res);
}
// the rest of a proof whose scalar side ran on the device: out = the program's outputs for this proof (numerator_at_x, then the MSM scalars), flags = its flag word.  The
// flag of x_in_domain maps back to that failure; any other flag sends the proof through the host's scalar side, which names what there is to name.
inline bool host_finish(const Protocol &P, const std::vector<Fr> &instances, const VerifyOptions &opt, const sdetail::ScalarProgram &prog, const ScalarWork &work, const Fr *out,
                        uint32_t flags, VerifyResult &res) {
  if (flags & (1u << sdetail::FLAG_BIT_X_IN_DOMAIN)) return failed(res, "x_in_domain", sdetail::x_in_domain_text());
  // any other flag: a zero went through the shared inverse, so every inverse of this job is zero and its outputs mean nothing -- shplonk_degenerate keeps its numerator_at_x,
  // and x = 0 is no failure at all, only on the host
  if (flags) { if (!scalar_side_on_host(P, instances.size(), work, res)) return false; return accumulator_part(instances, opt, P, res); }
  res.numerator_at_x = out[0];
  res.msm_scalars.assign(out + 1, out + 1 + prog.sources.size());
  points_of(prog.sources, work, res.msm_points);
  return accumulator_part(instances, opt, P, res);
}
inline void host_only_done(VerifyResult &res) { res.ok = true; res.error = ""; res.detail = "host-only: stopped before the multi-scalar multiplication and the pairing"; }
// the verdict over a proof's one or two pairing groups (res.pairing filled)
inline void judge(VerifyResult &res) {
  if (!res.pairing[0]) { failed(res, "pairing", "e(lhs, g2) e(W', -s_g2) != 1"); return; }
  if (res.pairing.size() == 2 && !res.pairing[1]) { failed(res, "accumulator_pairing", "the carried accumulator does not satisfy e(lhs, g2) e(rhs, -s_g2) == 1"); return; }
  res.ok = true;
}
// `groups` pairing groups of (P[2 g], g2) (P[2 g + 1], -s_g2): one mi355_pairing_products_host call
inline std::vector<uint32_t> pairing_groups(const std::vector<halo2::G1Affine> &Pp, const G2Pair &srs) {
  PhaseClock pc(phase_times().pairing);
  const uint32_t groups = (uint32_t)(Pp.size() / 2);
  std::vector<uint8_t> Qq(256 * (size_t)groups);
  for (uint32_t g = 0; g < groups; g++) { std::memcpy(Qq.data() + 256 * (size_t)g, srs.g2.data(), 128); std::memcpy(Qq.data() + 256 * (size_t)g + 128, srs.neg_s_g2.data(), 128); }
  std::vector<uint32_t> flags(groups, 0);
  device_calls()++; halo2::check(mi355_pairing_products_host(Pp.data(), Qq.data(), groups, 2, nullptr, flags.data()));
  return flags;
}
}  // namespace vdetail

// one proof: VerifyOptions::device_transcript and device_scalars are ignored here (one sponge, one scalar side: serial chains the host runs faster than one lane does)
inline VerifyResult verify_proof(const Protocol &P, const VerifyingKeyRef &vk, const std::vector<Fr> &instances, const std::vector<uint8_t> &proof, const G2Pair &srs, const VerifyOptions &opt) {
  using halo2::G1Affine;
  VerifyResult res; vdetail::Layout L;
  if (!vdetail::layout_of(P, vk, proof, opt, L, res)) return res;
  std::vector<G1Affine> decoded; vdetail::decode_words(L.words, decoded, opt.host_only);
  if (!vdetail::host_part(P, vk, instances, proof, opt, L, decoded.data(), res)) return res;
  if (opt.host_only) { vdetail::host_only_done(res); return res; }

  // ---- one MSM, one pairing call
  halo2::G1 sum{};
  vdetail::device_calls()++; halo2::check(mi355_msm_g1_adhoc_host(res.msm_points.data(), res.msm_scalars.data(), res.msm_scalars.size(), sum.data()));
  std::memcpy(res.msm_result.data(), sum.data(), 64);
  std::vector<G1Affine> Pp = {res.msm_result, res.w_prime}; if (res.has_accumulator) { Pp.push_back(res.acc_lhs); Pp.push_back(res.acc_rhs); }
  res.pairing = vdetail::pairing_groups(Pp, srs);
  vdetail::judge(res);
  return res;
}

// ------------------------------------------------------------------------------------------------ many proofs in one pass
// plonk::verify_proofs: N proofs, ONE decompression, ONE segmented MSM (mi355_msm_g1_segmented_host), ONE pairing call -- a pairing call costs one lane's latency whether it
// judges one group or hundreds (profiles/pairing.md).  Protocols, keys and transcripts may differ inside a batch.  A proof that fails its host part keeps its named failure and
// leaves the batch; when nothing survives no device call is made.  Every VerifyResult equals verify_proof's for that proof alone.  A proof with VerifyOptions::host_only decodes
// its points on the host and stops after its list, as in verify_proof.
struct ProofInput { const Protocol *protocol = nullptr; const VerifyingKeyRef *vk = nullptr; std::vector<Fr> instances; std::vector<uint8_t> proof; VerifyOptions opt; };

namespace vdetail {
// passed[i]: proof i reached the end of its host part (its list and, when it carries one, its accumulator are in res[i])
inline void host_parts(const std::vector<ProofInput> &in, std::vector<VerifyResult> &res, std::vector<char> &passed) {
  using halo2::G1Affine;
  const size_t N = in.size();
  res.assign(N, VerifyResult{}); passed.assign(N, 0);
  std::vector<Layout> L(N); std::vector<size_t> at(N, 0); std::vector<halo2::G1Bytes> words;
  std::vector<G1Affine> decoded;
  {
    PhaseClock pc(phase_times().decode);
    for (size_t i = 0; i < N; i++) {
      if (!in[i].protocol || !in[i].vk) throw std::invalid_argument("verify_proofs: proof " + std::to_string(i) + " has no protocol or no key");
      passed[i] = layout_of(*in[i].protocol, *in[i].vk, in[i].proof, in[i].opt, L[i], res[i]) ? 1 : 0;
      if (passed[i] && !in[i].opt.host_only) { at[i] = words.size(); words.insert(words.end(), L[i].words.begin(), L[i].words.end()); }
    }
    decode_words(words, decoded, false);
  }
  // device_transcript: record the script of every Poseidon proof that asks for it (a proof that fails here keeps its named failure and leaves the batch), hash all of them
  // in ONE call, hand each tape its challenges.  No Poseidon proof left: no call.
  std::vector<TranscriptTape> tapes(N); std::vector<size_t> dev;
  {
    PhaseClock pc(phase_times().record);
    for (size_t i = 0; i < N; i++) {
      if (!passed[i] || !in[i].opt.device_transcript || in[i].opt.host_only || L[i].kind != TranscriptKind::Poseidon) continue;
      passed[i] = host_part(*in[i].protocol, *in[i].vk, in[i].instances, in[i].proof, in[i].opt, L[i], decoded.data() + at[i], res[i], &tapes[i], HostPass::Record) ? 1 : 0;
      if (passed[i]) dev.push_back(i);
    }
  }
  if (!dev.empty()) {
    PhaseClock pc(phase_times().transcript_call);
    std::vector<Fr> w; std::vector<uint32_t> sq; std::vector<uint64_t> woff = {0}, soff = {0};
    for (size_t i : dev) { w.insert(w.end(), tapes[i].words.begin(), tapes[i].words.end()); sq.insert(sq.end(), tapes[i].squeeze_at.begin(), tapes[i].squeeze_at.end()); woff.push_back(w.size()); soff.push_back(sq.size()); }
    device_calls()++; const std::vector<Fr> ch = halo2::poseidon_transcripts(w, woff, sq, soff);
    for (size_t j = 0; j < dev.size(); j++) tapes[dev[j]].challenges.assign(ch.begin() + soff[j], ch.begin() + soff[j + 1]);
  }
  // device_scalars: the proofs that ask for it stop where the scalar side begins and wait in the group of their (protocol, number of instances), whose program is compiled when
  // the first of them arrives; a protocol that fails structurally has no program and its proofs run on the host, where that failure is named.  ONE call per group, then the
  // rest of each proof's host part.  No proof left in a group: no call.
  struct Group { sdetail::ScalarProgram prog; std::vector<size_t> members; };
  std::map<std::pair<const Protocol *, size_t>, Group> groups; std::vector<ScalarWork> work(N);
  {
    PhaseClock pc(phase_times().host_part);
    for (size_t i = 0; i < N; i++) {
      if (!passed[i]) continue;
      std::vector<G1Affine> own; if (in[i].opt.host_only) decode_words(L[i].words, own, true);
      const bool replay = std::find(dev.begin(), dev.end(), i) != dev.end();
      Group *grp = nullptr;
      if (in[i].opt.device_scalars && !in[i].opt.host_only) {
        const auto key = std::make_pair(in[i].protocol, in[i].instances.size());
        auto it = groups.find(key);
        if (it == groups.end()) { it = groups.emplace(key, Group{}).first; it->second.prog = sdetail::compile_scalar_program(*in[i].protocol, in[i].instances.size()); }
        if (it->second.prog.usable) grp = &it->second;
      }
      passed[i] = host_part(*in[i].protocol, *in[i].vk, in[i].instances, in[i].proof, in[i].opt, L[i], in[i].opt.host_only ? own.data() : decoded.data() + at[i], res[i],
                            replay ? &tapes[i] : nullptr, replay ? HostPass::Replay : HostPass::Whole, grp ? &work[i] : nullptr) ? 1 : 0;
      if (passed[i] && grp) grp->members.push_back(i);
    }
  }
  for (auto &kv : groups) {
    const Group &grp = kv.second; const sdetail::ScalarProgram &prog = grp.prog;
    if (grp.members.empty()) continue;
    std::vector<Fr> outputs; std::vector<uint32_t> flags;
    {
      PhaseClock pc(phase_times().scalar_call);
      std::vector<Fr> inputs; inputs.reserve(grp.members.size() * (size_t)prog.n_inputs);
      for (size_t i : grp.members) inputs.insert(inputs.end(), work[i].inputs.begin(), work[i].inputs.end());
      device_calls()++; outputs = halo2::fr_program(prog.code, prog.n_regs, prog.consts, inputs, prog.n_inputs, (uint32_t)grp.members.size(), prog.out_regs, flags);
    }
    PhaseClock pc(phase_times().host_part);
    for (size_t j = 0; j < grp.members.size(); j++) {
      const size_t i = grp.members[j];
      passed[i] = host_finish(*in[i].protocol, in[i].instances, in[i].opt, prog, work[i], outputs.data() + j * prog.out_regs.size(), flags[j], res[i]) ? 1 : 0;
    }
  }
}
// the lists of the proofs `idx` names, concatenated: one segmented MSM, the sums into msm_result
inline void msm_of_lists(std::vector<VerifyResult> &res, const std::vector<size_t> &idx) {
  PhaseClock pc(phase_times().msm);
  std::vector<Fr> sc; std::vector<halo2::G1Affine> pt; std::vector<uint64_t> off = {0};
  for (size_t i : idx) { sc.insert(sc.end(), res[i].msm_scalars.begin(), res[i].msm_scalars.end()); pt.insert(pt.end(), res[i].msm_points.begin(), res[i].msm_points.end()); off.push_back(sc.size()); }
  device_calls()++; const std::vector<halo2::G1Affine> sums = halo2::msm_g1_segmented(sc, pt, off);
  for (size_t j = 0; j < idx.size(); j++) res[idx[j]].msm_result = sums[j];
}
}  // namespace vdetail

inline std::vector<VerifyResult> verify_proofs(const std::vector<ProofInput> &in, const G2Pair &srs) {
  std::vector<VerifyResult> res; std::vector<char> passed;
  vdetail::host_parts(in, res, passed);
  std::vector<size_t> idx;
  for (size_t i = 0; i < in.size(); i++) if (passed[i]) { if (in[i].opt.host_only) vdetail::host_only_done(res[i]); else idx.push_back(i); }
  if (idx.empty()) return res;
  vdetail::msm_of_lists(res, idx);
  std::vector<halo2::G1Affine> Pp;   // one group per surviving proof plus one per carried accumulator
  for (size_t i : idx) { Pp.push_back(res[i].msm_result); Pp.push_back(res[i].w_prime); if (res[i].has_accumulator) { Pp.push_back(res[i].acc_lhs); Pp.push_back(res[i].acc_rhs); } }
  const std::vector<uint32_t> flags = vdetail::pairing_groups(Pp, srs);
  size_t g = 0;
  for (size_t i : idx) { const size_t n = res[i].has_accumulator ? 2 : 1; res[i].pairing.assign(flags.begin() + g, flags.begin() + g + n); g += n; vdetail::judge(res[i]); }
  return res;
}

// ------------------------------------------------------------------------------------------------ the accumulator the next layer's instances carry
// plonk::aggregate restates PlonkSuccinctVerifier::verify + KzgAs::create_proof [EXT-recalled snark-verifier verifier/plonk.rs, pcs/kzg/accumulation.rs]: what the aggregator does
// natively with the snarks of layer n before it proves layer n + 1.
//   1  host parts and ONE segmented MSM as in verify_proofs; proof i yields (msm_result_i, W'_i), and a proof that carries an accumulator yields (acc_lhs, acc_rhs) AFTER it
//   2  a fresh Poseidon transcript (no initial scalar; Poseidon also when a proof was read with the EVM transcript) absorbs lhs, rhs of every accumulator in list order; r = its challenge
//      (ONE sponge: it stays on the host whatever VerifyOptions::device_transcript says -- that option moves the N transcripts of step 1)
//   3  lhs = sum r^j lhs_j, rhs = sum r^j rhs_j (r^0 = 1): a second segmented MSM with two segments
//   4  limbs: three 88-bit limbs per canonical coordinate, lhs.x, lhs.y, rhs.x, rhs.y -- the first twelve instances of the next layer, what host_part's decoder reads back
//   5  with an SRS: one pairing group e(lhs, g2) e(rhs, -s_g2); failure "aggregate_pairing".  The proofs are judged TOGETHER here: proofs[i].pairing stays empty.
// A proof that fails its host part fails the aggregation with that proof's error and its index in `detail` (the reference panics there); no device call is made then.
// The order of the accumulators and the transcript of step 2 are recalled, not pinned by a fixture; the algebra is what the tests verify.
struct AggregateResult {
  bool ok = false; std::string error, detail; std::vector<VerifyResult> proofs; std::vector<std::pair<halo2::G1Affine, halo2::G1Affine>> accumulators;
  Fr r{}; halo2::G1Affine lhs{}, rhs{}; std::array<Fr, 12> limbs{}; uint32_t pairing = 0;
};
namespace vdetail {
inline bool g1_is_identity(const halo2::G1Affine &a) { bool z = true; for (auto w : a) z = z && w == 0; return z; }
// step 1's list from results whose msm_result is filled
inline std::vector<std::pair<halo2::G1Affine, halo2::G1Affine>> accumulators_of(const std::vector<VerifyResult> &proofs) {
  std::vector<std::pair<halo2::G1Affine, halo2::G1Affine>> out;
  for (const auto &p : proofs) { out.push_back({p.msm_result, p.w_prime}); if (p.has_accumulator) out.push_back({p.acc_lhs, p.acc_rhs}); }
  return out;
}
// step 2; false with the named failure accumulator_identity in `out` (the transcript refuses the identity)
inline bool aggregate_challenge(AggregateResult &out) {
  Transcript T(TranscriptKind::Poseidon);
  for (size_t j = 0; j < out.accumulators.size(); j++) {
    const auto &a = out.accumulators[j];
    if (g1_is_identity(a.first) || g1_is_identity(a.second)) { out.ok = false; out.error = "accumulator_identity"; out.detail = "accumulator " + std::to_string(j) + " holds the identity, which the transcript refuses"; return false; }
    T.common_point(a.first); T.common_point(a.second);
  }
  out.r = T.squeeze_challenge();
  return true;
}
// step 4: the inverse of host_part's limb decoder
inline void accumulator_limbs(const halo2::G1Affine &lhs, const halo2::G1Affine &rhs, std::array<Fr, 12> &limbs) {
  const halo2::G1Affine *pts[2] = {&lhs, &rhs};
  for (int cidx = 0; cidx < 4; cidx++) {
    zk::fe_t m; std::memcpy(&m, pts[cidx / 2]->data() + 4 * (cidx & 1), 32);
    const zk::fe_t c = zk::Fq::to_canonical(m); uint64_t w[4]; std::memcpy(w, &c, 32);
    const uint64_t lo[3] = {w[0], (w[1] >> 24) | (w[2] << 40), (w[2] >> 48) | (w[3] << 16)}, hi[3] = {w[1] & 0xffffffull, (w[2] >> 24) & 0xffffffull, w[3] >> 48};
    for (int l = 0; l < 3; l++) { zk::fe_t v = zk::Fr::zero(); const uint64_t two[2] = {lo[l], hi[l]}; std::memcpy(&v, two, 16); limbs[3 * cidx + l] = h2d::from_fe(zk::Fr::from_canonical(v)); }
  }
}
}  // namespace vdetail

inline AggregateResult aggregate(const std::vector<ProofInput> &in, const G2Pair *srs /* nullptr: fold only, no pairing */) {
  using halo2::G1Affine;
  AggregateResult out;
  if (in.empty()) { out.error = "no_proofs"; out.detail = "nothing to aggregate"; return out; }
  std::vector<char> passed;
  vdetail::host_parts(in, out.proofs, passed);
  for (size_t i = 0; i < in.size(); i++) if (!passed[i]) { out.error = out.proofs[i].error; out.detail = "proof " + std::to_string(i) + ": " + out.proofs[i].detail; return out; }
  std::vector<size_t> idx(in.size()); for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
  vdetail::msm_of_lists(out.proofs, idx);
  for (auto &p : out.proofs) { p.ok = true; p.error = ""; p.detail = "aggregated: judged by the aggregate's pairing"; }
  out.accumulators = vdetail::accumulators_of(out.proofs);
  if (!vdetail::aggregate_challenge(out)) return out;
  const size_t m = out.accumulators.size();
  std::vector<Fr> sc(2 * m); std::vector<G1Affine> pt(2 * m);
  Fr pw = fr_one();
  for (size_t j = 0; j < m; j++) { sc[j] = sc[m + j] = pw; pt[j] = out.accumulators[j].first; pt[m + j] = out.accumulators[j].second; pw = fr_mul(pw, out.r); }
  vdetail::device_calls()++; const std::vector<G1Affine> folded = halo2::msm_g1_segmented(sc, pt, {0, m, 2 * m});
  out.lhs = folded[0]; out.rhs = folded[1];
  vdetail::accumulator_limbs(out.lhs, out.rhs, out.limbs);
  if (!srs) { out.ok = true; return out; }
  out.pairing = vdetail::pairing_groups({out.lhs, out.rhs}, *srs)[0];
  if (!out.pairing) { out.error = "aggregate_pairing"; out.detail = "the folded accumulator does not satisfy e(lhs, g2) e(rhs, -s_g2) == 1"; return out; }
  out.ok = true;
  return out;
}
}  // namespace plonk
}  // namespace mi355zk
