// poseidon.hpp -- many Poseidon transcripts in one launch: the sponge of snark-verifier's PoseidonTranscript<NativeLoader> (T = 5, RATE = 4, R_F = 8, R_P = 60, S-box x^5,
// constants from the Grain LFSR, initial state (2^64, 0, 0, 0, 0)), the one include/mi355zk_transcript.hpp runs on the host and oracle/poseidon.py restates.
//
// A JOB is one fresh sponge with a known script: a list of words W (Fr, Montgomery, fully reduced) and a non-decreasing list of squeeze positions S, each <= len(W).
// Its outputs are those of
//     sp = Sponge(); prev = 0
//     for p in S: sp.update(W[prev:p]); prev = p; out.append(sp.squeeze())
// i.e. for the m words between two squeezes: floor(m / 4) times four words are added into state[1..4] and the state is permuted; then the m mod 4 remaining words are added
// into state[1..], 1 is added to state[1 + m mod 4] and the state is permuted once more (an exact multiple of RATE, zero included, takes this padded permutation with an
// empty chunk); the challenge is state[1].  Words behind the last squeeze influence no output and are not read.
//
//   poseidon_permute    R_F / 2 full rounds, the R_P partial rounds in the SPARSE schedule of the Poseidon paper's appendix B (per round: the S-box on word 0, ONE dot product
//                       and T - 1 multiply-adds instead of T dot products; what is left of the factored matrix is applied once, densely), R_F / 2 full rounds.
//                       1 065 field multiplications; the plain schedule (poseidon_permute_plain, 1 880) is kept for the check of the tables.
//   poseidon_job        one job, written as ONE loop whose every trip absorbs one chunk (full or padded) and permutes once: the lanes of a wave stay in lockstep through the
//                       permutation whatever their scripts are, and a lane whose script is finished drops out at the loop condition.
//   k_poseidon_transcripts   one lane per job, grid = ceil(jobs / 64).  Nothing crosses lanes: no barrier, no LDS, no atomics.  The state is five field elements in registers,
//                       indexed by fully unrolled constants only (a loop-indexed private array lands in scratch).  The round loops are NOT unrolled:
//                       their counters index the constant table, which every lane reads at the same address.  Challenges leave by plain 32-byte vector stores.
//   poseidon_tables     the constants, generated once per process on the host: Grain LFSR -> 340 round constants and the Cauchy matrix -> the sparse tables; checked against
//                       the plain schedule on a fixed state before anyone sees them.  One flat block of POS_TABLE_WORDS field elements, uploaded once per device slot.
// Field arithmetic: FrPs (fp_asm.hpp) multiplications and squarings, Fr additions; every value stays fully reduced.
#pragma once
#include "fp_asm.hpp"
#include <stdexcept>
#include <vector>

namespace zk {

constexpr int POS_T = 5, POS_RATE = 4, POS_RF = 8, POS_RP = 60;
// the flat table, in field elements
constexpr int POS_RC = 0;                                   // (R_F + R_P) x T round constants, row-major by round
constexpr int POS_MDS = POS_RC + (POS_RF + POS_RP) * POS_T;  // T x T
constexpr int POS_PRC = POS_MDS + POS_T * POS_T;             // R_P x T: the partial rounds' constants with the factored matrices pushed through
constexpr int POS_ROW0 = POS_PRC + POS_RP * POS_T;           // R_P x T: row 0 of each round's sparse matrix
constexpr int POS_WHAT = POS_ROW0 + POS_RP * POS_T;          // R_P x (T - 1): its first column below the diagonal
constexpr int POS_LEFT = POS_WHAT + POS_RP * (POS_T - 1);    // T x T: what is left after the last partial round
constexpr int POS_INIT = POS_LEFT + POS_T * POS_T;           // 2^64, word 0 of a fresh sponge
constexpr int POS_TABLE_WORDS = POS_INIT + 1;

template <class F> ZK_HD fe_t pos_pow5(const fe_t &a) { const fe_t a2 = F::sqr(a); return F::mul(F::sqr(a2), a); }
// one row of a matrix product, written out: the unroller gives up on a nest this large, and a row loop it leaves standing indexes the state by its counter
template <class F> ZK_HD fe_t pos_dot(const fe_t *row, const fe_t (&s)[POS_T]) {
  static_assert(POS_T == 5, "pos_dot is written out for T = 5");
  return F::add(F::add(F::add(F::add(F::mul(row[0], s[0]), F::mul(row[1], s[1])), F::mul(row[2], s[2])), F::mul(row[3], s[3])), F::mul(row[4], s[4]));
}
// s <- M s, M row-major
template <class F> ZK_HD void pos_dense(fe_t (&s)[POS_T], const fe_t *M) {
  const fe_t n0 = pos_dot<F>(M, s), n1 = pos_dot<F>(M + POS_T, s), n2 = pos_dot<F>(M + 2 * POS_T, s), n3 = pos_dot<F>(M + 3 * POS_T, s), n4 = pos_dot<F>(M + 4 * POS_T, s);
  s[0] = n0; s[1] = n1; s[2] = n2; s[3] = n3; s[4] = n4;
}
// plain rounds [r0, r1): constants, S-box (all words in a full round, word 0 in a partial one), the matrix
template <class F> ZK_HD void pos_plain_rounds(fe_t (&s)[POS_T], const fe_t *tab, int r0, int r1) {
#pragma nounroll
  for (int r = r0; r < r1; r++) {
    const fe_t *rc = tab + POS_RC + POS_T * r;
    const bool full = r < POS_RF / 2 || r >= POS_RF / 2 + POS_RP;
#pragma unroll
    for (int i = 0; i < POS_T; i++) s[i] = F::add(s[i], rc[i]);
    s[0] = pos_pow5<F>(s[0]);
    if (full) {
#pragma unroll
      for (int i = 1; i < POS_T; i++) s[i] = pos_pow5<F>(s[i]);
    }
    pos_dense<F>(s, tab + POS_MDS);
  }
}
template <class F> ZK_HD void pos_sparse_rounds(fe_t (&s)[POS_T], const fe_t *tab) {
#pragma nounroll
  for (int k = 0; k < POS_RP; k++) {
    const fe_t *prc = tab + POS_PRC + POS_T * k, *row0 = tab + POS_ROW0 + POS_T * k, *what = tab + POS_WHAT + (POS_T - 1) * k;
#pragma unroll
    for (int i = 0; i < POS_T; i++) s[i] = F::add(s[i], prc[i]);
    s[0] = pos_pow5<F>(s[0]);
    const fe_t d = pos_dot<F>(row0, s);
#pragma unroll
    for (int i = 1; i < POS_T; i++) s[i] = F::add(s[i], F::mul(what[i - 1], s[0]));
    s[0] = d;
  }
  pos_dense<F>(s, tab + POS_LEFT);
}
template <class F> ZK_HD void poseidon_permute(fe_t (&s)[POS_T], const fe_t *tab) {
#pragma nounroll
  for (int half = 0; half < 2; half++) {   // one copy of the full rounds' code for both ends
    const int r0 = half ? POS_RF / 2 + POS_RP : 0;
    pos_plain_rounds<F>(s, tab, r0, r0 + POS_RF / 2);
    if (half == 0) pos_sparse_rounds<F>(s, tab);
  }
}
template <class F> ZK_HD void poseidon_permute_plain(fe_t (&s)[POS_T], const fe_t *tab) { pos_plain_rounds<F>(s, tab, 0, POS_RF + POS_RP); }

ZK_HD void pos_store(fe_t *p, const fe_t &v) {
#if defined(__HIP_DEVICE_COMPILE__)
  g_store(p, v);
#else
  *p = v;
#endif
}

// W: the job's words; S: its nsq squeeze positions (non-decreasing, each <= the job's length: checked by the caller); out: nsq challenges
template <class F> ZK_HD void poseidon_job(const fe_t *tab, const fe_t *W, const uint32_t *S, uint32_t nsq, fe_t *out) {
  if (nsq == 0) return;
  fe_t s[POS_T];
  s[0] = tab[POS_INIT];
#pragma unroll
  for (int i = 1; i < POS_T; i++) s[i] = F::zero();
  const fe_t one = F::one();
  uint32_t q = 0, prev = 0, p = S[0];
  while (q < nsq) {
    const uint32_t avail = p - prev, take = avail < (uint32_t)POS_RATE ? avail : (uint32_t)POS_RATE;
#pragma unroll
    for (int i = 0; i < POS_RATE; i++) {   // the chunk, then the 1 behind a short one; reads stay below p
      fe_t a = F::zero();
      if ((uint32_t)i < take) a = W[prev + i];
      else if ((uint32_t)i == take) a = one;
      s[1 + i] = F::add(s[1 + i], a);
    }
    poseidon_permute<F>(s, tab);
    prev += take;
    if (avail < (uint32_t)POS_RATE) {      // that was the padded permutation: a challenge
      pos_store(&out[q], s[1]);
      q++;
      if (q < nsq) p = S[q];
    }
  }
}

// ---- the constants (host).  Grain LFSR: 80-bit state = field type 1 (2 bits) | s-box 0 (4) | field bits 254 (12) | t (12) | R_F (10) | R_P (10) | thirty 1s; 160 warm-up
// clocks; self-shrinking output; round constants by rejection sampling of 254-bit draws (most significant bit first), the Cauchy matrix 1 / (x_i + y_j) from 2 t draws
// reduced mod r.  Everything is stored in Montgomery form.
inline void poseidon_grain(std::vector<fe_t> &rc, fe_t (&mds)[POS_T][POS_T]) {
  std::vector<uint8_t> st;
  auto push_bits = [&](uint32_t v, int nb) { for (int i = nb - 1; i >= 0; i--) st.push_back((v >> i) & 1); };
  push_bits(1, 2); push_bits(0, 4); push_bits(254, 12); push_bits(POS_T, 12); push_bits(POS_RF, 10); push_bits(POS_RP, 10); for (int i = 0; i < 30; i++) st.push_back(1);
  size_t head = 0;   // st[head .. head + 80) is the register; clocking appends and advances
  auto clock = [&]() { const uint8_t nb = st[head + 62] ^ st[head + 51] ^ st[head + 38] ^ st[head + 23] ^ st[head + 13] ^ st[head]; st.push_back(nb); head++; return nb; };
  for (int i = 0; i < 160; i++) clock();
  auto next_bit = [&]() { uint8_t nb = clock(); while (nb == 0) { clock(); nb = clock(); } return clock(); };
  uint32_t modw[8]; for (int i = 0; i < 8; i++) modw[i] = FrP::mod(i);
  auto draw = [&](bool reject, bool &ok) {
    fe_t a = Fr::zero();
    for (int b = 253; b >= 0; b--) if (next_bit()) a.l[b / 32] |= 1u << (b % 32);
    ok = !Fr::w_geq(a.l, modw);
    if (!ok && !reject) { while (Fr::w_geq(a.l, modw)) Fr::w_sub(a.l, modw); ok = true; }
    return Fr::from_canonical(a);
  };
  rc.clear();
  while (rc.size() < (size_t)(POS_RF + POS_RP) * POS_T) { bool ok; const fe_t v = draw(true, ok); if (ok) rc.push_back(v); }
  fe_t xs[POS_T], ys[POS_T]; bool ok;
  for (auto &x : xs) x = draw(false, ok);
  for (auto &y : ys) y = draw(false, ok);
  for (int i = 0; i < POS_T; i++) for (int j = 0; j < POS_T; j++) mds[i][j] = Fr::inv(Fr::add(xs[i], ys[j]));
}
// The sparse schedule: a dense matrix D splits as D = D' D'' with D' = [[1, 0], [0, D^]] and D'' = [[D00, D[0, 1:]], [w^, I]], w^ = D^^-1 D[1:, 0]; D' leaves word 0 alone,
// so it commutes with the partial round's S-box and is pushed through the next round's constants into the next round's matrix (M D', split again).  What is left of D'
// after the last partial round is applied once, densely.
inline std::vector<fe_t> poseidon_build_tables() {
  constexpr int T = POS_T, N = POS_T - 1, RP = POS_RP, R0 = POS_RF / 2;
  std::vector<fe_t> tab(POS_TABLE_WORDS, Fr::zero());
  std::vector<fe_t> rc; fe_t mds[T][T];
  poseidon_grain(rc, mds);
  for (size_t i = 0; i < rc.size(); i++) tab[POS_RC + i] = rc[i];
  for (int i = 0; i < T; i++) for (int j = 0; j < T; j++) tab[POS_MDS + T * i + j] = mds[i][j];
  { fe_t c = Fr::zero(); c.l[2] = 1; tab[POS_INIT] = Fr::from_canonical(c); }
  const fe_t zero = Fr::zero(), one = Fr::one();
  fe_t D[T][T]; for (int i = 0; i < T; i++) for (int j = 0; j < T; j++) D[i][j] = mds[i][j];
  fe_t hinv[N][N];                                             // D^^-1 of the PREVIOUS round's split: applied to this round's constants
  for (int k = 0; k < RP; k++) {
    for (int i = 0; i < T; i++) tab[POS_PRC + T * k + i] = rc[(size_t)(R0 + k) * T + i];
    if (k > 0) for (int i = 0; i < N; i++) { fe_t acc = zero; for (int j = 0; j < N; j++) acc = Fr::add(acc, Fr::mul(hinv[i][j], rc[(size_t)(R0 + k) * T + 1 + j])); tab[POS_PRC + T * k + 1 + i] = acc; }
    fe_t A[N][2 * N];                                          // invert D^ = D[1:, 1:] (Gauss-Jordan over the field)
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) { A[i][j] = D[1 + i][1 + j]; A[i][N + j] = i == j ? one : zero; }
    for (int c = 0; c < N; c++) {
      int piv = c; while (piv < N && Fr::is_zero(A[piv][c])) piv++;
      if (piv == N) throw std::runtime_error("poseidon: singular sub-matrix in the sparse schedule");
      if (piv != c) for (int j = 0; j < 2 * N; j++) { const fe_t t = A[piv][j]; A[piv][j] = A[c][j]; A[c][j] = t; }
      const fe_t iv = Fr::inv(A[c][c]);
      for (int j = 0; j < 2 * N; j++) A[c][j] = Fr::mul(A[c][j], iv);
      for (int i = 0; i < N; i++) if (i != c) { const fe_t f = A[i][c]; for (int j = 0; j < 2 * N; j++) A[i][j] = Fr::sub(A[i][j], Fr::mul(f, A[c][j])); }
    }
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) hinv[i][j] = A[i][N + j];
    for (int j = 0; j < T; j++) tab[POS_ROW0 + T * k + j] = D[0][j];
    for (int i = 0; i < N; i++) { fe_t acc = zero; for (int j = 0; j < N; j++) acc = Fr::add(acc, Fr::mul(hinv[i][j], D[1 + j][0])); tab[POS_WHAT + N * k + i] = acc; }
    fe_t Dp[T][T]; for (int i = 0; i < T; i++) for (int j = 0; j < T; j++) Dp[i][j] = (i == 0 || j == 0) ? (i == j ? one : zero) : D[i][j];
    if (k + 1 < RP) { for (int i = 0; i < T; i++) for (int j = 0; j < T; j++) { fe_t acc = zero; for (int q = 0; q < T; q++) acc = Fr::add(acc, Fr::mul(mds[i][q], Dp[q][j])); D[i][j] = acc; } }
    else for (int i = 0; i < T; i++) for (int j = 0; j < T; j++) tab[POS_LEFT + T * i + j] = Dp[i][j];
  }
  // the check: the permutation the kernel runs against the plain schedule, on a fixed state
  fe_t a[T], b[T]; for (int i = 0; i < T; i++) a[i] = b[i] = rc[(size_t)(7 * i + 3) % rc.size()];
  poseidon_permute_plain<FrPs>(a, tab.data()); poseidon_permute<FrPs>(b, tab.data());
  for (int i = 0; i < T; i++) if (!Fr::eq(a[i], b[i])) throw std::runtime_error("poseidon: the sparse partial-round schedule disagrees with the plain one");
  return tab;
}
inline const std::vector<fe_t> &poseidon_tables() { static const std::vector<fe_t> t = poseidon_build_tables(); return t; }

}  // namespace zk

#ifdef __HIPCC__
namespace zk {

constexpr uint32_t POS_LANES = 64;

// job j: words [word_off[j], word_off[j + 1]), squeeze positions sq_at[sq_off[j] .. sq_off[j + 1]) relative to its first word, challenges at out[sq_off[j] ..)
__global__ void __launch_bounds__(POS_LANES) k_poseidon_transcripts(const fe_t *__restrict__ tab, const fe_t *__restrict__ words, const uint64_t *__restrict__ word_off,
                                                                    const uint32_t *__restrict__ sq_at, const uint64_t *__restrict__ sq_off, uint32_t jobs, fe_t *__restrict__ out) {
  const uint32_t j = blockIdx.x * POS_LANES + threadIdx.x;
  if (j >= jobs) return;
  const uint64_t s0 = sq_off[j];
  poseidon_job<FrPs>(tab, words + word_off[j], sq_at + s0, (uint32_t)(sq_off[j + 1] - s0), out + s0);
}

}  // namespace zk
#endif  // __HIPCC__
