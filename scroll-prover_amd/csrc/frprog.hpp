// frprog.hpp -- one straight-line program over Fr, run for many jobs at once: the interpreter behind mi355_fr_program_host.  The scalar side of a PLONK verifier (x^n, the
// Lagrange values, the numerator tree at x, the SHPLONK scalars) is, for a given protocol, one fixed sequence of field operations on the proof's challenges and evaluations;
// N proofs of one protocol are N runs of that sequence on different inputs (include/mi355zk_plonk_scalar.hpp compiles it, plonk::verify_proofs runs it).
//
// REGISTERS  n_regs of them, 32-byte Montgomery words, fully reduced.  [0, n_consts) are the constants, shared by every job and read-only; [n_consts, n_consts + n_inputs) hold
//            the job's inputs; the rest are temporaries, undefined until written.
// PROGRAM    n_instr instructions of four u32 words (op, dst, a, b):
//              FRP_ADD / FRP_SUB / FRP_MUL   dst = a (+ | - | *) b
//              FRP_SQRN                      dst = a^(2^b), b an immediate <= 64
//              FRP_INV                       dst = a^-1; a == 0 gives 0 and sets bit 0 of the job's flag word (b is ignored)
//              FRP_NZ                        sets bit b of the flag word (b an immediate in 1 .. 31) when a == 0; writes no register (dst is ignored)
//            dst may alias an operand; dst is never a constant or an input.
// LAYOUT     the per-job registers live in the workspace as regs[(r - n_consts) * stride + job], stride = jobs rounded up to the wave size: the 64 lanes of a wavefront read one
//            register as 64 consecutive 32-byte words.  The program words and the register numbers are the same for every lane (wave-uniform); the constants are read at a
//            wave-uniform address.  Nothing crosses lanes: no LDS, no barrier, no atomics.
//
//   frprog_job     one job: inputs in, the program, outputs out; returns the flag word.  __host__ __device__: the kernel calls it for one lane, frprog_run_host in a loop.
//   frprog_check   every argument check of the entry point (host memory only), the offending index in the message
//   k_fr_program   one lane per job, grid = ceil(jobs / 64)
// Field arithmetic: FrPs (fp_asm.hpp) products and squarings, Fr additions, Fr::inv_sgcd for the inverse (its instruction stream does not depend on the data).
#pragma once
#include "fp_asm.hpp"
#include <string>
#include <vector>

namespace zk {

enum : uint32_t { FRP_ADD = 0, FRP_SUB = 1, FRP_MUL = 2, FRP_SQRN = 3, FRP_INV = 4, FRP_NZ = 5, FRP_OPS = 6 };
constexpr uint32_t FRP_MAX_REGS = 1u << 16, FRP_MAX_INSTR = 1u << 20, FRP_MAX_JOBS = 1u << 20, FRP_MAX_SQRN = 64, FRP_LANES = 64;
constexpr uint32_t FRP_FLAG_INV_OF_ZERO = 1u;
inline uint64_t frprog_stride(uint32_t jobs) { return ((uint64_t)jobs + FRP_LANES - 1) / FRP_LANES * FRP_LANES; }

ZK_HD fe_t frp_load(const fe_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return g_load(p);
#else
  return *p;
#endif
}
ZK_HD void frp_store(fe_t *p, const fe_t &v) {
#if defined(__HIP_DEVICE_COMPILE__)
  g_store(p, v);
#else
  *p = v;
#endif
}
// register r of the job whose column starts at `regs` (r is wave-uniform, so is the branch)
ZK_HD fe_t frp_reg(const fe_t *consts, uint32_t n_consts, const fe_t *regs, uint64_t stride, uint32_t r) {
  if (r < n_consts) return consts[r];
  return frp_load(regs + (uint64_t)(r - n_consts) * stride);
}

// regs: this job's column of the workspace (register r >= n_consts at regs[(r - n_consts) * stride]); inputs / outputs: this job's n_inputs / n_outputs words
template <class F> ZK_HD uint32_t frprog_job(const uint32_t *code, uint32_t n_instr, const fe_t *consts, uint32_t n_consts, const fe_t *inputs, uint32_t n_inputs, fe_t *regs,
                                             uint64_t stride, const uint32_t *out_regs, uint32_t n_outputs, fe_t *outputs) {
  for (uint32_t t = 0; t < n_inputs; t++) frp_store(regs + (uint64_t)t * stride, frp_load(inputs + t));
  uint32_t flags = 0;
#pragma nounroll
  for (uint32_t i = 0; i < n_instr; i++) {
    const uint32_t op = code[4 * (uint64_t)i], d = code[4 * (uint64_t)i + 1], ra = code[4 * (uint64_t)i + 2], rb = code[4 * (uint64_t)i + 3];
    const fe_t a = frp_reg(consts, n_consts, regs, stride, ra);
    fe_t r = a;
    if (op <= FRP_MUL) {
      const fe_t b = frp_reg(consts, n_consts, regs, stride, rb);
      r = op == FRP_ADD ? F::add(a, b) : op == FRP_SUB ? F::sub(a, b) : F::mul(a, b);
    } else if (op == FRP_SQRN) {
#pragma nounroll
      for (uint32_t k = 0; k < rb; k++) r = F::sqr(r);
    } else if (op == FRP_INV) {
      if (F::is_zero(a)) flags |= FRP_FLAG_INV_OF_ZERO;
      r = F::inv_sgcd(a);
    } else {   // FRP_NZ
      if (F::is_zero(a)) flags |= 1u << rb;
      continue;
    }
    frp_store(regs + (uint64_t)(d - n_consts) * stride, r);
  }
  for (uint32_t t = 0; t < n_outputs; t++) frp_store(outputs + t, frp_reg(consts, n_consts, regs, stride, out_regs[t]));
  return flags;
}

// the argument checks of mi355_fr_program_host, in the order the entry point reports them; false with the reason in `why`.  Host memory only.
inline bool frprog_check(const uint32_t *code, uint32_t n_instr, uint32_t n_regs, const void *consts, uint32_t n_consts, const void *inputs, uint32_t n_inputs, uint32_t jobs,
                         const uint32_t *out_regs, uint32_t n_outputs, const void *outputs, const uint32_t *flags_out, std::string &why) {
  auto no = [&](const std::string &s) { why = s; return false; };
  if (n_regs > FRP_MAX_REGS) return no("more than 2^16 registers");
  if (n_instr > FRP_MAX_INSTR) return no("more than 2^20 instructions");
  if (jobs > FRP_MAX_JOBS) return no("more than 2^20 jobs");
  if ((uint64_t)n_consts + n_inputs > n_regs) return no("n_consts + n_inputs = " + std::to_string((uint64_t)n_consts + n_inputs) + " exceeds n_regs = " + std::to_string(n_regs));
  if ((n_instr && !code) || (n_consts && !consts) || (n_outputs && !out_regs)) return no("null pointer");
  if (jobs && ((n_inputs && !inputs) || (n_outputs && !outputs) || !flags_out)) return no("null pointer");
  const uint32_t first_temp = n_consts + n_inputs;
  for (uint32_t i = 0; i < n_instr; i++) {
    const uint32_t op = code[4 * (size_t)i], d = code[4 * (size_t)i + 1], a = code[4 * (size_t)i + 2], b = code[4 * (size_t)i + 3];
    const std::string at = "instruction " + std::to_string(i) + ": ";
    if (op >= FRP_OPS) return no(at + "unknown op " + std::to_string(op));
    if (a >= n_regs) return no(at + "operand register " + std::to_string(a) + " is not below n_regs = " + std::to_string(n_regs));
    if (op <= FRP_MUL && b >= n_regs) return no(at + "operand register " + std::to_string(b) + " is not below n_regs = " + std::to_string(n_regs));
    if (op == FRP_SQRN && b > FRP_MAX_SQRN) return no(at + "SQRN by " + std::to_string(b) + ", more than 64 squarings");
    if (op == FRP_NZ && (b < 1 || b > 31)) return no(at + "NZ names flag bit " + std::to_string(b) + ", not one of 1 .. 31");
    if (op != FRP_NZ) {
      if (d >= n_regs) return no(at + "destination register " + std::to_string(d) + " is not below n_regs = " + std::to_string(n_regs));
      if (d < first_temp) return no(at + "destination register " + std::to_string(d) + " is a constant or an input (the first temporary is " + std::to_string(first_temp) + ")");
    }
  }
  for (uint32_t t = 0; t < n_outputs; t++) if (out_regs[t] >= n_regs) return no("output " + std::to_string(t) + " names register " + std::to_string(out_regs[t]) + ", not below n_regs = " + std::to_string(n_regs));
  uint32_t m[8]; for (int i = 0; i < 8; i++) m[i] = FrP::mod(i);
  for (uint32_t i = 0; i < n_consts; i++) if (Fr::w_geq(((const fe_t *)consts)[i].l, m)) return no("constant " + std::to_string(i) + " is not below r");
  for (uint64_t i = 0; i < (uint64_t)jobs * n_inputs; i++)
    if (Fr::w_geq(((const fe_t *)inputs)[i].l, m)) return no("input " + std::to_string(i % n_inputs) + " of job " + std::to_string(i / n_inputs) + " is not below r");
  return true;
}

// the whole call on the CPU, in the kernel's layout: what tests/hostcheck runs, and what a caller without a device may use to CHECK a program (never a fallback of the library)
inline void frprog_run_host(const uint32_t *code, uint32_t n_instr, uint32_t n_regs, const fe_t *consts, uint32_t n_consts, const fe_t *inputs, uint32_t n_inputs, uint32_t jobs,
                            const uint32_t *out_regs, uint32_t n_outputs, fe_t *outputs, uint32_t *flags_out) {
  const uint64_t stride = frprog_stride(jobs);
  fe_t junk; for (int i = 0; i < 8; i++) junk.l[i] = 0xA5A5A5A5u;   // a temporary read before it is written shows
  std::vector<fe_t> regs((size_t)(n_regs - n_consts) * stride, junk);
  for (uint32_t j = 0; j < jobs; j++)
    flags_out[j] = frprog_job<FrPs>(code, n_instr, consts, n_consts, inputs + (size_t)j * n_inputs, n_inputs, regs.data() + j, stride, out_regs, n_outputs, outputs + (size_t)j * n_outputs);
}

}  // namespace zk

#ifdef __HIPCC__
namespace zk {

__global__ void __launch_bounds__(FRP_LANES) k_fr_program(const uint32_t *__restrict__ code, uint32_t n_instr, const fe_t *__restrict__ consts, uint32_t n_consts,
                                                          const fe_t *__restrict__ inputs, uint32_t n_inputs, uint32_t jobs, fe_t *__restrict__ regs, uint64_t stride,
                                                          const uint32_t *__restrict__ out_regs, uint32_t n_outputs, fe_t *__restrict__ outputs, uint32_t *__restrict__ flags) {
  const uint32_t j = blockIdx.x * FRP_LANES + threadIdx.x;
  if (j >= jobs) return;
  flags[j] = frprog_job<FrPs>(code, n_instr, consts, n_consts, inputs + (uint64_t)j * n_inputs, n_inputs, regs + j, stride, out_regs, n_outputs, outputs + (uint64_t)j * n_outputs);
}

}  // namespace zk
#endif  // __HIPCC__
