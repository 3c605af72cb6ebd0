/*
 * mi355zk.h -- C-ABI of libmi355zk.so: the MI355X (gfx950) BN254 G1-MSM / Fr-NTT hot path that slots in
 * under scroll-prover's `halo2_proofs` dependency.
 *
 * Boundary.  scroll-prover itself holds no proving arithmetic; its GPU builds replace the whole
 * `halo2_proofs` crate through a cargo path override [REF docker/chain-prover/gpu/Dockerfile:7-8],
 * [REF docker/trace-prover/gpu/Dockerfile:6-7], next to the existing `[patch]` redirect [REF Cargo.toml:40-41].
 * The functions below are what such a replacement crate's FFI binds (INTEGRATION.md shows the Rust `extern "C"`
 * block and the patched call sites).  Each entry point names the halo2_proofs / halo2curves function it
 * stands in for; those crates are pinned at scroll-tech/halo2@e5ddf67 and scroll-tech/halo2curves@112f5b9
 * [REF Cargo.lock:1886-1888,1911-1913] and reached from [REF integration/src/prove.rs:37,67,96].
 *
 * Data conventions (pinned by fixture KATs A1-A4):
 *   Fr, Fq       32 B   4 x u64 little-endian limbs, Montgomery form (R = 2^256), fully reduced
 *   G1Affine     64 B   {x, y};  identity = (0, 0)                       == halo2curves::bn256::G1Affine
 *   G1           96 B   Jacobian {x, y, z}; identity z = 0               == halo2curves::bn256::G1
 * Results returned as G1 are normalised: (x, y, R) with R = Montgomery one, or (0, 0, 0) for the identity,
 * so `to_affine()` on the Rust side is a no-op and byte comparison is meaningful.
 *
 * Pointer flavours: `*_host` arguments are ordinary process memory owned by the caller (Rust Vec<..>): the
 * library copies to HBM, computes and copies back before returning.  `*_dev` arguments are HIP device
 * pointers on a bound device: blocks from mi355_buf_alloc (what the Rust shim's DevicePoly holds) or any other device
 * allocation (torch tensors in the bench) -- for callers that keep polynomials resident, SURVEY §8f-1.
 *
 * Errors: every function returns 0 on success or one of MI355_E*; nothing throws, aborts or unwinds across
 * the boundary.  mi355_last_error() gives a thread-local message.  There is NO CPU fallback inside the
 * library: without a usable gfx950 device every compute entry point fails with MI355_ENODEVICE and the
 * caller (the Rust shim) decides what to do.
 *
 * Threading: entry points may be called from any thread (rayon workers); the bound device is re-selected on the calling thread.  Locks are PER
 * DEVICE: a call that works on one device (every transform, scan, evaluation, element-wise operation, buffer copy) holds that device's lock
 * only, so callers on different devices run concurrently; MSM entry points hold every bound device (the point range is sharded over all of
 * them); lifecycle and SRS management hold everything.  The MSM options (mi355_msm_set_normalise / _set_window_bits) are per calling
 * THREAD: a setting made on one thread does not affect MSMs issued from another.  mi355_profile_enable may be called before mi355_init.
 *
 * Devices: mi355_init(id) binds one device (one process per GPU).  mi355_init_multi(ids, n) binds n devices to ONE process -- the shape
 * of the reference, where one prover process holds one params_map [REF integration/src/prove.rs:11-21]: registered bases are then
 * sharded by point range over the devices, every MSM entry point fans out behind the same signature, the per-device partial sums are
 * exchanged with one ncclAllGather (RCCL over xGMI) and folded on the first device.  The NTT does not shard at k <= 26
 * ("replicas only"): a `*_dev` call runs on the device that owns its operands (mi355_buf_alloc(.., slot)), a `*_host` call on whichever
 * bound device is free (round-robin), and the `*_batch_*` transforms deal independent polynomials over all bound devices.
 */
#ifndef MI355ZK_H
#define MI355ZK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK 0
#define MI355_EBADARG 1
#define MI355_ENODEVICE 2
#define MI355_EOOM 3
#define MI355_EHIP 4
#define MI355_ERCCL 5

/* ---- lifecycle ------------------------------------------------------------------------------------------- */
/* Bind this process to HIP device `device_id` (ordinal within HIP_VISIBLE_DEVICES) and create the stream.    */
int mi355_init(int device_id);
/* SURVEY 8b's `mi355_init(const int *device_ids, int n_devices)`: bind n_devices (1..16) devices to this process, create one RCCL
 * communicator over them (ncclCommInitAll; librccl.so.1 is loaded on demand, MI355_ERCCL if that fails) and enable peer access.
 * device_ids[0] is the primary device.  Listing one physical device twice is a TEST mode (needs MI355_ALLOW_DUP_DEVICES=1: a one-GPU box
 * can then run the N = 2 control flow with real kernels; the exchange becomes a device copy because no communicator can span one device
 * twice).  MI355_MULTI_FORCE=1 sends even a one-device MSM through the partial + exchange + fold path (a real one-rank ncclAllGather).   */
int mi355_init_multi(const int *device_ids, int n_devices);
int mi355_device_count(int *n_out);
int mi355_shutdown(void);
const char *mi355_last_error(void);
const char *mi355_version(void);
/* Launch all kernels on `hip_stream` (a hipStream_t, e.g. torch's current stream).  NULL selects the HIP null
 * (legacy default) stream -- torch's default stream.  After mi355_init the library uses a private non-blocking
 * stream; mi355_reset_stream() returns to it.                                                                 */
int mi355_set_stream(void *hip_stream);
int mi355_reset_stream(void);
/* Block until everything queued by the library has finished.                                                  */
int mi355_synchronize(void);

/* ---- resident buffers: where a proof's polynomials live between the calls of create_proof (the reference's caller is one long
 *      create_proof per layer [REF integration/src/prove.rs:36-43,67,96]).  A Rust `DevicePoly` (rust_shim/mi355zk.rs) owns one block and frees
 *      it on Drop; every `*_dev` entry point accepts pointers into these blocks (at any offset) -- and any other HIP device pointer of a bound
 *      device -- and runs on the device that owns them.  device_slot indexes the list given to mi355_init_multi (0 = the primary / only device).
 *      mi355_buf_free returns the block to a pool (no hipFree, which would synchronise the device); work already queued on it stays valid.   */
int mi355_buf_alloc(uint64_t bytes, int device_slot, void **dev_ptr_out);
int mi355_buf_free(void *dev_ptr);
int mi355_buf_trim(void);                                   /* give every pooled (free) block back to HIP                                  */
int mi355_buf_slot(const void *dev_ptr, int *slot_out);     /* which device slot owns this pointer                                         */
/* host -> device on the owner's COPY stream: overlaps the compute queued before AND after it; an upload into a block no call has used since
 * mi355_buf_alloc waits only for the work queued on it before its last mi355_buf_free.  Synchronous: on return the data is in HBM (calls
 * issued afterwards see it) and the host buffer may be reused.  Takes no device lock.                                                   */
int mi355_buf_upload(void *dst_dev, const void *src_host, uint64_t bytes);
int mi355_buf_download(void *dst_host, const void *src_dev, uint64_t bytes);   /* ordered after everything queued on the owner; synchronous */
/* Narrow uploads for narrow columns (create_proof steps 2-3 are PCIe-bound at the many-column layers while most witness cells are zeros, bytes or 64-bit words: SURVEY 8d's
 * witness-like distribution; lookup_bits of [REF integration/configs/layer1.config:11]).  dst receives n 32-byte Montgomery words either way.
 *   packed  src = n little-endian unsigned integers of width_bytes in {1, 2, 4, 8} (CANONICAL values: selectors, byte / range-checked / limb columns, whose kind the caller
 *           knows statically); W bytes per cell cross the link, the device multiplies by R
 *   sparse  the non-zero cells as (index, 32-byte Montgomery value) pairs in any order; dst is zero-filled first; a pair whose index is >= n is dropped on the device (it never reaches memory).  mi355_host_compact_nonzero builds the pairs from a plain
 *           column with `threads` host threads (zero is zero in Montgomery form: the scan needs no arithmetic), idx_out / vals_out sized for n entries.
 * The narrow data crosses PCIe like mi355_buf_upload (copy stream, no device lock; the host buffers may be reused on return); the expansion is QUEUED on the owner's compute
 * stream: calls issued afterwards on that device see the data.                                                                                                          */
int mi355_buf_upload_packed(void *dst_dev, const void *src_host, uint64_t n, uint32_t width_bytes);
int mi355_buf_upload_sparse(void *dst_dev, uint64_t n, const uint32_t *idx_host, const void *vals_host, uint64_t count);
int mi355_host_compact_nonzero(const void *src_host, uint64_t n, uint32_t *idx_out, void *vals_out, uint64_t *count_out, int threads);
int mi355_buf_copy(void *dst_dev, const void *src_dev, uint64_t bytes);        /* within a device or between two bound devices (xGMI)       */
int mi355_buf_zero(void *dst_dev, uint64_t bytes);
/* Page-locked host memory for buffers that cross PCIe more than once, or once but on the critical path (the witness columns of the many-column layers):
 * a first copy out of ordinary (pageable) memory runs at ~34 GB/s on this platform, out of page-locked memory at the link's ~56 GB/s.  The caller writes
 * its column into the block (witness synthesis can write there directly) and passes it to mi355_buf_upload / any `*_host` entry point like any pointer. */
int mi355_host_alloc(uint64_t bytes, void **host_ptr_out);
int mi355_host_free(void *host_ptr);
/* HBM accounting of one bound device (any pointer may be NULL): what HIP reports free / in total, and what this library holds in live
 * mi355_buf blocks, in pooled (freed, reusable) blocks and in its grow-only workspace arena.  A prover keeps the SRS of its degree set
 * [REF bin/src/trace_prover.rs:35-36] AND the proving key's extended-coset polynomials resident: the caller budgets window tables
 * (mi355_srs_precompute: W x the basis) against this figure and stays on the table-free schedule when they do not fit.     */
int mi355_mem_info(int device_slot, uint64_t *free_bytes, uint64_t *total_bytes, uint64_t *live_buf_bytes, uint64_t *pooled_bytes, uint64_t *workspace_bytes);
/* A limit on the device memory this library holds on one device slot, for a prover that shares its device: a chunk prover process keeps the SRS of three degrees, three
 * proving keys and one proof's working set in one process [REF integration/src/prove.rs:30-43], [REF bin/src/trace_prover.rs:35-43], 274-278 GiB of 288 (DESIGN.md sections 9
 * and 13), and a shared device cannot promise all 288.  Every allocation the library makes from HIP is booked in one ledger (csrc/mem_budget.hpp), by class.  With a limit set
 * (bytes > 0; 0 lifts it), an allocation that would take the held bytes past it is decided ON THE HOST, before any HIP call: first the slot's pooled blocks and free slabs go
 * back to HIP (what mi355_buf_trim does), then the optional NTT tables (folded coset shifts, divisor-scaled and 2-D inter-level tables: their passes have table-free forms
 * with the same bits and the tables are rebuilt when there is room again), and if that made no room the call returns MI355_EOOM; mi355_last_error names the limit, the held
 * bytes by class and the request.  The same order runs on a real out-of-memory error with no limit set.  Window tables (mi355_srs_precompute) belong to the caller's handle:
 * counted, never reclaimed.  A limit below what is already held refuses new allocations and frees nothing.  No device lock is taken; the slot need not be bound yet.      */
int mi355_mem_set_limit(int device_slot, uint64_t bytes);
/* What the ledger holds for one device slot (any pointer may be NULL): held = the sum of the classes; the limit (0: none); the high-water mark of held since
 * mi355_mem_reset_peak (the measure plonk::plan_residency's figures [DESIGN.md section 9] are checked against); class_bytes[0 .. n_classes): 0 slabs and direct mi355_buf
 * blocks (live, pooled or free ranges), 1 the workspace arena, 2 required NTT tables, 3 optional NTT tables, 4 SRS shards and mi355_srs_downsize results, 5 window tables,
 * 6 the fixed-base and Poseidon tables (entries past 6 read 0); reclaims = how often a reclaim gave something back; refused_bytes = the sum of the refused requests.  */
int mi355_mem_usage(int device_slot, uint64_t *held_bytes, uint64_t *limit_bytes, uint64_t *high_water_bytes, uint64_t *class_bytes, uint32_t n_classes, uint64_t *reclaims, uint64_t *refused_bytes);
int mi355_mem_reset_peak(int device_slot);                                      /* high-water := held; one proof's peak is read between two of these            */

/* ---- SRS ownership: ParamsKZG { g, g_lagrange } [halo2_proofs poly/kzg/commitment.rs], held for the process
 *      lifetime by the caller's params_map [REF bin/src/trace_prover.rs:35-43], [REF integration/src/prove.rs:12,26,58].
 *      A handle is one basis (n affine points) resident in HBM.                                               */
int mi355_srs_register_host(const void *bases_affine_host, uint64_t n, uint64_t *handle_out);
int mi355_srs_register_dev(const void *bases_affine_dev, uint64_t n, int copy, uint64_t *handle_out);
/* Prover::load_params for one degree [REF bin/src/trace_prover.rs:35-36; prover/src/utils.rs EXT-recalled]: a RawBytes params{k} file
 * (u32 LE k | g[2^k] x 64 B | g_lagrange[2^k] x 64 B | g2 128 B | s_g2 128 B; any other length is rejected, as load_params does)
 * streamed straight into device memory through two pinned staging buffers and registered as two library-owned bases.
 * flags bit 0: validate every point on the device (identity, or reduced coordinates on y^2 = x^3 + 3 -- the check SerdeFormat::RawBytes
 * makes on the CPU and RawBytesUnchecked skips).  g2_out / s_g2_out (optional, 128 B each) receive the two G2 points untouched.
 * flags bit 1: the file is SerdeFormat::Processed, the other format ParamsKZG::read_custom accepts [EXT-recalled poly/kzg/commitment.rs]:
 * u32 LE k | g[2^k] x 32 B | g_lagrange[2^k] x 32 B | g2 64 B | s_g2 64 B, so the required length is 4 + 2 * 2^k * 32 + 128 (with bit 1 clear such a
 * file is rejected for its length as before; with bit 1 set a RawBytes file is).  The 32-byte words (G1Affine::to_bytes, see mi355_g1_decompress_dev)
 * stream through the same two pinned buffers into a pooled device block and every chunk is decompressed on the device straight into the SRS shard it
 * belongs to, the copy of chunk i + 1 under the square roots of chunk i.  A word that is no point: MI355_EBADARG naming basis (g / g_lagrange) and index,
 * nothing registered.  Bit 0 is implied (a decompressed point is on the curve by construction).  g2_out / s_g2_out still receive 128-byte G2Affine
 * values, decoded on the host inside the library and checked to be on the twist.  Their 64-byte layout is recalled from halo2curves at the pinned commit
 * and NOT pinned by any fixture of the reference: x.c0 then x.c1 as canonical little-endian words, bit 6 of byte 63 = parity of canonical y.c0,
 * identity = 64 zero bytes.                                                                                                              */
int mi355_srs_load_params_file(const char *path, uint32_t flags, uint32_t *k_out, uint64_t *g_handle_out, uint64_t *g_lagrange_handle_out, void *g2_out, void *s_g2_out);
/* `&params.g[..n]` as a handle of its own (ParamsKZG::downsize keeps g[..2^k]; load_params_map clones + downsizes
 * [REF integration/tests/integration.rs:17-22]): the first n points of `parent_handle`, SHARING its device memory and window tables --
 * no copy, no second 48 GiB table.  Handles that share memory may be released in any order; the last one frees it.                 */
int mi355_srs_register_prefix(uint64_t parent_handle, uint64_t n, uint64_t *handle_out);
int mi355_srs_release(uint64_t handle);
/* Optional, once per basis: build T[w][i] = 2^(c w) * P_i (w < W = ceil(255 / c), affine, W * n * 64 B of HBM) so that all
 * windows of an MSM on this basis share ONE bucket set: no per-window Horner (255 serial doublings), W x fewer bucket
 * reductions.  c = 0 picks the window for MSMs of n_hint points (0 = the whole basis).  MSMs on the handle then use the
 * table whenever it is the cheaper schedule for their length.  The SRS is fixed for the life of the prover (params_map
 * [REF bin/src/trace_prover.rs:35-43]), so this is registration-time work, like the reference's own g_lagrange set-up. */
int mi355_srs_precompute(uint64_t handle, uint64_t n_hint, int c);
int mi355_srs_pre_dev_ptr(uint64_t handle, void **dev_ptr_out, int *c_out, int *windows_out);
int mi355_srs_len(uint64_t handle, uint64_t *n_out);
/* device pointer of the resident basis (n x 64 B), for tests and chained device-side work                     */
int mi355_srs_dev_ptr(uint64_t handle, void **dev_ptr_out);

/* ---- MSM: halo2_proofs::arithmetic::best_multiexp(coeffs, bases) -> C::Curve, and the two wrappers
 *      ParamsKZG::commit / commit_lagrange = best_multiexp(poly, &g[..n] / &g_lagrange[..n]).
 *      out_g1 receives 96 B (normalised Jacobian, see above) in host memory.                                  */
int mi355_msm_g1_host(uint64_t srs_handle, uint64_t base_offset, const void *scalars_host, uint64_t n, void *out_g1_host);
int mi355_msm_g1_dev(uint64_t srs_handle, uint64_t base_offset, const void *scalars_dev, uint64_t n, void *out_g1_host);
/* multi-GPU leg: the per-GPU partial sum stays in device memory (96 B at out_g1_dev, written in stream order, no host
 * synchronisation) so that it can be handed to the RCCL all-gather directly; mi355_g1_sum_dev folds the gathered partials.        */
int mi355_msm_g1_dev_async(uint64_t srs_handle, uint64_t base_offset, const void *scalars_dev, uint64_t n, void *out_g1_dev);
int mi355_g1_sum_dev(const void *points_jac_dev, uint64_t n, void *out_g1_host);
/* `batch` commitments over the SAME basis slice in one pass (e.g. all advice columns of a phase: create_proof commits them one
 * after the other): scalars_dev is a host array of `batch` device pointers (n x 32 B each), out receives
 * batch x 96 B.  Results are identical to `batch` separate calls; the fixed per-call costs are paid once.                          */
int mi355_msm_g1_batch_dev(uint64_t srs_handle, uint64_t base_offset, const void *const *scalars_dev, uint32_t batch, uint64_t n, void *out_g1_host);
/* the same with `batch` host pointers (what the Rust loop over advice columns holds)                                              */
int mi355_msm_g1_batch_host(uint64_t srs_handle, uint64_t base_offset, const void *const *scalars_host, uint32_t batch, uint64_t n, void *out_g1_host);
/* ad-hoc bases (best_multiexp with bases that are not a registered SRS)                                        */
int mi355_msm_g1_adhoc_host(const void *bases_affine_host, const void *scalars_host, uint64_t n, void *out_g1_host);
/* MANY SHORT MSMs in one launch: the final MSM of a verifier (19-24 terms), once per proof of a batch.  Serves the aggregator's native succinct verification of
 * every chunk / layer snark behind gen_batch_proof [REF integration/src/prove.rs:67] (extract_accumulators_and_proof [EXT-recalled]) and plonk::verify_proofs / plonk::aggregate.
 * out[s] = sum_{offsets[s] <= i < offsets[s+1]} scalars[i] * bases[i], s < segments.  bases: G1Affine 64 B (identity (0,0) allowed), scalars: Fr 32 B Montgomery,
 * offsets: segments + 1 values, offsets[0] = 0, non-decreasing; out: segments x G1Affine (identity = all zero), the form mi355_pairing_products_host takes.
 * One wavefront per segment, one double-and-add per term: any length is correct, a long one is slow -- use mi355_msm_g1_adhoc_host for those.
 * MI355_EBADARG (before the device is looked at): null pointers, offsets[0] != 0, decreasing offsets, segments > 2^20, more than 2^24 terms.  segments == 0 touches nothing.
 * Bases are not validated (the contract of mi355_msm_g1_adhoc_host).                                                                                                  */
int mi355_msm_g1_segmented_host(const void *bases_affine_host, const void *scalars_host, const uint64_t *offsets_host, uint32_t segments, void *out_g1affine_host);
/* MANY POSEIDON TRANSCRIPTS in one launch: the sponge of snark-verifier's PoseidonTranscript<NativeLoader> (T = 5, RATE = 4, R_F = 8, R_P = 60, x^5, Grain LFSR constants,
 * initial state (2^64, 0, 0, 0, 0)) for every proof of a batch.  Serves gen_batch_proof [REF integration/src/prove.rs:67]: the aggregator's native succinct verifier reads every
 * chunk snark through that transcript; on the verifier's side every absorbed word is known before the first squeeze and the squeeze positions are fixed by the protocol, so
 * N proofs are N independent sponges with a known script (plonk::verify_proofs / plonk::aggregate with VerifyOptions::device_transcript).
 * Job j is one fresh sponge: its words are words[word_offsets[j] .. word_offsets[j+1]) (Fr, 32 B Montgomery, fully reduced), its squeeze positions
 * squeeze_at[squeeze_offsets[j] .. squeeze_offsets[j+1]) (non-decreasing, relative to the job's first word, each <= the job's length), and its challenges land at
 * challenges_out[squeeze_offsets[j] ..), 32 B each, Montgomery.  Challenge k of a job = squeeze() after update(words[.. squeeze_at[k]) not yet absorbed); words behind the last
 * squeeze are not hashed; a job without squeezes writes nothing.  The constants are the library's own (generated and checked once per process); the caller passes none.
 * One lane per job: the call costs one sponge's latency whatever `jobs` is.  Kernel time reports as "poseidon_transcripts" in mi355_profile_get.
 * MI355_EBADARG (before the device is looked at, each with its own message): a null pointer; an offsets array that does not start at 0 or decreases; a squeeze position that
 * decreases within a job or exceeds the job's length; more than 2^20 jobs, 2^24 words or 2^24 squeezes; a word that is not below r (the first such index is named).
 * jobs == 0 launches nothing.  No CPU fallback (MI355_ENODEVICE).                                                                                                    */
int mi355_poseidon_transcripts_host(const void *words_host, const uint64_t *word_offsets_host, const uint32_t *squeeze_at_host, const uint64_t *squeeze_offsets_host,
                                    uint32_t jobs, void *challenges_out_host);
/* ONE STRAIGHT-LINE PROGRAM OVER Fr, RUN FOR MANY JOBS in one launch: the scalar side of the same batch of verifiers behind gen_batch_proof [REF integration/src/prove.rs:67] --
 * x^n, the Lagrange values at x, the numerator tree at x, h(x) and the SHPLONK scalars are, for one protocol, one fixed sequence of field operations on the proof's challenges,
 * evaluations and instances (plonk::verify_proofs / plonk::aggregate with VerifyOptions::device_scalars; include/mi355zk_plonk_scalar.hpp compiles the sequence).
 * Registers: n_regs words of 32 B (Fr, Montgomery, fully reduced).  [0, n_consts) = consts, shared by every job; [n_consts, n_consts + n_inputs) = job j's inputs
 * inputs[j * n_inputs ..]; the rest are temporaries, undefined until written.  An instruction is four u32 words (op, dst, a, b): 0 ADD, 1 SUB, 2 MUL (dst = a op b);
 * 3 SQRN (dst = a^(2^b), b an immediate <= 64); 4 INV (dst = 1 / a; zero gives zero and sets bit 0 of the job's flag word); 5 NZ (sets flag bit b, an immediate in 1 .. 31,
 * when a == 0; writes no register, dst is ignored).  dst may alias an operand.  outputs[j * n_outputs + t] = register out_regs[t] of job j; flags_out[j] = its flag word.
 * One lane per job, the program read as wave-uniform data: the call costs one job's latency whatever `jobs` is.  Kernel time reports as "fr_program" in mi355_profile_get.
 * MI355_EBADARG (before the device is looked at, each with its own message and the offending index): a null pointer; an unknown op; a register >= n_regs; a dst below
 * n_consts + n_inputs; an immediate out of range; n_regs > 2^16, n_instr > 2^20, jobs > 2^20; a constant or an input that is not below r.  jobs == 0 launches nothing.
 * No CPU fallback (MI355_ENODEVICE).                                                                                                                                  */
int mi355_fr_program_host(const uint32_t *code_host, uint32_t n_instr, uint32_t n_regs, const void *consts_host, uint32_t n_consts, const void *inputs_host, uint32_t n_inputs,
                          uint32_t jobs, const uint32_t *out_regs_host, uint32_t n_outputs, void *outputs_host, uint32_t *flags_out_host);
/* sum of `n` G1 (Jacobian, any representative) points: the fold `results.iter().fold(identity, |a, b| a + b)` of
 * best_multiexp, used to combine per-GPU partial sums after the RCCL all-gather.                  */
int mi355_g1_sum_host(const void *g1_points_host, uint64_t n, void *out_g1_host);
/* group::Curve::batch_normalize(p: &[G1], q: &mut [G1Affine]) [EXT-recalled halo2curves bn256 / group crate; create_proof normalises each
 * vector of projective commitments with it before they enter the transcript]: n Jacobian points (96 B, any representative) -> n affine
 * points (64 B), the identity (Z = 0) becomes (0, 0).  One shared inversion per 256 points (Montgomery's trick).  Input and output
 * must not overlap; the _dev variant is asynchronous on the library stream.                                                          */
int mi355_g1_batch_normalize_dev(const void *g1_points_dev, void *affine_out_dev, uint64_t n);
int mi355_g1_batch_normalize_host(const void *g1_points_host, void *affine_out_host, uint64_t n);
/* halo2curves G1Affine::from_bytes / to_bytes over whole arrays [EXT-recalled halo2curves derive/curve.rs; the 32-byte form is pinned by fixture KAT A4]:
 * the compressed word of SerdeFormat::Processed params files, proofs and .vkey files = little-endian canonical x, bit 6 of byte 31 = parity of canonical y,
 * bit 7 ignored, identity = 32 zero bytes.  decompress: n words (32 B) -> n affine points (64 B, Montgomery, reduced), one square root in Fq per point on the
 * device.  A word that is no point (x >= q; x^3 + 3 a non-residue; x = 0 with the sign bit set) is written as the identity, the call returns MI355_EBADARG,
 * mi355_last_error() names the smallest such index and *first_bad_out (optional) receives it; *first_bad_out = ~0 when every word decodes.  compress: n affine
 * points (reduced coordinates, trusted as everywhere in this ABI) -> n words.  Input and output must not overlap; device pointers 16-byte aligned; n < 2^32.
 * _dev: runs on the library stream of the device that owns the output; decompress returns when the error word has been read (the result decides the return
 * code), compress is asynchronous.  _host: staged through device workspace in chunks of 2^22 points, synchronous.  No CPU fallback (MI355_ENODEVICE).
 * Kernels report as "g1_decompress" / "g1_compress" in mi355_profile_get.  No subgroup check (G1 of BN254 has cofactor 1).                              */
int mi355_g1_decompress_dev(const void *bytes_dev, void *affine_out_dev, uint64_t n, uint64_t *first_bad_out);
int mi355_g1_decompress_host(const void *bytes_host, void *affine_out_host, uint64_t n, uint64_t *first_bad_out);
int mi355_g1_compress_dev(const void *affine_dev, void *bytes_out_dev, uint64_t n);
int mi355_g1_compress_host(const void *affine_host, void *bytes_out_host, uint64_t n);
/* (per calling thread) normalise = 0: subsequent MSM results are SOME Jacobian representative of the sum (as best_multiexp's C::Curve is) instead of the
 * normalised one; saves the serial field inversion (~0.4 ms) where the result is folded again anyway (per-GPU partial sums).      */
int mi355_msm_set_normalise(int on);
/* tuning (per calling thread): window bits c for subsequent MSMs: 0 = automatic from n (window tables used when registered and cheaper),
 * -1 = automatic but ignoring window tables (the memory-lean schedule: per-window bucket sets + Horner), 2..24 = fixed, no tables       */
int mi355_msm_set_window_bits(int c);
/* pipelined schedule of a large single MSM: the point range is cut into `chunks` slices and the (memory-bound) sort of slice k + 1
 * runs under the (ALU-bound) accumulation of slice k on separate HIP streams; results are identical.  Off by default (measured
 * slower on MI355X: the accumulation holds every wave slot; env MI355_MSM_CHUNKS).  chunks = 1 disables, 0 restores the default;
 * min_log_n = smallest log2(n) that is cut.                                                                                       */
int mi355_msm_set_pipeline(uint32_t chunks, uint32_t min_log_n);

/* ---- NTT: halo2_proofs::arithmetic::best_fft(a, omega, log_n): in place, natural order in -> natural order out,
 *      a'[i] = sum_j a[j] omega^(ij), no scaling.  omega: 32 B Montgomery, must have order 2^log_n.            */
int mi355_ntt_fr_host(void *data_host, uint32_t log_n, const void *omega);
int mi355_ntt_fr_dev(void *data_dev, uint32_t log_n, const void *omega);
/* EvaluationDomain::ifft = best_fft(a, omega_inv, log_n) followed by a[i] *= divisor (= n^-1) [poly/domain.rs]   */
int mi355_intt_fr_host(void *data_host, uint32_t log_n, const void *omega_inv, const void *divisor);
int mi355_intt_fr_dev(void *data_dev, uint32_t log_n, const void *omega_inv, const void *divisor);
/* EvaluationDomain::coeff_to_extended: dst[2^log_ext] = fft_{extended_omega}( zero-pad(coeffs[2^log_n]) with
 * a[i] *= {1, g_coset, g_coset_inv}[i % 3] )  (distribute_powers_zeta, into the coset)                          */
int mi355_coeff_to_extended_host(void *dst_host, const void *coeffs_host, uint32_t log_n, uint32_t log_ext,
                                 const void *g_coset, const void *g_coset_inv, const void *extended_omega);
int mi355_coeff_to_extended_dev(void *dst_dev, const void *coeffs_dev, uint32_t log_n, uint32_t log_ext,
                                const void *g_coset, const void *g_coset_inv, const void *extended_omega);
/* EvaluationDomain::extended_to_coeff: in place ifft(extended_omega_inv, extended_ifft_divisor) then
 * a[i] *= {1, g_coset_inv, g_coset}[i % 3]; the caller truncates.                                               */
int mi355_extended_to_coeff_host(void *data_host, uint32_t log_ext, const void *g_coset, const void *g_coset_inv,
                                 const void *extended_omega_inv, const void *extended_ifft_divisor);
int mi355_extended_to_coeff_dev(void *data_dev, uint32_t log_ext, const void *g_coset, const void *g_coset_inv,
                                const void *extended_omega_inv, const void *extended_ifft_divisor);

/* distribute_powers: a[i] *= factor^i (in place), and the general coset transform dst = best_fft(coeffs[i] * coset_factor^i, omega):
 * what `coeff_to_extended_part(poly, g_coset * extended_omega^j)` of the scroll fork does per quotient part [EXT-recalled domain.rs]. */
int mi355_distribute_powers_fr_dev(void *data_dev, uint64_t n, const void *factor);
int mi355_coset_ntt_fr_dev(void *dst_dev, const void *coeffs_dev, uint32_t log_n, const void *coset_factor, const void *omega);
/* `batch` independent transforms in one call -- the loops of create_proof over columns (the iNTT of every advice column, the
 * coset NTTs of every polynomial that enters evaluate_h; 8 + 32 for a layer-4 proof [REF integration/configs/layer4.config:3-10]).
 * divisor == NULL: best_fft; divisor = n^-1: EvaluationDomain::ifft.  Host pointers are dealt round-robin over the bound devices (one
 * worker thread and PCIe link per device; on each device the upload of item i + 1, the transform of item i and the download of item
 * i - 1 overlap over two staging buffers: 56 ms instead of 87 ms per 2^26 polynomial); device pointers run on the device that owns
 * them, concurrently across devices.  Results equal the serial loop's.                                                              */
int mi355_ntt_fr_batch_host(void *const *data_host, uint32_t batch, uint32_t log_n, const void *omega, const void *divisor);
int mi355_ntt_fr_batch_dev(void *const *data_dev, uint32_t batch, uint32_t log_n, const void *omega, const void *divisor);
int mi355_coset_ntt_fr_batch_dev(void *const *dst_dev, const void *const *coeffs_dev, uint32_t batch, uint32_t log_n, const void *coset_factor, const void *omega);

/* element-wise operations on device-resident vectors of Fr (op 0: a + b, 1: a - b, 2: a * b; dst may alias a or b) and
 * data[i] *= table[i mod period] (period a power of two <= 4096; EvaluationDomain::divide_by_vanishing_poly multiplies the extended
 * evaluations by the inverted t_evaluations, whose period is 2^(extended_k - k)).  The pointwise glue of SURVEY 8f-1.            */
int mi355_fr_vec_op_dev(int op, void *dst_dev, const void *a_dev, const void *b_dev, uint64_t n);
/* dst = a + scalar * b (a_dev == NULL: dst = scalar * b; dst may alias a or b): the running linear combination sum_i v^i p_i(X) of the
 * multi-open argument and every other "poly * scalar" of create_proof [EXT-recalled halo2_proofs poly: Polynomial * F, + ].       */
int mi355_fr_vec_axpy_dev(void *dst_dev, const void *a_dev, const void *b_dev, const void *scalar, uint64_t n);
int mi355_fr_vec_mul_periodic_dev(void *data_dev, uint64_t n, const void *table_host, uint32_t period);
/* The operand shape of evaluate_h [EXT-recalled halo2_proofs src/plonk/evaluation.rs; SURVEY 3.2 step 7: gates read ROTATED columns,
 * a[(i + rot * 2^(extended_k - k)) mod n], and evaluate an expression over dozens of extended-domain polynomials]:
 *     dst[i] (+)= sum_{j < n_terms} coeffs[j] * prod_{k < term_len[j]} polys[factor_poly[.]][(i + factor_rot[.]) mod n]
 * in ONE launch instead of a chain of mi355_fr_vec_op_dev calls (each a full HBM round trip).  Term j owns term_len[j] consecutive entries
 * of factor_poly / factor_rot (host arrays); coeffs: n_terms x 32 B Montgomery (host); rotations in ELEMENTS, already scaled by the caller,
 * negative values allowed; n a power of two (the extended domain, or one 2^k coset part).  Limits per launch: 24 polynomials, 16 terms,
 * 16 factors per term, 48 factors in all (larger expressions are split, accumulate = 1 adds to dst).  dst may alias a polynomial only
 * when every rotation of that polynomial is zero.  Terms with c_j = 1 or c_j = -1 cost no multiplication for the coefficient (2^26, 9 terms /
 * 20 factors: 8.7 ms against 12.2 ms with general coefficients).                                                                                   */
int mi355_fr_gate_eval_dev(void *dst_dev, const void *const *polys_dev, uint32_t n_polys, const void *coeffs_fr_host, const uint32_t *term_len,
                           uint32_t n_terms, const uint32_t *factor_poly, const int32_t *factor_rot, uint64_t n, int accumulate);
/* the extended-domain vector from its Q <= 8 coset parts (scroll fork: evaluate_h works part by part, part q = the evaluations at
 * zeta * extended_omega^(q + Q i), i < n): dst[i * Q + q] = parts[q][i], i.e. the natural order mi355_extended_to_coeff_dev inverts           */
int mi355_fr_interleave_dev(void *dst_dev, const void *const *parts_dev, uint32_t q_parts, uint64_t n);
/* the multiplicative scans of the permutation / lookup arguments [EXT-recalled halo2_proofs src/plonk/permutation/prover.rs,
 * src/plonk/lookup/prover.rs]: data[i] = data[i]^-1 with zeros left zero (ff::BatchInvert), and the grand product
 * dst[0] = 1, dst[i] = prod_{j<i} src[j] (dst may alias src; total_out_host, optional, receives prod_{j<n} src[j] and makes the
 * call synchronous).  Asynchronous on the library stream otherwise.                                                               */
int mi355_fr_batch_invert_dev(void *data_dev, uint64_t n);
/* kate_division(poly, z) = (poly(X) - poly(z)) / (X - z) [EXT-recalled halo2_proofs src/arithmetic.rs], the quotient polynomials of the
 * multi-open argument: n coefficients in, n - 1 out (q_i = a_(i+1) + z q_(i+1), a parallel scan).  dst must not overlap poly, except
 * dst == poly + 1 element (the quotient then replaces coefficients 1 .. n-1 in place).                                             */
int mi355_fr_kate_division_dev(void *dst_dev, const void *poly_dev, uint64_t n, const void *z);
int mi355_fr_prefix_product_dev(void *dst_dev, const void *src_dev, uint64_t n, void *total_out_host);
/* the additive counterpart: dst[0] = 0, dst[i] = sum_{j<i} src[j] -- the running sum phi of the log-derivative (mv-lookup) argument of the
 * scroll fork [EXT-recalled halo2_proofs src/plonk/mv_lookup/prover.rs: phi[i + 1] = phi[i] + sum_j 1 / (beta + f_j[i]) - m[i] / (beta + t[i]);
 * SURVEY 3.2 step 4 "lookup grand-sum"].  Same aliasing and total_out_host rules (the total must be zero for a valid argument).       */
int mi355_fr_prefix_sum_dev(void *dst_dev, const void *src_dev, uint64_t n, void *total_out_host);
/* the multiplicity column m of the log-derivative (mv) lookup argument, which the scroll fork computes inside the prover after theta
 * [EXT-recalled halo2_proofs src/plonk/mv_lookup/prover.rs, `prepare`: a map from each compressed table value to a row of the usable range,
 * m[row] += 1 per compressed input cell, Error::ConstraintSystemFailure for an input value the table lacks].  m_dev: n words out;
 * table_dev: n words, rows < table_rows are the table; inputs_dev: host array of n_inputs device pointers, rows < input_rows are read.
 * m[r] counts the input cells (every column, rows < input_rows) equal to the value table row r holds, where r is the FIRST row of the
 * table holding that value (flags bit 0: the LAST row); rows >= table_rows of m are zero.  Values are compared as 32-byte words, which
 * is field equality because Fr words are fully reduced (Data conventions above).  A value absent from the table: MI355_EBADARG,
 * *missing_out (optional) = (input index << 40) | row of the smallest such pair, m_dev unspecified; otherwise *missing_out = ~0.
 * n < 2^31, n_inputs x input_rows < 2^32.  Workspace: one pooled mi355_buf block of ~12 B per row (mi355_mem_info counts it, mi355_buf_trim
 * returns it).  Runs on the library stream of the device that owns m_dev and returns when m is written (the result decides the error).  */
int mi355_fr_lookup_multiplicities_dev(void *m_dev, uint64_t n, const void *table_dev, uint64_t table_rows, const void *const *inputs_dev,
                                       uint32_t n_inputs, uint64_t input_rows, uint32_t flags, uint64_t *missing_out);
/* the permuted columns A' and S' of the classic halo2 lookup argument (upstream PSE / zcash halo2, before the scroll fork's mv-lookup), which halo2
 * computes inside the prover after theta [EXT-recalled halo2_proofs src/plonk/lookup/prover.rs, `permute_expression_pair`].  All four operands are
 * DEVICE memory (mi355_buf ranges of at least `rows` words, 16-byte aligned): perm_input and perm_table out, input and table (the theta-compressed
 * columns) in; rows >= `rows` of the outputs are not touched (the caller's blinding rows).  perm_input is `input` sorted ascending by the canonical
 * integer value (halo2curves' Ord; the Montgomery words are converted before they are compared).  Every row of perm_input that starts a run of equal
 * values takes the same value in perm_table and uses up one copy of it in the table; the copies of the table left over, in ascending order with
 * duplicates, fill the other rows from the LAST such row backwards (halo2 pop()s them).  Every output word is a copy of a table word.  An input value
 * absent from the table: MI355_EBADARG, *missing_out (optional) = the smallest row of `input`, in its original order, with such a value, outputs
 * unspecified; otherwise *missing_out = ~0.  MI355_EBADARG with the reason in mi355_last_error(), before the device is asked for, for rows >= 2^31, a
 * null or misaligned pointer, a range that leaves its block, outputs that overlap each other or an input, and operands on different devices.
 * rows == 0 writes nothing.  Workspace: one pooled mi355_buf block of 52 .. 60 B per row (mi355_mem_info counts it, mi355_buf_trim returns it,
 * mi355_mem_set_limit applies: MI355_EOOM).  Runs on the library stream of the device that owns the outputs and returns when they are written; the
 * same operands give the same bytes on every run.                                                                                                  */
int mi355_fr_lookup_permute_dev(void *perm_input, void *perm_table, const void *input, const void *table, uint64_t rows, uint64_t *missing_out);
/* sigma columns of the permutation argument from the copy mapping [EXT-recalled halo2_proofs src/plonk/permutation/keygen.rs, build_pk / build_vk:
 * permutations[i][j] = delta^i' omega^j' for mapping[i][j] = (i', j'), which halo2 fills on the CPU from a num_cols x n table].  sigma_dev: host array of
 * n_cols device pointers, each n = 2^log_n words out (Lagrange basis); delta, omega: 32-byte words on the host.  A cell is the integer column * n + row
 * (column = position in the permutation).  Every cell gets sigma[j][r] = delta^j omega^r (the identity permutation); every t < count then overrides
 * sigma[cells_host[t]] = delta^j' omega^r' for (j', r') = images_host[t].  count == 0 gives the identity, count == n_cols * n is the dense mapping.  The
 * lists are checked on the host before anything is uploaded or launched: MI355_EBADARG, with the first offending index t in mi355_last_error(), for a cell
 * or image >= n_cols * n, a cell listed twice, or images that are not exactly the listed cells (on MI355_EBADARG the columns are untouched); also for
 * n_cols == 0, log_n > 28 and columns on different devices.  flags bit 0: the caller vouches for its mapping (halo2's Assembly is a permutation by
 * construction) and only the range check runs; cells listed twice then end on either value.  Only the listed cells cross the link (16 B each).
 * Workspace: one pooled mi355_buf block (pointers, n_cols + 2^ceil(log_n / 2) + 2^floor(log_n / 2) table words, at most 2^22 staged overrides;
 * mi355_mem_info counts it, mi355_buf_trim returns it).  Runs on the library stream of the device that owns the columns and returns when they are written.  */
int mi355_fr_permutation_sigma_dev(void *const *sigma_dev, uint32_t n_cols, uint32_t log_n, const void *delta, const void *omega,
                                   const uint64_t *cells_host, const uint64_t *images_host, uint64_t count, uint32_t flags);
/* ---- a witness judged where it lives [EXT-recalled halo2_proofs src/dev.rs, MockProver::verify: gate, lookup and permutation failures]: the two reductions that turn
 * "a gate evaluated on every row" and "the copy mapping" into a short list of failures (csrc/check.hpp); plonk::check_witness (mi355zk_plonk.hpp) is the driver.
 * A failing witness is NOT an error: both calls return MI355_OK and report through their outputs.  Both are synchronous (the result is the answer), run on the library
 * stream of the device that owns the operands, and are deterministic: same counts, same indices on every run.  cap <= 65536; cap == 0 returns the counts only (the index
 * output may then be NULL).  Workspace: one pooled mi355_buf block (mi355_mem_info counts it, mi355_buf_trim returns it).  MI355_EBADARG, before any launch, with the
 * offending index in mi355_last_error(): batch == 0, n == 0, n_cols == 0, log_n > 28, cap > 65536, a cell or image >= n_cols << log_n, operands on different devices.
 *
 * MockProver's gate check: vecs_dev is a host array of `batch` device pointers, each n words (n need not be a power of two).  counts_out_host[v] = the rows of vector v
 * whose 32-byte word is not all-zero (all eight 32-bit limbs take part); rows_out_host[v * cap ..] = the smallest `cap` such rows, ascending, unused slots ~0.          */
int mi355_fr_nonzero_rows_dev(const void *const *vecs_dev, uint32_t batch, uint64_t n, uint32_t cap, uint64_t *counts_out_host, uint64_t *rows_out_host);
/* MockProver's permutation check: cols_dev is a host array of n_cols device pointers, each 2^log_n words (the columns in permutation position order); a cell is the integer
 * column * n + row, as mi355_fr_permutation_sigma_dev takes it.  Pair t fails when the words of cells_host[t] and images_host[t] differ.  *n_failed_out = the failing pairs,
 * failed_t_out_host[0 .. cap) = the smallest `cap` failing t, ascending, unused slots ~0.  The lists need not be a permutation; they are staged in pieces of at most 2^22
 * pairs (16 B per pair cross the link).                                                                                                                                  */
int mi355_fr_copy_check_dev(const void *const *cols_dev, uint32_t n_cols, uint32_t log_n, const uint64_t *cells_host, const uint64_t *images_host, uint64_t count,
                            uint32_t cap, uint64_t *n_failed_out, uint64_t *failed_t_out_host);

/* ---- the prover's randomness, drawn where the polynomials live (csrc/frrand.hpp): uniform field elements from ChaCha20 (RFC 8439 block function, 20 rounds).  One
 * 64-byte block per element: state words 4..11 = key32 as eight little-endian words, words 12..13 = the 64-bit block counter, words 14..15 = the 64-bit stream
 * identifier (with stream = 0 and a counter below 2^32: RFC 8439 with a zero nonce) [EXT-recalled: also the state layout of rand_chacha's ChaCha20Rng, whose block
 * is the eight next_u64 words halo2curves' Fr::random consumes].  The block, read as a 512-bit little-endian integer, is reduced mod r
 * [EXT-recalled halo2curves Fr::from_u512: d0 R^2 + d1 R^3 by two Montgomery products]; the word written is fully reduced, Montgomery form.  Every element is a pure
 * function of (key, stream, counter): the result does not depend on the grid, on the device or on how a vector is cut into calls, and a caller can recompute it on
 * the CPU (halo2::fr_random_reference).  Asynchronous on the library stream of the device that owns the destination; n == 0 / n_cols == 0 / rows == 0: MI355_OK, no
 * launch.  MI355_EBADARG: a draw whose counters counter0 .. counter0 + count would wrap 2^64 (checked first: a stream must never repeat a block), a null or misaligned
 * pointer, a range that leaves its mi355_buf block, columns on different devices.  No CPU path (MI355_ENODEVICE).  The key is passed to the kernel and nowhere else: it
 * never appears in mi355_last_error(), in MI355_TRACE output or in a range name.  Choosing the key (an operating-system source in production) and never reusing a
 * (key, stream, counter) triple across proofs is the caller's business.
 *
 * dst[i] = element(key32, stream, counter0 + i), i < n.                                                                                                              */
int mi355_fr_random_dev(void *dst, uint64_t n, const uint8_t *key32, uint64_t stream, uint64_t counter0);
/* cols: host array of n_cols device pointers; rows [row0, row0 + rows) of column c = element(key32, stream, counter0 + c * rows + j), j < rows: the blinding rows of a
 * batch of columns in one launch.  Rows outside the range are not touched.  The call does not mark the columns' blocks as in use: a mi355_buf_upload into OTHER rows of a
 * column is not ordered against it (and keeps its overlap with the compute stream); an upload into the SAME rows must wait for mi355_synchronize.                                                                                           */
int mi355_fr_random_rows_dev(void *const *cols, uint32_t n_cols, uint64_t row0, uint32_t rows, const uint8_t *key32, uint64_t stream, uint64_t counter0);
/* halo2curves' Fr::from_uniform_bytes over an array: src = n 64-byte little-endian integers, dst = n words, their residues mod r (Montgomery, fully reduced).  src and
 * dst must not overlap.                                                                                                                                              */
int mi355_fr_from_u512_dev(void *dst, const void *src, uint64_t n);

/* ---- halo2_proofs::arithmetic::eval_polynomial(poly, point) = sum_i poly[i] * point^i  (the evaluations written to the
 *      transcript in step 9 of create_proof); out_fr_host receives 32 B.  First widening into SURVEY 8f-3.   */
int mi355_eval_polynomial_dev(const void *poly_dev, uint64_t n, const void *point, void *out_fr_host);
/* `batch` evaluations with one device synchronisation (step 9 of create_proof: every queried (polynomial, rotation) pair): polys_dev[i] has n
 * coefficients, points = batch x 32 B (Montgomery), out_fr_host = batch x 32 B.  Same values as `batch` calls of mi355_eval_polynomial_dev.      */
int mi355_eval_polynomial_batch_dev(const void *const *polys_dev, uint32_t batch, uint64_t n, const void *points, void *out_fr_host);
int mi355_eval_polynomial_host(const void *poly_host, uint64_t n, const void *point, void *out_fr_host);

/* ---- synthetic SRS: ParamsKZG::setup(k, rng) restated on the device [poly/kzg/commitment.rs]:
 *      g[i] = tau^i G,  g_lagrange[i] = L_i(tau) G.  Writes n = 2^k affine points per basis to device memory.   */
int mi355_srs_setup_dev(void *g_dev, void *g_lagrange_dev, uint32_t k, const void *tau, const void *omega);
/* points[i] = scalars[i] * G (fixed-base, batch-normalised); building block of the above                      */
int mi355_g1_fixed_base_mul_dev(void *points_affine_dev, const void *scalars_dev, uint64_t n);

/* ---- G2: out = scalar * p on the twist y^2 = x^3 + 3 / (9 + u) over Fq2.  Points are 128-byte halo2curves G2Affine values
 * (x.c0 | x.c1 | y.c0 | y.c1, Montgomery limbs; identity = all zero) -- the layout of `g2` / `s_g2` in a RawBytes params file.  The one G2
 * operation on the path: ParamsKZG::setup's s_g2 = tau * G2 [EXT-recalled poly/kzg/commitment.rs]; a G2 MSM does not exist in create_proof
 * (SURVEY 8a a7), but the library provides one below for callers that commit in G2.  MI355_EBADARG when p is not on the twist.  The
 * generator constant is halo2curves' G2 generator, pinned by the pairing input of the released verifier
 * [REF release-v0.13.1/evm_verifier.yul:1230-1233].                                                                                    */
int mi355_g2_mul_host(const void *p_g2affine_host, const void *scalar_fr, void *out_g2affine_host);
/* ---- G2 MSM: out = sum_i scalars[i] * bases[i] on the twist (Pippenger; the digit and sort stages of the G1 MSM, G2 bucket kernels).
 * bases: n x 128-byte G2Affine as above (identity = all zero); scalars: n x 32-byte Fr, Montgomery form as for mi355_msm_g1_*; out: one
 * normalised G2Affine (identity = 128 zero bytes; n == 0 gives the identity).  Every base is checked to be on the twist in a device pass:
 * MI355_EBADARG, and mi355_last_error() names the first bad index, when one is not.  Bases are NOT checked for subgroup membership (a
 * point of the twist outside the r-torsion is summed like any other: its scalar multiplies it as the canonical integer below r, exactly as
 * mi355_g2_mul_host does).  One device (the primary), no CPU fallback (MI355_ENODEVICE
 * without a gfx950 device); same locking and stream order as the G1 entry points.  mi355_msm_last_plan reports the call's window
 * bits, windows and entries; mi355_msm_set_window_bits applies as for G1.  The kernels report under msm_g2_* in mi355_profile_get.
 *   _adhoc_host: bases and scalars in host memory.   _dev: both in device memory of the primary device (mi355_buf_alloc blocks or any
 *   device pointer).   _batch_dev: `batch` scalar vectors over one basis, out = batch x 128 B.                                          */
int mi355_msm_g2_adhoc_host(const void *bases_g2affine_host, const void *scalars_host, uint64_t n, void *out_g2affine_host);
int mi355_msm_g2_dev(const void *bases_g2affine_dev, const void *scalars_dev, uint64_t n, void *out_g2affine_host);
int mi355_msm_g2_batch_dev(const void *bases_g2affine_dev, const void *const *scalars_dev, uint32_t batch, uint64_t n, void *out_g2affine_host);

/* ---- the optimal ate pairing of BN254 on the device: products of pairings, one per group of consecutive pairs
 *      out[g] = prod_{j < pairs_per_group} e(P[g * ppg + j], Q[g * ppg + j])   for g < groups
 * P: 64-byte G1Affine, Q: 128-byte G2Affine (Montgomery limbs, identity = all zero; a pair with an identity contributes 1).
 * gt_out (optional): groups x 384 B, halo2curves' Fq12 memory layout c0.c0.c0 | c0.c0.c1 | c0.c1.c0 | ... | c1.c2.c1 (Fq12 = c0 + c1 w,
 * Fq6 = c0 + c1 v + c2 v^2, Fq2 = c0 + c1 u; 32-byte Montgomery words).  is_one_out (optional): groups x u32, 1 where the product is 1 --
 * what the EVM precompile at address 8 answers for that group.
 * Every P is checked to be on the curve and every Q on the twist in a device pass: MI355_EBADARG, and mi355_last_error() names the first
 * bad pair, when one is not; nothing else is launched then.  Q is NOT checked for membership of the subgroup of order r: that stays the
 * caller's responsibility, as for the bases of mi355_msm_g2_*.  For a Q outside the subgroup the result is unspecified (the call returns).
 * The device is looked up first, as in every entry point: without a bound device every call, groups == 0 included, is MI355_ENODEVICE.  With one,
 * groups == 0 is a no-op; pairs_per_group == 0, both outputs NULL, or more than 2^20 pairs in one call are MI355_EBADARG.  One Miller loop
 * per pair (one lane each), a tree of pairwise products inside each group, one final exponentiation per group; the workspace (two
 * 384-byte values per pair) is one pooled mi355_buf block, back in the pool on return.  Same device choice, lock and stream order as
 * mi355_g2_mul_host; synchronous; no CPU fallback (MI355_ENODEVICE).  The kernels report under pairing_* in mi355_profile_get.            */
int mi355_pairing_products_host(const void *p_g1affine_host, const void *q_g2affine_host, uint32_t groups, uint32_t pairs_per_group,
                                void *gt_out_host, uint32_t *is_one_out_host);

/* ---- best_fft::<Fr, G1> -- the same DFT over G1 points, a'[i] = sum_j omega^(ij) a[j] -- and its one caller, g_to_lagrange, which
 * ParamsKZG::downsize(k) [REF integration/tests/integration.rs:17-22] and ParamsKZG::setup run to rebuild g_lagrange from
 * g[..2^k]: g_lagrange = n^-1 * DFT_{omega^-1}(g) [EXT-recalled halo2_proofs src/arithmetic.rs g_to_lagrange].
 * Points: 96-byte Jacobian in place (any representative in, normalised z = R / all-zero identity out); g_to_lagrange takes and
 * returns 64-byte affine points (input and output may be the same buffer).                                                        */
int mi355_g1_fft_dev(void *points_jac_dev, uint32_t log_n, const void *omega);
int mi355_g1_fft_host(void *points_jac_host, uint32_t log_n, const void *omega);
int mi355_g_to_lagrange_dev(const void *g_affine_dev, void *g_lagrange_affine_dev, uint32_t log_n, const void *omega_inv, const void *n_inv);
/* downsize on handles: a NEW library-owned basis g_lagrange' = g_to_lagrange(g[..2^k]) from a registered coefficient basis
 * (omega_inv = omega_k^-1, n_inv = 2^-k, Montgomery); mi355_srs_read_host copies points of any registered basis back, which is
 * how the Rust ParamsKZG refills its g_lagrange Vec after downsize.                                                                */
int mi355_srs_downsize(uint64_t g_handle, uint32_t k, const void *omega_inv, const void *n_inv, uint64_t *g_lagrange_handle_out);
int mi355_srs_read_host(uint64_t handle, uint64_t offset, uint64_t n, void *out_affine_host);

/* ---- the prover and the verifier behind the C-ABI: what the operators above exist for, one FFI call each.  The reference reaches halo2_proofs::plonk::create_proof once
 * per layer and verifies what comes out [REF integration/src/prove.rs:36-43,50-53,67,75-80,95-97]; a `halo2_proofs` fork calls the entry points below instead of transcribing
 * that flow into Rust (rust_shim/create_proof_ffi.rs; INTEGRATION.md "tier C without a transcription").  They wrap the C++ of include/mi355zk_plonk*.hpp, mi355zk_transcript.hpp
 * and mi355zk_plonk_verify.hpp -- plonk::keygen, create_proof, check_witness, verify_proof, verify_proofs, aggregate -- unchanged: the same device calls, the same bytes.
 *
 * Objects are uint64_t HANDLES of five kinds: protocol, circuit, proving key, options, record.  Handles come from one counter and a value is never issued twice; a freed,
 * never-issued or wrong-kind handle is MI355_EBADARG with the expected kind in mi355_last_error(), never a dereference.  mi355_plonk_free takes any kind.  A circuit and a key
 * KEEP THEIR PROTOCOL ALIVE: freeing the protocol's handle first is allowed (the handle dies at once, the memory with its last user).  A key does not refer to the circuit it
 * was made from.  Freeing a key returns its device blocks to the pool (mi355_buf_trim gives them back to HIP).  An options handle of 0 means the defaults everywhere.
 * Errors: no exception crosses; halo2::Error keeps its code, std::bad_alloc is MI355_EOOM, every complaint about an argument, a protocol or a layout is MI355_EBADARG, the
 * message in the calling thread's mi355_last_error().  The entry points that compute on the device (keygen, create_proof, check_witness, verification without host_only) look
 * the device up first: without one they are MI355_ENODEVICE whatever their other arguments.
 * Byte outputs (out, cap, bytes_out): *bytes_out receives the size; cap == 0 asks for the size alone; 0 < cap < size is MI355_EBADARG and nothing is written.
 * Threading: an object is used by one thread at a time; distinct objects may be used from distinct threads (keygen and proofs of different keys run concurrently as far as the
 * per-device locks above allow); the verification entry point serialises on one mutex inside the library (the verifier's headers keep their phase clocks in function statics).
 *
 * PlonkProtocol: snark-verifier's JSON of a circuit's constraint system, as [REF release-v0.13.1/chunk.protocol] and what `compile` serialises (mi355zk_plonk_protocol.hpp);
 * from text (len bytes, no terminator needed) or from a file.  Malformed text or a protocol outside the recognised shape: MI355_EBADARG, nothing issued.                     */
int mi355_plonk_protocol_from_json(const char *json, uint64_t len, uint64_t *protocol_out);
int mi355_plonk_protocol_from_file(const char *path, uint64_t *protocol_out);
/* one figure of the protocol by name: k, n, layer (~0 when the file names none), num_preprocessed, num_instance, num_advice, num_lookups, num_perm_columns, num_perm_chunks,
 * num_gates, num_witness (all phases), num_commitments, blind, usable, quotient_pieces, extended_k, num_evaluations, num_queries, lookup_bits, proof_bytes_poseidon (also the
 * Blake2b layout), proof_bytes_evm, has_initial_state, has_accumulator, lookup_permuted (1: the classic halo2 lookup argument, 0: mv-lookup).  An unknown field: MI355_EBADARG naming it.                                                          */
int mi355_plonk_protocol_info(uint64_t protocol, const char *field, uint64_t *value_out);
int mi355_plonk_free(uint64_t handle);
/* plonk::Circuit, owned by the library: what keygen assigns and `synthesize` fills in the reference [EXT-recalled halo2_proofs plonk/keygen.rs, plonk/prover.rs].  _new: every
 * column present and zero, no copy constraints, no instance values.  _synthetic: plonk::build_circuit(protocol, CircuitOptions{seed, blind_seed, fill, assign_density, flags
 * bit 0 pinned, bit 1 zero_blinding}) -- a satisfying instance for the protocol; the same arguments give the same instance.
 * _set / _get move one part, named by `what` (index = which column / lookup / permutation chunk; 0 where there is one).  Words are 32-byte Fr, Montgomery, as everywhere here:
 *   preprocessed  n words, Lagrange values of fixed column `index` (_get also answers for the sigma columns, derived from the copies; _set refuses them)
 *   advice, m     n words                    m_counts      n x uint32_t, the multiplicities as integers
 *   m_blind, z_blind, phi_blind   `blind` words (protocol_info)          random_poly   n words, coefficients
 *   perm_blind    2 x (blind + 1) words, lz_blind  `blind` words: protocols with the classic (permuted) lookup argument only (protocol_info "lookup_permuted"), per lookup --
 *                 the rows from the l_last row on of A', then of S'; the last rows of the lookup's grand product.  Such protocols have no m, m_counts, m_blind, phi_blind
 *   instances     at most num_instance words                             copies        records of four uint64_t (position a, row a, position b, row b): two cells of
 *                                                                                      the permutation's columns, in the protocol's order, that must be equal; replaces the list
 * A size that does not match the protocol, an index out of range, a cell outside the permutation: MI355_EBADARG, the circuit unchanged.                                      */
int mi355_plonk_circuit_new(uint64_t protocol, uint64_t *circuit_out);
int mi355_plonk_circuit_synthetic(uint64_t protocol, uint64_t seed, uint64_t blind_seed, double fill, double assign_density, uint32_t flags, uint64_t *circuit_out);
int mi355_plonk_circuit_set(uint64_t circuit, const char *what, uint32_t index, const void *data, uint64_t bytes);
int mi355_plonk_circuit_get(uint64_t circuit, const char *what, uint32_t index, void *out, uint64_t cap, uint64_t *bytes_out);
/* plonk::keygen = halo2's keygen_vk + keygen_pk [EXT-recalled halo2_proofs plonk/keygen.rs]: the fixed and sigma columns committed on srs_g_lagrange (a handle of
 * mi355_srs_register_*), the proving key resident in HBM until its handle is freed.  flags bit 0: the extended-coset parts stay resident too; bit 1: device_sigma (the sigma
 * columns from one mi355_fr_permutation_sigma_dev call).  devices: as ProofOptions::devices of the proofs to come.  The circuit must belong to `protocol`.
 * _pk_vk: the verifying key serialised like [REF release-v0.13.1/vk_chunk.vkey] (u32 BE k | u32 BE fixed columns | 32-byte compressed commitments).                          */
int mi355_plonk_keygen(uint64_t protocol, uint64_t circuit, uint64_t srs_g_lagrange, uint32_t flags, int devices, uint64_t *pk_out);
int mi355_plonk_pk_vk(uint64_t pk, void *out, uint64_t cap, uint64_t *bytes_out);
/* the fields of plonk::ProofOptions, VerifyOptions and CheckOptions by name, values as text: integers in decimal, booleans 0 / 1 / true / false, transcript = blake2b |
 * poseidon | evm | by_layer, rng_key = 64 hexadecimal digits (the 32 key bytes in order), initial_state = 64 hexadecimal digits (a big-endian integer, reduced mod r: the
 * verifier's first transcript scalar).  Names: devices threads commit_batch upload_threads early_intt sparse_uploads packed_multiplicities device_multiplicities
 * multiplicity_rule_last check_witness device_randomness rng_key rng_key_from_os coset_group_polys transcript | check_accumulator accumulator host_only device_transcript
 * device_scalars initial_state | cap theta_seed.  What is not set keeps the default of its struct.  An unknown name, or a value that does not parse or is out of range: MI355_EBADARG naming it. */
int mi355_plonk_options_new(uint64_t *opts_out);
int mi355_plonk_options_set(uint64_t opts, const char *name, const char *value);
/* halo2_proofs::plonk::create_proof [REF integration/src/prove.rs:37,67,96] = plonk::create_proof over the key and the circuit's witness; srs_g / srs_g_lagrange: the two bases
 * of ParamsKZG.  The proof (the reference's byte layout, protocol_info's proof_bytes_* long) goes to proof_out; a cap below that size is refused before any work.  record_out
 * (optional) receives a record handle (mi355_plonk_record_json).  With check_witness set and a failing witness: MI355_EBADARG, the first failure in the message, every failure
 * in the record, nothing written to proof_out.
 * _check_witness = MockProver::verify on the device (plonk::check_witness).  A failing witness is NOT an error, as for mi355_fr_copy_check_dev: MI355_OK, the number of
 * reported failures in *n_failures_out, the failures in the record.                                                                                                          */
int mi355_plonk_create_proof(uint64_t srs_g, uint64_t srs_g_lagrange, uint64_t pk, uint64_t circuit, uint64_t opts, void *proof_out, uint64_t cap, uint64_t *bytes_out, uint64_t *record_out);
int mi355_plonk_check_witness(uint64_t pk, uint64_t circuit, uint64_t opts, uint64_t *n_failures_out, uint64_t *record_out);
/* the verifier of [REF integration/src/prove.rs:50-53,75-80] and the aggregator's native verification behind gen_batch_proof [REF integration/src/prove.rs:67] over n proofs.
 * mode 0: plonk::verify_proofs (one decompression, one segmented MSM, one pairing call); 1: plonk::verify_proof in a loop; 2: plonk::aggregate with its pairing; 3: aggregate,
 * fold only (g2 / s_g2 may be NULL).  Per proof i: its protocol handle; vk_bytes[i] / vk_len[i] the .vkey, NULL (or vk_bytes == NULL) = the protocol file's own preprocessed
 * commitments; instances[i] = n_instances[i] words; proofs[i] = proof_len[i] bytes.  g2, s_g2: 128-byte G2Affine of ParamsKZG; s_g2_is_negated != 0: s_g2 holds -[s]g2 already.
 * opts applies to every proof.  A REJECTED proof is not an error: MI355_OK, ok_out[i] = 0, the named failure (proof_length, non_canonical_scalar, invalid_point,
 * accumulator_limb, pairing, ...) in the record.  Modes 2 and 3 judge the proofs together: ok_out[i] = 1 when the aggregation stands and proof i passed its own part.
 * host_only (modes 0 and 1) stops every proof after its (scalars, points) list and needs no device.                                                                          */
int mi355_plonk_verify_proofs(uint32_t n, const uint64_t *protocols, const void *const *vk_bytes, const uint64_t *vk_len, const void *const *instances, const uint64_t *n_instances,
                              const void *const *proofs, const uint64_t *proof_len, const void *g2, const void *s_g2, uint32_t s_g2_is_negated, uint64_t opts, uint32_t mode,
                              uint8_t *ok_out, uint64_t *record_out);
/* a record as strict JSON text (no terminator; cap == 0 asks for the size).  "kind": "proof" -- ProofResult: proof_bytes, transcript, total_ms, step_ms {...}, msm, intt,
 * coset_ntt, gate_launches, evals, rotation_sets, plan_launches / _terms / _tmps / _constraints / _prefix_groups, peak_hbm_bytes, hbm_total_bytes, sparse_columns,
 * packed_columns, witness_link_bytes, coset_groups, coset_retransforms, random_ms, multiplicity_ms; after a refused witness "ok": false, "error" and "failures".
 * "kind": "check" -- n_failures, failures [{kind, index, row, count, col_a, col_b, row_b, message}].  "kind": "verify" -- mode, device_calls, proofs [{ok, error, detail,
 * host_only, challenges, numerator_at_x, msm {scalars, points, result, w_prime}, has_accumulator, pairing}] with field elements and coordinates as 64 hexadecimal digits
 * (big-endian, canonical), and for modes 2 and 3 "aggregate" {ok, error, detail, accumulators, r, lhs, rhs, limbs, pairing}.                                                 */
int mi355_plonk_record_json(uint64_t record, char *out, uint64_t cap, uint64_t *bytes_out);

/* ---- measurement hooks (bench.py): HIP-event timing of the kernels of the most recent MSM / NTT call.       */
int mi355_profile_enable(int on);
/* name in {"msm_total","msm_digits","msm_sort","msm_accumulate","msm_reduce","ntt_total","ntt_pass","g1_decompress","g1_compress"}; returns the
 * accumulated milliseconds and launch count since the last mi355_profile_reset().                             */
int mi355_profile_get(const char *name, double *ms_out, uint64_t *launches_out);
int mi355_profile_reset(void);
/* (c, windows, entries) chosen by the last MSM (on the primary device), for G1-adds accounting                 */
int mi355_msm_last_plan(int *c_out, int *windows_out, uint64_t *entries_out);
/* how the last MSM ran: device slots that took part; the exchange: "none" | "rccl_allgather" | "device_copy" (static string); whether the
 * window tables (one shared bucket set) were used on the primary device; point-range slices of the host-pointer path (1 = one copy)  */
int mi355_msm_last_run(int *devices_out, const char **exchange_out, int *shared_tables_out, int *host_slices_out);

/* test hook: copy `bytes` of the internal workspace buffer `role` (e.g. "msm.offsets", "msm.sorted") to the host   */
int mi355_debug_ws_read(const char *role, uint64_t offset, void *dst_host, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif
