/* zkp_toolbox.h -- C ABI of the HOST side of the MI355X zkp engine: Merlin transcripts and the
 * Prover / Verifier / BatchVerifier flows of dalek-cryptography/zkp (src/toolbox/), batched so that the
 * GPU is entered once per phase for a whole batch of proofs instead of once per 2-term MSM.
 *
 * Layering:  this library (libzkp_toolbox.so, C++/g++)  ->  zkp_mi355x.h (libzkp_mi355x.so, HIP).
 * Group arithmetic goes through the zkp_mi355x.h entry points, except for TINY calls and calls without a context (ctx == NULL), which
 * run the same field / group headers on the host (zkp_toolbox_set_host_max_terms below) -- a backend choice by size, never a silent
 * fallback: a call that needs the GPU and cannot have it fails with a negative code.  Host work (STROBE/Keccak transcripts, scalar arithmetic mod l, coefficient build) runs on
 * `n_threads` host threads (0 = all hardware threads).
 *
 * Reference mapping (what each call replaces, for N proofs of ONE statement at a time):
 *   zkp_prove_batch            N x { macros.rs:206-258 build_prover ; prover.rs:76-112 prove_impl }
 *   zkp_verify_compact_batch   N x { macros.rs:280-311 build_verifier ; verifier.rs:80-120 }
 *   zkp_verify_batchable_each  N x { build_verifier ; verifier.rs:123-173 }
 *   zkp_batch_verify           macros.rs:336-370 batch_verify ; batch_verifier.rs:67-235
 * Return codes: 0 = done (per-proof verdicts in `results`); ZKP_TB_VERIFICATION_FAILURE /
 * ZKP_TB_BATCH_SIZE_MISMATCH mirror src/errors.rs:4-11; negative = infrastructure failure (see
 * zkp_mi355x.h) -- never treat a non-zero code as "verified".
 */
#ifndef ZKP_TOOLBOX_H
#define ZKP_TOOLBOX_H

#include <stddef.h>
#include <stdint.h>
#include "zkp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKP_TB_OK 0
#define ZKP_TB_VERIFICATION_FAILURE 1   /* ProofError::VerificationFailure (errors.rs:6)  */
#define ZKP_TB_BATCH_SIZE_MISMATCH 2    /* ProofError::BatchSizeMismatch   (errors.rs:9)  */
#define ZKP_TB_BAD_STATEMENT (-10)      /* malformed statement descriptor / NULL argument  */
#define ZKP_TB_INVALID_POINT (-11)      /* prover was handed an encoding that does not decode */
#define ZKP_TB_NO_ENTROPY (-12)         /* entropy / weights16 == NULL and the operating system's getrandom() failed */
#define ZKP_TB_TOO_LONG (-14)           /* a transcript message, output or label longer than UINT32_MAX bytes (merlin asserts) */

/* ---- Merlin transcripts (merlin::Transcript, re-exported by the reference at lib.rs:35) ----------- */
#define ZKP_TRANSCRIPT_BYTES 208        /* opaque, plain-old-data: memcpy = Clone */
void zkp_transcript_init(uint8_t t[ZKP_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len);
/* Merlin frames every message / output with its length as a u32 and asserts that the length fits (merlin 2.x
 * `encode_usize_as_u32`; the reference's tests/sig_and_vrf_example.rs:224-241 is the `#[ignore]`d > 4 GiB case): a `len`
 * above UINT32_MAX -- or a label longer than that -- is ZKP_TB_TOO_LONG and leaves the transcript untouched, never a
 * silently truncated length prefix.  Returns ZKP_TB_OK otherwise. */
int zkp_transcript_append_message(uint8_t t[ZKP_TRANSCRIPT_BYTES], const char* label, const uint8_t* msg, size_t len);
int zkp_transcript_challenge_bytes(uint8_t t[ZKP_TRANSCRIPT_BYTES], const char* label, uint8_t* out, size_t len);
/* N x append_message(label, msgs[offsets[j], offsets[j + 1])) on host threads; shared_initial != 0: every transcript starts from ts[0].  The
 * ZKP_TB_TOO_LONG rule above per message; decreasing offsets or NULL buffers are ZKP_TB_BAD_STATEMENT; nothing changes on an error. */
int zkp_transcripts_append_message_batch(uint8_t* ts /*[N][208]*/, uint32_t N, int shared_initial, const char* label, const uint8_t* msgs,
                                         const uint64_t* offsets /*[N + 1]*/, int n_threads);
/* The same with a context, and its counterpart for challenge_bytes (zkp_mi355x.h (7)).  Both route as the other batch calls do: ctx == NULL
 * or N <= zkp_toolbox_get_host_max_terms() on the host threads (host Merlin), anything else on the device, one lane per transcript
 * (a label of more than 248 bytes stays on the host; so does an append whose messages hold fewer than 128 bytes per transcript on
 * average: the device call moves every blob over the bus, and measured, profiles/transcript_ops_bench.txt, it loses to the host threads
 * on 32-byte messages at every N).  Same bytes on both routes; with ctx == NULL the append gives the bytes of
 * zkp_transcripts_append_message_batch.  The transcripts may stand at any mix of positions.  Errors as above, and a position byte
 * (byte 200 of a blob) of 166 or more is ZKP_TB_BAD_STATEMENT: it is no STROBE state.  Nothing changes on an error.
 *   zkp_transcripts_challenge_bytes_batch: N x challenge_bytes(label, out[j], len), the blobs advanced in place; len = 0 is allowed (the
 *   frame and the PRF's begin still advance the transcript; out may then be NULL). */
int zkp_transcripts_append_message_batch_ctx(zkp_ctx* ctx, uint8_t* ts /*[N][208]*/, uint32_t N, int shared_initial, const char* label,
                                             const uint8_t* msgs, const uint64_t* offsets /*[N + 1]*/, int n_threads);
int zkp_transcripts_challenge_bytes_batch(zkp_ctx* ctx, uint8_t* ts /*[N][208]*/, uint32_t N, const char* label, uint32_t len, int n_threads,
                                          uint8_t* out /*[N][len]*/);
/* The rest of the reference's TranscriptProtocol (src/toolbox/mod.rs:165-228) and its prover's TranscriptRng (src/toolbox/prover.rs:78-89)
 * over N transcripts at any mix of positions, for protocols the constraint system cannot express: semantics in zkp_mi355x.h (7).
 * (domain_sep and append_scalar_var are append_message with the labels "dom-sep" and "scvar".)
 *   zkp_transcripts_witness_rng_batch: build_rng; rekey_with_witness_bytes(label, witness k) for k < m; finalize; then count x Scalar::random
 *     (mode ZKP_RNG_SCALARS, out [N][count][32] canonical) or one fill_bytes(count) (ZKP_RNG_BYTES, out [N][count]).  The transcripts are
 *     read, never written.  witnesses [N][m][wlen]; entropy [N][32], or NULL: drawn the way zkp_prove_batch draws the prover's entropy
 *     (ZKP_TB_NO_ENTROPY if the operating system gives none).
 *   zkp_transcripts_challenge_scalars_batch: get_challenge(label) -> out [N][32], canonical; the blobs advance in place.
 *   zkp_transcripts_append_points_batch: append_message(kind, var_label); append_message("val", points[j]) -- kind "ptvar" is
 *     append_point_var, "blindcom" append_blinding_commitment.  validate != 0: the validating forms, status[j] = 1 and blob j unchanged for
 *     a row of 32 zero bytes; status [N] is required then, optional otherwise, and gets 0 for every other row.
 * ctx == NULL runs the lane code the kernels compile (zkp_amd/csrc/strobe_lane.h) on n_threads host threads; with a context, a batch of at
 * least zkp_toolbox_get_*_min_batch() transcripts goes to the device (UINT32_MAX = never, 0 = always).  Same bytes on both routes.  The
 * defaults follow the toolbox's rule -- the smallest measured N from which the synchronous device call is ahead of the host backend at 16
 * threads, beyond the spread of the rounds, at every measured shape -- over profiles/transcript_rng_bench.txt.
 * N = 0 is a no-op.  A NULL buffer with N > 0, a NULL label, a label of more than 248 bytes, another mode, N > 2^31 - 1 or a position byte
 * (byte 200 of a blob) of 166 or more is ZKP_TB_BAD_STATEMENT, and nothing changes on an error.
 * Secrets: the calls wipe the entropy they drew and the keyed STROBE state of every host lane before they return, on error paths too, and
 * make no host copy of the witnesses.  On the device route the staging of entropy and witnesses in the context's workspace is zeroed
 * (zkp_mi355x.h); NOT wiped: the outputs' device staging, which stays in the workspace until the next call reuses it, and whatever the
 * HIP runtime stages for its copies. */
int zkp_transcripts_witness_rng_batch(zkp_ctx* ctx, const uint8_t* ts /*[N][208]*/, uint32_t N, const char* label, uint32_t m, uint32_t wlen,
                                      const uint8_t* witnesses /*[N][m][wlen]*/, const uint8_t* entropy /*[N][32] or NULL*/, int mode, uint32_t count,
                                      int n_threads, uint8_t* out);
int zkp_transcripts_challenge_scalars_batch(zkp_ctx* ctx, uint8_t* ts /*[N][208]*/, uint32_t N, const char* label, int n_threads,
                                            uint8_t* out /*[N][32]*/);
int zkp_transcripts_append_points_batch(zkp_ctx* ctx, uint8_t* ts /*[N][208]*/, uint32_t N, const char* kind, const char* var_label,
                                        const uint8_t* points /*[N][32]*/, int validate, int n_threads, uint8_t* status /*[N]*/);
void zkp_toolbox_set_witness_rng_min_batch(uint32_t n);
uint32_t zkp_toolbox_get_witness_rng_min_batch(void);
void zkp_toolbox_set_challenge_scalars_min_batch(uint32_t n);
uint32_t zkp_toolbox_get_challenge_scalars_min_batch(void);
void zkp_toolbox_set_append_points_min_batch(uint32_t n);
uint32_t zkp_toolbox_get_append_points_min_batch(void);

/* ---- scalars mod l (curve25519_dalek::scalar::Scalar) -------------------------------------------- */
void zkp_scalar_from_wide(uint8_t out[32], const uint8_t in[64]);   /* from_bytes_mod_order_wide */
void zkp_scalar_muladd(uint8_t out[32], const uint8_t a[32], const uint8_t b[32], const uint8_t c[32]);   /* a*b + c */
void zkp_scalar_neg(uint8_t out[32], const uint8_t a[32]);

/* ---- statement descriptor: what define_proof! fixes (macros.rs:124-138, 159-170) ------------------ */
typedef struct zkp_statement zkp_statement;
zkp_statement* zkp_statement_new(const char* proof_label);
void zkp_statement_free(zkp_statement* st);
/* Variables are numbered in ALLOCATION order, which is part of the statement (it fixes the transcript).
 * The macro allocates all secrets, then instance points, then common points (macros.rs:215-242). */
int zkp_statement_add_secret(zkp_statement* st, const char* name);                 /* -> secret index  */
int zkp_statement_add_point(zkp_statement* st, const char* name, int is_common);   /* -> point index   */
/* lhs = sum_i secrets[i] * points[i]   (SchnorrCS::constrain, toolbox/mod.rs:86-98) */
int zkp_statement_constrain(zkp_statement* st, uint32_t lhs_point, uint32_t n_terms, const uint32_t* secrets,
                            const uint32_t* points);
uint32_t zkp_statement_num_secrets(const zkp_statement* st);
uint32_t zkp_statement_num_instance(const zkp_statement* st);
uint32_t zkp_statement_num_common(const zkp_statement* st);
uint32_t zkp_statement_num_constraints(const zkp_statement* st);

/* Data layout shared by all batch calls (N = batch size, m = #secrets, ni / ns = #instance / #common
 * points, nc = #constraints; "rank" = position among the points of the same kind, in allocation order):
 *   transcripts   [N][ZKP_TRANSCRIPT_BYTES]  in/out: advanced exactly as the reference advances them
 *   secrets       [N][m][32]    each witness as the 32 bytes of the caller's Scalar, reduced or not: the prover's RNG is re-keyed
 *                               with the bytes as given (prover.rs:80), the response is (s mod l) * c + b mod l; outputs are canonical
 *   inst_points   [ni][N][32]   row = variable, column = proof (what allocate_instance_point receives,
 *                               batch_verifier.rs:115-134; Matrix layout util.rs:21-37)
 *   common_points [ns][32]
 *   challenges    [N][32]   responses [N][m][32]   commitments [N][nc][32]
 *   results       [N]       0 = Ok(()), 1 = Err(VerificationFailure)
 * Canonical-scalar rule: the verify calls take proofs as raw 32-byte fields, i.e. where the reference has
 * `bincode::deserialize` in front of its verifiers (tests/zkp.rs:54, :97).  dalek's Deserialize refuses a Scalar whose
 * value is >= l (proofs.rs:14-32), so such a proof never verifies there; here a response (or compact challenge) >= l is
 * Err(VerificationFailure) for that proof -- for the whole batch in zkp_batch_verify*.  (The wire codec below applies the
 * same rule when it parses.)
 * Witnesses are the other way round: zkp_prove_batch / zkp_pipe_prove_batch / zkp_prove_phase_a / _b accept ANY 32 bytes per secret (a
 * `Scalar::from_bits` value in the reference).  s and s + l prove the same statement with different blindings, hence different proofs,
 * exactly as two such Scalars do in the reference; the host backend, the device and both oracles agree on them byte for byte.
 */

/* Prove N statements.  entropy = [N][32] bytes replacing the thread_rng contribution of prover.rs:82, or
 * NULL to draw them from the OS.  Produces BOTH proof formats' fields: compact = (challenge, responses)
 * (proofs.rs:15-20), batchable = (commitments, responses) (proofs.rs:27-32). */
int zkp_prove_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                    const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* entropy, int n_threads,
                    uint8_t* challenges, uint8_t* responses, uint8_t* commitments);

int zkp_verify_compact_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint8_t* transcripts,
                             const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* challenges,
                             const uint8_t* responses, int n_threads, uint8_t* results);

/* weights16 = [N][nc][16] replacing the u128 draws of verifier.rs:153, or NULL for OS randomness */
int zkp_verify_batchable_each(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint8_t* transcripts,
                              const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                              const uint8_t* responses, const uint8_t* weights16, int n_threads, uint8_t* results);

/* One verdict for the whole batch (batch_verifier.rs:230-234): returns ZKP_TB_OK or
 * ZKP_TB_VERIFICATION_FAILURE.  n_transcripts must equal N (else ZKP_TB_BATCH_SIZE_MISMATCH,
 * batch_verifier.rs:72-74).  weights16 = [nc][N][16] replacing batch_verifier.rs:179, or NULL. */
int zkp_batch_verify(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* transcripts,
                     const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                     const uint8_t* responses, const uint8_t* weights16, int n_threads);

/* K batch verifications in one call: the N = n_batches * N_each proofs lie next to each other in every array (layouts as in
 * zkp_batch_verify with that N), batch b = proofs [b * N_each, (b + 1) * N_each); verdicts [n_batches]: ZKP_TB_OK or
 * ZKP_TB_VERIFICATION_FAILURE per batch, each exactly what zkp_batch_verify returns for that batch alone (its own weights,
 * its own sums of the static coefficients, its own MSM: K x batch_verifier.rs:137-235).  On the device this is one
 * transcript launch, one coefficient grid and one segmented Pippenger for all batches (zkp_fused_batch_verify_many);
 * batches whose transcripts do not stand at one STROBE position, or below the fused threshold, are verified one by one.
 * Returns ZKP_TB_OK when every verdict was computed (look at verdicts[]), ZKP_TB_BATCH_SIZE_MISMATCH if n_transcripts !=
 * N, negative on infrastructure failure. */
int zkp_batch_verify_many(zkp_ctx* ctx, const zkp_statement* st, uint32_t n_batches, uint32_t N_each, uint32_t n_transcripts,
                          uint8_t* transcripts, const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                          const uint8_t* responses, const uint8_t* weights16, int n_threads, int* verdicts);

/* zkp_batch_verify with bad-proof localisation.  The reference's batch verifier can only say that
 * SOME proof of the batch is wrong (batch_verifier.rs:233); finding it means verifying one by one.  This call runs the batch
 * check and, only if it fails, re-verifies every proof on its own (verifier.rs:123-173 semantics, from copies of the incoming
 * transcripts) and writes results[N]: 0 = that proof verifies, 1 = it does not.  Returns ZKP_TB_OK (results all 0) or
 * ZKP_TB_VERIFICATION_FAILURE (results say which).  A batch can also fail as a whole without any single proof failing
 * only with negligible probability (the random linear combination), so results then are all 0 and the code is still
 * ZKP_TB_VERIFICATION_FAILURE.  The transcripts are left as the batch check leaves them. */
int zkp_batch_verify_locate(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* transcripts,
                            const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                            const uint8_t* responses, const uint8_t* weights16, int n_threads, uint8_t* results);

/* zkp_batch_verify, additionally returning the coefficient vector the GPU built (zkp_batch_check's debug_scalars:
 * ns + (ni + nc) * N scalars in the operand order of batch_verifier.rs:219-223), so tests can compare it with the
 * host/oracle restatement of batch_verifier.rs:173-206. */
int zkp_batch_verify_coeffs(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* transcripts,
                            const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                            const uint8_t* responses, const uint8_t* weights16, int n_threads, uint8_t* coeffs);

/* ---- pipelines and device groups (round 4) ---------------------------------------------------------------------------
 * A zkp_pipe owns `contexts_per_device` engine contexts on each of the listed GPUs (HIP ordinals; an ordinal may be listed more than once)
 * and offers the calls above in two forms:
 *
 * (a) ASYNCHRONOUS JOBS -- zkp_*_submit puts one call on the next free context and returns a zkp_job; zkp_job_wait returns what the
 *     synchronous call would have returned and fills the outputs.  With >= 3 jobs in flight the host <-> device copies of one job overlap
 *     the kernels of the others: this is the throughput a caller with host buffers gets (bench.py: e2e_host_buffers.pipelined).
 *       - every buffer named by a submit stays valid and untouched until zkp_job_wait returns (which also frees the job);
 *       - buffers in pinned memory (zkp_host_alloc / zkp_host_register of zkp_mi355x.h) go to the DMA engines as they are; others are
 *         staged through pinned rings the pipe owns (one host memcpy each way);
 *       - flags = ZKP_JOB_SHARED_TRANSCRIPT: `transcripts` is ONE blob every proof starts from (`Transcript::new(label)` per proof, as the
 *         reference's callers write); transcripts_out = NULL or [N][208] for the advanced states;
 *       - inst_stride / weights_stride = proofs per row of the caller's [.][stride][32|16] arrays (>= N): a proof range of a larger batch
 *         is passed by pointer offset, nothing is gathered by the caller;
 *       - entropy == NULL / weights16 == NULL: 40 bytes of getrandom() per job key a ChaCha20 stream that is expanded ON THE DEVICE
 *         (the reference's thread_rng(), prover.rs:82 / verifier.rs:153 / batch_verifier.rs:179); getrandom failing = ZKP_TB_NO_ENTROPY;
 *       - all contexts busy = ZKP_TB_PIPE_FULL (wait for the oldest job); jobs complete independently: a failing job -- a rejected batch,
 *         ZKP_ERR_OOM on one context, a device fault -- leaves the verdicts of the others intact, and its own outputs fail closed
 *         (results / verdicts set to "rejected", negative return code from zkp_job_wait);
 *       - batches below the fused threshold or with ragged transcripts run the synchronous call inside submit (same results).
 *     A pipe and its jobs belong to one host thread at a time.
 *     SUBMITTER THREADS (round 5): a pipe over more than one entry of the device list carries out its submits on one host thread per entry --
 *     zkp_*_submit reserves a context, queues the call for that device's thread and returns; the thread stages the buffers (its pinned rings
 *     live on the GPU's NUMA node: zkp_host_alloc_on), enqueues the job, polls the contexts of ITS device so that a finished job's copies
 *     out start at once, and retires finished jobs (staged outputs copied back, verdicts written); zkp_job_wait picks the result up.  A
 *     single caller thread no longer pays 0.1 - 0.4 ms of host work per job per GPU (profiles/r05_pipe_host_scaling.txt: one submitting
 *     thread is host-bound near three GPUs).  Consequences for the caller: errors the submit itself would have returned (a malformed call,
 *     ZKP_ERR_OOM) arrive from zkp_job_wait; the STATEMENT, like every buffer, must stay alive until zkp_job_wait.  zkp_pipe_set_submit_threads
 *     forces the mode (1 = threads also for one device, 0 = the caller's thread does everything, -1 = default) while no job is in flight.
 *
 * (b) SYNCHRONOUS CALLS OVER ALL CONTEXTS -- zkp_pipe_prove_batch, _verify_compact_batch, _verify_batchable_each, _batch_verify[_many],
 *     _batch_verify_locate: same arguments and results as the single-context calls, the N proofs sharded as contiguous ranges
 *     [g N / G, (g + 1) N / G) over the G = min(contexts, N) contexts, one host thread per GPU, common points replicated.  Proving and
 *     per-proof verification give the bytes / verdicts of the single-context call.  zkp_pipe_batch_verify gives ONE verdict: each range
 *     is a batch check of its own (own weights, own static-coefficient sums: batch_verifier.rs:173-206 per range) and the batch verifies
 *     iff every range does -- the AND is taken on the host, no collective, no other process.  zkp_pipe_batch_verify_many
 *     hands whole batches to the contexts.  This is how one process uses the 8 GPUs of a node.
 */
#define ZKP_TB_PIPE_FULL 3              /* every context of the pipe has a job in flight */
typedef struct zkp_pipe zkp_pipe;
typedef struct zkp_job zkp_job;
int zkp_pipe_create(zkp_pipe** out, const int* device_ids, int n_devices, int contexts_per_device);
void zkp_pipe_destroy(zkp_pipe* pipe);                    /* jobs nobody waited for are DISCARDED: kernels waited for, nothing written to caller memory.  A handle
                                                           * that outlives its pipe: one made by a SUBMITTER THREAD may still go to zkp_job_wait (error code, the
                                                           * handle is freed -- otherwise it leaks); any other handle must not be touched after zkp_pipe_destroy */
int zkp_pipe_num_contexts(const zkp_pipe* pipe);
int zkp_pipe_num_devices(const zkp_pipe* pipe);
zkp_ctx* zkp_pipe_context(zkp_pipe* pipe, int i);        /* context i (tuning options, ZKP_OPT_WS_LIMIT_BYTES); do not destroy it */
int zkp_pipe_context_device(const zkp_pipe* pipe, int i);
/* The partition the synchronous calls of (b) use, as plain arithmetic (no pipe, no GPU): n_items proofs -- or whole batches of `unit` proofs each for
 * zkp_pipe_batch_verify_many -- over at most n_contexts contexts, every range at least fused_min_batch proofs wide; writes the G <= n_contexts non-empty
 * ranges [lo[g], hi[g]) (lo / hi: n_contexts words each) and returns G.  Range g runs on context g. */
uint32_t zkp_pipe_shard_plan(uint32_t n_items, uint32_t unit, uint32_t n_contexts, uint32_t fused_min_batch, uint32_t* lo, uint32_t* hi);
int zkp_pipe_jobs_in_flight(const zkp_pipe* pipe);
int zkp_pipe_set_submit_threads(zkp_pipe* pipe, int on);  /* -1 default (threads when the device list has more than one entry), 0 off, 1 on */
const char* zkp_pipe_last_error(const zkp_pipe* pipe);    /* text of the last failure of a pipe call (never NULL) */

int zkp_prove_batch_submit(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint32_t flags, const uint8_t* transcripts,
                           const uint8_t* secrets, const uint8_t* inst_points, uint32_t inst_stride, const uint8_t* common_points,
                           const uint8_t* entropy, uint8_t* transcripts_out, uint8_t* challenges, uint8_t* responses,
                           uint8_t* commitments, zkp_job** job);
int zkp_verify_compact_batch_submit(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint32_t flags, const uint8_t* transcripts,
                                    const uint8_t* inst_points, uint32_t inst_stride, const uint8_t* common_points,
                                    const uint8_t* challenges, const uint8_t* responses, uint8_t* transcripts_out, uint8_t* results,
                                    zkp_job** job);
int zkp_verify_batchable_each_submit(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint32_t flags, const uint8_t* transcripts,
                                     const uint8_t* inst_points, uint32_t inst_stride, const uint8_t* common_points,
                                     const uint8_t* commitments, const uint8_t* responses, const uint8_t* weights16 /*[N][nc][16]*/,
                                     uint8_t* transcripts_out, uint8_t* results, zkp_job** job);
int zkp_batch_verify_many_submit(zkp_pipe* pipe, const zkp_statement* st, uint32_t n_batches, uint32_t N_each, uint32_t flags,
                                 const uint8_t* transcripts, const uint8_t* inst_points, uint32_t inst_stride,
                                 const uint8_t* common_points, const uint8_t* commitments, const uint8_t* responses,
                                 const uint8_t* weights16 /*[nc][weights_stride][16]*/, uint32_t weights_stride, uint8_t* transcripts_out,
                                 int* verdicts /*[n_batches]: ZKP_TB_OK | ZKP_TB_VERIFICATION_FAILURE after zkp_job_wait*/, zkp_job** job);
int zkp_job_context_index(const zkp_job* job);   /* which context of the pipe carries the job (zkp_pipe_context; profiling: zkp_ctx_job_timing) */
int zkp_job_done(const zkp_job* job);    /* 1 = zkp_job_wait would not block */
int zkp_job_wait(zkp_job* job);          /* the synchronous call's return code; frees the job */

int zkp_pipe_prove_batch(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                         const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* entropy, uint8_t* challenges,
                         uint8_t* responses, uint8_t* commitments);
int zkp_pipe_verify_compact_batch(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* inst_points,
                                  const uint8_t* common_points, const uint8_t* challenges, const uint8_t* responses, uint8_t* results);
int zkp_pipe_verify_batchable_each(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* inst_points,
                                   const uint8_t* common_points, const uint8_t* commitments, const uint8_t* responses,
                                   const uint8_t* weights16, uint8_t* results);
int zkp_pipe_batch_verify(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* transcripts,
                          const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments, const uint8_t* responses,
                          const uint8_t* weights16);
int zkp_pipe_batch_verify_many(zkp_pipe* pipe, const zkp_statement* st, uint32_t n_batches, uint32_t N_each, uint32_t n_transcripts,
                               uint8_t* transcripts, const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                               const uint8_t* responses, const uint8_t* weights16, int* verdicts);
int zkp_pipe_batch_verify_locate(zkp_pipe* pipe, const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* transcripts,
                                 const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                                 const uint8_t* responses, const uint8_t* weights16, uint8_t* results);

/* Batches of at least this many proofs run entirely on the device (zkp_mi355x.h section 2c: transcripts, scalars and MSMs); ragged
 * batches (transcripts at different STROBE positions) through the _ragged calls, except zkp_batch_verify_coeffs.  Smaller batches hash
 * their transcripts on the host threads and use the GPU for the group arithmetic only.  Both routes produce the same bytes.  Default 32 (the measured crossover for the CMZ statement);
 * 0 = always fused, UINT32_MAX = never. */
void zkp_toolbox_set_fused_min_batch(uint32_t n);
/* Host backend (zkp_amd/csrc/host/host_backend.cpp: the kernels' own point formulas and ristretto codec compiled for the host over a
 * 5 x 51-bit field, host/fe51.h).  Every call above accepts
 * ctx == NULL: the whole call then runs on the host cores -- no GPU needed (BASELINE configs[0]: "DLEQ proof single prove + verify on CPU").
 * With a context, calls whose group arithmetic is at most `n` (scalar, point) terms do the same, because a GPU call is a ~1 ms chain of
 * launches whatever its size and a 2-term multiscalar multiplication is ~0.1 ms on one core.  Default 16 (a single DLEQ proof: 2 terms to
 * prove, 4 to verify); 0 = never with a context.  Same bytes either way (canonical encodings); the prover's multiplications stay constant
 * time on the host (masked table look-ups, no skipped digits). */
void zkp_toolbox_set_host_max_terms(uint32_t n);
uint32_t zkp_toolbox_get_host_max_terms(void);
uint32_t zkp_toolbox_get_fused_min_batch(void);

/* Hash to the group (RFC 9496 section 4.3.4; zkp_mi355x.h (5)).
 * zkp_from_uniform_bytes_batch: n x RistrettoPoint::from_uniform_bytes, in [n][64] -> canonical encodings out [n][32].  ctx == NULL or
 *   n <= zkp_toolbox_get_host_max_terms() runs on the host backend (n_threads threads), anything else on the device.
 * zkp_hash_to_group_batch: N x { transcript.challenge_bytes(label, 64) ; from_uniform_bytes } -- the `hash_to_group` of
 *   tests/sig_and_vrf_example.rs:36-40 -- with the transcripts [N][208] advanced in place as merlin advances them.  With a context, batches
 *   of at least fused_min_batch transcripts that stand at one STROBE position squeeze on the device (zkp_fused_hash_to_group); the others
 *   squeeze on the host threads and map as zkp_from_uniform_bytes_batch does; batches of transcripts at different positions squeeze on the
 *   device per position class (zkp_fused_hash_to_group_ragged).  Same bytes on every route.
 * Both: n = 0 is a no-op; a NULL buffer (with n > 0) or a NULL label is ZKP_TB_BAD_STATEMENT; the map never fails. */
int zkp_from_uniform_bytes_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* in /*[n][64]*/, int n_threads, uint8_t* out /*[n][32]*/);
int zkp_hash_to_group_batch(zkp_ctx* ctx, uint32_t N, uint8_t* transcripts /*[N][208]*/, const char* label, int n_threads, uint8_t* out /*[N][32]*/);
/* zkp_hash_from_bytes_sha512_batch: n x RistrettoPoint::hash_from_bytes::<Sha512>(message) (reference tests/zkp.rs:34) over a CSR batch,
 *   message i = msgs[offsets[i], offsets[i + 1]) (any lengths, any byte offsets), -> canonical encodings out [n][32].  Routes as
 *   zkp_from_uniform_bytes_batch: ctx == NULL or n <= zkp_toolbox_get_host_max_terms() on the host backend (n_threads threads), anything
 *   else on the device (zkp_hash_from_bytes_sha512).  Same bytes on every route.  n = 0 is a no-op; a NULL buffer (with n > 0) or
 *   decreasing offsets are ZKP_TB_BAD_STATEMENT. */
int zkp_hash_from_bytes_sha512_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* msgs, const uint64_t* offsets /*[n+1]*/, int n_threads,
                                     uint8_t* out /*[n][32]*/);

/* Scalars mod l, batched (zkp_mi355x.h (6)): every output a canonical scalar, inputs any 32 bytes.  Each call routes as
 * zkp_hash_from_bytes_sha512_batch does: ctx == NULL or n <= zkp_toolbox_get_host_max_terms() on the host threads (the kernels' scalar
 * header and SHA-512 compiled for the host), anything else on the device; same bytes on both routes.  n = 0 is a no-op; a NULL buffer (with
 * n > 0), decreasing offsets or a stride other than 0 and 1 are ZKP_TB_BAD_STATEMENT.
 *   zkp_scalar_invert_batch: out[i] = (in[i] mod l)^-1, 0 -> 0 (Scalar::invert, reference tests/zkp.rs:35); out may equal in.
 *   zkp_scalar_from_wide_batch: n x Scalar::from_bytes_mod_order_wide.
 *   zkp_scalar_muladd_batch: out[i] = a[i a_stride] b[i b_stride] + c[i c_stride] mod l; stride 0 = one scalar for all i; c == NULL: + 0;
 *     out may equal an operand of stride 1.
 *   zkp_scalar_hash_from_bytes_sha512_batch: n x Scalar::hash_from_bytes::<Sha512> over a CSR batch.
 *   zkp_scalar_random_batch: n x Scalar::random (tests/sig_and_vrf_example.rs:49): out[i] = from_bytes_mod_order_wide(zkp_chacha20_block(key, i,
 *     nonce)); key == NULL: 32 bytes of getrandom() (ZKP_TB_NO_ENTROPY if that fails).  On the device the stream is drawn there. */
int zkp_scalar_invert_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* in /*[n][32]*/, int n_threads, uint8_t* out /*[n][32]*/);
int zkp_scalar_from_wide_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* in /*[n][64]*/, int n_threads, uint8_t* out /*[n][32]*/);
int zkp_scalar_muladd_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, const uint8_t* c,
                            uint32_t c_stride, int n_threads, uint8_t* out /*[n][32]*/);
int zkp_scalar_hash_from_bytes_sha512_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* msgs, const uint64_t* offsets /*[n+1]*/, int n_threads,
                                            uint8_t* out /*[n][32]*/);
int zkp_scalar_random_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* key /*[32] or NULL*/, uint64_t nonce, int n_threads, uint8_t* out /*[n][32]*/);

/* Scalar sums, products and dot products over segments of any length (zkp_mi355x.h (12)): out[i] = the fold of the terms [off[i], off[i + 1]) --
 * ZKP_SC_SUM of a[ai(t)] (empty: 0), ZKP_SC_PRODUCT of a[ai(t)] (empty: 1), ZKP_SC_DOT of a[ai(t)] * b[bi(t)] (empty: 0), ai(t) = aidx ? aidx[t] : t
 * and likewise for b; operands any 32 bytes, outputs canonical; b, n_b, bidx NULL / 0 / NULL unless ZKP_SC_DOT.  Argument errors (those of
 * zkp_sc_reduce's host-pointer form) are ZKP_TB_BAD_STATEMENT with nothing written.  Same bytes on both routes:
 *   ctx == NULL, or fewer than zkp_toolbox_get_scalar_reduce_min_terms(op) terms: the host threads.  They share the TERM axis: a segment longer
 *     than a thread's share becomes per-thread partials that are combined at the end.
 *   anything else: zkp_sc_reduce on the device.
 * zkp_toolbox_set_scalar_reduce_min_terms(op, n): 0 = always the device, UINT64_MAX = never.  The default per op follows from
 * profiles/scalar_reduce_bench.txt by this rule: the smallest measured term count from which the synchronous device call is ahead of the host
 * backend at 16 threads, beyond the min-max spread of the rounds, at every measured segment mix; if there is none up to 2^22 terms: never.
 * The sweep of that file: 2^12 .. 2^22 terms in steps of 4, in segments of 2, 32 and 1,024 terms and in one segment (device | host, ms, medians).
 *   ZKP_SC_SUM: NEVER (UINT64_MAX).  The device call is ahead beyond the spread at 23 of the 24 cells (2^12 in one segment 0.071 | 0.375; 2^20 in one
 *     segment 0.682 | 1.379; 2^22 in one segment 2.530 | 4.477), but at 2^22 terms in segments of 2 -- 2^21 outputs to bring back -- the two are level
 *     (10.31 / 10.99 / 11.45 | 10.38 / 10.94 / 11.45), so there is no size from which every mix is ahead.  A caller whose sums are not millions of
 *     pairs gains x 1.2 (2^20 terms in pairs) to x 5 (2^12 terms) by setting a threshold of 4,096.
 *   ZKP_SC_PRODUCT: 4,096, the smallest measured size: ahead at every cell (2^12: 0.086 to 0.098 | 0.439 to 0.457; 2^20: 0.799 to 1.672 | 4.524 to
 *     5.075; 2^22 in segments of 2: 11.16 | 23.29).  Below 4,096 terms nothing is measured.
 *   ZKP_SC_DOT: 65,536.  Ahead at every cell from there on (2^16: 0.163 to 0.252 | 0.625 to 0.669; 2^22: 4.982 to 13.14 | 17.96 to 23.97); at 2^14 x 32
 *     one round of five took 7.758 ms (0.105 / 0.110 / 7.758 | 0.500 / 0.505 / 0.641), which the rule counts as within the spread.
 * zkp_sc_reduce_dev is the call for pipelines whose operands are resident either way. */
int zkp_scalar_reduce_batch(zkp_ctx* ctx, int op, uint32_t n_out, const uint32_t* off /*[n_out+1]*/, const uint8_t* a /*[n_a][32]*/, uint32_t n_a,
                            const uint32_t* aidx /*[T] or NULL*/, const uint8_t* b /*[n_b][32] or NULL*/, uint32_t n_b,
                            const uint32_t* bidx /*[T] or NULL*/, int n_threads, uint8_t* out /*[n_out][32]*/);
void zkp_toolbox_set_scalar_reduce_min_terms(int op, uint64_t n);
size_t zkp_toolbox_get_scalar_reduce_min_terms(int op);   /* (64 bits on every platform the library builds for; SIZE_MAX = never) */

/* Scalar * basepoint, Scalar * point and multiscalar products, batched (zkp_mi355x.h (8), (1)): key generation `&sk * &RISTRETTO_BASEPOINT_TABLE`
 * (tests/sig_and_vrf_example.rs:58), `&H * &x` (:112) and RistrettoPoint::[vartime_]multiscalar_mul, each with the `compress()` that follows.
 * Routing is that of the scalar calls above: ctx == NULL or n <= zkp_toolbox_get_host_max_terms() on the host threads (the kernels' point
 * formulas compiled for the host: a signed radix-16 walk per output), anything else on the device; same bytes on both routes.  For
 * zkp_multiscalar_mul_batch n is the number of terms, off[n_msm].  n = 0 is a no-op; a NULL buffer (with n > 0), n > 2^31 - 1, a stride other
 * than 0 and 1, flags other than ZKP_CT / ZKP_VARTIME, decreasing offsets, off[0] != 0 or a point index out of range are ZKP_TB_BAD_STATEMENT
 * with nothing written.  Scalars are any 32 bytes.
 *   zkp_basepoint_mul_batch: out[i] = encode(scalars[i] * B); always constant time.
 *   zkp_point_mul_batch: out[i] = encode(scalars[i s_stride] * decode(points[i p_stride])); stride 0 = one operand for all i; status[i] = 1 and
 *     out[i] = 32 zero bytes where the point does not decode; out may equal points when p_stride = 1.  ZKP_CT keeps masked look-ups and skips
 *     no digit on either route.
 *   zkp_multiscalar_mul_batch: zkp_msm_many (arguments and results as there) behind the routing above. */
int zkp_basepoint_mul_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* scalars /*[n][32]*/, int n_threads, uint8_t* out /*[n][32]*/);
int zkp_point_mul_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* scalars, uint32_t s_stride, const uint8_t* points, uint32_t p_stride, int flags,
                        int n_threads, uint8_t* out /*[n][32]*/, uint8_t* status /*[n]*/);
int zkp_multiscalar_mul_batch(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* off /*[n_msm+1]*/, const uint8_t* scalars /*[T][32]*/,
                              const uint32_t* pidx /*[T]*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points, int flags, int n_threads,
                              uint8_t* out /*[n_msm][32]*/, uint8_t* status /*[n_msm]*/);

/* Multiscalar sums with segments of ANY length (zkp_mi355x.h (11)): zkp_multiscalar_mul_batch's meaning, checks and bytes -- out[i] =
 * encode(sum over t in [off[i], off[i + 1]) of scalars[t] * decode(points[pidx[t]])), status[i] = 1 and zeros where a referenced point does not
 * decode, an empty range 32 zero bytes and status 0, ZKP_CT or ZKP_VARTIME -- for a vector Pedersen commitment, a weighted tally, an aggregated
 * key.  pidx == NULL: term t uses point t and n_points must be off[n_msm].  Argument errors (as for zkp_multiscalar_mul_batch, and pidx == NULL
 * with n_points != off[n_msm]) are ZKP_TB_BAD_STATEMENT with nothing written.  Routing, same bytes on every route:
 *   1. ctx == NULL or off[n_msm] <= zkp_toolbox_get_host_max_terms(): the host threads.  They share the TERM axis: a segment longer than a
 *      thread's share is cut into per-thread partial sums that are added at the end (zkp_multiscalar_mul_batch gives an MSM to one thread).
 *   2. otherwise, the longest segment shorter than zkp_toolbox_get_msm_fold_min_segment(): zkp_msm_many, whose shared-inversion encoder wins on
 *      short segments (with pidx == NULL the toolbox supplies 0, 1, 2, ...).
 *   3. otherwise zkp_msm_segments.
 * zkp_toolbox_set_msm_fold_min_segment moves the threshold of step 2 (0: always fold; 0xffffffff: never).  The default is 1,024, from
 * profiles/msm_segments_bench.txt (stream time, medians, fold against zkp_msm_many, variable time; constant time reads the same): the rule is the
 * shortest measured length at which the fold is ahead beyond the spread at every measured output count.  Of 2, 11, 32 and 128 terms none is:
 * 4,096 x 2: 1.086 against 0.747; 4,096 x 11: 1.176 against 0.834; 4,096 x 32: 1.920 against 1.562; 4,096 x 128: 6.521 against 6.557; 65,536 x 2: 1.948 against 1.501; 65,536 x 11: 8.745 against 8.279; 65,536 x 32: 23.45 against 23.42; 65,536 x 128: 85.10 against 84.62.  At 1,024 terms it is: 1.290 against 4.194 ms at 64 segments, 12.64 against 15.96 ms at 1,024.  Between 128 and 1,024 terms nothing is measured; the fold's gain comes from
 * FEW long segments (one lane per MSM already fills the chip at 65,536 outputs), so a caller with a handful of segments of a few hundred terms
 * may lower the threshold. */
int zkp_multiscalar_sum_batch(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* off /*[n_msm+1]*/, const uint8_t* scalars /*[T][32]*/,
                              const uint32_t* pidx /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points, int flags,
                              int n_threads, uint8_t* out /*[n_msm][32]*/, uint8_t* status /*[n_msm]*/);
void zkp_toolbox_set_msm_fold_min_segment(uint32_t n);
uint32_t zkp_toolbox_get_msm_fold_min_segment(void);

/* MANY variable-time multiscalar sums, each with its own verdict (zkp_mi355x.h (14)): dalek's RistrettoPoint::optional_multiscalar_mul for a batch
 * of segments.  zkp_multiscalar_sum_batch's meaning, checks and bytes with ZKP_VARTIME; there is no flags argument, THE CALL IS VARIABLE TIME BY
 * DEFINITION (public scalars only).  pidx == NULL: a point per term, n_points must be off[n_seg].  Routing, same bytes on every route:
 *   1. ctx == NULL or off[n_seg] <= zkp_toolbox_get_host_max_terms(): the host threads (the host backend has no bucket method: the CSR MSM behind
 *      zkp_multiscalar_sum_batch, variable time).
 *   2. otherwise, the longest segment shorter than zkp_toolbox_get_msm_bucket_min_segment(): the route zkp_multiscalar_sum_batch gives the job.
 *   3. otherwise zkp_msm_optional_many, the bucket method on the device.
 * zkp_toolbox_set_msm_bucket_min_segment moves the threshold of step 2 (0: always the bucket method; 0xffffffff: never).  Its default follows the
 * toolbox's standing rule: the smallest measured segment length from which the new call is ahead beyond the spread of the rounds at every
 * measured segment count, "never" if there is none.  The default is 256, from
 * profiles/msm_optional_many_bench.txt (stream medians, ms, the call against zkp_msm_segments | zkp_msm_many, ahead beyond the spread in every row): 256
 * terms at 4 segments 0.377 against 0.974 | 1.615, at 16 0.394 against 1.024 | 1.659, at 4,096 9.009 against 12.35 | 12.74; 1,024 terms at 4 segments
 * 0.375 against 1.025 | 3.958, at 1,024 5.301 against 12.39 | 16.62.  256 is the shortest length measured: between 193 and 255 terms nothing is. */
int zkp_multiscalar_optional_batch(zkp_ctx* ctx, uint32_t n_seg, const uint32_t* off /*[n_seg+1]*/, const uint8_t* scalars /*[T][32]*/,
                                   const uint32_t* pidx /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points, int n_threads,
                                   uint8_t* out /*[n_seg][32]*/, uint8_t* status /*[n_seg]*/);
void zkp_toolbox_set_msm_bucket_min_segment(uint32_t n);
uint32_t zkp_toolbox_get_msm_bucket_min_segment(void);

/* RistrettoPoint sums, batched (zkp_mi355x.h (9)): `P + Q`, `P - Q`, `-P` (ZKP_PT_SUB from the identity, 32 zero bytes at stride 0) and
 * `iter().sum()`, each with the `compress()` that follows.  Routing is that of the calls above: ctx == NULL or n <= zkp_toolbox_get_host_max_terms()
 * (for zkp_point_sum_batch n is the number of terms, off[n_sums]) on the host threads, anything else on the device; same bytes on both routes.
 * n = 0 is a no-op.  A NULL buffer with n > 0, a stride other than 0 and 1, an op other than ZKP_PT_ADD / ZKP_PT_SUB, decreasing offsets,
 * off[0] != 0, a point index out of range or pidx == NULL with n_points != off[n_sums] are ZKP_TB_BAD_STATEMENT with nothing written.
 *   zkp_point_add_batch: out[i] = encode(decode(a[i a_stride]) +- decode(b[i b_stride])); status[i] = 1 and out[i] = 32 zero bytes where an operand
 *     does not decode; out may be a or b where that operand has stride 1.
 *   zkp_point_sum_batch: out[i] = encode(sum over t in [off[i], off[i + 1]) of +- decode(points[pidx[t]])); pidx == NULL: term t is point t;
 *     neg == NULL: every term is added, else neg[t] != 0 subtracts term t; an empty range is 32 zero bytes with status 0; status[i] = 1 and zeros
 *     where a point sum i references does not decode.  On the host the sums are spread over the threads by their terms, and a sum longer than a
 *     thread's share is split into per-thread partial sums that are added at the end. */
int zkp_point_add_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, int op, int n_threads,
                        uint8_t* out /*[n][32]*/, uint8_t* status /*[n]*/);
int zkp_point_sum_batch(zkp_ctx* ctx, uint32_t n_sums, const uint32_t* off /*[n_sums+1]*/, const uint32_t* pidx /*[T] or NULL*/,
                        const uint8_t* neg /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points, int n_threads,
                        uint8_t* out /*[n_sums][32]*/, uint8_t* status /*[n_sums]*/);

/* Prefix sums and products of scalars and running sums of points over segments (zkp_mi355x.h (13)): one row per TERM.  For term t of segment s,
 * mode ZKP_SCAN_INCLUSIVE folds the terms [off[s], t], ZKP_SCAN_EXCLUSIVE the terms [off[s], t) -- the identity (0, 1, 32 zero bytes) at a
 * segment's first term.  A scan never crosses a segment boundary; an empty segment owns no rows; n_seg = 0 or off[n_seg] = 0 is a no-op.
 *   zkp_scalar_scan_batch: op ZKP_SC_SUM or ZKP_SC_PRODUCT of a[ai(t)], ai(t) = aidx ? aidx[t] : t; operands any 32 bytes, outputs canonical.  The
 *     exclusive product scan of t references to one row j is the table j^0 .. j^(t-1).  ZKP_SC_DOT is refused: zkp_scalar_muladd_batch, then a sum scan.
 *   zkp_point_scan_batch: pidx, neg, n_points and decoding as in zkp_point_sum_batch; status[t] = 1 and zeros where a point among the terms row t
 *     depends on does not decode: its own row (the next in exclusive mode) and every later row of its segment, nothing else.
 * Argument errors (those of the host-pointer forms of zkp_sc_scan / zkp_scan_points) are ZKP_TB_BAD_STATEMENT with nothing written.  Same bytes on
 * both routes:
 *   ctx == NULL, or fewer than zkp_toolbox_get_scalar_scan_min_terms(op) / zkp_toolbox_get_point_scan_min_terms() terms: the host threads.  They
 *     share the TERM axis, at least 64 terms per stretch: each scans its stretch, the stretch totals are scanned serially, each fixes up its first run.
 *   anything else: zkp_sc_scan / zkp_scan_points on the device.
 * zkp_toolbox_set_*_scan_min_terms: 0 = always the device, UINT64_MAX = never.  The defaults follow from profiles/scan_bench.txt by the rule of
 * zkp_toolbox_get_scalar_reduce_min_terms: the smallest measured term count from which the synchronous device call is ahead of the host backend at
 * 16 threads, beyond the min-max spread of the rounds, at every measured segment mix; if there is none: never.
 * The sweep of that file: scalars at 2^12 .. 2^22 terms, points at 2^6 .. 2^18, in steps of 4, in segments of 2, 32 and 1,024 terms and in one
 * segment (device | host, ms, medians).
 *   ZKP_SC_SUM: NEVER (UINT64_MAX).  Ahead beyond the spread at every cell up to 2^18 terms (2^12: 0.088 to 0.094 | 0.790 to 0.834; 2^18: 0.664 to
 *     0.708 | 1.229 to 1.377), level at 2^20 (4.505 to 4.752 | 4.562 to 5.323) and behind at 2^22 in segments of 2 and of 1,024 (17.25 | 16.12 and
 *     16.26 | 15.44): the call brings 32 bytes back for every 32 it sends.  A caller whose scans stay below a quarter of a million terms gains x 1.8
 *     (2^18) to x 9 (2^12) by setting a threshold of 4,096.
 *   ZKP_SC_PRODUCT: 4,194,304.  Ahead at every cell up to 2^18 (2^12: 0.116 to 0.122 | 0.859 to 0.985; 2^18: 0.725 to 0.797 | 1.882 to 2.910) and at
 *     2^22 (16.86 to 18.29 | 27.48 to 45.17), but at 2^20 the device call took anything from 6 to 34 ms from round to round (medians 16.05 to 20.73 |
 *     9.284 to 13.92), behind or within the spread at all four mixes; the rule therefore starts at 2^22.  THE 2^20 CELL IS UNEXPLAINED: the identical
 *     call (one segment of 2^20 terms, exclusive) took 2.302 / 2.320 / 2.347 ms in the shapes part of the same file, x 4.7 ahead of the host, and SUM
 *     at that size reads 4.5 ms in both parts.  The slow rows are no property of the call; they were not reproduced or traced, and the default, which
 *     only keeps work on the host, is read off the sweep as it stands.  A caller with product scans of 2^12 to 2^20 terms gains x 2.4 to x 8 by setting
 *     a threshold of 4,096.
 *   points: 64, the smallest measured size: ahead at every cell (2^6: 0.365 to 0.369 | 0.400 to 0.405; 2^12: 0.632 to 0.651 | 2.538 to 4.287; 2^18:
 *     1.780 to 1.969 | 118.2 to 220.9).  Below 64 terms nothing is measured.
 * zkp_sc_scan_dev / zkp_scan_points_dev are the calls for pipelines whose operands are resident either way. */
int zkp_scalar_scan_batch(zkp_ctx* ctx, int op, int mode, uint32_t n_seg, const uint32_t* off /*[n_seg+1]*/, const uint8_t* a /*[n_a][32]*/, uint32_t n_a,
                          const uint32_t* aidx /*[T] or NULL*/, int n_threads, uint8_t* out /*[T][32]*/);
int zkp_point_scan_batch(zkp_ctx* ctx, int mode, uint32_t n_seg, const uint32_t* off /*[n_seg+1]*/, const uint32_t* pidx /*[T] or NULL*/,
                         const uint8_t* neg /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points, int n_threads,
                         uint8_t* out /*[T][32]*/, uint8_t* status /*[T]*/);
void zkp_toolbox_set_scalar_scan_min_terms(int op, uint64_t n);
size_t zkp_toolbox_get_scalar_scan_min_terms(int op);     /* (SIZE_MAX = never, and for an op that has no scan) */
void zkp_toolbox_set_point_scan_min_terms(uint64_t n);
size_t zkp_toolbox_get_point_scan_min_terms(void);

/* Bounded discrete logarithms to the basepoint, batched (zkp_mi355x.h (10)): out[i] = the k in [0, 2^bits) with encode(k B) == points[i] and
 * status[i] = ZKP_DLOG_FOUND; ZKP_DLOG_INVALID and 0 where the encoding does not decode; ZKP_DLOG_NOT_FOUND and 0 where no k is in range.  bits is
 * 1 .. 48.  VARIABLE TIME: the duration depends on the logarithms.  n = 0 is a no-op; a NULL buffer with n > 0 or bits out of range is
 * ZKP_TB_BAD_STATEMENT with nothing written.  Routing: ctx == NULL, or a call whose host work n (2^(bits - host baby_bits) + 128) -- giant steps of
 * the host table, a point counting 128 for its decode and halving -- is at most zkp_toolbox_get_dlog_host_max_steps() PER THREAD (n_threads, or the
 * machine's when 0, counted up to 16), runs on the host threads.  The default is 2,048, from profiles/dlog_bench.txt: no device call goes under
 * 0.81 ms (2.5 ms once it has giant steps); one thread takes 0.51 ms for 14 points at 16 bits (work 2,016) and 0.49 ms for one point at 22 bits;
 * sixteen threads take 0.11 ms for 16 points at 16 bits, 0.87 ms for 227 (work 32,688: the break-even, the device takes 0.82) and 0.77 ms for one
 * point at 26 bits (device 2.6).  Larger calls go to the device: 228 points at 16 bits, one point at 27 bits, and with n_threads = 1 already 15
 * points or one point at 23 bits.  The host runs the same algorithm from the same headers (dlog.h, ge25519.h): every point is halved once, and a
 * point's giant-step axis split over the threads when there are fewer points than threads; anything else is zkp_dlog_base on ctx, with the
 * table the context holds (zkp_ctx_prepare_dlog; 2^16 rows by default).  Same results on both routes.  The host's baby-step table
 * (2^baby_bits rows of 32 bytes and as many 16-byte probe entries; default 2^12) is built at the first call that needs it and kept per size
 * for the process behind a mutex; zkp_toolbox_set_dlog_baby_bits picks the size later calls use (4 .. 22, else ZKP_TB_BAD_STATEMENT). */
int zkp_basepoint_dlog_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* points /*[n][32]*/, uint32_t bits, uint64_t* out /*[n]*/, uint8_t* status /*[n]*/,
                             int n_threads);
int zkp_toolbox_set_dlog_baby_bits(uint32_t baby_bits);
uint32_t zkp_toolbox_get_dlog_baby_bits(void);
void zkp_toolbox_set_dlog_host_max_steps(uint32_t steps);
uint32_t zkp_toolbox_get_dlog_host_max_steps(void);
/* The same to a base of the caller's and over signed ranges (zkp_mi355x.h (10): zkp_dlog_point): out[i] = the k with
 * encode(k G) == points[i], G = decode(base); flags = 0: k in [0, 2^bits); flags = ZKP_DLOG_SIGNED: k in [-2^(bits - 1), 2^(bits - 1)) as a
 * two's-complement int64 in the uint64 row.  status as above.  A base that does not decode is ZKP_TB_INVALID_POINT; the identity as base (32 zero
 * bytes), a NULL buffer with n > 0, bits outside 1 .. 48 or an unknown flag is ZKP_TB_BAD_STATEMENT; nothing is written on an error; n = 0 is a
 * no-op.  ROUTING is the rule above word for word -- the host work n (2^(bits - host baby_bits) + 128) per thread against
 * zkp_toolbox_get_dlog_host_max_steps(), zkp_toolbox_set_dlog_baby_bits for the host table's size: the rule counts group operations, and those
 * do not depend on the base.  The 2,048 was measured on B; a first call on a new base additionally pays one table build on either route (the
 * host keeps up to 8 tables per process keyed by base and size, least recently used out).  On the device route the call looks the base up with
 * zkp_dlog_point_find; a base without a slot gets a free slot, else the least recently used one (zkp_dlog_point_last_use), prepared with 2^16
 * rows: a caller who wants another size prepares the slot first (zkp_ctx_prepare_dlog_point).  In signed mode both routes search outward from
 * k = 0 (zkp_dlog_slice_order: the device over its slices, the host over its groups of giant steps).  Same results on both routes. */
int zkp_point_dlog_batch(zkp_ctx* ctx, const uint8_t base[32], uint64_t n, const uint8_t* points /*[n][32]*/, uint32_t bits, int flags,
                         uint64_t* out /*[n]*/, uint8_t* status /*[n]*/, int n_threads);

/* The ChaCha20 block function (RFC 8439 section 2.3; state words 12-13 = counter, 14-15 = nonce) behind the default
 * entropy / weights of the calls above (`entropy == NULL`, `weights16 == NULL`): like the reference's `thread_rng()`, a
 * ChaCha stream keyed from the operating system.  Exposed for the known-answer test. */
void zkp_chacha20_block(const uint8_t key[32], uint64_t counter, uint64_t nonce, uint8_t out[64]);

/* ---- proof wire format (src/proofs.rs:14-32 under `bincode::serialize`, tests/zkp.rs:53-54, :96-97) ---------------
 * The reference derives serde's Serialize / Deserialize and its tests move proofs through bincode 1.x's top-level
 * functions: fixed-width little-endian integers, `u64` sequence lengths, a `Scalar` / `CompressedRistretto` as its 32
 * bytes (serde tuples carry no length):
 *   CompactProof   = challenge[32] | u64 m | m x response[32]                         (40 + 32 m bytes)
 *   BatchableProof = u64 nc | nc x commitment[32] | u64 m | m x response[32]          (16 + 32 (nc + m) bytes)
 * Decoding applies what curve25519-dalek's Deserialize applies: every scalar must be canonical (< l) -- a non-canonical
 * challenge or response is ZKP_TB_BAD_ENCODING -- while a CompressedRistretto is any 32 bytes (validity is decided by
 * decompress() during verification).  A length prefix larger than the bytes that follow is ZKP_TB_BAD_ENCODING.
 * *consumed receives the bytes used; bincode's top-level deserialize ignores trailing bytes, so does this decoder
 * (strict callers compare *consumed with len).  [No golden bytes exist in the reference: its tests only round-trip.]
 * Sizes in elements; the decoders never write more than max_* elements (ZKP_TB_BAD_STATEMENT if the proof holds more). */
#define ZKP_TB_BAD_ENCODING (-13)
size_t zkp_proof_compact_size(uint32_t m);
size_t zkp_proof_batchable_size(uint32_t nc, uint32_t m);
int zkp_proof_compact_encode(const uint8_t challenge[32], const uint8_t* responses /*[m][32]*/, uint32_t m, uint8_t* out,
                             size_t out_len);
int zkp_proof_compact_decode(const uint8_t* in, size_t len, uint8_t challenge[32], uint8_t* responses /*[max_m][32]*/,
                             uint32_t max_m, uint32_t* m, size_t* consumed);
int zkp_proof_batchable_encode(const uint8_t* commitments /*[nc][32]*/, uint32_t nc, const uint8_t* responses /*[m][32]*/,
                               uint32_t m, uint8_t* out, size_t out_len);
int zkp_proof_batchable_decode(const uint8_t* in, size_t len, uint8_t* commitments /*[max_nc][32]*/, uint32_t max_nc,
                               uint32_t* nc, uint8_t* responses /*[max_m][32]*/, uint32_t max_m, uint32_t* m, size_t* consumed);

/* ---- host-only halves, exposed so the host logic can be tested without a GPU ----------------------- */
/* Everything of zkp_batch_verify up to (not including) the MSM: writes the exact operand sequence of
 * batch_verifier.rs:219-228, ns + (ni + nc) * N scalars and encodings.  Returns 0 or the error the
 * reference would have returned before the MSM. */
int zkp_batch_verify_build(const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* transcripts,
                           const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                           const uint8_t* responses, const uint8_t* weights16, int n_threads, uint8_t* msm_scalars,
                           uint8_t* msm_points);
/* Prover phase A (prover.rs:78-97 without the MSM): transcripts absorb the public points, blindings are
 * derived; writes blindings [N][m][32] and the CSR multiscalar job for zkp_msm_many:
 *   off [N*nc + 1], scalars [N*T][32], pidx [N*T] into the point table common_points || inst_points. */
int zkp_prove_phase_a(const zkp_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                      const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* entropy, int n_threads,
                      uint8_t* blindings, uint32_t* off, uint8_t* scalars, uint32_t* pidx);
/* Prover phase B (prover.rs:98-109): absorb the commitments, derive challenges, compute responses. */
int zkp_prove_phase_b(const zkp_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                      const uint8_t* blindings, const uint8_t* commitments, int n_threads, uint8_t* challenges,
                      uint8_t* responses);
/* total number of constraint terms T = sum |rhs| */
uint32_t zkp_statement_num_terms(const zkp_statement* st);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_TOOLBOX_H */
