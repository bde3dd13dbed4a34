/* zkp_or_batch_mi355x.h -- batchable 1-of-k OR-proofs on the MI355X engine: the proofs of zkp_or_mi355x.h with their commitments sent
 * along, a per-proof verifier of that form, and a batch verifier that checks N proofs with ONE multiscalar sum (device library;
 * zkp_or_batch_toolbox.h is the toolbox form, with bad-proof localisation).
 *
 * The protocol.  Binding, nonces, commitments, challenge and responses are exactly those stated in zkp_or_mi355x.h: nothing about the
 * prover's transcript changes.  A batchable proof of one disjunction is commitments [k][nc][32] -- the com[b][c] the prover appended,
 * in append order --, challenges [k][32] and responses [k][m][32].
 *   per-proof verification (zkp_or_verify_batchable; exact, no randomness)
 *     1  the validating binding, as zkp_or_verify runs it;
 *     2  reject if a challenge or a response is not below l;
 *     3  reject if a given commitment is 32 zero bytes (validate_and_append_blinding_commitment, src/toolbox/mod.rs:210-218; the
 *        transcript of a rejected proof is unspecified, so the walk of step 4 need not stop there);
 *     4  append the GIVEN commitments with append_blinding_commitment frames, for b and c in order;
 *     5  c = get_challenge("chal");
 *     6  accepted iff sum_b challenges[b] == c mod l, every recomputed com[b][c] = sum_t responses[b][sec] P_b[pt] + (l - challenges[b])
 *        P_b[lhs] encodes to the given 32 bytes, and no point failed to decode.  The recomputation is the term path with ZKP_VARTIME.
 *        Comparing bytes with the canonical encoding is the reference's "decode the commitment, compare points": an encoding that does
 *        not decode equals no canonical encoding.
 *     An accepted proof's transcript ends where the prover's ended.
 *   batch verification (zkp_or_batch_verify): one verdict for N proofs under the weights r_jbc = weights16 [N][k][nc][16], little-endian
 *     u128, which the caller draws at random and keeps from the provers (Scalar::from(thread_rng().gen::<u128>()), batch_verifier.rs:179).
 *     1  steps 1 - 5 for every proof with the exact check sum_b challenges[b] == c; a proof that fails makes the verdict 1, as any `?` of
 *        batch_verifier.rs fails the batch;
 *     2  the coefficient vector over the operands [common points by point id (ns) | inst[b][v][j] in table order (k ni N) | commitments
 *        [N][k][nc]], all mod l:  commitment (j, b, c): l - r_jbc;  instance point (b, v, j): sum_c r_jbc (sum_{t in c, pt(t) = ns + v}
 *        responses[j][b][sec(t)] - [lhs(c) = ns + v] challenges[j][b]);  common point p: the same expression with pt = p, summed over
 *        all j, b, c;
 *     3  one optional_multiscalar_mul over these ns + N k (ni + nc) operands: verdict 0 iff it is the identity, every point decoded and
 *        step 1 rejected nothing.
 *     If step 1 rejects a proof the coefficient rows (debug_scalars) are unspecified.  A wrong proof passes with probability 2^-128.
 *
 * Kernels per call: prove_batchable = zkp_or_prove's, then one copy of the commitments it hashed (in the host-pointer form the
 * download itself; the same launches, the same wipe of the nonce region: challenges, responses, status and transcripts are
 * byte-identical to zkp_or_prove's); verify_batchable = k_or_plan,
 * k_or_bind, k_or_challenge over the GIVEN commitments (nothing waits for a sum), k_or_check, the term path, k_or_given_check;
 * batch_verify = k_or_bind, k_or_challenge, k_or_given_check, k_or_batch_coeff (one lane per (proof, branch): ni + nc rows into
 * the operand vector, ns partial rows), the fold of zkp_sc_reduce (ZKP_SC_SUM) over the ns segments of partials, zkp_msm_optional's
 * kernels, k_or_batch_verdict.  zkp_ctx_last_kernels names them.  The batch verifier makes no size-dependent choice of its own: below
 * 193 operands the sum is the term path, above it the bucket method, as in zkp_msm_optional.
 *
 * Layouts are zkp_or_mi355x.h's, plus commitments [N][k][nc][32] and weights16 [N][k][nc][16].  The commitments of a proof whose status
 * is 1 are unspecified.  Error rules are those of zkp_or_prove / zkp_or_verify; in addition ns + N k (ni + nc) >= 2^32 is ZKP_ERR_ARG
 * (so is anything above 2^31 - 1 operands: what one zkp_msm_optional takes); calls between zkp_ctx_capture_begin and _end return
 * ZKP_ERR_ARG; N = 0 is a no-op with verdict 0 (the _dev form enqueues that one word).  debug_scalars: NULL or [ns + N k (ni + nc)][32],
 * the coefficient vector.  _dev forms: every buffer a device pointer, 16-byte aligned where it holds rows, weights or transcripts;
 * zkp_or_batch_verify_dev writes d_verdict [1] on the context's stream and reads nothing on the host.
 *
 * Measured (profiles/or_batch_verify_bench.txt, one MI355X, DLEQ ballots, five rounds, routes alternated, min / median / max of the
 * synchronous calls): zkp_or_batch_verify against zkp_or_verify on the same proofs -- k = 2: 1.27 / 1.30 / 1.33 against 1.87 / 1.93 /
 * 2.02 ms at N = 4,096 and 4.64 / 4.67 / 24.13 against 7.05 / 7.11 / 7.15 ms at 65,536; k = 4: 1.67 / 1.70 / 1.77 against 2.19 / 2.25 /
 * 2.30 ms and 5.85 / 5.91 / 6.39 against 11.64 / 11.83 / 11.92 ms; k = 16 at 4,096: 3.39 / 3.39 / 3.40 against 4.78 / 4.85 / 4.91 ms.
 * Stream time of the _dev forms: 0.84 against 1.66 ms (k = 2, 4,096), 1.91 against 5.15 ms (k = 2, 65,536), 3.10 against 9.28 ms (k = 4,
 * 65,536).  zkp_or_prove and zkp_or_verify are level with the parent commit's library.
 * Where it does not win: at k = 2, N = 65,536 the synchronous call is within the spread of the rounds, not ahead (one round of 24 ms);
 * the gain per call is 1.3 to 2.0 x, not the ratio of the per-term figures: the transcript walk, the copies of the inputs and the
 * statement's upload stay; zkp_or_prove_batchable is behind zkp_or_prove at four of five shapes (2.01 against 1.95 ms at k = 2,
 * N = 4,096; 19.52 against 15.98 ms at k = 4, N = 65,536: the commitments' 32 N k nc bytes come back from the device); the verdict says only that some
 * proof is wrong; nothing below N = 4,096 was measured.
 */
#ifndef ZKP_OR_BATCH_MI355X_H
#define ZKP_OR_BATCH_MI355X_H

#include "zkp_or_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_or_prove_batchable(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts /*[N][208] in/out*/,
                           const uint8_t* secrets /*[N][m][32]*/, const uint8_t* real /*[N]*/, const uint8_t* inst /*[k][ni][N][32]*/,
                           const uint8_t* common /*[ns][32]*/, const uint8_t* entropy /*[N][32]*/, uint8_t* commitments /*[N][k][nc][32]*/,
                           uint8_t* challenges /*[N][k][32]*/, uint8_t* responses /*[N][k][m][32]*/, uint8_t* status /*[N]*/);
int zkp_or_verify_batchable(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts /*[N][208] in/out*/,
                            const uint8_t* inst /*[k][ni][N][32]*/, const uint8_t* common /*[ns][32]*/,
                            const uint8_t* commitments /*[N][k][nc][32]*/, const uint8_t* challenges /*[N][k][32]*/,
                            const uint8_t* responses /*[N][k][m][32]*/, uint8_t* results /*[N]*/);
int zkp_or_batch_verify(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts /*[N][208] in/out*/,
                        const uint8_t* inst /*[k][ni][N][32]*/, const uint8_t* common /*[ns][32]*/,
                        const uint8_t* commitments /*[N][k][nc][32]*/, const uint8_t* challenges /*[N][k][32]*/,
                        const uint8_t* responses /*[N][k][m][32]*/, const uint8_t* weights16 /*[N][k][nc][16]*/, int* verdict,
                        uint8_t* debug_scalars /*NULL or [ns + N k (ni + nc)][32]*/);
int zkp_or_prove_batchable_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_transcripts,
                               const uint8_t* d_secrets, const uint8_t* d_real, const uint8_t* d_inst, const uint8_t* d_common,
                               const uint8_t* d_entropy, uint8_t* d_commitments, uint8_t* d_challenges, uint8_t* d_responses,
                               uint8_t* d_status);
int zkp_or_verify_batchable_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_transcripts,
                                const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_commitments, const uint8_t* d_challenges,
                                const uint8_t* d_responses, uint8_t* d_results);
int zkp_or_batch_verify_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_transcripts,
                            const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_commitments, const uint8_t* d_challenges,
                            const uint8_t* d_responses, const uint8_t* d_weights16, uint32_t* d_verdict /*[1]*/);

#ifdef __cplusplus
}
#endif
#endif
