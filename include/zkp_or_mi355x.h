/* zkp_or_mi355x.h -- batched 1-of-k OR-proofs of a statement on the MI355X engine (device library; zkp_or_toolbox.h is the toolbox form).
 *
 * A disjunction "I know a witness of ONE of these k instances of statement st" for a batch of N proofs: the Cramer-Damgard-Schoenmakers
 * composition over the reference's Prover / Verifier steps (src/toolbox/prover.rs:76-112, verifier.rs:80-120).  Branch b is st over the
 * instance points inst[b][.] and the shared common points.  Typical uses: a ciphertext that encrypts one of k values, the secret key of
 * one of k public keys (a ring signature), one of k credentials.
 *
 * The protocol.  m secrets, ni instance points, ns common points, nc constraints, 1 <= k <= ZKP_OR_MAX_BRANCHES.  A proof is
 * challenges [k][32] and responses [k][m][32], all canonical.
 *   binding      domain_sep(label); append_message("or-branches", u32le(k)); append_scalar_var per secret; append_point_var for the
 *                instance points of branch 0 .. k - 1 in allocation order, then for the common points.  The verifier uses the
 *                validating form: an encoding of 32 zero bytes rejects that proof.
 *   nonces       build_rng(); rekey_with_witness_bytes("", secret_i) on the bytes as given; rekey_with_witness_bytes("", real as 32
 *                little-endian bytes) -- the branch index is a witness too --; finalize(entropy); m + k (m + 1) x Scalar::random:
 *                blind[0..m), then per branch c'[b], s'[b][0..m).  The draws of the real branch are made and discarded.
 *   commitments  is_b = (b == real);  C[b] = is_b ? 0 : c'[b];  S[b][i] = is_b ? blind[i] : s'[b][i];
 *                com[b][c] = sum_t S[b][sec(c,t)] P_b[pt(c,t)] + (l - C[b]) P_b[lhs(c)], appended with
 *                append_blinding_commitment(name of lhs(c), com[b][c]) for b, c in order.
 *   challenge    c = get_challenge("chal");  c_real = c - sum_b C[b];  challenges[b] = is_b ? c_real : c'[b];
 *                responses[b][i] = is_b ? blind[i] + c_real (secret_i mod l) : s'[b][i].
 *   verification the binding (validating), every com[b][c] recomputed from (responses[b], challenges[b]), appended, c drawn; accepted
 *                iff sum_b challenges[b] == c mod l, every challenge and response is below l, and no point failed validation or decoding.
 *
 * Constant time in the branch.  Nothing that reaches a branch condition, a trip count, an address, a launch dimension or the choice of
 * which call runs depends on real, on a secret, on a drawn scalar or on entropy -- with one exception, the validity bit real[j] < k.  The
 * real branch is assembled with word-wise masked selects (zkp_amd/csrc/or_lane.h: k_or_assemble, k_or_respond), runs the same
 * multiscalar multiplication as the simulated ones with a zero challenge (the term path of zkp_msm_many with ZKP_CT), and the index
 * arrays of that call follow from (statement, k, N) alone.  The verifier's term path runs with ZKP_VARTIME: it sees public data only.
 *
 * Kernels per call, whatever N and real are: prove = k_or_plan, k_or_bind, k_or_witness, k_strobe_witness_rng, k_or_assemble, the term
 * path, k_or_challenge, k_or_respond; verify = k_or_plan, k_or_bind, k_or_check, the term path, k_or_challenge, k_or_verdict.  The
 * binding is ONE launch and the commitments plus the challenge a second, both on strobe_lane.h's part walker, so the transcripts may
 * stand at any mix of STROBE positions.  zkp_ctx_last_kernels names them; their time is filed under ZKP_K_TRANSCRIPT, ZKP_K_SCALARS and
 * the term path's classes.
 *
 * Layouts: transcripts [N][208] in/out; secrets [N][m][32] (any 256-bit values: the RNG is keyed with the bytes as given, the response
 * uses the value mod l); real [N] bytes; inst [k][ni][N][32]; common [ns][32]; entropy [N][32]; challenges [N][k][32];
 * responses [N][k][m][32].
 *   status[j]   1 = some point of proof j, or a common point, did not decode: the proof rows are 32-byte zeros and blob j is unspecified;
 *               0 otherwise.
 *   results[j]  0 = accepted, 1 = rejected.
 *   transcripts for an accepted proof blob j ends where the prover's ended; for a rejected or flagged proof its content is unspecified.
 *               Nothing outside blob j changes; the 5 padding bytes behind its 203 meaningful ones are written as zeros, as every
 *               transcript call of zkp_mi355x.h (7) writes them.
 * Host-pointer forms: synchronous.  k outside 1 .. 64, N > 2^31 - 1, N k (terms + nc) >= 2^32, a position byte of 166 or more, a
 * real[j] >= k or a NULL buffer is ZKP_ERR_ARG with nothing written; N = 0 is a no-op.  The staged secrets, real, entropy, the drawn
 * scalars and the assembled rows are zeroed on the device before the call returns, on error paths too; as with
 * zkp_transcripts_witness_rng, the outputs' staging is not wiped, nor is anything the HIP runtime stages for a copy from pageable memory.
 * _dev forms: every buffer a device pointer, 16-byte aligned where it holds 32-byte rows or transcripts (real, status and results of any
 * alignment); they inspect nothing on the host, copy d_common and d_inst into one table of the context's workspace, enqueue on the
 * context's stream without synchronising, and clear the nonce region (witnesses, drawn scalars, rows) with an enqueued memset.  A row
 * with real[j] >= k gets status 1 and zero rows; a corrupt blob (position byte >= 166) stays as it is and its proof is flagged /
 * rejected.  They upload the statement's description from host memory on every call and so may NOT be recorded into a graph: between
 * zkp_ctx_capture_begin and _end they return ZKP_ERR_ARG.
 *
 * Measured (profiles/or_proof_bench.txt, one MI355X, DLEQ ballots): the synchronous call proves 4,096 disjunctions of k = 2 in 2.0 ms and
 * 65,536 in 8.5 ms, copies included (the _dev form: 1.7 and 6.0 ms of stream time), against 9.6 and 53 ms for the same proofs written
 * out of the single transcript, scalar and MSM calls (examples/or_ballot_batch.py), which also leak the branch.  k = 4: 2.5 and 14.4 ms;
 * k = 16 at 4,096: 6.2 ms.  Verification is 10 - 20 % shorter.  profiles/or_proof_ct_counters.txt: instruction and LDS counters of
 * k_or_witness, k_strobe_witness_rng, k_or_assemble, the term kernel, k_or_challenge and k_or_respond are identical across real all 0 /
 * all k - 1 / j mod k / random and witness all 0 / all l - 1 / random.
 * Where it does not win: the cost grows with k N (terms + constraints) multiplications of 253 bits -- every branch is a full constant-time
 * multiscalar multiplication, the real one included -- so k = 16 costs 2.5 x what k = 4 does; nothing below N = 4,096 was measured; and the
 * commitments are recomputed per proof: zkp_or_batch_mi355x.h has the batchable form, whose batch verification is one multiscalar sum.
 */
#ifndef ZKP_OR_MI355X_H
#define ZKP_OR_MI355X_H

#include "zkp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKP_OR_MAX_BRANCHES 64

int zkp_or_prove(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts /*[N][208] in/out*/,
                 const uint8_t* secrets /*[N][m][32]*/, const uint8_t* real /*[N]*/, const uint8_t* inst /*[k][ni][N][32]*/,
                 const uint8_t* common /*[ns][32]*/, const uint8_t* entropy /*[N][32]*/, uint8_t* challenges /*[N][k][32]*/,
                 uint8_t* responses /*[N][k][m][32]*/, uint8_t* status /*[N]*/);
int zkp_or_verify(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts /*[N][208] in/out*/,
                  const uint8_t* inst /*[k][ni][N][32]*/, const uint8_t* common /*[ns][32]*/, const uint8_t* challenges /*[N][k][32]*/,
                  const uint8_t* responses /*[N][k][m][32]*/, uint8_t* results /*[N]*/);
int zkp_or_prove_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_transcripts, const uint8_t* d_secrets,
                     const uint8_t* d_real, const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_entropy,
                     uint8_t* d_challenges, uint8_t* d_responses, uint8_t* d_status);
int zkp_or_verify_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_transcripts, const uint8_t* d_inst,
                      const uint8_t* d_common, const uint8_t* d_challenges, const uint8_t* d_responses, uint8_t* d_results);

#ifdef __cplusplus
}
#endif
#endif
