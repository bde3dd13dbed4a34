/* zkp_or_batch_toolbox.h -- batchable 1-of-k OR-proofs of a zkp_statement (toolbox form; the protocol is stated in
 * zkp_or_batch_mi355x.h): the proofs of zkp_or_toolbox.h with their commitments sent along, verified one by one or as a batch with one
 * multiscalar sum, and bad-proof localisation.
 *
 * Layouts are zkp_or_toolbox.h's, plus commitments [N][k][nc][32] and weights16 [N][k][nc][16] (little-endian u128; NULL: drawn the way
 * zkp_batch_verify draws them, ZKP_TB_NO_ENTROPY if the operating system gives none).
 *   zkp_or_prove_batchable_batch    zkp_or_prove_batch plus the commitments: challenges, responses, status and transcripts are its bytes.
 *   zkp_or_verify_batchable_batch   the exact per-proof verifier: results [N], 0 = accepted; returns ZKP_TB_OK whatever the verdicts are.
 *   zkp_or_batch_verify_batch       one verdict: ZKP_TB_OK, or ZKP_TB_VERIFICATION_FAILURE when some proof is wrong.
 *   zkp_or_batch_verify_locate      the batch check and, only if it fails, zkp_or_verify_batchable_batch on copies of the incoming
 *                                   transcripts: results [N] says which.  Return codes and transcript rule are zkp_batch_verify_locate's:
 *                                   ZKP_TB_OK (results all 0) or ZKP_TB_VERIFICATION_FAILURE; the transcripts are left as the batch check
 *                                   leaves them.
 *   zkp_or_batch_verify_coeffs      the batch check, also returning the coefficient vector [ns + N k (ni + nc)][32] (unspecified when a
 *                                   proof was rejected before the sum).
 *
 * Routing: ctx == NULL, or a batch below the threshold, runs the host backend over n_threads threads (<= 0: one per core): the same lane
 * text (zkp_amd/csrc/or_batch_lane.h), the host backend's variable-time multiscalar sums and the host lane code of the transcripts.  Both
 * routes give the same bytes and verdicts.  The prover and the per-proof verifier are zkp_or_prove's and zkp_or_verify's launches and
 * follow zkp_toolbox_get_or_min_batch(); the batch check follows zkp_toolbox_get_or_batch_min_batch().
 *
 * The threshold.  The toolbox's rule: the smallest measured N from which the synchronous device call is ahead of the host backend at
 * 16 threads beyond the spread of the rounds, at every measured shape, or UINT32_MAX if there is none.  The figures are in
 * profiles/or_batch_verify_bench.txt (DLEQ ballots; k = 2 and 4 at N = 4,096 and 65,536, k = 16 at 4,096; five rounds, routes alternated).
 * The device is ahead at every measured shape: the synchronous batch check takes 1.30 / 1.70 / 3.39 ms (medians) at N = 4,096 for
 * k = 2 / 4 / 16 and 4.67 / 5.91 ms at N = 65,536 for k = 2 / 4, against 0.36 to 16 s on the host backend, whose one multiscalar sum runs
 * on one thread.  The smallest measured N is 4,096, so the default of zkp_toolbox_get_or_batch_min_batch is 4096 (0 = always on the
 * device, UINT32_MAX = never).  Against zkp_or_verify_batch on the device the batch check is ahead at four of the five shapes (1.30
 * against 1.93 ms at k = 2, 5.91 against 11.83 ms at k = 4, N = 65,536).  Where it does not win: at k = 2, N = 65,536 it is within the
 * spread of the rounds (4.64 / 4.67 / 24.13 against 7.05 / 7.11 / 7.15 ms); zkp_or_prove_batchable_batch is behind zkp_or_prove_batch
 * at four of five shapes (19.52 against 15.98 ms at k = 4, N = 65,536: 32 N k nc more bytes come back from the device); nothing below
 * 4,096 was measured, so smaller batches stay on the host backend; and a failed batch costs the per-proof pass on top.
 *
 * Returns as zkp_or_toolbox.h's calls: ZKP_TB_BAD_STATEMENT for a NULL argument, k outside 1 .. ZKP_OR_MAX_BRANCHES, sizes out of range
 * (also more than 2^31 - 1 operands in the batch check) or a position byte of 166 or more, with nothing written; ZKP_TB_NO_ENTROPY; or
 * the device library's negative code.  N = 0 is a no-op (the batch check returns ZKP_TB_OK).
 */
#ifndef ZKP_OR_BATCH_TOOLBOX_H
#define ZKP_OR_BATCH_TOOLBOX_H

#include "zkp_or_batch_mi355x.h"
#include "zkp_or_toolbox.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_or_prove_batchable_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                                 const uint8_t* real, const uint8_t* inst_points, const uint8_t* common_points,
                                 const uint8_t* entropy /*or NULL*/, int n_threads, uint8_t* commitments, uint8_t* challenges,
                                 uint8_t* responses, uint8_t* status);
int zkp_or_verify_batchable_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts,
                                  const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* commitments,
                                  const uint8_t* challenges, const uint8_t* responses, int n_threads, uint8_t* results);
int zkp_or_batch_verify_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts, const uint8_t* inst_points,
                              const uint8_t* common_points, const uint8_t* commitments, const uint8_t* challenges, const uint8_t* responses,
                              const uint8_t* weights16 /*or NULL*/, int n_threads);
int zkp_or_batch_verify_locate(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts, const uint8_t* inst_points,
                               const uint8_t* common_points, const uint8_t* commitments, const uint8_t* challenges, const uint8_t* responses,
                               const uint8_t* weights16 /*or NULL*/, int n_threads, uint8_t* results);
int zkp_or_batch_verify_coeffs(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts, const uint8_t* inst_points,
                               const uint8_t* common_points, const uint8_t* commitments, const uint8_t* challenges, const uint8_t* responses,
                               const uint8_t* weights16 /*or NULL*/, int n_threads, uint8_t* coeffs);
void zkp_toolbox_set_or_batch_min_batch(uint32_t n);
uint32_t zkp_toolbox_get_or_batch_min_batch(void);

#ifdef __cplusplus
}
#endif
#endif
