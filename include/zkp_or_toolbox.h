/* zkp_or_toolbox.h -- batched 1-of-k OR-proofs of a zkp_statement (toolbox form; the protocol is stated in zkp_or_mi355x.h).
 *
 * zkp_or_prove_batch / zkp_or_verify_batch prove and verify N disjunctions of k instances of `st`: branch b is the statement over
 * inst_points[b][.] and the shared common points, real[j] names the branch proof j's witness satisfies.  Layouts: transcripts
 * [N][ZKP_TRANSCRIPT_BYTES] in/out (any mix of STROBE positions); secrets [N][m][32]; real [N]; inst_points [k][ni][N][32];
 * common_points [ns][32]; entropy [N][32] or NULL (drawn the way zkp_prove_batch draws it, and wiped); challenges [N][k][32];
 * responses [N][k][m][32]; status [N] (1 = a point of that proof did not decode: zero rows); results [N] (0 = accepted, 1 = rejected).
 * The binding allocates every secret, then the instance points of each branch in the statement's allocation order, then the common
 * points, whatever order the statement's own allocations were made in.
 *
 * Routing: ctx == NULL, or a batch of fewer than zkp_toolbox_get_or_min_batch() proofs, runs the host backend over n_threads threads
 * (<= 0: one per core): the same masked selects (zkp_amd/csrc/or_lane.h, one text for both), the host backend's constant-time
 * multiscalar multiplication (ZKP_CT; the verifier's is ZKP_VARTIME) and the host lane code of the transcripts.  Otherwise the call is
 * zkp_or_prove / zkp_or_verify of zkp_or_mi355x.h.  Both routes give the same bytes.  On neither route does a branch, an address or the
 * sequence of calls depend on real, a secret, a drawn scalar or entropy.
 *
 * The threshold.  The toolbox's rule: the smallest measured N from which the synchronous device call is ahead of the host backend at
 * 16 threads beyond the spread, at every measured shape, or UINT32_MAX if there is none.  profiles/or_proof_bench.txt (DLEQ ballots; k = 2
 * and 4 at N = 4,096 and 65,536, k = 16 at 4,096; five rounds, routes alternated) has the device ahead at every measured shape: prove
 * 2.0 / 2.5 / 6.2 ms against 61 / 103 / 342 ms at N = 4,096 for k = 2 / 4 / 16, 8.5 against 739 ms at N = 65,536 for k = 2.  The smallest
 * measured N is 4,096, so the default of zkp_toolbox_get_or_min_batch is 4096 (0 = always on the device, UINT32_MAX = never).  Where it
 * does not win: nothing below 4,096 was measured, so smaller batches stay on the host backend -- a lone wavefront needs ~10 us per Keccak
 * permutation where a host thread needs ~0.4 -- and a caller who wants them on the device lowers the threshold.
 *
 * Returns ZKP_TB_OK; ZKP_TB_BAD_STATEMENT for a NULL argument, k outside 1 .. ZKP_OR_MAX_BRANCHES, N k (terms + constraints) >= 2^32,
 * a position byte of 166 or more or a real[j] >= k, with nothing written; ZKP_TB_NO_ENTROPY; or the device library's negative code.
 * zkp_or_verify_batch returns ZKP_TB_OK whatever the verdicts are: results says which proofs are rejected.  N = 0 is a no-op.
 * The host backend zeroes its copies of the nonces, rows and keyed transcript states before it returns.
 * zkp_or_batch_toolbox.h has the batchable form of these proofs, which a verifier checks as a batch with one multiscalar sum.
 */
#ifndef ZKP_OR_TOOLBOX_H
#define ZKP_OR_TOOLBOX_H

#include "zkp_or_mi355x.h"
#include "zkp_toolbox.h"

#ifdef __cplusplus
extern "C" {
#endif

int zkp_or_prove_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                       const uint8_t* real, const uint8_t* inst_points, const uint8_t* common_points, const uint8_t* entropy /*or NULL*/,
                       int n_threads, uint8_t* challenges, uint8_t* responses, uint8_t* status);
int zkp_or_verify_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* transcripts, const uint8_t* inst_points,
                        const uint8_t* common_points, const uint8_t* challenges, const uint8_t* responses, int n_threads, uint8_t* results);
void zkp_toolbox_set_or_min_batch(uint32_t n);
uint32_t zkp_toolbox_get_or_min_batch(void);

#ifdef __cplusplus
}
#endif
#endif
