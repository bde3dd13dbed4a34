// Batchable 1-of-k OR-proofs of a zkp_statement (zkp_or_batch_toolbox.h): the device calls of zkp_or_batch_mi355x.h from a minimum batch
// on, else the host backend -- ../or_batch_lane.h's items (the text the kernels compile) on the host threads, the host backend's
// variable-time multiscalar sums and the one-lane STROBE of ../strobe_lane.h.  Same bytes and verdicts on both routes.
#include <string.h>

#include <atomic>
#include <cstring>
#include <vector>

#include "../../../include/zkp_or_batch_toolbox.h"
#include "../or_batch_lane.h"
#include "or_host.hpp"

using namespace zkp::host;

// The minimum batch from which zkp_or_batch_verify_batch (and _locate's and _coeffs' batch check) with a context goes to the device;
// UINT32_MAX = never.  The toolbox's rule over profiles/or_batch_verify_bench.txt; the header states the figures.  The prover and the
// per-proof verifier of the batchable form are zkp_or_prove's and zkp_or_verify's launches and follow zkp_toolbox_get_or_min_batch().
static std::atomic<uint32_t> g_or_batch_min_batch{4096};

namespace {

inline bool on_device(const zkp_ctx* ctx, uint32_t N, uint32_t min_batch) { return ctx && min_batch != 0xffffffffu && N >= min_batch; }

// the verifier's two walks of proof j, the second over the given commitments -> c [32]; 1 = the binding refused a point (the blob stays as
// it is, c = 0), as k_or_bind and k_or_challenge leave it.  A commitment of 32 zero bytes is the check item's to refuse.
uint32_t given_walk(const zkp::or_stmt& s, const uint8_t* table, const uint8_t* given_j, uint32_t j, uint8_t* blob, uint8_t* c) {
  std::memset(c, 0, 32);
  if (zkp::or_bind_rejects(s, table, j)) return 1;
  alignas(8) uint64_t col[25];
  zkp::strobe_lane L{col, 1, 0, 0, 0};
  lane_load(L, blob);
  zkp::or_bind_seq bind{s, table, j};
  zkp::strobe_walk(L, bind);
  zkp::or_challenge_seq chal{s, given_j, c};
  zkp::strobe_walk(L, chal);
  lane_store(L, blob);
  return 0;
}

// the batch check on either route; coeffs: NULL or [ns + N k (ni + nc)][32]
int batch_check(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common, const uint8_t* given,
                const uint8_t* challenges, const uint8_t* responses, const uint8_t* weights16, int n_threads, uint8_t* coeffs) {
  or_host_call h;
  int rc = h.prepare(st, k, N, ts, inst, common);
  if (rc || N == 0) return rc;
  const zkp::or_stmt& s = h.s;
  if (!given || !challenges || (s.m && !responses)) return ZKP_TB_BAD_STATEMENT;
  const uint64_t n_ops = (uint64_t)s.ns + (uint64_t)h.z.n_blocks * ((uint64_t)s.ni + s.nc);
  if (n_ops > 0x7fffffffull || (uint64_t)s.ns * h.z.n_blocks > 0x7fffffffull) return ZKP_TB_BAD_STATEMENT;
  std::vector<uint8_t> own_w;                                          // batch_verifier.rs:179 `thread_rng().gen::<u128>()`, as zkp_batch_verify draws them
  if (!weights16) {
    own_w.resize(16 * (size_t)h.z.n_msm);
    if (!os_random(own_w.data(), own_w.size())) return ZKP_TB_NO_ENTROPY;
    weights16 = own_w.data();
  }
  if (on_device(ctx, N, g_or_batch_min_batch.load())) {
    FusedView fv(*st);
    int verdict = 1;
    rc = zkp_or_batch_verify(ctx, &fv.fs, k, N, ts, inst, common, given, challenges, responses, weights16, &verdict, coeffs);
    if (rc) return rc;
    return verdict ? ZKP_TB_VERIFICATION_FAILURE : ZKP_TB_OK;
  }
  const size_t n_blocks = h.z.n_blocks;
  std::vector<uint8_t> points(32 * (size_t)n_ops), own_scalars(coeffs ? 0 : 32 * (size_t)n_ops), partial(32 * (size_t)s.ns * n_blocks);
  uint8_t* scalars = coeffs ? coeffs : own_scalars.data();
  if (s.ns) std::memcpy(points.data(), common, 32 * (size_t)s.ns);
  if (s.ni) std::memcpy(points.data() + 32 * (size_t)s.ns, inst, 32 * n_blocks * s.ni);
  std::memcpy(points.data() + 32 * (size_t)h.z.n_points, given, 32 * (size_t)h.z.n_msm);
  std::atomic<uint32_t> any{0};
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      alignas(4) uint8_t c[32];
      const uint8_t* given_j = given + 32 * (size_t)s.k * s.nc * j;
      const uint8_t* chal_j = challenges + 32 * (size_t)s.k * j;
      const uint8_t* resp_j = responses + 32 * (size_t)s.k * s.m * j;
      const uint32_t refused = given_walk(s, points.data(), given_j, j, ts + TB * (size_t)j, c);
      if (zkp::or_given_check_item(s, chal_j, resp_j, given_j, c, refused)) any = 1;
      for (uint32_t b = 0; b < s.k; ++b)
        zkp::or_batch_coeff_item(s, j, b, weights16 + 16 * (size_t)s.nc * ((size_t)j * s.k + b), chal_j + 32 * (size_t)b, resp_j + 32 * (size_t)b * s.m, scalars,
                                 partial.data());
    }
  });
  if (s.ns) {
    std::vector<uint32_t> seg(s.ns + 1);
    for (uint32_t p = 0; p <= s.ns; ++p) seg[p] = p * (uint32_t)n_blocks;
    if (zkp::hostbk::sc_reduce_n(ZKP_SC_SUM, s.ns, seg.data(), partial.data(), s.ns * (uint32_t)n_blocks, nullptr, nullptr, 0, nullptr, n_threads, scalars))
      return ZKP_TB_BAD_STATEMENT;
  }
  uint8_t sum[32];
  int status = 1;
  if (zkp::hostbk::msm_optional(n_ops, scalars, points.data(), sum, &status)) return ZKP_TB_BAD_STATEMENT;
  uint32_t bad = (uint32_t)status | any.load();
  for (int i = 0; i < 32; ++i) bad |= sum[i];
  return bad ? ZKP_TB_VERIFICATION_FAILURE : ZKP_TB_OK;
}

}  // namespace

extern "C" {

void zkp_toolbox_set_or_batch_min_batch(uint32_t n) { g_or_batch_min_batch = n; }
uint32_t zkp_toolbox_get_or_batch_min_batch(void) { return g_or_batch_min_batch.load(); }

int zkp_or_prove_batchable_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* secrets, const uint8_t* real,
                                 const uint8_t* inst, const uint8_t* common, const uint8_t* entropy, int n_threads, uint8_t* commitments, uint8_t* challenges,
                                 uint8_t* responses, uint8_t* status) {
  or_host_call h;
  int rc = h.prepare(st, k, N, ts, inst, common);
  if (rc || N == 0) return rc;
  const zkp::or_stmt& s = h.s;
  if (!real || !commitments || !challenges || !status || (s.m && (!secrets || !responses))) return ZKP_TB_BAD_STATEMENT;
  for (uint32_t j = 0; j < N; ++j)
    if (real[j] >= k) return ZKP_TB_BAD_STATEMENT;
  std::vector<uint8_t> seed;                                           // prover.rs:82 `thread_rng()`, drawn as zkp_or_prove_batch draws it
  if (!entropy) {
    seed.resize(32 * (size_t)N);
    if (!os_random(seed.data(), seed.size())) {
      explicit_bzero(seed.data(), seed.size());
      return ZKP_TB_NO_ENTROPY;
    }
    entropy = seed.data();
  }
  if (on_device(ctx, N, zkp_toolbox_get_or_min_batch())) {
    FusedView fv(*st);
    rc = zkp_or_prove_batchable(ctx, &fv.fs, k, N, ts, secrets, real, inst, common, entropy, commitments, challenges, responses, status);
  } else {
    rc = or_prove_host(h, ts, secrets, real, inst, common, entropy, n_threads, commitments, challenges, responses, status);
  }
  if (!seed.empty()) explicit_bzero(seed.data(), seed.size());
  return rc;
}

int zkp_or_verify_batchable_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                                  const uint8_t* commitments, const uint8_t* challenges, const uint8_t* responses, int n_threads, uint8_t* results) {
  or_host_call h;
  int rc = h.prepare(st, k, N, ts, inst, common);
  if (rc || N == 0) return rc;
  const zkp::or_stmt& s = h.s;
  if (!commitments || !challenges || !results || (s.m && !responses)) return ZKP_TB_BAD_STATEMENT;
  if (on_device(ctx, N, zkp_toolbox_get_or_min_batch())) {
    FusedView fv(*st);
    return zkp_or_verify_batchable(ctx, &fv.fs, k, N, ts, inst, common, commitments, challenges, responses, results);
  }
  h.plan(inst, common, n_threads);
  const size_t blk_rows = (size_t)s.k * s.nterm, blk_coms = (size_t)s.k * s.nc;
  std::atomic<int> failed{0};
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    const uint32_t n = hi - lo;
    std::vector<uint8_t> rows(32 * blk_rows * n), coms(32 * blk_coms * n), mstat(blk_coms * n), c(32 * (size_t)n), refused(n);
    for (uint32_t j = lo; j < hi; ++j) {
      refused[j - lo] = (uint8_t)given_walk(s, h.table.data(), commitments + 32 * blk_coms * j, j, ts + TB * (size_t)j, c.data() + 32 * (size_t)(j - lo));
      for (uint32_t b = 0; b < s.k; ++b)
        (void)zkp::or_check_item(s, challenges + 32 * ((size_t)s.k * j + b), responses + 32 * ((size_t)s.k * j + b) * s.m,
                                 rows.data() + 32 * (blk_rows * (j - lo) + (size_t)b * s.nterm));
    }
    if (h.msm(lo, hi, rows.data(), ZKP_VARTIME, coms.data(), mstat.data())) failed = 1;
    for (uint32_t j = lo; j < hi; ++j) {
      const uint8_t* given_j = commitments + 32 * blk_coms * j;
      const uint32_t bad = zkp::or_given_check_item(s, challenges + 32 * (size_t)s.k * j, responses + 32 * (size_t)s.k * s.m * j, given_j,
                                                    c.data() + 32 * (size_t)(j - lo), refused[j - lo]) |
                           zkp::or_given_match_item(s, given_j, coms.data() + 32 * blk_coms * (j - lo), mstat.data() + blk_coms * (j - lo));
      results[j] = (uint8_t)bad;
    }
  });
  return failed.load() ? ZKP_TB_BAD_STATEMENT : ZKP_TB_OK;
}

int zkp_or_batch_verify_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                              const uint8_t* commitments, const uint8_t* challenges, const uint8_t* responses, const uint8_t* weights16, int n_threads) {
  return batch_check(ctx, st, k, N, ts, inst, common, commitments, challenges, responses, weights16, n_threads, nullptr);
}

int zkp_or_batch_verify_coeffs(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                               const uint8_t* commitments, const uint8_t* challenges, const uint8_t* responses, const uint8_t* weights16, int n_threads,
                               uint8_t* coeffs) {
  if (N && !coeffs) return ZKP_TB_BAD_STATEMENT;
  return batch_check(ctx, st, k, N, ts, inst, common, commitments, challenges, responses, weights16, n_threads, coeffs);
}

int zkp_or_batch_verify_locate(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                               const uint8_t* commitments, const uint8_t* challenges, const uint8_t* responses, const uint8_t* weights16, int n_threads,
                               uint8_t* results) {
  if (!st || !results || (N && !ts)) return ZKP_TB_BAD_STATEMENT;
  const std::vector<uint8_t> saved(ts, ts + (N ? TB * (size_t)N : 0));   // the per-proof pass starts where the batch check started
  const int rc = batch_check(ctx, st, k, N, ts, inst, common, commitments, challenges, responses, weights16, n_threads, nullptr);
  if (rc == ZKP_TB_OK || rc == ZKP_TB_VERIFICATION_FAILURE) std::memset(results, 0, N);
  if (rc != ZKP_TB_VERIFICATION_FAILURE || N == 0) return rc;
  std::vector<uint8_t> again(saved);
  const int rc2 = zkp_or_verify_batchable_batch(ctx, st, k, N, again.data(), inst, common, commitments, challenges, responses, n_threads, results);
  if (rc2 < 0) return rc2;                                              // infrastructure failure: nothing may be trusted
  return ZKP_TB_VERIFICATION_FAILURE;
}

}  // extern "C"
