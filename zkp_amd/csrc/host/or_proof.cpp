// Batched 1-of-k OR-proofs of a zkp_statement (zkp_or_toolbox.h): the device call of zkp_or_mi355x.h from a minimum batch on, else the
// host backend -- ../or_lane.h's items (the text the kernels compile) on the host threads, the host backend's msm_many and the one-lane
// STROBE of ../strobe_lane.h.  Same bytes on both routes.
#include <string.h>

#include <atomic>
#include <cstring>
#include <vector>

#include "../../../include/zkp_or_toolbox.h"
#include "or_host.hpp"

using namespace zkp::host;

// The minimum batch from which a call with a context goes to the device; UINT32_MAX = never.  The toolbox's rule: the smallest measured N
// from which the synchronous device call is ahead of the host backend at 16 threads, beyond the spread of the rounds, at every measured
// shape.  Measured (profiles/or_proof_bench.txt: DLEQ ballots, k = 2 and 4 at N = 4,096 and 65,536, k = 16 at 4,096): the device is ahead
// at every shape from the smallest measured N on -- 2.0 .. 6.2 ms against 61 .. 342 ms at 4,096.  Nothing below 4,096 was measured.
static std::atomic<uint32_t> g_or_min_batch{4096};

namespace {

inline bool on_device(const zkp_ctx* ctx, uint32_t N) {
  const uint32_t min_batch = g_or_min_batch.load();
  return ctx && min_batch != 0xffffffffu && N >= min_batch;
}
inline void wipe(std::vector<uint8_t>& v) {
  if (!v.empty()) explicit_bzero(v.data(), v.size());
}

}  // namespace

// The prover on the host threads; commitments: NULL or [N][k][nc][32], what was appended (or_batch.cpp's batchable form)
namespace zkp {
namespace host {
int or_prove_host(or_host_call& h, uint8_t* ts, const uint8_t* secrets, const uint8_t* real, const uint8_t* inst, const uint8_t* common, const uint8_t* entropy,
                  int n_threads, uint8_t* commitments, uint8_t* challenges, uint8_t* responses, uint8_t* status) {
  const zkp::or_stmt& s = h.s;
  const uint32_t N = s.N;
  h.plan(inst, common, n_threads);
  const size_t drawn = h.z.drawn, blk_rows = (size_t)s.k * s.nterm, blk_coms = (size_t)s.k * s.nc;
  const zkp::strobe_label empty{};
  std::atomic<int> failed{0};
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    const uint32_t n = hi - lo;
    std::vector<uint8_t> nonces(32 * drawn * n), rows(32 * blk_rows * n), coms(32 * blk_coms * n), mstat(blk_coms * n), wit(32 * ((size_t)s.m + 1));
    alignas(8) uint64_t col[25];
    for (uint32_t j = lo; j < hi; ++j) {                               // the binding, the nonces, the rows
      zkp::strobe_lane L{col, 1, 0, 0, 0};
      lane_load(L, ts + TB * (size_t)j);
      zkp::or_bind_seq bind{s, h.table.data(), j};
      zkp::strobe_walk(L, bind);
      lane_store(L, ts + TB * (size_t)j);
      zkp::or_witness_item(s.m, secrets + 32 * (size_t)s.m * j, real[j], wit.data());
      uint8_t* d = nonces.data() + 32 * drawn * (j - lo);
      zkp::strobe_rng_seq<zkp::STROBE_RNG_SCALARS> rng{empty.w, 0, s.m + 1, 32, (uint32_t)drawn, wit.data(), entropy + 32 * (size_t)j, d};
      zkp::strobe_walk(L, rng);                                        // (on the lane as a clone: the blob was stored above)
      for (uint32_t b = 0; b < s.k; ++b) zkp::or_assemble_item(s, b, real[j], d, rows.data() + 32 * (blk_rows * (j - lo) + (size_t)b * s.nterm));
    }
    if (h.msm(lo, hi, rows.data(), ZKP_CT, coms.data(), mstat.data())) failed = 1;
    for (uint32_t j = lo; j < hi; ++j) {                               // the commitments, the challenge, the responses
      alignas(4) uint8_t c[32];
      zkp::strobe_lane L{col, 1, 0, 0, 0};
      lane_load(L, ts + TB * (size_t)j);
      zkp::or_challenge_seq chal{s, coms.data() + 32 * blk_coms * (j - lo), c};
      zkp::strobe_walk(L, chal);
      lane_store(L, ts + TB * (size_t)j);
      uint32_t bad = 0;
      for (size_t i = 0; i < blk_coms; ++i) bad |= mstat[blk_coms * (j - lo) + i];
      bad = bad != 0;
      zkp::or_respond_item(s, real[j], nonces.data() + 32 * drawn * (j - lo), secrets + 32 * (size_t)s.m * j, c, 1u - bad, challenges + 32 * (size_t)s.k * j,
                           responses + 32 * (size_t)s.k * s.m * j);
      status[j] = (uint8_t)bad;
    }
    if (commitments) std::memcpy(commitments + 32 * blk_coms * lo, coms.data(), coms.size());
    explicit_bzero(col, sizeof(col));                                  // the keyed state
    wipe(nonces);
    wipe(rows);
    wipe(wit);
  });
  return failed.load() ? ZKP_TB_BAD_STATEMENT : ZKP_TB_OK;
}
}  // namespace host
}  // namespace zkp

extern "C" {

void zkp_toolbox_set_or_min_batch(uint32_t n) { g_or_min_batch = n; }
uint32_t zkp_toolbox_get_or_min_batch(void) { return g_or_min_batch.load(); }

int zkp_or_prove_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* secrets, const uint8_t* real,
                       const uint8_t* inst, const uint8_t* common, const uint8_t* entropy, int n_threads, uint8_t* challenges, uint8_t* responses,
                       uint8_t* status) {
  or_host_call h;
  int rc = h.prepare(st, k, N, ts, inst, common);
  if (rc || N == 0) return rc;
  const zkp::or_stmt& s = h.s;
  if (!real || !challenges || !status || (s.m && (!secrets || !responses))) return ZKP_TB_BAD_STATEMENT;
  for (uint32_t j = 0; j < N; ++j)
    if (real[j] >= k) return ZKP_TB_BAD_STATEMENT;
  std::vector<uint8_t> seed;                                           // prover.rs:82 `thread_rng()`, drawn as zkp_prove_batch draws it
  if (!entropy) {
    seed.resize(32 * (size_t)N);
    if (!os_random(seed.data(), seed.size())) {
      wipe(seed);
      return ZKP_TB_NO_ENTROPY;
    }
    entropy = seed.data();
  }
  if (on_device(ctx, N)) {
    FusedView fv(*st);
    rc = zkp_or_prove(ctx, &fv.fs, k, N, ts, secrets, real, inst, common, entropy, challenges, responses, status);
    wipe(seed);
    return rc;
  }
  rc = or_prove_host(h, ts, secrets, real, inst, common, entropy, n_threads, nullptr, challenges, responses, status);
  wipe(seed);
  return rc;
}

int zkp_or_verify_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                        const uint8_t* challenges, const uint8_t* responses, int n_threads, uint8_t* results) {
  or_host_call h;
  int rc = h.prepare(st, k, N, ts, inst, common);
  if (rc || N == 0) return rc;
  const zkp::or_stmt& s = h.s;
  if (!challenges || !results || (s.m && !responses)) return ZKP_TB_BAD_STATEMENT;
  if (on_device(ctx, N)) {
    FusedView fv(*st);
    return zkp_or_verify(ctx, &fv.fs, k, N, ts, inst, common, challenges, responses, results);
  }
  h.plan(inst, common, n_threads);
  const size_t blk_rows = (size_t)s.k * s.nterm, blk_coms = (size_t)s.k * s.nc;
  std::atomic<int> failed{0};
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    const uint32_t n = hi - lo;
    std::vector<uint8_t> rows(32 * blk_rows * n), coms(32 * blk_coms * n), mstat(blk_coms * n), flags((size_t)s.k * n), rejected(n);
    alignas(8) uint64_t col[25];
    for (uint32_t j = lo; j < hi; ++j) {
      rejected[j - lo] = zkp::or_bind_rejects(s, h.table.data(), j) ? 1 : 0;
      if (!rejected[j - lo]) {
        zkp::strobe_lane L{col, 1, 0, 0, 0};
        lane_load(L, ts + TB * (size_t)j);
        zkp::or_bind_seq bind{s, h.table.data(), j};
        zkp::strobe_walk(L, bind);
        lane_store(L, ts + TB * (size_t)j);
      }
      for (uint32_t b = 0; b < s.k; ++b)
        flags[(size_t)s.k * (j - lo) + b] = (uint8_t)zkp::or_check_item(s, challenges + 32 * ((size_t)s.k * j + b), responses + 32 * ((size_t)s.k * j + b) * s.m,
                                                                         rows.data() + 32 * (blk_rows * (j - lo) + (size_t)b * s.nterm));
    }
    if (h.msm(lo, hi, rows.data(), ZKP_VARTIME, coms.data(), mstat.data())) failed = 1;
    for (uint32_t j = lo; j < hi; ++j) {
      alignas(4) uint8_t c[32] = {0};
      if (!rejected[j - lo]) {
        zkp::strobe_lane L{col, 1, 0, 0, 0};
        lane_load(L, ts + TB * (size_t)j);
        zkp::or_challenge_seq chal{s, coms.data() + 32 * blk_coms * (j - lo), c};
        zkp::strobe_walk(L, chal);
        lane_store(L, ts + TB * (size_t)j);
      }
      results[j] = zkp::or_verdict_item(s, challenges + 32 * (size_t)s.k * j, c, flags.data() + (size_t)s.k * (j - lo), rejected[j - lo],
                                        mstat.data() + blk_coms * (j - lo));
    }
  });
  return failed.load() ? ZKP_TB_BAD_STATEMENT : ZKP_TB_OK;
}

}  // extern "C"
