// The witness RNG, get_challenge and the point appends of the reference's TranscriptProtocol over N transcripts (zkp_toolbox.h): the
// lane code of ../strobe_lane.h -- the text the device kernels compile -- on the host threads, or the device call of zkp_mi355x.h (7)
// from a minimum batch on.  Same bytes on both routes.
#include <string.h>

#include <atomic>
#include <cstring>
#include <vector>

#include "../strobe_lane.h"
#include "toolbox_internal.hpp"

using namespace zkp::host;

// The minimum batch from which a call with a context goes to the device; UINT32_MAX = never.  The rule of the toolbox's other thresholds:
// the smallest measured N from which the synchronous device call is ahead of the host backend at 16 threads, beyond the spread of the
// rounds, at every measured shape.  Measured (profiles/transcript_rng_bench.txt, N = 64, 256, 4,096 and 65,536):
//   witness RNG        every shape but the smallest -- (1, 32) -> 1 scalar, which goes to the host at 64 (0.09 against 0.10 ms) and is within
//                      the spread at 256 -- is ahead on the device from N = 64 (0.25 against 0.30 ms); all four shapes from 4,096 (0.16 ..
//                      0.59 against 1.3 .. 7.9 ms)
//   challenge scalars  the host is ahead at 64 and 256 (0.03 .. 0.04 against 0.06 .. 0.07 ms), the device from 4,096 (0.15 against 0.35 ms)
//   point appends      two short appends and no permutation to speak of: the host is ahead up to 4,096 (0.11 .. 0.13 against 0.16 .. 0.17
//                      ms), the device only at 65,536 (0.83 against 1.45 ms)
static std::atomic<uint32_t> g_witness_rng_min_batch{4096};
static std::atomic<uint32_t> g_challenge_scalars_min_batch{4096};
static std::atomic<uint32_t> g_append_points_min_batch{65536};

namespace {

bool positions_ok(const uint8_t* ts, uint32_t n) {
  for (uint32_t j = 0; j < n; ++j)
    if (ts[TB * (size_t)j + 200] >= zkp::STROBE_RATE) return false;
  return true;
}
inline bool on_device(const zkp_ctx* ctx, uint32_t N, uint32_t min_batch) { return ctx && min_batch != 0xffffffffu && N >= min_batch; }

// blob j of ts -> lane over col; false = a corrupt blob (the callers have checked: never here)
inline void lane_load(zkp::strobe_lane& L, const uint8_t* blob) {
  alignas(8) uint64_t in[26];
  std::memcpy(in, blob, TB);
  zkp::strobe_load(L, in);
}
inline void lane_store(const zkp::strobe_lane& L, uint8_t* blob) {
  alignas(8) uint64_t out[26];
  zkp::strobe_store(L, out, zkp::strobe_tail(L));
  std::memcpy(blob, out, TB);
}

}  // namespace

extern "C" {

void zkp_toolbox_set_witness_rng_min_batch(uint32_t n) { g_witness_rng_min_batch = n; }
uint32_t zkp_toolbox_get_witness_rng_min_batch(void) { return g_witness_rng_min_batch.load(); }
void zkp_toolbox_set_challenge_scalars_min_batch(uint32_t n) { g_challenge_scalars_min_batch = n; }
uint32_t zkp_toolbox_get_challenge_scalars_min_batch(void) { return g_challenge_scalars_min_batch.load(); }
void zkp_toolbox_set_append_points_min_batch(uint32_t n) { g_append_points_min_batch = n; }
uint32_t zkp_toolbox_get_append_points_min_batch(void) { return g_append_points_min_batch.load(); }

int zkp_transcripts_witness_rng_batch(zkp_ctx* ctx, const uint8_t* ts, uint32_t N, const char* label, uint32_t m, uint32_t wlen, const uint8_t* witnesses,
                                      const uint8_t* entropy, int mode, uint32_t count, int n_threads, uint8_t* out) {
  zkp::strobe_label lab;
  if (!label || !zkp::strobe_label_pack(lab, label, std::strlen(label))) return ZKP_TB_BAD_STATEMENT;
  if (mode != ZKP_RNG_SCALARS && mode != ZKP_RNG_BYTES) return ZKP_TB_BAD_STATEMENT;
  if (N > 0x7fffffffu || (mode == ZKP_RNG_SCALARS && count > 0x03ffffffu)) return ZKP_TB_BAD_STATEMENT;
  if (N == 0) return ZKP_TB_OK;
  const size_t row = mode == ZKP_RNG_SCALARS ? 32 * (size_t)count : (size_t)count;
  if (!ts || (m && wlen && !witnesses) || (row && !out) || !positions_ok(ts, N)) return ZKP_TB_BAD_STATEMENT;
  std::vector<uint8_t> seed;                                           // prover.rs:82 `thread_rng()`, drawn as zkp_prove_batch draws it
  if (!entropy) {
    seed.resize(32 * (size_t)N);
    if (!os_random(seed.data(), seed.size())) {
      explicit_bzero(seed.data(), seed.size());
      return ZKP_TB_NO_ENTROPY;
    }
    entropy = seed.data();
  }
  int rc = ZKP_TB_OK;
  if (on_device(ctx, N, g_witness_rng_min_batch.load())) {
    rc = zkp_transcripts_witness_rng(ctx, N, ts, label, m, wlen, witnesses, entropy, mode, count, out);
  } else {
    parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
      alignas(8) uint64_t col[25];
      for (uint32_t j = lo; j < hi; ++j) {
        zkp::strobe_lane L{col, 1, 0, 0, 0};
        lane_load(L, ts + TB * (size_t)j);
        const uint8_t* wit = witnesses + (size_t)j * m * wlen;
        if (mode == ZKP_RNG_SCALARS) {
          zkp::strobe_rng_seq<zkp::STROBE_RNG_SCALARS> seq{lab.w, lab.len, m, wlen, count, wit, entropy + 32 * (size_t)j, out + row * j};
          zkp::strobe_walk(L, seq);
        } else {
          zkp::strobe_rng_seq<zkp::STROBE_RNG_BYTES> seq{lab.w, lab.len, m, wlen, count, wit, entropy + 32 * (size_t)j, out + row * j};
          zkp::strobe_walk(L, seq);
        }
      }
      explicit_bzero(col, sizeof(col));                                // the keyed state
    });
  }
  if (!seed.empty()) explicit_bzero(seed.data(), seed.size());
  return rc;
}

int zkp_transcripts_challenge_scalars_batch(zkp_ctx* ctx, uint8_t* ts, uint32_t N, const char* label, int n_threads, uint8_t* out) {
  zkp::strobe_label lab;
  if (!label || !zkp::strobe_label_pack(lab, label, std::strlen(label)) || N > 0x7fffffffu) return ZKP_TB_BAD_STATEMENT;
  if (N == 0) return ZKP_TB_OK;
  if (!ts || !out || !positions_ok(ts, N)) return ZKP_TB_BAD_STATEMENT;
  if (on_device(ctx, N, g_challenge_scalars_min_batch.load())) return zkp_transcripts_challenge_scalars(ctx, N, ts, label, out);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    alignas(8) uint64_t col[25];
    for (uint32_t j = lo; j < hi; ++j) {
      zkp::strobe_lane L{col, 1, 0, 0, 0};
      lane_load(L, ts + TB * (size_t)j);
      zkp::strobe_challenge_scalar_seq seq{lab.w, lab.len, out + 32 * (size_t)j};
      zkp::strobe_walk(L, seq);
      lane_store(L, ts + TB * (size_t)j);
    }
  });
  return ZKP_TB_OK;
}

int zkp_transcripts_append_points_batch(zkp_ctx* ctx, uint8_t* ts, uint32_t N, const char* kind, const char* var_label, const uint8_t* points, int validate,
                                        int n_threads, uint8_t* status) {
  zkp::strobe_label k, v;
  if (!kind || !var_label || !zkp::strobe_label_pack(k, kind, std::strlen(kind)) || !zkp::strobe_label_pack(v, var_label, std::strlen(var_label)))
    return ZKP_TB_BAD_STATEMENT;
  if (N > 0x7fffffffu) return ZKP_TB_BAD_STATEMENT;
  if (N == 0) return ZKP_TB_OK;
  if (!ts || !points || (validate && !status) || !positions_ok(ts, N)) return ZKP_TB_BAD_STATEMENT;
  if (on_device(ctx, N, g_append_points_min_batch.load())) return zkp_transcripts_append_points(ctx, N, ts, kind, var_label, points, validate, status);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    alignas(8) uint64_t col[25];
    for (uint32_t j = lo; j < hi; ++j) {
      const uint8_t* pt = points + 32 * (size_t)j;
      const bool rejected = validate && zkp::strobe_is_identity(pt);
      if (status) status[j] = rejected ? 1 : 0;
      if (rejected) continue;                                          // mod.rs:191, :215: the early return
      zkp::strobe_lane L{col, 1, 0, 0, 0};
      lane_load(L, ts + TB * (size_t)j);
      zkp::strobe_append_point_seq seq{k.w, v.w, k.len, v.len, pt};
      zkp::strobe_walk(L, seq);
      lane_store(L, ts + TB * (size_t)j);
    }
  });
  return ZKP_TB_OK;
}

}  // extern "C"
