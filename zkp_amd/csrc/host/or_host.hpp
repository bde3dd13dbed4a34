// What the host routes of the OR-proof calls share (or_proof.cpp, or_batch.cpp): the one-lane STROBE over a blob, and the statement blob,
// sizes, table [common | inst] and CSR arrays of the term path.  Not part of the C ABI.
#pragma once
#include <cstring>
#include <vector>

#include "../or_meta.h"
#include "host_backend.hpp"
#include "toolbox_internal.hpp"

namespace zkp {
namespace host {

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

struct or_host_call {
  zkp::or_meta M;
  zkp::or_sizes z{};
  zkp::or_stmt s{};
  std::vector<uint8_t> table;
  std::vector<uint32_t> off, pidx;
  // ZKP_TB_OK, or ZKP_TB_BAD_STATEMENT before anything is written
  int prepare(const zkp_statement* st, uint32_t k, uint32_t N, const uint8_t* ts, const uint8_t* inst, const uint8_t* common) {
    if (!st) return ZKP_TB_BAD_STATEMENT;
    FusedView fv(*st);
    if (!zkp::or_meta_build(&fv.fs, M) || M.nc == 0 || !zkp::or_sizes_of(M, k, N, z)) return ZKP_TB_BAD_STATEMENT;
    if (N == 0) return ZKP_TB_OK;
    if (!ts || (M.ni && !inst) || (M.ns && !common)) return ZKP_TB_BAD_STATEMENT;
    for (uint32_t j = 0; j < N; ++j)
      if (ts[TB * (size_t)j + 200] >= zkp::STROBE_RATE) return ZKP_TB_BAD_STATEMENT;
    s = M.view(M.blob.data(), k, N);
    return ZKP_TB_OK;
  }
  void plan(const uint8_t* inst, const uint8_t* common, int n_threads) {
    table.resize(32 * (size_t)z.n_points);
    if (M.ns) std::memcpy(table.data(), common, 32 * (size_t)M.ns);
    if (M.ni) std::memcpy(table.data() + 32 * (size_t)M.ns, inst, 32 * (size_t)z.n_blocks * M.ni);
    off.resize((size_t)z.n_msm + 1);
    pidx.resize(z.n_terms);
    parallel_for(s.N, n_threads, [&](uint32_t lo, uint32_t hi) {
      for (uint32_t j = lo; j < hi; ++j)
        for (uint32_t b = 0; b < s.k; ++b) zkp::or_plan_item(s, j, b, off.data(), pidx.data());
    });
  }
  // the MSMs of the proofs [lo, hi): rows = their [hi - lo][k][nterm][32] scalars -> coms [hi - lo][k][nc][32], status [hi - lo][k][nc]
  int msm(uint32_t lo, uint32_t hi, const uint8_t* rows, int flags, uint8_t* coms, uint8_t* status) const {
    const uint32_t m0 = lo * s.k * s.nc, n = (hi - lo) * s.k * s.nc;
    std::vector<uint32_t> o(n + 1);
    for (uint32_t i = 0; i <= n; ++i) o[i] = off[m0 + i] - off[m0];
    return zkp::hostbk::msm_many(n, o.data(), rows, pidx.data() + off[m0], table.data(), z.n_points, flags, coms, status);
  }
};

// or_proof.cpp: the prover on the host threads over a prepared call (arguments checked, entropy given); commitments: NULL or
// [N][k][nc][32], what was appended.  ZKP_TB_OK or ZKP_TB_BAD_STATEMENT
int or_prove_host(or_host_call& h, uint8_t* ts, const uint8_t* secrets, const uint8_t* real, const uint8_t* inst, const uint8_t* common, const uint8_t* entropy,
                  int n_threads, uint8_t* commitments, uint8_t* challenges, uint8_t* responses, uint8_t* status);

}  // namespace host
}  // namespace zkp
