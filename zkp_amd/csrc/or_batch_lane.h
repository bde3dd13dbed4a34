// The per-item code of the batchable 1-of-k OR-proofs (zkp_or_batch_mi355x.h, zkp_or_batch_toolbox.h): the proof of or_lane.h with its
// commitments sent along, so that the verifier hashes the GIVEN commitments and a batch of N proofs is checked with ONE multiscalar sum.
// g++ (host/or_batch.cpp, tests/host/or_batch_host_main.cpp) and hipcc compile the same text; the kernels at the end are one lane per item.
// Everything here reads public data only: branches and trip counts may follow it.
//
// Layouts beyond or_lane.h's (proof j, branch b, constraint c):
//   given    [N][k][nc][32]                 the commitments of the proofs, in the order the prover appended them
//   weights  [N][k][nc][16]                 r_jbc, little-endian u128
//   operands [ns + k ni N + N k nc][32]     points: or_lane.h's table (common, then inst[b][v][j]), then the given commitments;
//                                           scalars: the coefficient of each, in the same order
//   partial  [ns][N k][32]                  what (proof, branch) adds to the coefficient of common point p; seg [ns + 1] = p N k
// Rows move as two 16-byte accesses on the device, a weight as one.
#pragma once
#include "or_lane.h"

namespace zkp {

ZKP_HD size_t or_batch_commitment_row(const or_stmt& s, uint32_t j, uint32_t b, uint32_t c) {
  return (size_t)s.ns + (size_t)s.k * s.ni * s.N + ((size_t)j * s.k + b) * s.nc + c;
}
ZKP_HD void or_weight_load(uint32_t w[4], const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint4 x = reinterpret_cast<const uint4*>(p)[0];
  w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
#else
  memcpy(w, p, 16);
#endif
}
ZKP_HD uint32_t or_rows_differ(const uint8_t* a, const uint8_t* b) {
  sc x, y;
  or_row_load(x, a);
  or_row_load(y, b);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= x.v[i] ^ y.v[i];
  return diff != 0;
}

// validate_and_append_blinding_commitment refuses a commitment of 32 zero bytes
ZKP_HD bool or_given_rejects(const or_stmt& s, const uint8_t* given_j) {
  bool bad = false;
  for (uint32_t i = 0; i < s.k * s.nc; ++i) bad |= strobe_is_identity(given_j + 32 * (size_t)i);
  return bad;
}

// What is exact about proof j and needs no point arithmetic: every challenge and response below l, no commitment of 32 zero bytes,
// sum_b challenges[b] == c, and the walk refused nothing (rejected).  1 = rejected
ZKP_HD uint32_t or_given_check_item(const or_stmt& s, const uint8_t* chal_j, const uint8_t* resp_j, const uint8_t* given_j, const uint8_t* c_j,
                                    uint32_t rejected) {
  sc sum, c;
  sc_zero(sum);
  uint32_t bad = rejected;
  for (uint32_t b = 0; b < s.k; ++b) {
    sc cb;
    or_row_load(cb, chal_j + 32 * (size_t)b);
    const uint32_t wide = sc_not_canonical(cb.v);
    bad |= wide;
    if (!wide) sc_add(sum, sum, cb);                                                // (sc_add wants operands below l)
  }
  for (uint32_t i = 0; i < s.k * s.m; ++i) {
    sc r;
    or_row_load(r, resp_j + 32 * (size_t)i);
    bad |= sc_not_canonical(r.v);
  }
  bad |= or_given_rejects(s, given_j) ? 1u : 0u;
  or_row_load(c, c_j);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= sum.v[i] ^ c.v[i];
  return (bad | diff) != 0;
}
// the per-proof verifier's point check: every recomputed commitment [k][nc] encodes to the given bytes and every one of its sums decoded its
// points.  1 = rejected
ZKP_HD uint32_t or_given_match_item(const or_stmt& s, const uint8_t* given_j, const uint8_t* recomputed_j, const uint8_t* msm_status_j) {
  uint32_t bad = 0;
  for (uint32_t i = 0; i < s.k * s.nc; ++i) bad |= msm_status_j[i] | or_rows_differ(given_j + 32 * (size_t)i, recomputed_j + 32 * (size_t)i);
  return bad != 0;
}

// The coefficients (proof j, branch b) contributes to the batch check  sum_jbc r_jbc (sum_t row(t) P_b[pt(t)] - com[j][b][c]) == 0,  row(t)
// being responses[sec(t)] for a right-hand-side term and l - challenges[b] for the left-hand side:
//   commitment (j, b, c)    l - r_jbc                                                  -> scalars[or_batch_commitment_row]
//   point id p              sum_c r_jbc sum_{t in c, pt(t) = p} row(t)                 -> scalars[or_table_row] for an instance point,
//                                                                                         partial[p][j k + b] for a common one
// Challenge and responses are reduced first, so the rows are defined for any 32 bytes.
ZKP_HD void or_batch_coeff_item(const or_stmt& s, uint32_t j, uint32_t b, const uint8_t* weights_jb, const uint8_t* chal_jb, const uint8_t* resp_jb,
                                uint8_t* scalars, uint8_t* partial) {
  const size_t blk = (size_t)j * s.k + b;
  sc negc, x;
  or_row_load(x, chal_jb);
  sc_reduce(x, x);
  sc_neg(negc, x);
  for (uint32_t c = 0; c < s.nc; ++c) {
    sc r;
    sc_zero(r);
    or_weight_load(r.v, weights_jb + 16 * (size_t)c);
    sc_neg(x, r);                                                                   // r < 2^128 < l
    or_row_store(scalars + 32 * or_batch_commitment_row(s, j, b, c), x);
  }
  for (uint32_t p = 0; p < s.ns + s.ni; ++p) {
    sc acc;
    sc_zero(acc);
    for (uint32_t c = 0; c < s.nc; ++c) {
      sc e;
      sc_zero(e);
      bool hit = false;
      for (uint32_t t = s.msm_off[c]; t < s.msm_off[c + 1]; ++t) {
        if (s.term_pt[t] != p) continue;
        const uint32_t sec = s.term_sec[t];
        sc row = negc;
        if (sec != OR_LHS) {
          or_row_load(row, resp_jb + 32 * (size_t)sec);
          sc_reduce(row, row);
        }
        sc_add(e, e, row);
        hit = true;
      }
      if (!hit) continue;
      uint32_t w[4];
      or_weight_load(w, weights_jb + 16 * (size_t)c);
      sc_mul_u128(x, e, w);
      sc_add(acc, acc, x);
    }
    if (p < s.ns) or_row_store(partial + 32 * ((size_t)p * s.N * s.k + blk), acc);
    else or_row_store(scalars + 32 * (size_t)or_table_row(s, p, b, j), acc);
  }
}

// ---- the kernels ----------------------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
// (the transcripts are walked by or_lane.h's k_or_bind and k_or_challenge, the second over the GIVEN commitments: nothing waits for a sum)
// results [N]: one lane per proof.  recomputed / msm_status: the per-proof verifier's (NULL in the batch verifier); any (NULL or one
// zeroed word): set to 1 by every rejected proof
__global__ void __launch_bounds__(OR_BLOCK) k_or_given_check(const or_stmt s, const uint8_t* __restrict__ chal, const uint8_t* __restrict__ resp,
                                                             const uint8_t* __restrict__ given, const uint8_t* __restrict__ c,
                                                             const uint8_t* __restrict__ rejected, const uint8_t* __restrict__ recomputed,
                                                             const uint8_t* __restrict__ msm_status, uint8_t* __restrict__ results,
                                                             uint32_t* __restrict__ any) {
  const uint32_t j = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (j >= s.N) return;
  const size_t coms = (size_t)s.k * s.nc * j;
  uint32_t bad = or_given_check_item(s, chal + 32 * (size_t)s.k * j, resp + 32 * (size_t)s.k * s.m * j, given + 32 * coms, c + 32 * (size_t)j, rejected[j]);
  if (recomputed) bad |= or_given_match_item(s, given + 32 * coms, recomputed + 32 * coms, msm_status + coms);
  results[j] = (uint8_t)bad;
  if (any && bad) atomicOr(any, 1u);
}
// the coefficient rows and the partials: one lane per (proof, branch); lane 0 also writes the ns + 1 segment offsets of the partials
__global__ void __launch_bounds__(OR_BLOCK) k_or_batch_coeff(const or_stmt s, const uint8_t* __restrict__ weights, const uint8_t* __restrict__ chal,
                                                             const uint8_t* __restrict__ resp, uint8_t* __restrict__ scalars,
                                                             uint8_t* __restrict__ partial, uint32_t* __restrict__ seg) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i >= s.N * s.k) return;
  if (i == 0)
    for (uint32_t p = 0; p <= s.ns; ++p) seg[p] = p * s.N * s.k;
  const uint32_t j = i / s.k, b = i - j * s.k;
  or_batch_coeff_item(s, j, b, weights + 16 * (size_t)s.nc * i, chal + 32 * (size_t)i, resp + 32 * (size_t)s.m * i, scalars, partial);
}
// verdict[0] = 0 iff the sum is the identity, every point decoded and no proof was rejected: one lane
__global__ void k_or_batch_verdict(const uint8_t* __restrict__ sum, const uint32_t* __restrict__ msm_status, const uint32_t* __restrict__ any,
                                   uint32_t* __restrict__ verdict) {
  if (blockIdx.x || threadIdx.x) return;
  sc x;
  or_row_load(x, sum);
  uint32_t bad = msm_status[0] | any[0];
#pragma unroll
  for (int i = 0; i < 8; ++i) bad |= x.v[i];
  verdict[0] = bad != 0;
}
#endif  // __HIPCC__

}  // namespace zkp
