// Segmented running sums of points (zkp_mi355x.h (13): zkp_scan_points): the plan and the kernels.
//
// The job is point_sum.h's: terms sorted by segment in CSR form, term t names a decoded point and a sign.  Here EVERY term gets a row: out[t] is the
// sum of the terms of its segment up to t (inclusive) or before t (exclusive; the identity at the segment's first term).  REDUCE-THEN-SCAN over
// dependent launches, with k_sum_fold's lanes: a lane takes PT_SCAN_GROUP consecutive items of its level and walks them once.  An ITEM is a partial
// sum (sum_item), its bad flag and a HEAD flag in the item's `seg` word: the item does not add to what lies to its left (a term that is the first
// of its segment: off[segment] == t).
//   UP-SWEEP    (levels 1 .. L - 1)  lane g hands on ONE item: the sum and the bad flag of its last run and the OR of its head flags.
//               n_{k+1} = ceil(n_k / PT_SCAN_GROUP).
//   TOP         (level L, n_L <= PT_SCAN_GROUP)  one lane walks its items and stores every inclusive prefix.
//   DOWN-SWEEP  (levels L - 1 .. 1)  lane g starts from its carry -- the inclusive prefix of item g - 1 of the level above: what is open at the end
//               of group g - 1, with the OR of the bad flags so far -- drops it at the first head, walks its items once more and stores every prefix
//               with the bad flags so far: inclusive for the level below, by the call's mode at level 1.
//   ENCODE      one lane per term encodes its prefix (the body behind k_sum_encode: one inversion per row): zeros and status 1 where bad.
// The points are decoded once, before level 1 (k_decode_affine).  Launches: decode, 2 L - 1 walks, encode; they follow from n_terms alone.  One
// writer per row, no atomics, no lane waits for another, and every workspace item that is read was written by this call.  The additions are the
// complete ones: P, P, P, .. gives P, 2P, 3P, .. and P, -P the identity with no special case.
//
// Workspace per term: 160 bytes for its prefix (sum_item), and per point 112 bytes for the decoded point (dev_affine); the levels above add
// 2 x 160 / 31 = 10.3 bytes per term (hand-ons and carries).
//
// Resources (the compiler's resource report for gfx950, tools/kernel_resources.py): k_pt_scan 113 to 121 VGPRs over its four instances, 4 wavefronts
// per SIMD, no LDS, no scratch; k_pt_scan_encode 192 VGPRs, 2 wavefronts per SIMD, no LDS, no scratch -- the inversion chain of ristretto_encode under
// __launch_bounds__(256, 2), as in k_sum_encode.  At 2^20 terms the encode is a third of the call (0.92 of 2.71 ms).
#pragma once
#include "point_sum.h"

namespace zkp {

constexpr uint32_t PT_SCAN_GROUP = SUM_GROUP;          // items one lane walks per level
constexpr int PT_SCAN_MAX_LEVELS = 7;                  // 2^31 - 1 terms: 2^26, 2^21, 2^16, 2^11, 2^6, 2 items above them

inline uint32_t pt_scan_next_items(uint32_t n) { return (uint32_t)(((uint64_t)n + PT_SCAN_GROUP - 1) / PT_SCAN_GROUP); }
inline uint32_t pt_scan_levels(uint32_t n_terms) {
  if (n_terms == 0) return 0;
  uint32_t levels = 1;
  for (uint32_t n = n_terms; n > PT_SCAN_GROUP; n = pt_scan_next_items(n)) ++levels;
  return levels;
}
inline uint32_t pt_scan_launches(uint32_t n_terms) { return n_terms ? 2 * pt_scan_levels(n_terms) + 1 : 0; }

#ifdef __HIPCC__
// k_pt_scan: one launch of one level.  Lane g walks items [g PT_SCAN_GROUP, (g + 1) PT_SCAN_GROUP) of n_items.  TERMS (level 1): item j is term j, as
// in k_sum_fold<true> (an index at or beyond n_points flags the row and reads point 0), its head flag off[s] == j for the segment s the walk along off
// has reached.  Otherwise item j is in[j].  DOWN = false: the lane's hand-on goes to agg[g].  DOWN = true: the walk starts from carry[g - 1] (none for
// lane 0) and stores every prefix to out[j], before the item is added where excl != 0.  Every index that reaches memory is below its array's length
// whatever off and pidx hold.
template <bool TERMS, bool DOWN>
__global__ void __launch_bounds__(256, 2)
k_pt_scan(uint32_t n_items, uint32_t excl, const uint32_t* __restrict__ off, uint32_t n_seg, const uint32_t* __restrict__ pidx,
          const uint8_t* __restrict__ neg, uint32_t n_points, const dev_affine* __restrict__ pts, const sum_item* __restrict__ in,
          const sum_item* __restrict__ carry, sum_item* __restrict__ agg, sum_item* __restrict__ out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t b64 = (uint64_t)g * PT_SCAN_GROUP;
  if (b64 >= n_items) return;
  const uint32_t b = (uint32_t)b64, e = b64 + PT_SCAN_GROUP < n_items ? b + PT_SCAN_GROUP : n_items;
  ge_p3 acc;
  ge_identity(acc);
  uint32_t cur = 0, end = 0, bad = 0, heads = 0;
  if (DOWN && g) {
    uint32_t h;
    load_item(acc, h, bad, carry + (g - 1));
  }
  if (TERMS) {
    cur = segment_of_term(off, n_seg, b);
    end = off[cur + 1];
  }
#pragma unroll 1
  for (uint32_t j = b; j < e; ++j) {
    uint32_t head, ibad;
    ge_p3 q;
    ge_niels qn;
    if (TERMS) {
      while (j >= end && cur + 1 < n_seg) { ++cur; end = off[cur + 1]; }
      head = off[cur] == j;
      const uint32_t pi = pidx ? pidx[j] : j;
      const uint32_t oob = (uint32_t)(pi >= n_points);
      const uint32_t valid = load_affine(q, pts + (oob ? 0u : pi));
      ibad = oob | (valid ^ 1u);
      ge_affine_to_niels(qn, q);
      ge_niels_cneg(qn, neg ? (uint32_t)(neg[j] != 0) : 0u);
    } else {
      load_item(q, head, ibad, in + j);
    }
    if (head) {                                                   // a segment begins here: what came before does not reach this item
      ge_identity(acc);
      bad = 0;
      heads = 1;
    }
    if (DOWN && excl) store_item(out + j, acc, head, bad);
    bad |= ibad;
    if (TERMS) ge_madd(acc, acc, qn);
    else ge_add_p3(acc, acc, q);
    if (DOWN && !excl) store_item(out + j, acc, head, bad);
  }
  if (!DOWN) store_item(agg + g, acc, heads, bad);                // the run that is open at the group's end, and whether it began inside
}

// k_pt_scan_encode: out[t] = the encoding of pre[t]; zeros and status 1 where the prefix met a point that does not decode.
__global__ void __launch_bounds__(256, 2)
k_pt_scan_encode(uint32_t n, const sum_item* __restrict__ pre, uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  ge_p3 p;
  uint32_t head, bad, w[8];
  load_item(p, head, bad, pre + t);
  ristretto_encode(w, p);
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = bad ? 0u : w[k];
  store_vec<2>(out + 32 * (size_t)t, w);
  status[t] = (uint8_t)(bad != 0);
}
#endif  // __HIPCC__

}  // namespace zkp
