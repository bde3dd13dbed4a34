// Sums of points without scalars (zkp_mi355x.h (9): zkp_add_points, zkp_sum_points): the pair body and the segmented fold.
//
// A segmented sum is a job in CSR form: sum i adds the terms [off[i], off[i + 1]), term t names a decoded point and a sign.  The fold runs in
// LEVELS over a sorted axis of items.  Level 1's items are the terms; a lane takes SUM_GROUP consecutive items and walks them once, starting a new
// accumulator wherever the segment changes.  The stretch of one segment inside a group is a RUN.  A run that is neither the group's first nor
// its last began and ended inside the group, so its segment is complete: the lane writes it to the segment's slot and nobody else ever does.
// The first and the last run may go on in the neighbouring groups, so the lane hands them on as the two items (2g, 2g + 1) of the next level
// (a group that is one run hands on the run and the identity under the same segment number: the formulas are complete, the identity adds
// nothing and every slot of the next level holds an item).  Items stay sorted by segment, items_{k+1} = 2 ceil(items_k / SUM_GROUP), and the level
// with at most SUM_GROUP items is one lane that finishes every run it meets.  The launch shapes follow from the number of terms alone; no lane waits
// for another, nothing is accumulated with atomics, and a slot has exactly one writer.
#pragma once
#include "dev_layout.h"

namespace zkp {

// Items one lane folds per level.  One addition is 8 field products next to ~250 squarings and ~25 products for a decode or an encode, so a serial
// fold of 32 costs about what the decode of one of its terms costs, and every level is 1/16 of the one before it.
constexpr uint32_t SUM_GROUP = 32;
// Lanes per workgroup of a fold launch.  A lane is a serial chain of SUM_GROUP additions that shares nothing with its neighbours, and a call of T
// terms has only T / SUM_GROUP of them: one wavefront per workgroup spreads a narrow call over four times as many compute units as 256 lanes would.
constexpr int SUM_FOLD_BLOCK = 64;

struct alignas(16) sum_item {     // a partial sum on its way up, or a finished one in its segment's slot     160 B
  uint32_t X[9], Y[9], Z[9], T[9];
  uint32_t seg, bad, pad[2];
};
static_assert(sizeof(sum_item) == 160, "layout");

__device__ __forceinline__ void load_item(ge_p3& p, uint32_t& seg, uint32_t& bad, const sum_item* src) {
  uint32_t w[40];
  load_vec<10>(w, src);
  fe_set(p.X, w); fe_set(p.Y, w + 9); fe_set(p.Z, w + 18); fe_set(p.T, w + 27);
  seg = w[36];
  bad = w[37];
}
__device__ __forceinline__ void store_item(sum_item* dst, const ge_p3& p, uint32_t seg, uint32_t bad) {
  uint32_t w[40];
  fe_get(w, p.X); fe_get(w + 9, p.Y); fe_get(w + 18, p.Z); fe_get(w + 27, p.T);
  w[36] = seg; w[37] = bad; w[38] = 0; w[39] = 0;
  store_vec<10>(dst, w);
}

// The largest s in [0, n_sums) with off[s] <= t, or 0: the segment of term t when off is what the call requires (off[0] = 0, non-decreasing,
// t < off[n_sums]; the empty segments that share an offset are passed over).  Whatever off holds, the result is below n_sums.
__device__ __forceinline__ uint32_t segment_of_term(const uint32_t* __restrict__ off, uint32_t n_sums, uint32_t t) {
  uint32_t lo = 0, hi = n_sums;            // off[lo] <= t (or lo = 0), off[hi] > t (or hi = n_sums)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// r = decode(a) + decode(b) or decode(a) - decode(b) (sub in {0, 1}); returns 1 when both decode.  A rolled loop over the operands, b first: one copy
// of the decoder in the code and one decode's registers live at a time (ristretto_from_uniform_words does the same with its two maps).  An operand
// that does not decode is the identity here, so the schedule does not depend on validity.
__device__ __forceinline__ uint32_t ristretto_add_pair(ge_p3& r, const uint32_t a[8], const uint32_t b[8], uint32_t sub) {
  ge_cached q;
  uint32_t ok = 1;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    uint32_t x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = h ? a[i] : b[i];
    ge_p3 p;
    ok &= ristretto_decode(p, x);
    if (h == 0) { ge_to_cached(q, p); ge_cached_cneg(q, sub); }
    else ge_add_cached(r, p, q);
  }
  return ok;
}

}  // namespace zkp
