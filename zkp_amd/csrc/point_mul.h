// One scalar times one point, start to finish in a lane (zkp_mi355x.h (8): zkp_mul_points): the walk of term_ladder16 (comb_tables.h) on a point
// that arrives in registers and an accumulator that stays there -- the caller decodes before it and encodes after it, so a product costs one
// launch and no record in memory but the lane's eight multiples.
#pragma once
#include "comb_tables.h"

namespace zkp {

// acc = s * P for any 256-bit s.  The scalar is reduced mod l here (sc_reduce: one Barrett tail, ~60 instructions), which buys the FOLDED walk of
// term_ladder16: min(s, l - s) in the recoding of sc_fold_recode16 -- nibble 62 read as it stands (0 .. 8), its entry the accumulator, then
// 62 x (4 doublings + 1 addition) on signed digits nibble - 8 instead of 64 and a carry digit -- and the sum negated where l - s was walked.
// The eight multiples of P live in the lane's slot of a wave-interleaved ladder group (tbl = this lane's slot 0; ladder_store_entry).
// CT: every entry of the table is read for every digit and kept with ge_cached_cmov, the sign is a select and a zero digit adds the identity
// like any other -- no address, bank or branch depends on s.  Otherwise the entry the digit names is loaded, a zero digit loads nothing.
// ecol = the lane's LDS column of 8 words, 256 apart (the recoded scalar, indexed by the outer loop without register indexing).
// P may be the identity (an encoding that did not decode): the formulas are complete and the walk is the same.
// KEEP IN STEP with term_ladder16 (comb_tables.h), whose folded branch this restates: the build of the eight multiples, the start at nibble 62 and
// the digit loop are the same text.  term_ladder16 was left as it is so that the term kernels compile to the instruction stream they had; a
// change to either walk belongs in both.
template <bool CT>
__device__ __forceinline__ void ladder16_point(ge_p3& acc, const uint32_t s[8], const ge_p3& P, uint4* tbl, uint32_t* ecol) {
  sc red;
#pragma unroll
  for (int j = 0; j < 8; ++j) red.v[j] = s[j];
  sc_reduce(red, red);
  uint32_t e[8];
  const uint32_t flip = sc_fold_recode16(e, red.v);
#pragma unroll
  for (int j = 0; j < 8; ++j) ecol[256 * j] = e[j];
  {
    ge_p3 m2, m3, m4, m;
    ge_cached c1, c;
    ge_to_cached(c1, P);
    ladder_store_entry(tbl, 0, c1);
    ge_double<true>(m2, P);
    ge_to_cached(c, m2); ladder_store_entry(tbl, 1, c);
    ge_add_cached(m3, m2, c1);
    ge_to_cached(c, m3); ladder_store_entry(tbl, 2, c);
    ge_double<true>(m4, m2);
    ge_to_cached(c, m4); ladder_store_entry(tbl, 3, c);
    ge_add_cached(m, m4, c1);
    ge_to_cached(c, m); ladder_store_entry(tbl, 4, c);
    ge_double<true>(m, m3);
    ge_to_cached(c, m); ladder_store_entry(tbl, 5, c);
    ge_add_cached(m, m, c1);
    ge_to_cached(c, m); ladder_store_entry(tbl, 6, c);
    ge_double<true>(m, m4);
    ge_to_cached(c, m); ladder_store_entry(tbl, 7, c);
  }
  {
    ge_cached sel;
    ladder_select<CT>(sel, tbl, ecol[256 * 7] >> 24);           // nibble 62 as it stands (nibble 63 is empty): 0 .. 8
    ge_from_cached(acc, sel);
  }
#pragma unroll 1
  for (int j = 7; j >= 0; --j) {
    uint32_t cur = ecol[256 * j];
    int k = 0;
    if (j == 7) { cur <<= 8; k = 2; }                           // (uniform) the walk goes on at nibble 61
#pragma unroll 1
    for (; k < 8; ++k) {
      ge_double4(acc);
      const uint32_t nib = cur >> 28;
      cur <<= 4;
      const uint32_t neg = (uint32_t)(nib < 8u);
      const uint32_t mag = neg ? 8u - nib : nib - 8u;           // 0..8
      ge_cached sel;
      ladder_select<CT>(sel, tbl, mag);
      ge_cached_cneg(sel, neg);
      ge_add_cached(acc, acc, sel);
    }
  }
  ge_cneg(acc, flip);
}

}  // namespace zkp
