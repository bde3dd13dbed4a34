// Segmented prefix sums and prefix products of scalars mod l (zkp_mi355x.h (13): zkp_sc_scan): the plan and the scan kernel.
//
// The job is sc_reduce.h's: terms sorted by segment in CSR form.  Here EVERY term gets a row: out[t] folds the terms of its segment up to t
// (inclusive) or before t (exclusive; the identity at the segment's first term).  The scan is REDUCE-THEN-SCAN over dependent launches: no lane
// waits for another workgroup.  The work unit is k_sc_fold's: a workgroup of SC_SCAN_GROUP lanes takes SC_SCAN_GROUP consecutive items of its
// level, one item per lane; rows in order come through the LDS tile as 16-byte coalesced loads (sc_red_operand); the lanes run the segmented
// Hillis-Steele scan with head flags held limb by limb.  An ITEM is a value and a HEAD flag: the item does not combine with what lies to its left
// (a term that is the first of its segment: off[segment] == t).
//   UP-SWEEP    (levels 1 .. L - 1)  unit g hands on ONE item: the fold of its last run (what lane SC_SCAN_GROUP - 1 holds after the scan) and the
//               OR of its head flags -- whether a segment begins inside it.  n_{k+1} = ceil(n_k / SC_SCAN_GROUP).
//   TOP         (level L, n_L <= SC_SCAN_GROUP)  one unit scans its items and writes every inclusive prefix.
//   DOWN-SWEEP  (levels L - 1 .. 1)  unit g scans its items again; the carry of its level is the inclusive prefix of item g - 1 of the level above
//               (what is open at the end of unit g - 1) and goes into the lanes with no head at or below them: the unit's first run when that run
//               began in an earlier unit.  A middle level writes inclusive prefixes for the level below; level 1 writes out, where the exclusive mode
//               takes the left neighbour inside the run (lane 0: the carry) or the identity at a head.  Rows leave through the tile on consecutive
//               addresses, 16 bytes per lane.
// Launches: 2 L - 1 (1 up to 256 terms, 3 up to 65,536, 5 up to 2^24, 7 beyond); they follow from n_terms alone.  Every row has one writer, nothing
// is accumulated with atomics, and every workspace row that is read was written by this call (a unit's hand-on by its up-sweep, a carry by the
// down-sweep above).  Workspace: (32 + 4 + 32) bytes per unit of every level but the top: 0.27 bytes per term.
//
// NOTHING HERE BRANCHES ON, INDEXES BY OR COUNTS WITH A SCALAR'S VALUE: every lane computes the scan step and the carry step and keeps or drops the
// result by a select on the head flags, which come from off alone.  A zero factor does not end a product scan.
//
// Resources (the compiler's resource report for gfx950, tools/kernel_resources.py): k_sc_scan<SUM, ..> 50 VGPRs (54 for the down-sweep of a middle
// level), k_sc_scan<PRODUCT, ..> 64 (68); 18 KiB of LDS (sc_red_tile); no scratch in any of the eight instances; 8 wavefronts per SIMD (7 for
// k_sc_scan<PRODUCT, false, true>).
#pragma once
#include "sc_reduce.h"

namespace zkp {

constexpr uint32_t SC_SCAN_GROUP = SC_RED_GROUP;       // items per work unit and level; the workgroup's size (the tile is sc_red_tile)
constexpr int SC_SCAN_MAX_LEVELS = 4;                  // 2^31 - 1 terms: 2^23, 2^15, 2^7 items above them

inline uint32_t sc_scan_next_items(uint32_t n) { return (uint32_t)(((uint64_t)n + SC_SCAN_GROUP - 1) / SC_SCAN_GROUP); }
inline uint32_t sc_scan_levels(uint32_t n_terms) {
  if (n_terms == 0) return 0;
  uint32_t levels = 1;
  for (uint32_t n = n_terms; n > SC_SCAN_GROUP; n = sc_scan_next_items(n)) ++levels;
  return levels;
}
inline uint32_t sc_scan_launches(uint32_t n_terms) { return n_terms ? 2 * sc_scan_levels(n_terms) - 1 : 0; }

#ifdef __HIPCC__
// k_sc_scan: one launch of one level.  Workgroup g scans items [g SC_SCAN_GROUP, (g + 1) SC_SCAN_GROUP) of n_items.  TERMS (level 1): item t is term t
// -- a[ai(t)] reduced, its head flag off[segment_of_term(t)] == t -- otherwise item j is (in_v[j], in_f[j]).  MUL: products (identity 1), else sums.
// DOWN = false: lane SC_SCAN_GROUP - 1 writes the unit's hand-on to (agg_v[g], agg_f[g]).  DOWN = true: the carry is carry[g - 1] (none for unit 0)
// and every item's prefix goes to out[j], exclusive where excl != 0.  Every index that reaches memory is below its array's length whatever off and
// aidx hold.
template <int OP, bool TERMS, bool DOWN>
__global__ void __launch_bounds__(SC_SCAN_GROUP)
k_sc_scan(uint32_t n_items, uint32_t excl, const uint32_t* __restrict__ off, uint32_t n_seg, const uint8_t* __restrict__ a, uint32_t n_a,
          const uint32_t* __restrict__ aidx, const uint8_t* __restrict__ in_v, const uint32_t* __restrict__ in_f, const uint8_t* __restrict__ carry,
          uint8_t* __restrict__ agg_v, uint32_t* __restrict__ agg_f, uint8_t* __restrict__ out) {
  constexpr bool MUL = OP == SC_RED_PRODUCT;
  __shared__ sc_red_tile t;
  const uint32_t i = threadIdx.x, g = blockIdx.x;
  sc ident;
  sc_zero(ident);
  ident.v[0] = MUL ? 1u : 0u;
  const uint32_t base = g * SC_SCAN_GROUP;
  if (base >= n_items) return;                                    // (uniform in the workgroup)
  const uint32_t cnt = n_items - base < SC_SCAN_GROUP ? n_items - base : SC_SCAN_GROUP;
  const uint32_t j = base + (i < cnt ? i : cnt - 1);              // a lane beyond the items carries the identity and no head
  sc v;
  uint32_t head;
  if (TERMS) {
    sc x;
    sc_red_operand(x, t, a, aidx, n_a, base, cnt, i);
    sc_reduce(v, x);
    head = off[segment_of_term(off, n_seg, j)] == j;
  } else {
    sc_red_operand(v, t, in_v, nullptr, n_items, base, cnt, i);
    head = in_f[j] != 0;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) v.v[k] = i < cnt ? v.v[k] : ident.v[k];
  head = i < cnt ? head : 0u;
  uint32_t f = head;                                              // scanned: a head at or below this lane
#pragma unroll
  for (int k = 0; k < 8; ++k) t.v[k * SC_SCAN_GROUP + i] = v.v[k];
  t.f[i] = f;
  __syncthreads();
#pragma unroll 1
  for (uint32_t d = 1; d < SC_SCAN_GROUP; d <<= 1) {
    const bool act = i >= d;
    const uint32_t left = act ? i - d : i;
    sc l, r;
#pragma unroll
    for (int k = 0; k < 8; ++k) l.v[k] = t.v[k * SC_SCAN_GROUP + left];
    const uint32_t lf = t.f[left];
    __syncthreads();
    if (MUL) sc_mul(r, l, v);
    else sc_add(r, l, v);
    const bool take = act && !f;                                  // the stretch [i - d, i] holds no head: it is one run
#pragma unroll
    for (int k = 0; k < 8; ++k) v.v[k] = take ? r.v[k] : v.v[k];
    f |= act ? lf : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) t.v[k * SC_SCAN_GROUP + i] = v.v[k];
    t.f[i] = f;
    __syncthreads();
  }
  if (!DOWN) {
    if (i == SC_SCAN_GROUP - 1) {                                 // the run that is open at the unit's end, and whether it began inside
      store_vec<2>(agg_v + 32 * (size_t)g, v.v);
      agg_f[g] = f;
    }
    return;
  }
  sc c = ident;
  if (g) load_vec<2>(c.v, carry + 32 * (size_t)(g - 1));          // (uniform)
  {
    sc r;
    if (MUL) sc_mul(r, c, v);
    else sc_add(r, c, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) v.v[k] = f ? v.v[k] : r.v[k];     // the carry enters the run that began in an earlier unit
  }
  if (excl) {                                                     // (uniform) the left neighbour inside the run, the carry for lane 0, the identity at a head
#pragma unroll
    for (int k = 0; k < 8; ++k) t.v[k * SC_SCAN_GROUP + i] = v.v[k];
    __syncthreads();
    const uint32_t left = i ? i - 1 : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t lv = t.v[k * SC_SCAN_GROUP + left];
      v.v[k] = head ? ident.v[k] : (i ? lv : c.v[k]);
    }
  }
  t.stage[2 * i] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  t.stage[2 * i + 1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(out) + 2 * (size_t)base;
#pragma unroll
  for (uint32_t h = 0; h < 2; ++h) {
    const uint32_t q = i + h * SC_SCAN_GROUP;
    if (q < 2 * cnt) dst[q] = t.stage[q];
  }
}
#endif  // __HIPCC__

}  // namespace zkp
