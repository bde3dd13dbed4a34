// Segmented sums, products and dot products of scalars mod l (zkp_mi355x.h (12): zkp_sc_reduce): the plan and the fold kernel.
//
// The job is in CSR form, as in point_sum.h: output i folds the terms [off[i], off[i + 1]).  The fold runs in LEVELS over an axis of items sorted by
// segment.  Level 1's items are the terms (a[ai(t)], or a[ai(t)] * b[bi(t)] for the dot product), the items of a later level are what the level
// below handed on.  The WORK UNIT IS A WORKGROUP of SC_RED_GROUP lanes, and it folds SC_RED_GROUP consecutive items, ONE ITEM PER LANE -- not a lane
// that walks consecutive items as k_sum_fold does: an item here is a 32-byte load and some tens of instructions, so the lanes must sit on consecutive
// addresses.  Rows that are read in order (no index array; every later level) come in as 16 bytes per lane with consecutive lanes on consecutive
// addresses -- two such loads per workgroup cover its 8 KiB -- into an LDS tile, from which every lane takes its own 32 bytes; gathered rows are read
// by their lane directly.  The stretch of one segment inside a unit is a RUN.  The runs of a unit are folded by a segmented inclusive scan with head
// flags over the unit's lanes (Hillis-Steele in an LDS tile held limb by limb, so a wavefront's accesses fall on consecutive banks; log2(SC_RED_GROUP)
// steps), after which the last lane of a run holds the run.  A run that is neither the unit's first nor its last is complete and goes to out[segment];
// the first and the last are handed on as the items (2g, 2g + 1) of the next level (a unit that is one run hands on the run and the identity under
// the same segment).  items_{k+1} = 2 ceil(items_k / SC_RED_GROUP); the level with at most SC_RED_GROUP items is one unit that finishes every run.
// The launches follow from the number of terms and outputs alone, every output has one writer (an empty segment is written by the lane of level 1
// that carries its number), nothing is accumulated with atomics and no lane waits for another workgroup.
//
// NOTHING HERE BRANCHES ON, INDEXES BY OR COUNTS WITH A SCALAR'S VALUE: every lane computes the scan step's sum or product and keeps or drops it by
// a select on the head flags, which come from off alone.  A zero factor does not end a product.
#pragma once
#include "dev_layout.h"
#include "point_sum.h"   // segment_of_term
#include "sc25519.h"

namespace zkp {

constexpr uint32_t SC_RED_GROUP = 256;     // items per work unit (a workgroup) and level; the workgroup's size
constexpr int SC_RED_SUM = 0, SC_RED_PRODUCT = 1, SC_RED_DOT = 2;

// items a level of n items hands on (n > SC_RED_GROUP), and the number of fold launches of a call of n_terms terms
inline uint32_t sc_red_next_items(uint32_t n) { return 2 * ((n + SC_RED_GROUP - 1) / SC_RED_GROUP); }
inline uint32_t sc_red_levels(uint32_t n_terms) {
  if (n_terms == 0) return 0;
  uint32_t levels = 1;
  for (uint32_t n = n_terms; n > SC_RED_GROUP; n = sc_red_next_items(n)) ++levels;
  return levels;
}

#ifdef __HIPCC__
struct sc_red_tile {
  uint4 stage[2 * SC_RED_GROUP];           // rows as they lie in memory
  uint32_t v[8 * SC_RED_GROUP];            // the scan: limb k of lane i at v[k SC_RED_GROUP + i]
  uint32_t f[SC_RED_GROUP];                // the scanned head flags
  uint32_t seg[SC_RED_GROUP];
};

// x = row ai(base + i) of the operand p of n_rows rows for the cnt <= SC_RED_GROUP items of a unit (zeros for a lane at or beyond cnt).  Without idx
// the unit's rows [base, base + cnt) are staged through the tile by coalesced 16-byte loads; no row at or beyond n_rows is read either way.  Called by
// every lane of the workgroup (barriers).
__device__ __forceinline__ void sc_red_operand(sc& x, sc_red_tile& t, const uint8_t* __restrict__ p, const uint32_t* __restrict__ idx, uint32_t n_rows,
                                               uint32_t base, uint32_t cnt, uint32_t i) {
  if (idx) {
    sc_zero(x);
    if (i < cnt) {
      const uint32_t r = idx[base + i];
      load_vec<2>(x.v, p + 32 * (size_t)(r < n_rows ? r : n_rows - 1));
    }
  } else {
    const uint32_t have = base < n_rows ? (cnt < n_rows - base ? cnt : n_rows - base) : 0u;
    const uint4* src = reinterpret_cast<const uint4*>(p) + 2 * (size_t)base;
    __syncthreads();                                              // (the tile may still be read for the operand before)
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t q = i + h * SC_RED_GROUP;
      t.stage[q] = q < 2 * have ? src[q] : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const uint4 lo = t.stage[2 * i], hi = t.stage[2 * i + 1];
    x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w;
    x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w;
  }
}

// k_sc_fold: one level.  Workgroup g folds items [g SC_RED_GROUP, (g + 1) SC_RED_GROUP) of n_items.  TERMS (level 1): item t is term t, its segment one
// binary search in off (always below n_out); the grid also covers n_out lanes, and lane s writes the identity to out[s] where segment s is empty.
// Otherwise item j is (in_v[j], in_seg[j]).  MUL: the runs are products (identity 1), else sums (identity 0).  `last`: the launch is one unit and every
// run goes to out.  Every index that reaches memory is below its array's length whatever off, aidx and bidx hold.
template <int OP, bool TERMS>
__global__ void __launch_bounds__(SC_RED_GROUP)
k_sc_fold(uint32_t n_items, uint32_t units, uint32_t last, const uint32_t* __restrict__ off, uint32_t n_out, const uint8_t* __restrict__ a, uint32_t n_a,
          const uint32_t* __restrict__ aidx, const uint8_t* __restrict__ b, uint32_t n_b, const uint32_t* __restrict__ bidx,
          const uint8_t* __restrict__ in_v, const uint32_t* __restrict__ in_seg, uint8_t* __restrict__ hand_v, uint32_t* __restrict__ hand_seg,
          uint8_t* __restrict__ out) {
  constexpr bool MUL = OP == SC_RED_PRODUCT;
  __shared__ sc_red_tile t;
  const uint32_t i = threadIdx.x, g = blockIdx.x;
  sc ident;
  sc_zero(ident);
  ident.v[0] = MUL ? 1u : 0u;
  if (TERMS) {
    const uint32_t s = g * SC_RED_GROUP + i;
    if (s < n_out && off[s + 1] == off[s]) store_vec<2>(out + 32 * (size_t)s, ident.v);
    if (g >= units) return;                                       // (uniform in the workgroup)
  }
  const uint32_t base = g * SC_RED_GROUP, cnt = n_items - base < SC_RED_GROUP ? n_items - base : SC_RED_GROUP;
  const uint32_t j = base + (i < cnt ? i : cnt - 1);              // a lane beyond the items carries the identity under the last item's segment
  sc v;
  uint32_t seg;
  if (TERMS) {
    sc x;
    sc_red_operand(x, t, a, aidx, n_a, base, cnt, i);
    if (OP == SC_RED_DOT) {
      sc y;
      sc_red_operand(y, t, b, bidx, n_b, base, cnt, i);
      sc_mul(v, x, y);
    } else {
      sc_reduce(v, x);
    }
    seg = segment_of_term(off, n_out, j);
  } else {
    sc_red_operand(v, t, in_v, nullptr, n_items, base, cnt, i);
    seg = in_seg[j];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) v.v[k] = i < cnt ? v.v[k] : ident.v[k];
  t.seg[i] = seg;
  __syncthreads();
  const uint32_t tail = i == SC_RED_GROUP - 1 || t.seg[i + 1 < SC_RED_GROUP ? i + 1 : i] != seg;
  uint32_t f = i != 0 && t.seg[i ? i - 1 : 0] != seg;             // head flag (lane 0 opens the first run without one); scanned: a head at or below this lane
#pragma unroll
  for (int k = 0; k < 8; ++k) t.v[k * SC_RED_GROUP + i] = v.v[k];
  t.f[i] = f;
  __syncthreads();
#pragma unroll 1
  for (uint32_t d = 1; d < SC_RED_GROUP; d <<= 1) {
    const bool act = i >= d;
    const uint32_t left = act ? i - d : i;
    sc l, r;
#pragma unroll
    for (int k = 0; k < 8; ++k) l.v[k] = t.v[k * SC_RED_GROUP + left];
    const uint32_t lf = t.f[left];
    __syncthreads();
    if (MUL) sc_mul(r, l, v);
    else sc_add(r, l, v);
    const bool take = act && !f;                                  // the stretch [i - d, i] holds no head: it is one run
#pragma unroll
    for (int k = 0; k < 8; ++k) v.v[k] = take ? r.v[k] : v.v[k];
    f |= act ? lf : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) t.v[k * SC_RED_GROUP + i] = v.v[k];
    t.f[i] = f;
    __syncthreads();
  }
  if (!tail) return;
  if (last || (f && i != SC_RED_GROUP - 1)) {                     // a complete run
    store_vec<2>(out + 32 * (size_t)seg, v.v);
    return;
  }
  const size_t slot = 2 * (size_t)g + (f ? 1u : 0u);              // the first run (no head up to here) or the last
  store_vec<2>(hand_v + 32 * slot, v.v);
  hand_seg[slot] = seg;
  if (!f && i == SC_RED_GROUP - 1) {                              // one run: the second item is the identity under the same segment
    store_vec<2>(hand_v + 32 * (slot + 1), ident.v);
    hand_seg[slot + 1] = seg;
  }
}
#endif  // __HIPCC__

}  // namespace zkp
