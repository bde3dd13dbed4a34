// Bounded discrete logarithms to the basepoint (zkp_mi355x.h (10): zkp_dlog_base) and to a base of the caller's (zkp_dlog_point): the plan and the probe of baby-step / giant-step on ristretto255.
//
// With m = 2^baby_bits, k = j m + i: candidate j of a point Q is Q - j m B, and k is found when the ENCODING of a candidate equals the encoding of a
// baby step i B (equality in the group is equality of canonical encodings).  An encoding costs an inverse square root (~265 field products, 40
// additions' worth) -- unless the point is a double: encode(2 P) needs only 1 / (e g f h) (ristretto_dc_prepare / _finish, ge25519.h), and plain
// inversions are shared by Montgomery's trick.  So everything is walked in HALVES: the call first multiplies Q by (l + 1) / 2, candidate j is
// H_j = Q / 2 - j (m / 2) B (m / 2 is an integer: baby_bits >= 4), one addition of -(m / 2) B per giant step, and the bytes compared are encode(2 H_j).
// The baby rows are built the same way from i / 2 B.
//
// A GROUP is the set of candidates that share one inversion.  On the device it is a workgroup: DLOG_GROUP lanes, each with its own candidate of
// the same step, a product tree over the lanes' x = e g f h in LDS, ONE inversion, and the tree walked down again -- about three field products per
// candidate, and a lane never holds more than one encoder state (54 words) in registers.  On the host a group is DLOG_GROUP consecutive giant steps
// of one point with the serial form of the same trick.
//
// THE ZERO CASE.  x = 0 exactly when the doubled candidate is the identity, i.e. whenever k is a multiple of m (k = 0 included: the input itself
// is the identity).  A zero factor would make the group's product zero and every inverse of the group garbage.  It is handled by a SELECT: the
// factor becomes 1, the candidate's bytes become the identity's encoding (32 zero bytes), which is baby row 0.  No branch changes the product.
//
// The probe structure is an open-addressing table of 2 m slots (load 1/2, linear probing) keyed by 32 bits of the encoding, each slot a second 32-bit
// word of the encoding (the tag) and the baby index + 1.  A tag match is a candidate only: it is confirmed against all 32 bytes of the stored row,
// and a refuted candidate does not end the probe -- the walk goes on to the next slot until it meets an empty one.  Prepare is synchronous, so the
// slots are filled on the host from the downloaded rows (dlog_fill_slots): no device atomics.
//
// Work items of the search are (point, chunk of DLOG_CHUNK consecutive giant steps): one point with a large range fills the chip as well as 2^20
// points with small ranges.  The chunk axis is cut into SLICES launched in ascending order on the stream (dlog_slice_chunks): small logarithms are
// found by the first launch, later launches leave at once for finished points, no launch is long, and nothing synchronises with the host.
// k is unique (2^bits < l), so an output has at most one writer and nothing uses atomics.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ge25519.h"

namespace zkp {

constexpr uint32_t DLOG_BITS_MAX = 48;            // cost grows as 2^(bits - baby_bits) per point: a mistyped range must not hold a shared GPU for hours
constexpr uint32_t DLOG_BABY_MIN = 4, DLOG_BABY_MAX = 22, DLOG_BABY_DEFAULT = 16;
constexpr int DLOG_GROUP = 256;                   // candidates per shared inversion (device: the lanes of a workgroup)
#ifndef ZKP_DLOG_CHUNK
#define ZKP_DLOG_CHUNK 32                         // (-DZKP_DLOG_CHUNK / -DZKP_DLOG_SLICE_ITEMS build the A/B variants of tools/dlog_bench.py)
#endif
#ifndef ZKP_DLOG_SLICE_ITEMS
#define ZKP_DLOG_SLICE_ITEMS (1ull << 20)
#endif
constexpr uint32_t DLOG_CHUNK = ZKP_DLOG_CHUNK;   // consecutive giant steps per work item
constexpr uint64_t DLOG_SLICE_ITEMS = ZKP_DLOG_SLICE_ITEMS;      // work items per launch: 16 wavefronts for each of the 1,024 SIMDs of an MI355X (measured against 2^16 and 2^18: CHANGELOG.md)
constexpr uint32_t DLOG_ROW_RUN = 16;             // consecutive baby rows a lane of the table build walks (even: its start i0 / 2 is an integer)
constexpr uint64_t DLOG_MAX_LAUNCHES = 65536;     // a call that would need more step launches is refused (prepare a larger table, or split the call)
constexpr uint32_t DLOG_NONE = 0xffffffffu;

struct dlog_slot { uint32_t tag, idx1; };         // idx1 = baby index + 1, 0 = empty

// giant steps of a call: j in [0, J), J = ceil(2^bits / m); chunks per point; chunks per point in one launch for n points
ZKP_HD uint64_t dlog_giant_steps(uint32_t bits, uint32_t baby_bits) { return bits <= baby_bits ? 1ull : 1ull << (bits - baby_bits); }
ZKP_HD uint64_t dlog_chunks(uint32_t bits, uint32_t baby_bits) { return (dlog_giant_steps(bits, baby_bits) + DLOG_CHUNK - 1) / DLOG_CHUNK; }
ZKP_HD uint64_t dlog_slice_chunks(uint64_t n) {
  const uint64_t c = DLOG_SLICE_ITEMS / (n ? n : 1);
  return c ? c : 1;
}

// 32 bits of position and 32 bits of tag from disjoint words of the encoding (word 0 has a fixed low bit, word 7 a fixed high one)
ZKP_HD uint32_t dlog_hash(const uint32_t w[8]) { return (w[1] ^ (w[2] << 5) ^ (w[3] >> 7)) * 0x9e3779b1u; }
ZKP_HD uint32_t dlog_tag(const uint32_t w[8]) { return w[4] ^ w[6]; }
ZKP_HD uint32_t dlog_slot_count(uint32_t baby_bits) { return 2u << baby_bits; }

// The baby index whose row equals the encoding w, or DLOG_NONE.  rows: [2^baby_bits][8] words, slots: [dlog_slot_count].  The table is half
// empty, so the walk ends; the bound on it only keeps a damaged table from holding the lane.
ZKP_HD uint32_t dlog_probe(const uint32_t w[8], const dlog_slot* slots, const uint32_t* rows, uint32_t baby_bits) {
  const uint32_t mask = dlog_slot_count(baby_bits) - 1u;
  const uint32_t tag = dlog_tag(w);
  uint32_t h = dlog_hash(w) >> (31u - baby_bits);
  for (uint32_t walked = 0; walked <= mask; ++walked) {
    const dlog_slot s = slots[h];
    if (s.idx1 == 0u) return DLOG_NONE;
    if (s.tag == tag) {                                       // a candidate: confirmed against the whole row, and a refuted one is passed over
      const uint32_t* r = rows + 8 * (size_t)(s.idx1 - 1u);
      uint32_t diff = 0;
      for (int k = 0; k < 8; ++k) diff |= r[k] ^ w[k];
      if (diff == 0u) return s.idx1 - 1u;
    }
    h = (h + 1u) & mask;
  }
  return DLOG_NONE;
}

// host: the slots of rows [2^baby_bits][8] (slots zeroed by the caller)
inline void dlog_fill_slots(dlog_slot* slots, const uint32_t* rows, uint32_t baby_bits) {
  const uint32_t mask = dlog_slot_count(baby_bits) - 1u, m = 1u << baby_bits;
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t* w = rows + 8 * (size_t)i;
    uint32_t h = dlog_hash(w) >> (31u - baby_bits);
    while (slots[h].idx1) h = (h + 1u) & mask;
    slots[h].tag = dlog_tag(w);
    slots[h].idx1 = i + 1u;
  }
}

// Any base, signed ranges (zkp_mi355x.h (10): zkp_dlog_point).  A SLOT is the same table for a base G of the caller's: G's fixed-base table, the rows
// encode(i G), their probe slots and the walk points (1/2) G and (m / 2) G; nothing in the search knows which base it walks.  A signed range
// [-2^(bits - 1), 2^(bits - 1)) is the unsigned search on Q + 2^(bits - 1) G: the prepare step adds 2^(bits - 1) (G / 2) to the halved point (one
// point per call, from the slot's fixed-base table), a hit k' is written as k' - 2^(bits - 1).  What keeps small magnitudes early is the ORDER of
// the launches alone: slices go on the stream in ascending distance from the slice that starts at k = 0 (dlog_slice_order).  For that slice to
// exist, a signed call's slice length is rounded down to a power of two (dlog_slice_chunks_signed): the chunks of a point are a power of two as
// well, so k' = 2^(bits - 1) is the first step of slice n_slices / 2 whenever there is more than one slice.
constexpr uint32_t DLOG_POINT_SLOTS = 8;
ZKP_HD uint64_t dlog_slice_chunks_signed(uint64_t n) {
  uint64_t c = dlog_slice_chunks(n), p = 1;
  while (p * 2 <= c) p *= 2;
  return p;
}
// The slice launched i-th of n_slices.  Unsigned: i.  Signed: z = n_slices / 2 first, then z - 1, z + 1, z - 2, ... and, once one end is reached,
// the rest of the other side outward.  A permutation of 0 .. n_slices - 1; i >= n_slices is answered with i.
ZKP_HD uint64_t dlog_slice_order(uint64_t n_slices, bool is_signed, uint64_t i) {
  if (!is_signed || i >= n_slices) return i;
  const uint64_t z = n_slices / 2, below = z, above = n_slices - 1 - z, both = below < above ? below : above;
  if (i == 0) return z;
  if (i <= 2 * both) return (i & 1) ? z - (i + 1) / 2 : z + i / 2;
  const uint64_t r = i - 2 * both;
  return below > above ? z - both - r : z + both + r;
}

// k = j m + i is an answer only below 2^bits (bits < baby_bits: the table is longer than the range)
ZKP_HD bool dlog_in_range(uint64_t k, uint32_t bits) { return (k >> bits) == 0; }

}  // namespace zkp
