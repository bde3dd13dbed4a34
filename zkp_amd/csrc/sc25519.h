// Scalars modulo l = 2^252 + 27742317777372353535851937790883648493 on the GPU: eight 32-bit limbs, products from the same full-rate
// v_mad_u64_u32 the field code uses.  A product, a * b + c and a 64-byte string are reduced in ONE pass with l = 2^252 + delta
// (2^252 == -delta, delta < 2^125: sc_reduce_wide); the chain of the inversion stays in Montgomery form (R = 2^256, sc_mont), whose
// reduction uses only the four non-zero low limbs of l and a shift for limb 7.
// Needed by the batch-verification coefficient build (reference src/toolbox/batch_verifier.rs:173-206:
// `random_factor * minus_c[j]`, `random_factor * resp`, accumulation into the coefficient matrix).
// Host + device header, tested on the CPU against Python integers (tests/test_host_field.py, tests/test_host_scalar_edges.py) and on
// the device against the same integers (tools/microbench/sc_probe.hip, tests/test_gpu_sc_probe.py).
#pragma once
#include <stdint.h>
#include "fe25519.h"   // ZKP_HD

namespace zkp {

struct sc { uint32_t v[8]; };     // little-endian limbs, always < l unless stated otherwise

ZKP_HD uint32_t sc_l(int i) {
  return i == 0 ? 0x5cf5d3edu : i == 1 ? 0x5812631au : i == 2 ? 0xa2f79cd6u : i == 3 ? 0x14def9deu : i == 4 ? 0x00000000u : i == 5 ? 0x00000000u : i == 6 ? 0x00000000u : 0x10000000u;
}
// R^2 mod l, R = 2^256 (generated: pow(2, 512, l))
ZKP_HD uint32_t sc_rr(int i) {
  return i == 0 ? 0x449c0f01u : i == 1 ? 0xa40611e3u : i == 2 ? 0x68859347u : i == 3 ? 0xd00e1ba7u : i == 4 ? 0x17f5be65u : i == 5 ? 0xceec73d2u : i == 6 ? 0x7c309a3du : 0x0399411bu;
}
// R mod l
ZKP_HD uint32_t sc_r1(int i) {
  return i == 0 ? 0x8d98951du : i == 1 ? 0xd6ec3174u : i == 2 ? 0x737dcf70u : i == 3 ? 0xc6ef5bf4u : i == 4 ? 0xfffffffeu : i == 5 ? 0xffffffffu : i == 6 ? 0xffffffffu : 0x0fffffffu;
}
// (l - 1) / 2
ZKP_HD uint32_t sc_half(int i) {
  return i == 0 ? 0x2e7ae9f6u : i == 1 ? 0x2c09318du : i == 2 ? 0x517bce6bu : i == 3 ? 0x0a6f7cefu : i == 7 ? 0x08000000u : 0u;
}
constexpr uint32_t SC_N0INV = 0x12547e1bu;      // -l^-1 mod 2^32

ZKP_HD void sc_zero(sc& r) {
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = 0;
}
// a -= l if a >= l   (a < 2 l)
ZKP_HD void sc_cond_sub_l(sc& a) {
  uint32_t d[8];
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a.v[i] - sc_l(i) - br;
    d[i] = (uint32_t)t;
    br = (t >> 63) & 1u;
  }
  const bool ge = br == 0;                    // no borrow: a >= l
#pragma unroll
  for (int i = 0; i < 8; ++i) a.v[i] = ge ? d[i] : a.v[i];
}
// r = a + b mod l   (a, b < l)
ZKP_HD void sc_add(sc& r, const sc& a, const sc& b) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.v[i] + b.v[i];
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  sc_cond_sub_l(r);                           // a + b < 2 l < 2^254: no carry out
}
// r = -a mod l   (a < l)
ZKP_HD void sc_neg(sc& r, const sc& a) {
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) nz |= a.v[i];
  const uint32_t m = 0u - (uint32_t)(nz != 0);
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)sc_l(i) - a.v[i] - br;
    r.v[i] = (uint32_t)t & m;
    br = (t >> 63) & 1u;
  }
}
// ---- one-pass reduction --------------------------------------------------------------------------------------------------------
// delta = l - 2^252 (125 bits) = the four low limbs of l
ZKP_HD uint32_t sc_delta(int i) { return sc_l(i); }
// 2^252 - 66 delta   (the bias of sc_reduce_tail)
ZKP_HD uint32_t sc_bias(int i) {
  return i == 0 ? 0x089f5ce6u : i == 1 ? 0x4b427334u : i == 2 ? 0xfc2990bdu : i == 3 ? 0x9e839499u : i == 4 ? 0xfffffffau : i == 7 ? 0x0fffffffu : 0xffffffffu;
}
// 32 l (nine limbs)
ZKP_HD uint32_t sc_32l(int i) {
  return i == 0 ? 0x9eba7da0u : i == 1 ? 0x024c634bu : i == 2 ? 0x5ef39acbu : i == 3 ? 0x9bdf3bd4u : i == 4 ? 0x00000002u : i == 8 ? 0x00000002u : 0u;
}

// out[NA + NB] = a * b (+ add[0 .. NB) when add != nullptr): operand scanning, one v_mad_u64_u32 per product with the carry and the
// running limb in its 64-bit addend ((2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1: it never overflows)
template <int NA, int NB>
ZKP_HD void sc_mul_words(uint32_t* out, const uint32_t* a, const uint32_t* b, const uint32_t* add = nullptr) {
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      c += (uint64_t)a[i] * b[j] + (i ? out[i + j] : add ? add[j] : 0u);
      out[i + j] = (uint32_t)c;
      c >>= 32;
    }
    out[i + NB] = (uint32_t)c;
  }
}
// out[NA + 4] = delta * a
template <int NA>
ZKP_HD void sc_mul_delta(uint32_t* out, const uint32_t* a) {
  uint32_t d[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = sc_delta(i);
  sc_mul_words<4, NA>(out, d, a);
}
// x = lo + 2^252 hi: lo[8] < 2^252, hi[NH] = the NH limbs above bit 252 (x has at least NH + 8 limbs, or exactly NH + 7 when TOP: then
// its missing limb counts as zero)
template <int NH, bool TOP>
ZKP_HD void sc_split252(uint32_t* lo, uint32_t* hi, const uint32_t* x) {
#pragma unroll
  for (int i = 0; i < 7; ++i) lo[i] = x[i];
  lo[7] = x[7] & 0x0fffffffu;
#pragma unroll
  for (int k = 0; k < NH; ++k) hi[k] = (TOP && k == NH - 1) ? x[7 + k] >> 28 : (x[7 + k] >> 28) | (x[8 + k] << 4);
}
// The last step of every reduction: v[9] = any value below 67 * 2^252 -> its canonical representative.  With q = v >> 252 (<= 66) and
// 2^252 == -delta:  v == (v mod 2^252) - q delta =: t, -66 delta <= t < 2^252.  The sum w = (v mod 2^252) + (66 - q) delta + (2^252 - 66 delta)
// = t + 2^252 is positive and below 2^253: bit 252 of w says whether t is negative (then the result is t + l = w + delta, which is
// below l) or not (then it is t = w - 2^252, which is below 2^252 < l).  No conditional subtraction of l is left to do.
ZKP_HD void sc_reduce_tail(sc& r, const uint32_t* v) {
  const uint32_t n = 66u - ((v[8] << 4) | (v[7] >> 28));
  uint32_t w[8];
  uint64_t c = 0, m = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < 4) m += (uint64_t)n * sc_delta(i);
    c += (uint64_t)(i == 7 ? v[7] & 0x0fffffffu : v[i]) + sc_bias(i) + (uint32_t)m;
    w[i] = (uint32_t)c;
    c >>= 32;
    m >>= 32;
  }
  const uint32_t neg = 0u - (uint32_t)((w[7] >> 28) == 0);       // t < 0
  c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)w[i] + (i < 4 ? sc_delta(i) & neg : 0u);
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  r.v[7] -= ~neg & 0x10000000u;
}
// x[16] (any 512-bit value) -> canonical scalar.  Two folds of what lies above bit 252:
//   x = L + 2^252 H == L - delta H,  delta H = L2 + 2^252 H2 == L2 - delta H2  =>  x == L + delta H2 + (l - L2)
// H < 2^260 (9 limbs), delta H < 2^385 (13 limbs), H2 < 2^133 (5 limbs), delta H2 < 2^258 (9 limbs): the sum is below 2^258 + 2^253 + delta.
ZKP_HD void sc_reduce_wide(sc& r, const uint32_t* x) {
  uint32_t L[8], H[9], y[13], L2[8], H2[5], z[9], v[9];
  sc_split252<9, true>(L, H, x);
  sc_mul_delta<9>(y, H);
  sc_split252<5, false>(L2, H2, y);
  sc_mul_delta<5>(z, H2);
  uint64_t c = 0, br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)sc_l(i) - L2[i] - br;           // l - L2 > 0: no borrow out of limb 7
    br = (t >> 63) & 1u;
    c += (uint64_t)L[i] + z[i] + (uint32_t)t;
    v[i] = (uint32_t)c;
    c >>= 32;
  }
  v[8] = (uint32_t)c + z[8];
  sc_reduce_tail(r, v);
}
// x[12] (any 384-bit value) -> canonical scalar.  One fold: H < 2^132 (5 limbs), delta H < 2^257 (9 limbs), x == L + (32 l - delta H),
// below 2^252 + 2^257 + 32 delta.
ZKP_HD void sc_reduce_384(sc& r, const uint32_t* x) {
  uint32_t L[8], H[5], y[9], v[9];
  sc_split252<5, true>(L, H, x);
  sc_mul_delta<5>(y, H);
  uint64_t c = 0, br = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const uint64_t t = (uint64_t)sc_32l(i) - y[i] - br;          // 32 l > 2^257 > delta H: no borrow out of limb 8
    br = (t >> 63) & 1u;
    c += (uint64_t)(i < 8 ? L[i] : 0u) + (uint32_t)t;
    v[i] = (uint32_t)c;
    c >>= 32;
  }
  sc_reduce_tail(r, v);
}

// r = a * b + c mod l: one product, one reduction.  a, b, c: ANY 256-bit values (a b + c < 2^512).  r may be an operand.
ZKP_HD void sc_muladd(sc& r, const sc& a, const sc& b, const sc& c) {
  uint32_t x[16];
  sc_mul_words<8, 8>(x, a.v, b.v, c.v);
  sc_reduce_wide(r, x);
}
// r = a * b mod l   (a, b: any 256-bit values)
ZKP_HD void sc_mul(sc& r, const sc& a, const sc& b) {
  uint32_t x[16];
  sc_mul_words<8, 8>(x, a.v, b.v);
  sc_reduce_wide(r, x);
}
// r = a * w mod l for a 128-bit w (the batch verifier's weights: Scalar::from(u128)) and any 256-bit a
ZKP_HD void sc_mul_u128(sc& r, const sc& a, const uint32_t w[4]) {
  uint32_t x[12];
  sc_mul_words<4, 8>(x, w, a.v);
  sc_reduce_384(r, x);
}
// any 256-bit value -> canonical representative
ZKP_HD void sc_reduce(sc& r, const sc& a) {
  uint32_t v[9];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = a.v[i];
  v[8] = 0;
  sc_reduce_tail(r, v);
}

// ---- Montgomery form (the inversion chain) ---------------------------------------------------------------------------------------
// Montgomery product a * b * 2^-256 mod l.  b < l; a any 256-bit value.  Result < l.  Each row adds m l with l's limbs 4 .. 6 = 0
// (only the carry passes through) and limb 7 = 2^28 (a shift): four products by l instead of eight.
ZKP_HD void sc_mont(sc& r, const sc& a, const sc& b) {
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c += (uint64_t)a.v[i] * b.v[j] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[8] = (uint32_t)c;
    t[9] = (uint32_t)(c >> 32);
    const uint32_t m = t[0] * SC_N0INV;
    c = (uint64_t)m * sc_l(0) + t[0];
    c >>= 32;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      c += (uint64_t)m * sc_l(j) + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
#pragma unroll
    for (int j = 4; j < 7; ++j) {
      c += t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += ((uint64_t)m << 28) + t[7];
    t[6] = (uint32_t)c;
    c >>= 32;
    c += t[8];
    t[7] = (uint32_t)c;
    t[8] = t[9] + (uint32_t)(c >> 32);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = t[i];
  sc_cond_sub_l(r);                           // < 2 l before
}
// to Montgomery form: a * R mod l  (so that sc_mont(to_mont(a), b) = a * b)
ZKP_HD void sc_to_mont(sc& r, const sc& a) {
  sc rr;
#pragma unroll
  for (int i = 0; i < 8; ++i) rr.v[i] = sc_rr(i);
  sc_mont(r, a, rr);
}

// l <= the 256-bit little-endian value?  (Scalar::from_canonical_bytes / dalek's Deserialize accept only values < l.)
ZKP_HD uint32_t sc_not_canonical(const uint32_t v[8]) {
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) br = (((uint64_t)v[i] - sc_l(i) - br) >> 63) & 1u;
  return br ? 0u : 1u;                              // no borrow: v >= l
}

// e = s + K where K has the bit pattern `pattern` in every word: signed-digit recoding without a
// sequential carry (digit_i = e_i - 2^(c-1)).  top receives the carry out of bit 255.
ZKP_HD void sc_add_pattern(uint32_t e[8], uint32_t& top, const uint32_t s[8], uint32_t pattern) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)s[i] + pattern;
    e[i] = (uint32_t)c;
    c >>= 32;
  }
  top = (uint32_t)c;
}

// Sign folding for multiscalar multiplication: s * P = (l - s) * (-P).  If (l-1)/2 < s <= l, replaces s by l - s and
// returns 1 (the caller negates the point or the digits); otherwise leaves s alone (also when s > l: non-canonical
// scalars keep their value).  The folded scalar is < 2^252, and the negated 128-bit weights of the batch verifier
// (batch_verifier.rs:183: l - r) come out as r: 128 bits instead of 253, with none of the all-ones digit runs.
ZKP_HD uint32_t sc_fold_sign(uint32_t s[8]) {
  uint32_t d[8];
  uint64_t b1 = 0, b2 = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t1 = (uint64_t)sc_half(i) - s[i] - b1;      // borrow out  <=>  s > half
    b1 = (t1 >> 63) & 1u;
    const uint64_t t2 = (uint64_t)sc_l(i) - s[i] - b2;         // l - s, borrow out  <=>  s > l
    d[i] = (uint32_t)t2;
    b2 = (t2 >> 63) & 1u;
  }
  const bool fold = b1 && !b2;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = fold ? d[i] : s[i];
  return fold ? 1u : 0u;
}

// The sign fold for the signed radix-16 walks (comb_tables.h: term_comb, comb_group_xbar, term_ladder16) of a scalar the caller vouches is reduced
// (at most l).  f = min(s, l - s) <= (l - 1) / 2 = 2^251 + (delta - 1) / 2 with delta = l - 2^252 < 2^125; e = f + K62 with K62 = sum_{i < 62} 8 * 16^i
// puts the offset on nibbles 0 .. 61 only:
//     nibble i < 62 of e:  the signed digit nibble - 8 in [-8, 7], as in the unfolded recoding
//     e >> 248:            the digit of nibble 62 as it stands, 0 .. 8 (every row has an entry 8); nibble 63 does not exist.
// K62 < 0.534 * 2^248.  For f >= 2^251 the bits 125 .. 250 of f are zero, so the offsets cannot carry into bit 248 and the top digit is 8; below
// 2^251 the sum stays under 8.534 * 2^248.  Returns 1 where l - s was taken: the caller negates the sum of the walk (ge_cneg).
constexpr uint32_t SC_FOLD16_TOP_NIBBLE = 62;
ZKP_HD uint32_t sc_fold_recode16(uint32_t e[8], const uint32_t s[8]) {
  uint32_t f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = s[i];
  const uint32_t flip = sc_fold_sign(f);
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)f[i] + (i < 7 ? 0x88888888u : 0x00888888u);
    e[i] = (uint32_t)c;
    c >>= 32;
  }
  return flip;
}

// r = a / 2 mod l for any 256-bit a (reduced first): (a + (a odd ? l : 0)) >> 1
ZKP_HD void sc_halve(sc& r, const sc& a) {
  sc t;
  sc_reduce(t, a);
  const uint32_t odd = 0u - (t.v[0] & 1u);
  uint64_t c = 0;
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)t.v[i] + (sc_l(i) & odd);
    w[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) r.v[i] = (w[i] >> 1) | (w[i + 1] << 31);
  r.v[7] = w[7] >> 1;                         // t + l < 2^254: no carry out
}

// the same for an input that is already canonical (< l): no reduction
ZKP_HD void sc_halve_canonical(sc& r, const sc& t) {
  const uint32_t odd = 0u - (t.v[0] & 1u);
  uint64_t c = 0;
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)t.v[i] + (sc_l(i) & odd);
    w[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) r.v[i] = (w[i] >> 1) | (w[i + 1] << 31);
  r.v[7] = w[7] >> 1;
}

// 512-bit little-endian value (lo + hi * 2^256) -> canonical scalar: Scalar::from_bytes_mod_order_wide
ZKP_HD void sc_from_wide(sc& r, const sc& lo, const sc& hi) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) { x[i] = lo.v[i]; x[8 + i] = hi.v[i]; }
  sc_reduce_wide(r, x);
}

// y = y^(2^n) * t in Montgomery form: n squarings in a rolled loop (n is a constant at every call site), one product
ZKP_HD void sc_sqmul(sc& y, int n, const sc& t) {
#pragma unroll 1
  for (int k = 0; k < n; ++k) sc_mont(y, y, y);
  sc_mont(y, y, t);
}
// r = a^(l-2) mod l: the inverse, 0 for 0 (Scalar::invert).  a < l (any 256-bit a works: sc_to_mont reduces it).  The exponent
// l - 2 = 2^252 + 0x14def9dea2f79cd65812631a5cf5d3eb is public: a fixed chain, a 4-bit sliding window over the odd powers a^3 .. a^15
// held in named values.  289 Montgomery products: 1 into Montgomery form, 8 for a^2 and the seven odd powers, 252 squarings and 27
// products of the walk, 1 out.  No branch, address or trip count depends on a.
ZKP_HD void sc_invert(sc& r, const sc& a) {
  sc y, a2, t3, t5, t7, t9, t11, t13, t15, one;
  sc_to_mont(y, a);
  sc_mont(a2, y, y);
  sc_mont(t3, a2, y);
  sc_mont(t5, a2, t3);
  sc_mont(t7, a2, t5);
  sc_mont(t9, a2, t7);
  sc_mont(t11, a2, t9);
  sc_mont(t13, a2, t11);
  sc_mont(t15, a2, t13);
  // bits 251 .. 0 of l - 2 after the leading one (y = a): 127 zeros, then the 125-bit tail window by window
  sc_sqmul(y, 130, t5);
  sc_sqmul(y, 6, t13);
  sc_sqmul(y, 3, t7);
  sc_sqmul(y, 5, t15);
  sc_sqmul(y, 4, t9);
  sc_sqmul(y, 4, t13);
  sc_sqmul(y, 3, t7);
  sc_sqmul(y, 4, t5);
  sc_sqmul(y, 7, t11);
  sc_sqmul(y, 4, t13);
  sc_sqmul(y, 3, t7);
  sc_sqmul(y, 5, t7);
  sc_sqmul(y, 6, t13);
  sc_sqmul(y, 3, t3);
  sc_sqmul(y, 6, t11);
  sc_sqmul(y, 10, t9);
  sc_sqmul(y, 4, t3);
  sc_sqmul(y, 5, t3);
  sc_sqmul(y, 7, t13);
  sc_sqmul(y, 6, t11);
  sc_sqmul(y, 4, t9);
  sc_sqmul(y, 3, t7);
  sc_sqmul(y, 5, t11);
  sc_sqmul(y, 3, t5);
  sc_sqmul(y, 6, t15);
  sc_sqmul(y, 3, t5);
  sc_sqmul(y, 3, t3);
  sc_zero(one);
  one.v[0] = 1;
  sc_mont(r, y, one);
}

}  // namespace zkp
