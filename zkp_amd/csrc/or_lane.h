// The per-item code of the batched 1-of-k OR-proofs (zkp_or_mi355x.h, zkp_or_toolbox.h): a Cramer-Damgard-Schoenmakers disjunction of k
// instances of one statement, for the host and the device.  g++ (host/or_proof.cpp, tests/host/or_proof_host_main.cpp) and hipcc compile
// the same text; the kernels at the end are one lane per item over these functions.
//
// Rule of this file: nothing that reaches a branch condition, a trip count or an address depends on `real` (which branch the witness
// satisfies), on a secret, on a drawn scalar or on entropy.  Selects are word-wise with an arithmetic mask (or_eq_mask: no comparison),
// the real branch is assembled, multiplied and hashed exactly as the simulated ones, and the draws of the real branch are made and
// discarded.  Public are k, N, the statement, the points, the STROBE positions, and in the _dev forms the validity bit real < k.
//
// Layouts (proof j, branch b, secret i; m secrets, nc constraints, T right-hand-side terms, nterm = T + nc):
//   drawn   [N][m + k (m + 1)][32]   blind[0..m), then per branch c'[b], s'[b][0..m): the witness RNG's output in draw order
//   rows    [N][k][nterm][32]        the term path's scalars: per constraint its terms' S[b][sec], then l - C[b] for the left-hand side
//   table   [ns + k ni N][32]        the common points, then inst[b][v][j]
//   coms    [N][k][nc][32]           the commitments, in the order they are appended
// Rows move as two 16-byte accesses on the device: every row pointer is 16-byte aligned there.
#pragma once
#include <stdint.h>
#include <string.h>
#include "sc25519.h"
#include "strobe_lane.h"

namespace zkp {

constexpr uint32_t OR_MAX_BRANCHES = 64;
constexpr uint32_t OR_LHS = 0xffffffffu;            // term_sec of a constraint's left-hand-side term

// all ones when a == b, without a comparison: x | -x has its top bit set exactly when x != 0
ZKP_HD uint32_t or_eq_mask(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  return ((x | (0u - x)) >> 31) - 1u;
}
// mask ? a : b, word by word
ZKP_HD void or_select(sc& r, uint32_t mask, const sc& a, const sc& b) {
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = b.v[i] ^ (mask & (a.v[i] ^ b.v[i]));
}
ZKP_HD void or_row_load(sc& r, const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
  r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
  r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
#else
  memcpy(r.v, p, 32);
#endif
}
ZKP_HD void or_row_store(uint8_t* p, const sc& r) {
#ifdef __HIP_DEVICE_COMPILE__
  reinterpret_cast<uint4*>(p)[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
#else
  memcpy(p, r.v, 32);
#endif
}

// The statement as the items read it.  Point ids: common points 0 .. ns - 1, instance points ns .. ns + ni - 1 (zkp_fused_statement's).
// Label ids: 0 = the proof label, 1 + i = secret i, 1 + m + p = point id p.
struct or_stmt {
  uint32_t m, ns, ni, nc, nterm, k, N, n_labels;
  const uint32_t* term_sec;      // [nterm] secret of each term, OR_LHS for a left-hand side
  const uint32_t* term_pt;       // [nterm] point id of each term
  const uint32_t* msm_off;       // [nc + 1] first term of constraint c among the nterm terms of a (proof, branch)
  const uint32_t* lhs_label;     // [nc] label id of constraint c's left-hand side
  const uint32_t* inst_order;    // [ni] instance ranks (point id - ns) in allocation order
  const uint32_t* common_order;  // [ns] common point ids in allocation order
  const uint32_t* lab_off;       // [n_labels] first word of label i in lab_w
  const uint32_t* lab_len;       // [n_labels] its length in bytes
  const uint64_t* lab_w;         // the labels' bytes, each followed by one spare word (strobe_label_fetch)
};
ZKP_HD size_t or_drawn_count(uint32_t m, uint32_t k) { return (size_t)m + (size_t)k * (m + 1); }
// the table row of point id p for (proof j, branch b): a function of public values alone
ZKP_HD uint32_t or_table_row(const or_stmt& s, uint32_t p, uint32_t b, uint32_t j) {
  return p < s.ns ? p : s.ns + (b * s.ni + (p - s.ns)) * s.N + j;
}

// ---- the CSR arrays of the term path: (statement, k, N) alone ------------------------------------------------------------------
// MSM (j, b, c) = terms [off, off + len) of the (j, b) block; off has N k nc + 1 entries, the last written by item (N - 1, k - 1).
ZKP_HD void or_plan_item(const or_stmt& s, uint32_t j, uint32_t b, uint32_t* off, uint32_t* pidx) {
  const uint32_t blk = j * s.k + b, t0 = blk * s.nterm;
  for (uint32_t c = 0; c < s.nc; ++c) off[blk * s.nc + c] = t0 + s.msm_off[c];
  if (blk + 1 == s.N * s.k) off[(blk + 1) * s.nc] = t0 + s.nterm;
  for (uint32_t t = 0; t < s.nterm; ++t) pidx[t0 + t] = or_table_row(s, s.term_pt[t], b, j);
}

// ---- the prover -------------------------------------------------------------------------------------------------------------------
// The witnesses of the nonce RNG: the m secrets as given, then `real` as 32 little-endian bytes.  wit = [m + 1][32] of proof j.
ZKP_HD void or_witness_item(uint32_t m, const uint8_t* secrets_j, uint32_t real, uint8_t* wit) {
  sc x;
  for (uint32_t i = 0; i < m; ++i) {
    or_row_load(x, secrets_j + 32 * (size_t)i);
    or_row_store(wit + 32 * (size_t)i, x);
  }
  sc_zero(x);
  x.v[0] = real;
  or_row_store(wit + 32 * (size_t)m, x);
}
// rows of (proof, branch b):  S[b][sec] = is_b ? blind[sec] : s'[b][sec],  l - C[b] with C[b] = is_b ? 0 : c'[b]
ZKP_HD void or_assemble_item(const or_stmt& s, uint32_t b, uint32_t real, const uint8_t* drawn_j, uint8_t* rows_jb) {
  const uint32_t mask = or_eq_mask(b, real);
  const uint8_t* sim = drawn_j + 32 * ((size_t)s.m + (size_t)b * (s.m + 1));      // c'[b], s'[b][..]
  sc zero, c, negc;
  sc_zero(zero);
  or_row_load(c, sim);
  or_select(c, mask, zero, c);
  sc_neg(negc, c);
  for (uint32_t t = 0; t < s.nterm; ++t) {
    const uint32_t sec = s.term_sec[t];                                             // public
    sc row = negc;
    if (sec != OR_LHS) {
      sc blind, sp;
      or_row_load(blind, drawn_j + 32 * (size_t)sec);
      or_row_load(sp, sim + 32 * ((size_t)sec + 1));
      or_select(row, mask, blind, sp);
    }
    or_row_store(rows_jb + 32 * (size_t)t, row);
  }
}
// c_real = c - sum_b C[b];  challenges[b] = is_b ? c_real : c'[b];  responses[b][i] = is_b ? blind[i] + c_real x_i : s'[b][i].
// keep = 0 zeroes every row (a proof whose points did not decode, or real >= k in the _dev forms): public.
ZKP_HD void or_respond_item(const or_stmt& s, uint32_t real, const uint8_t* drawn_j, const uint8_t* secrets_j, const uint8_t* c_j, uint32_t keep,
                            uint8_t* chal_j, uint8_t* resp_j) {
  const uint32_t km = 0u - (keep & 1u);
  sc zero, sum, c, c_real;
  sc_zero(zero);
  sc_zero(sum);
  for (uint32_t b = 0; b < s.k; ++b) {
    sc cb;
    or_row_load(cb, drawn_j + 32 * ((size_t)s.m + (size_t)b * (s.m + 1)));
    or_select(cb, or_eq_mask(b, real), zero, cb);
    sc_add(sum, sum, cb);
  }
  or_row_load(c, c_j);
  sc_neg(sum, sum);
  sc_add(c_real, c, sum);
  for (uint32_t b = 0; b < s.k; ++b) {
    sc cb;
    or_row_load(cb, drawn_j + 32 * ((size_t)s.m + (size_t)b * (s.m + 1)));
    or_select(cb, or_eq_mask(b, real), c_real, cb);
    or_select(cb, km, cb, zero);
    or_row_store(chal_j + 32 * (size_t)b, cb);
  }
  for (uint32_t i = 0; i < s.m; ++i) {
    sc x, blind, r;
    or_row_load(x, secrets_j + 32 * (size_t)i);
    or_row_load(blind, drawn_j + 32 * (size_t)i);
    sc_muladd(r, c_real, x, blind);                                                 // any 256-bit x: (x mod l) c_real + blind
    for (uint32_t b = 0; b < s.k; ++b) {
      sc sp;
      or_row_load(sp, drawn_j + 32 * ((size_t)s.m + (size_t)b * (s.m + 1) + 1 + i));
      or_select(sp, or_eq_mask(b, real), r, sp);
      or_select(sp, km, sp, zero);
      or_row_store(resp_j + 32 * ((size_t)b * s.m + i), sp);
    }
  }
}

// ---- the verifier (everything it reads is public) ---------------------------------------------------------------------------------
// rows of (proof, branch b) from (responses[b], l - challenges[b]); returns 1 when the challenge or a response is not below l
ZKP_HD uint32_t or_check_item(const or_stmt& s, const uint8_t* chal_jb, const uint8_t* resp_jb, uint8_t* rows_jb) {
  sc c, negc;
  or_row_load(c, chal_jb);
  uint32_t bad = sc_not_canonical(c.v);
  sc_neg(negc, c);
  for (uint32_t i = 0; i < s.m; ++i) {
    sc r;
    or_row_load(r, resp_jb + 32 * (size_t)i);
    bad |= sc_not_canonical(r.v);
  }
  for (uint32_t t = 0; t < s.nterm; ++t) {
    const uint32_t sec = s.term_sec[t];
    sc row = negc;
    if (sec != OR_LHS) or_row_load(row, resp_jb + 32 * (size_t)sec);
    or_row_store(rows_jb + 32 * (size_t)t, row);
  }
  return bad;
}
// 0 = accepted: sum_b challenges[b] == c, every scalar canonical (flags_j [k]), no point refused by the binding (rejected), every MSM's
// points decoded (msm_status_j [k nc])
ZKP_HD uint8_t or_verdict_item(const or_stmt& s, const uint8_t* chal_j, const uint8_t* c_j, const uint8_t* flags_j, uint32_t rejected,
                               const uint8_t* msm_status_j) {
  sc sum, c;
  sc_zero(sum);
  uint32_t bad = rejected;
  for (uint32_t b = 0; b < s.k; ++b) {
    sc cb;
    or_row_load(cb, chal_j + 32 * (size_t)b);
    bad |= flags_j[b];
    if (!flags_j[b]) sc_add(sum, sum, cb);                                          // (sc_add wants operands below l)
  }
  for (uint32_t i = 0; i < s.k * s.nc; ++i) bad |= msm_status_j[i];
  or_row_load(c, c_j);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= sum.v[i] ^ c.v[i];
  return (uint8_t)((bad | diff) != 0);
}

// ---- the transcripts: two walks of strobe_lane.h's part walker ----------------------------------------------------------------------
// An append_message(label, data) is a frame of nine slots: header of meta_ad, the Merlin label in two values (at most 16 bytes),
// u32le(length), header of ad, and four data slots -- a constant of up to 32 bytes in four values, or a statement label, or 32 bytes of
// memory in the first and nothing in the others.  An empty slot is a part of 0 bytes.
constexpr uint64_t or_le(const char* s, int n) {
  uint64_t x = 0;
  for (int i = 0; i < n && i < 8; ++i) x |= (uint64_t)(uint8_t)s[i] << (8 * i);
  return x;
}
enum : uint32_t { OR_D_CONST, OR_D_LABEL, OR_D_MEM };
struct or_frame {
  uint64_t lab0, lab1;
  uint32_t lab_len, kind, len, which;        // len: the data's length; which: OR_D_LABEL's label id
  uint64_t d0, d1, d2, d3;                   // OR_D_CONST
  const uint8_t* src;                        // OR_D_MEM
};
constexpr uint32_t OR_FRAME_SLOTS = 9;
ZKP_HD strobe_part or_frame_part(const or_frame& f, uint32_t r) {
  const uint32_t l0 = f.lab_len < 8 ? f.lab_len : 8, l1 = f.lab_len - l0;
  if (r == 0) return strobe_part_hdr(STROBE_M | STROBE_A);
  if (r == 1) return strobe_part_val(f.lab0, l0);
  if (r == 2) return strobe_part_val(f.lab1, l1);
  if (r == 3) return strobe_part_val(f.len, 4);
  if (r == 4) return strobe_part_hdr(STROBE_A);
  if (f.kind == OR_D_LABEL) return strobe_part_label(f.which, r == 5 ? f.len : 0);
  if (f.kind == OR_D_MEM) return strobe_part_make(SP_AD, 0, r == 5 ? 32 : 0, 0, f.src, nullptr);
  const uint32_t done = 8 * (r - 5), left = f.len > done ? f.len - done : 0;
  return strobe_part_val(r == 5 ? f.d0 : r == 6 ? f.d1 : r == 7 ? f.d2 : f.d3, left < 8 ? left : 8);
}
ZKP_HD or_frame or_frame_make(uint64_t lab0, uint64_t lab1, uint32_t lab_len, uint32_t kind, uint32_t len, uint32_t which, const uint8_t* src) {
  or_frame f;
  f.lab0 = lab0; f.lab1 = lab1; f.lab_len = lab_len; f.kind = kind; f.len = len; f.which = which;
  f.d0 = f.d1 = f.d2 = f.d3 = 0;
  f.src = src;
  return f;
}
// the two frames of append_point_var / append_blinding_commitment: (kind, statement label), ("val", 32 bytes)
ZKP_HD or_frame or_point_frame(const or_stmt& s, uint32_t half, uint64_t kind, uint32_t kind_len, uint32_t label, const uint8_t* enc) {
  if (half == 0) return or_frame_make(kind, 0, kind_len, OR_D_LABEL, s.lab_len[label], label, nullptr);
  return or_frame_make(or_le("val", 3), 0, 3, OR_D_MEM, 32, 0, enc);
}

// The binding: domain_sep(proof label); append_message("or-branches", u32le(k)); append_scalar_var per secret; append_point_var for the
// instance points of branch 0 .. k - 1 in allocation order, then for the common points.
struct or_bind_seq {
  const or_stmt& s;
  const uint8_t* table;
  uint32_t j;
  ZKP_HD uint32_t frames() const { return 3 + s.m + 2 * (s.k * s.ni + s.ns); }
  ZKP_HD or_frame frame(uint32_t f) const {
    if (f == 0) {
      or_frame x = or_frame_make(or_le("dom-sep", 7), 0, 7, OR_D_CONST, 27, 0, nullptr);
      x.d0 = or_le("schnorrz", 8); x.d1 = or_le("kp/1.0/r", 8); x.d2 = or_le("istretto", 8); x.d3 = or_le("255", 3);
      return x;
    }
    if (f == 1) return or_frame_make(or_le("dom-sep", 7), 0, 7, OR_D_LABEL, s.lab_len[0], 0, nullptr);
    if (f == 2) {
      or_frame x = or_frame_make(or_le("or-branc", 8), or_le("hes", 3), 11, OR_D_CONST, 4, 0, nullptr);
      x.d0 = s.k;
      return x;
    }
    if (f < 3 + s.m) return or_frame_make(or_le("scvar", 5), 0, 5, OR_D_LABEL, s.lab_len[f - 2], f - 2, nullptr);
    const uint32_t q = f - 3 - s.m, pi = q >> 1, n_inst = s.k * s.ni;
    uint32_t p, row;
    if (pi < n_inst) {
      const uint32_t b = pi / s.ni, v = s.inst_order[pi - b * s.ni];
      p = s.ns + v;
      row = or_table_row(s, p, b, j);
    } else {
      p = s.common_order[pi - n_inst];
      row = p;
    }
    return or_point_frame(s, q & 1, or_le("ptvar", 5), 5, 1 + s.m + p, table + 32 * (size_t)row);
  }
  ZKP_HD strobe_part part(uint32_t idx) const {
    const uint32_t f = idx / OR_FRAME_SLOTS;
    if (f >= frames()) return strobe_part_end();
    return or_frame_part(frame(f), idx - f * OR_FRAME_SLOTS);
  }
  ZKP_HD const uint64_t* label(uint32_t i) const { return s.lab_w + s.lab_off[i]; }
  ZKP_HD void wide(uint32_t, const uint64_t*) const {}
};
// the validating binding refuses a proof with an instance or common point of 32 zero bytes (validate_and_append_point_var)
ZKP_HD bool or_bind_rejects(const or_stmt& s, const uint8_t* table, uint32_t j) {
  bool bad = false;
  for (uint32_t p = 0; p < s.ns; ++p) bad |= strobe_is_identity(table + 32 * (size_t)p);
  for (uint32_t b = 0; b < s.k; ++b)
    for (uint32_t v = 0; v < s.ni; ++v) bad |= strobe_is_identity(table + 32 * (size_t)or_table_row(s, s.ns + v, b, j));
  return bad;
}

// The commitments and the challenge: append_blinding_commitment(name of lhs(c), com[b][c]) for b, c in order, then get_challenge("chal")
// -> out[32]
struct or_challenge_seq {
  const or_stmt& s;
  const uint8_t* coms_j;           // [k][nc][32]
  uint8_t* out;
  ZKP_HD strobe_part part(uint32_t idx) const {
    const uint32_t f = idx / OR_FRAME_SLOTS, F = 2 * s.k * s.nc;
    if (f < F) {
      const uint32_t pi = f >> 1, c = pi % s.nc;
      return or_frame_part(or_point_frame(s, f & 1, or_le("blindcom", 8), 8, s.lhs_label[c], coms_j + 32 * (size_t)pi), idx - f * OR_FRAME_SLOTS);
    }
    const uint32_t r = idx - F * OR_FRAME_SLOTS;
    if (r == 0) return strobe_part_hdr(STROBE_M | STROBE_A);
    if (r == 1) return strobe_part_val(or_le("chal", 4), 4);
    if (r == 2) return strobe_part_val(64, 4);
    if (r == 3) return strobe_part_hdr(STROBE_I | STROBE_A | STROBE_C);
    if (r == 4) return strobe_part_make(SP_PRF64, 0, 64, 0, nullptr, nullptr);
    return strobe_part_end();
  }
  ZKP_HD const uint64_t* label(uint32_t i) const { return s.lab_w + s.lab_off[i]; }
  ZKP_HD void wide(uint32_t, const uint64_t w[8]) const { strobe_wide_to_scalar(w, out); }
};

// ---- the kernels: one lane per item -------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
constexpr int OR_BLOCK = 256;

// off [N k nc + 1] and pidx [N k nterm]: one lane per (proof, branch)
__global__ void __launch_bounds__(OR_BLOCK) k_or_plan(const or_stmt s, uint32_t* __restrict__ off, uint32_t* __restrict__ pidx) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i >= s.N * s.k) return;
  or_plan_item(s, i / s.k, i % s.k, off, pidx);
}
// wit [N][m + 1][32]: one lane per proof
__global__ void __launch_bounds__(OR_BLOCK) k_or_witness(const or_stmt s, const uint8_t* __restrict__ secrets, const uint8_t* __restrict__ real,
                                                         uint8_t* __restrict__ wit) {
  const uint32_t j = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (j >= s.N) return;
  or_witness_item(s.m, secrets + 32 * (size_t)s.m * j, real[j], wit + 32 * (size_t)(s.m + 1) * j);
}
// rows [N][k][nterm][32]: one lane per (proof, branch)
__global__ void __launch_bounds__(OR_BLOCK) k_or_assemble(const or_stmt s, const uint8_t* __restrict__ real, const uint8_t* __restrict__ drawn,
                                                          uint8_t* __restrict__ rows) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i >= s.N * s.k) return;
  const uint32_t j = i / s.k, b = i - j * s.k;
  or_assemble_item(s, b, real[j], drawn + 32 * or_drawn_count(s.m, s.k) * j, rows + 32 * (size_t)s.nterm * i);
}
// challenges [N][k][32], responses [N][k][m][32], status [N]: one lane per proof.  A proof one of whose MSMs met a point that does not
// decode, or whose real is k or more, gets status 1 and zero rows.
__global__ void __launch_bounds__(OR_BLOCK) k_or_respond(const or_stmt s, const uint8_t* __restrict__ real, const uint8_t* __restrict__ drawn,
                                                         const uint8_t* __restrict__ secrets, const uint8_t* __restrict__ c,
                                                         const uint8_t* __restrict__ msm_status, uint8_t* __restrict__ chal,
                                                         uint8_t* __restrict__ resp, uint8_t* __restrict__ status) {
  const uint32_t j = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (j >= s.N) return;
  const uint32_t r = real[j];
  uint32_t bad = r >= s.k;                                                          // the validity bit: public
  for (uint32_t i = 0; i < s.k * s.nc; ++i) bad |= msm_status[(size_t)s.k * s.nc * j + i];
  bad = bad != 0;
  or_respond_item(s, r, drawn + 32 * or_drawn_count(s.m, s.k) * j, secrets + 32 * (size_t)s.m * j, c + 32 * (size_t)j, 1u - bad,
                  chal + 32 * (size_t)s.k * j, resp + 32 * (size_t)s.k * s.m * j);
  status[j] = (uint8_t)bad;
}
// the verifier's rows and canonical flags [N][k]: one lane per (proof, branch)
__global__ void __launch_bounds__(OR_BLOCK) k_or_check(const or_stmt s, const uint8_t* __restrict__ chal, const uint8_t* __restrict__ resp,
                                                       uint8_t* __restrict__ rows, uint8_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i >= s.N * s.k) return;
  flags[i] = (uint8_t)or_check_item(s, chal + 32 * (size_t)i, resp + 32 * (size_t)s.m * i, rows + 32 * (size_t)s.nterm * i);
}
// results [N]: one lane per proof
__global__ void __launch_bounds__(OR_BLOCK) k_or_verdict(const or_stmt s, const uint8_t* __restrict__ chal, const uint8_t* __restrict__ c,
                                                         const uint8_t* __restrict__ flags, const uint8_t* __restrict__ rejected,
                                                         const uint8_t* __restrict__ msm_status, uint8_t* __restrict__ results) {
  const uint32_t j = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (j >= s.N) return;
  results[j] = or_verdict_item(s, chal + 32 * (size_t)s.k * j, c + 32 * (size_t)j, flags + (size_t)s.k * j, rejected[j],
                               msm_status + (size_t)s.k * s.nc * j);
}

// The statement's fields are live across a walk and uniform: as kernel arguments they would sit in scalar registers, of which the walk
// leaves too few (strobe_park of transcript_kernels.h): the walks read a copy parked in vector registers.
__device__ __forceinline__ or_stmt or_stmt_park(const or_stmt& a) {
  or_stmt s;
  s.m = strobe_park(a.m); s.ns = strobe_park(a.ns); s.ni = strobe_park(a.ni); s.nc = strobe_park(a.nc);
  s.nterm = strobe_park(a.nterm); s.k = strobe_park(a.k); s.N = strobe_park(a.N); s.n_labels = strobe_park(a.n_labels);
  s.term_sec = strobe_park(a.term_sec); s.term_pt = strobe_park(a.term_pt); s.msm_off = strobe_park(a.msm_off);
  s.lhs_label = strobe_park(a.lhs_label); s.inst_order = strobe_park(a.inst_order); s.common_order = strobe_park(a.common_order);
  s.lab_off = strobe_park(a.lab_off); s.lab_len = strobe_park(a.lab_len); s.lab_w = strobe_park(a.lab_w);
  return s;
}

// The two transcript launches, in the shape of k_strobe_append_points: a wavefront per workgroup, the state an LDS column per lane,
// grid-stride; transcripts at any mix of positions.  A blob whose position byte is 166 or more stays as it is and counts as rejected.
// k_or_bind: the binding; validate != 0 refuses a proof with an identity encoding among its points (rejected[j] = 1, blob unchanged).
__global__ void __launch_bounds__(STROBE_BLOCK)
k_or_bind(const or_stmt arg, uint8_t* __restrict__ ts, const uint8_t* __restrict__ table, uint32_t validate, uint8_t* __restrict__ rejected) {
  __shared__ uint64_t S[25 * STROBE_BLOCK];
  const or_stmt s = or_stmt_park(arg);
  const uint32_t step = strobe_park(gridDim.x * STROBE_BLOCK);
  ts = strobe_park(ts);
  table = strobe_park(table);
  rejected = strobe_park(rejected);
  validate = strobe_park(validate);
  for (uint32_t j = blockIdx.x * STROBE_BLOCK + threadIdx.x; j < s.N; j += step) {
    strobe_lane L{S + threadIdx.x, STROBE_BLOCK, 0, 0, 0};
    uint64_t* blob = reinterpret_cast<uint64_t*>(ts + 208 * (size_t)j);
    strobe_load(L, blob);
    const bool bad = !strobe_valid(L) || (validate && or_bind_rejects(s, table, j));
    if (!bad) {
      or_bind_seq seq{s, table, j};
      strobe_walk(L, seq);
      strobe_store(L, blob, strobe_tail(L));
    }
    rejected[j] = bad ? 1 : 0;
  }
}
// k_or_challenge: the k nc commitments appended, then c = get_challenge("chal") -> c [N][32]; skip[j] != 0 leaves blob j and writes zeros
__global__ void __launch_bounds__(STROBE_BLOCK)
k_or_challenge(const or_stmt arg, uint8_t* __restrict__ ts, const uint8_t* __restrict__ coms, const uint8_t* __restrict__ skip, uint8_t* __restrict__ c) {
  __shared__ uint64_t S[25 * STROBE_BLOCK];
  const or_stmt s = or_stmt_park(arg);
  const uint32_t step = strobe_park(gridDim.x * STROBE_BLOCK);
  ts = strobe_park(ts);
  coms = strobe_park(coms);
  skip = strobe_park(skip);
  c = strobe_park(c);
  for (uint32_t j = blockIdx.x * STROBE_BLOCK + threadIdx.x; j < s.N; j += step) {
    strobe_lane L{S + threadIdx.x, STROBE_BLOCK, 0, 0, 0};
    uint64_t* blob = reinterpret_cast<uint64_t*>(ts + 208 * (size_t)j);
    uint8_t* o = c + 32 * (size_t)j;
    strobe_load(L, blob);
    if (strobe_valid(L) && !skip[j]) {
      or_challenge_seq seq{s, coms + 32 * (size_t)s.k * s.nc * j, o};
      strobe_walk(L, seq);
      strobe_store(L, blob, strobe_tail(L));
    } else {
      sc zero;
      sc_zero(zero);
      or_row_store(o, zero);
    }
  }
}
#endif  // __HIPCC__

}  // namespace zkp
