// The statement of an OR-proof call as or_lane.h's items read it (or_stmt), packed into ONE blob of 32-bit words followed by the labels'
// 64-bit words, so that the device flow uploads it with one copy and the host backend reads it in place.  Host code (hipcc's host pass and
// g++); built from a zkp_fused_statement on every call: it is a few hundred bytes.
#pragma once
#include <cstring>
#include <vector>

#include "../../include/zkp_or_mi355x.h"
#include "or_lane.h"

namespace zkp {

struct or_meta {
  std::vector<uint64_t> blob;        // (64-bit elements: the label words want 8-byte alignment)
  uint32_t m = 0, ns = 0, ni = 0, nc = 0, nterm = 0, n_labels = 0;
  size_t o_term_sec = 0, o_term_pt = 0, o_msm_off = 0, o_lhs_label = 0, o_inst_order = 0, o_common_order = 0, o_lab_off = 0, o_lab_len = 0, o_lab_w = 0;
  size_t bytes() const { return blob.size() * 8; }
  // the item view over a copy of the blob at `base` (device or host memory, 8-byte aligned)
  or_stmt view(const void* base, uint32_t k, uint32_t N) const {
    const char* p = static_cast<const char*>(base);
    auto u32 = [&](size_t o) { return reinterpret_cast<const uint32_t*>(p + o); };
    or_stmt s;
    s.m = m; s.ns = ns; s.ni = ni; s.nc = nc; s.nterm = nterm; s.k = k; s.N = N; s.n_labels = n_labels;
    s.term_sec = u32(o_term_sec); s.term_pt = u32(o_term_pt); s.msm_off = u32(o_msm_off); s.lhs_label = u32(o_lhs_label);
    s.inst_order = u32(o_inst_order); s.common_order = u32(o_common_order); s.lab_off = u32(o_lab_off); s.lab_len = u32(o_lab_len);
    s.lab_w = reinterpret_cast<const uint64_t*>(p + o_lab_w);
    return s;
  }
};

// false: the statement is malformed (a NULL array or label, an index out of range, a label longer than STROBE_LABEL_MAX bytes, alloc_order
// not a permutation of the point ids)
inline bool or_meta_build(const zkp_fused_statement* st, or_meta& M) {
  if (!st || !st->label) return false;
  const zkp_batch_statement& sh = st->shape;
  const uint32_t m = sh.n_secrets, ns = sh.n_static, ni = sh.n_instance, nc = sh.n_constraints;
  if ((uint64_t)ns + ni > 0x00ffffffu || m > 0x00ffffffu || nc > 0x00ffffffu) return false;
  const uint32_t np = ns + ni;
  if (nc && (!sh.cons_lhs || !sh.cons_off)) return false;
  if (m && !st->secret_labels) return false;
  if (np && (!st->point_labels || !st->alloc_order)) return false;
  const uint32_t T = nc ? sh.cons_off[nc] : 0;
  if (T > 0x00ffffffu || (T && (!sh.cons_sc || !sh.cons_pt))) return false;
  if (nc && sh.cons_off[0] != 0) return false;
  std::vector<uint32_t> term_sec, term_pt, msm_off, lhs_label, inst_order, common_order;
  for (uint32_t c = 0; c < nc; ++c) {
    if (sh.cons_off[c + 1] < sh.cons_off[c] || sh.cons_off[c + 1] > T || sh.cons_lhs[c] >= np) return false;
    msm_off.push_back((uint32_t)term_sec.size());
    for (uint32_t t = sh.cons_off[c]; t < sh.cons_off[c + 1]; ++t) {
      if (sh.cons_sc[t] >= m || sh.cons_pt[t] >= np) return false;
      term_sec.push_back(sh.cons_sc[t]);
      term_pt.push_back(sh.cons_pt[t]);
    }
    term_sec.push_back(OR_LHS);
    term_pt.push_back(sh.cons_lhs[c]);
    lhs_label.push_back(1 + m + sh.cons_lhs[c]);
  }
  msm_off.push_back((uint32_t)term_sec.size());
  std::vector<uint8_t> seen(np, 0);
  for (uint32_t v = 0; v < np; ++v) {
    const uint32_t p = st->alloc_order[v];
    if (p >= np || seen[p]) return false;
    seen[p] = 1;
    if (p < ns) common_order.push_back(p);
    else inst_order.push_back(p - ns);
  }
  std::vector<const char*> labels;
  labels.push_back(st->label);
  for (uint32_t i = 0; i < m; ++i) labels.push_back(st->secret_labels[i]);
  for (uint32_t p = 0; p < np; ++p) labels.push_back(st->point_labels[p]);
  std::vector<uint32_t> lab_off, lab_len;
  std::vector<uint64_t> lab_w;
  for (const char* l : labels) {
    if (!l) return false;
    const size_t n = std::strlen(l);
    if (n > STROBE_LABEL_MAX) return false;
    lab_off.push_back((uint32_t)lab_w.size());
    lab_len.push_back((uint32_t)n);
    const size_t words = n / 8 + 2;                                  // the label, zero padded, and the spare word strobe_label_fetch may read
    const size_t at = lab_w.size();
    lab_w.resize(at + words, 0);
    std::memcpy(lab_w.data() + at, l, n);
  }
  M = or_meta();
  M.m = m; M.ns = ns; M.ni = ni; M.nc = nc; M.nterm = (uint32_t)term_sec.size(); M.n_labels = (uint32_t)labels.size();
  std::vector<uint32_t> words;
  auto put = [&](const std::vector<uint32_t>& v) {
    const size_t o = words.size() * 4;
    words.insert(words.end(), v.begin(), v.end());
    words.push_back(0);                                              // (no region is empty: a view's pointer is always inside the blob)
    return o;
  };
  M.o_term_sec = put(term_sec); M.o_term_pt = put(term_pt); M.o_msm_off = put(msm_off); M.o_lhs_label = put(lhs_label);
  M.o_inst_order = put(inst_order); M.o_common_order = put(common_order); M.o_lab_off = put(lab_off); M.o_lab_len = put(lab_len);
  if (words.size() & 1) words.push_back(0);
  M.o_lab_w = words.size() * 4;
  M.blob.assign(words.size() / 2 + lab_w.size(), 0);
  std::memcpy(M.blob.data(), words.data(), words.size() * 4);
  std::memcpy(reinterpret_cast<char*>(M.blob.data()) + M.o_lab_w, lab_w.data(), lab_w.size() * 8);
  return true;
}

// the sizes a call derives from (statement, k, N); false: k, N or the products are out of range
struct or_sizes { uint32_t n_blocks, n_msm, n_terms, n_points; size_t drawn; };
inline bool or_sizes_of(const or_meta& M, uint32_t k, uint32_t N, or_sizes& z) {
  if (k < 1 || k > OR_MAX_BRANCHES || N > 0x7fffffffu) return false;
  const uint64_t blocks = (uint64_t)N * k, terms = blocks * M.nterm, points = (uint64_t)M.ns + blocks * M.ni;
  if (terms >= (1ull << 32) || points >= (1ull << 32) || blocks * M.nc >= (1ull << 32)) return false;
  z.n_blocks = (uint32_t)blocks;
  z.n_msm = (uint32_t)(blocks * M.nc);
  z.n_terms = (uint32_t)terms;
  z.n_points = (uint32_t)points;
  z.drawn = or_drawn_count(M.m, k);
  return true;
}

}  // namespace zkp
