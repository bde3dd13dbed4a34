// Host build of the field core of zkp_amd/csrc/fe25519.h (fe_mul, fe_sq, fe_sqn and the chains on top) next to the formulation it
// replaced, for tests/test_host_fe_core.py and tests/test_gpu_fe_core.py: raw limbs in, raw limbs and canonical words out; and the
// point arithmetic of quad.h lane by lane over the same header (t_quad_probe, for tests/test_gpu_row_quad_probe.py).
// Built plain and with -DZKP_FE_TRACK, where the operands carry the bounds of their CLASS (not of their values), so a column or a
// carry that could overflow for some member of the class aborts.
#include "../../zkp_amd/csrc/fe_constants.h"
#include <cstring>
using namespace zkp;

// ---- the earlier formulation: every column summed on its own, then the carries rippled down with a 64-bit add per column --------
static void ref_reduce_columns(uint32_t r[9], uint64_t c[9]) {
  for (int k = 0; k < 8; ++k) {
    c[k + 1] += c[k] >> 29;
    r[k] = (uint32_t)c[k] & FE_M29;
  }
  r[8] = (uint32_t)c[8] & FE_M23;
  const uint64_t t = c[8] >> 23;
  const uint64_t c0 = (uint64_t)r[0] + 19ull * (uint32_t)t;
  r[0] = (uint32_t)c0 & FE_M29;
  r[1] += (uint32_t)(c0 >> 29) + 152u * (uint32_t)(t >> 32);
}
static void ref_mul(uint32_t r[9], const uint32_t a[9], const uint32_t b[9]) {
  uint64_t c[17];
  for (int k = 0; k < 17; ++k) c[k] = 0;
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) c[i + j] += (uint64_t)a[i] * b[j];
  for (int k = 0; k < 8; ++k) {
    c[k] += 1216ull * (uint32_t)c[k + 9];
    c[k + 1] += 9728ull * (uint32_t)(c[k + 9] >> 32);
  }
  ref_reduce_columns(r, c);
}
static void ref_sqn(uint32_t r[9], const uint32_t a[9], int n) {
  uint32_t x[9], y[9];
  memcpy(x, a, sizeof(x));
  for (int i = 0; i < n; ++i) { ref_mul(y, x, x); memcpy(x, y, sizeof(x)); }
  memcpy(r, x, sizeof(x));
}

static void load(fe& x, const uint32_t* limbs, const uint32_t* ub) {
  for (int i = 0; i < 9; ++i) x.v[i] = limbs[i];
#ifdef ZKP_FE_TRACK
  for (int i = 0; i < 9; ++i) x.ub[i] = ub[i];
#endif
  (void)ub;
}

extern "C" {
int t_core_tracked(void) {
#ifdef ZKP_FE_TRACK
  return 1;
#else
  return 0;
#endif
}
// op: 0 a*b, 1 a^2, 2 a^(2^n) through fe_sqn.  a, b = raw limbs, ub_a, ub_b = the inclusive limb bounds of their classes.
// out_new / out_ref = the 9 limbs of the header's result and of the earlier formulation's; words_new / words_ref = their
// canonical encodings.  Returns 1 if every limb of the header's result is within the "tight" class.
int t_core_op(int op, int n, const uint32_t* a, const uint32_t* ub_a, const uint32_t* b, const uint32_t* ub_b,
              uint32_t* out_new, uint32_t* out_ref, uint32_t* words_new, uint32_t* words_ref) {
  fe x, y, r;
  load(x, a, ub_a); load(y, b, ub_b);
  if (op == 0) { fe_mul(r, x, y); ref_mul(out_ref, a, b); }
  else if (op == 1) { fe_sq(r, x); ref_mul(out_ref, a, a); }
  else { fe_sqn(r, x, n); ref_sqn(out_ref, a, n); }
  int tight = 1;
  for (int i = 0; i < 9; ++i) {
    out_new[i] = r.v[i];
    tight &= r.v[i] < (i == 8 ? (1u << 23) + (1u << 4) : (1u << 29) + (1u << 18));
  }
  fe_towords(words_new, r);
  fe q;
  uint32_t tight_ub[9];
  for (int i = 0; i < 9; ++i) tight_ub[i] = i == 8 ? (1u << 23) + (1u << 4) : (1u << 29) + (1u << 18);
  load(q, out_ref, tight_ub);
  fe_towords(words_ref, q);
  return tight;
}
// what tools/microbench/fe_probe.hip computes per record, through the host path of the header: in = [n][18] limbs (a, b),
// out = [n][6][9] limbs (a*b, b*a, a^2, a^(2^5), a^(2^10), a*d with the curve constant d); ub = [2][9] class bounds of a and b for the tracked build
void t_core_probe(uint32_t n, const uint32_t* in, const uint32_t* ub, uint32_t* out) {
  for (uint32_t i = 0; i < n; ++i) {
    fe a, b, d, r[6];
    load(a, in + 18 * (size_t)i, ub + 18 * (size_t)i); load(b, in + 18 * (size_t)i + 9, ub + 18 * (size_t)i + 9);
    fe_mul(r[0], a, b); fe_mul(r[1], b, a); fe_sq(r[2], a); fe_sqn(r[3], a, 5); fe_sqn(r[4], a, 10);
    fe_from_const(d, FE_D); fe_mul(r[5], a, d);
    for (int k = 0; k < 6; ++k)
      for (int j = 0; j < 9; ++j) out[(size_t)i * 54 + 9 * k + j] = r[k].v[j];
  }
}
// what tools/microbench/quad_probe.hip computes per record: the point arithmetic of zkp_amd/csrc/quad.h, whose four lanes are four fe
// here.  Every lane makes quad.h's calls in quad.h's order (the ones whose result its lane drops too, as the device does), a DPP
// quad_perm move is a copy between the four, and fe_pick copies the element whole, so the tracked build carries each LANE's class through
// the selections (G x H in one lane and E x F in the next), not their union.  in = [n][2][4][9] limbs (p, s), ub = [9] class bounds of all
// eight coordinates, out = [n][6][4][9] limbs: q_double(p), q_add_cached(p, s), q_add(p, s), q_to_cached(p), q_add_cached(p, niels(s)),
// q_add_cached(p, -niels(s)) with niels(s) = rows 0, 1, 3 of s as (y+x, y-x, 2dxy).
struct hquad { fe l[4]; };
static void hq_perm(hquad& r, const hquad& a, int s0, int s1, int s2, int s3) {
  const hquad t = a;
  r.l[0] = t.l[s0]; r.l[1] = t.l[s1]; r.l[2] = t.l[s2]; r.l[3] = t.l[s3];
}
static void hq_pick(hquad& r, const hquad& a, int lane) { r.l[lane] = a.l[lane]; }
#define HQ_EACH(stmt) for (int q = 0; q < 4; ++q) { stmt; }
static void hq_to_cached(hquad& r, const hquad& p) {
  hquad o, s, a, z2, t, m;
  fe d2, one;
  hq_perm(o, p, 1, 0, 3, 2);
  HQ_EACH(fe_sub(s.l[q], o.l[q], p.l[q]))
  HQ_EACH(fe_add(a.l[q], p.l[q], o.l[q]))
  HQ_EACH(fe_add(z2.l[q], p.l[q], p.l[q]))
  t = p;
  hq_pick(t, s, 0); hq_pick(t, a, 1); hq_pick(t, z2, 2);
  HQ_EACH(fe_carry(t.l[q], t.l[q]))
  fe_from_const(d2, FE_D2);
  fe_1(one);
  HQ_EACH(m.l[q] = q == 3 ? d2 : one)
  HQ_EACH(fe_mul(r.l[q], t.l[q], m.l[q]))
}
static void hq_add_cached(hquad& r, const hquad& p, const hquad& c) {
  hquad o, s, a, t, u, v, sum, d1, d2;
  hq_perm(o, p, 1, 0, 3, 2);
  HQ_EACH(fe_sub(s.l[q], o.l[q], p.l[q]))
  HQ_EACH(fe_add(a.l[q], p.l[q], o.l[q]))
  t = p;
  hq_pick(t, s, 0); hq_pick(t, a, 1);
  HQ_EACH(fe_mul(u.l[q], t.l[q], c.l[q]))
  hq_perm(o, u, 1, 0, 3, 2);
  HQ_EACH(fe_add(sum.l[q], u.l[q], o.l[q]))
  HQ_EACH(fe_sub(d1.l[q], o.l[q], u.l[q]))
  HQ_EACH(fe_sub(d2.l[q], u.l[q], o.l[q]))
  v = sum;
  hq_pick(v, d1, 0); hq_pick(v, d2, 2);
  HQ_EACH(fe_carry(v.l[q], v.l[q]))
  hq_perm(o, v, 2, 0, 3, 1);
  HQ_EACH(fe_mul(u.l[q], v.l[q], o.l[q]))
  hq_perm(r, u, 0, 3, 2, 1);
}
static void hq_double(hquad& r, const hquad& p) {
  hquad x, y, w, t, s, a, b, h, g, e, f, ee, ff, m1, m2;
  hq_perm(x, p, 0, 0, 0, 0);
  hq_perm(y, p, 1, 1, 1, 1);
  HQ_EACH(fe_add(w.l[q], x.l[q], y.l[q]))
  t = p;
  hq_pick(t, w, 3);
  HQ_EACH(fe_sq(s.l[q], t.l[q]))
  hq_perm(a, s, 0, 0, 0, 0);
  hq_perm(b, s, 1, 1, 1, 1);
  HQ_EACH(fe_add(h.l[q], b.l[q], a.l[q]))
  HQ_EACH(fe_sub(g.l[q], b.l[q], a.l[q]))
  HQ_EACH(fe_sub4(e.l[q], s.l[q], h.l[q]))
  HQ_EACH(fe_add(w.l[q], s.l[q], s.l[q]))
  HQ_EACH(fe_sub4(f.l[q], w.l[q], g.l[q]))
  HQ_EACH(fe_carry(e.l[q], e.l[q]))
  HQ_EACH(fe_carry(f.l[q], f.l[q]))
  hq_perm(ee, e, 3, 3, 3, 3);
  hq_perm(ff, f, 2, 2, 2, 2);
  m1 = ee; m2 = h;
  hq_pick(m1, g, 1); hq_pick(m1, ff, 2);
  hq_pick(m2, ff, 0); hq_pick(m2, g, 2);
  HQ_EACH(fe_mul(r.l[q], m1.l[q], m2.l[q]))
}
static void hq_load_niels(hquad& c, const fe nl[3] /*ypx, ymx, xy2d*/, int negate) {
  for (int q = 0; q < 4; ++q) {
    const fe t = nl[q == 0 ? (negate ? 0 : 1) : (q == 1 ? (negate ? 1 : 0) : 2)];
    fe two, n;
    fe_0(two);
    two.v[0] = 2;
    FE_TRACK(fe_set_ub_exact(two));
    fe_neg(n, t);
    fe_carry(n, n);
    c.l[q] = t;
    if (q == 3 && negate) c.l[q] = n;
    if (q == 2) c.l[q] = two;
  }
}
void t_quad_probe(uint32_t n, const uint32_t* in, const uint32_t* ub, uint32_t* out) {
  for (uint32_t i = 0; i < n; ++i) {
    hquad p, s, c, r[6];
    for (int q = 0; q < 4; ++q) { load(p.l[q], in + 72 * (size_t)i + 9 * q, ub); load(s.l[q], in + 72 * (size_t)i + 36 + 9 * q, ub); }
    const fe nl[3] = {s.l[0], s.l[1], s.l[3]};
    hq_double(r[0], p);
    hq_add_cached(r[1], p, s);
    hq_to_cached(c, s);
    hq_add_cached(r[2], p, c);
    hq_to_cached(r[3], p);
    hq_load_niels(c, nl, 0);
    hq_add_cached(r[4], p, c);
    hq_load_niels(c, nl, 1);
    hq_add_cached(r[5], p, c);
    for (int k = 0; k < 6; ++k)
      for (int q = 0; q < 4; ++q)
        for (int j = 0; j < 9; ++j) out[(size_t)i * 216 + 36 * k + 9 * q + j] = r[k].l[q].v[j];
  }
}
// the chains: op 0 pow22523, 1 invert; canonical words out
void t_core_chain(int op, const uint32_t* a, const uint32_t* ub_a, uint32_t* words) {
  fe x, r;
  load(x, a, ub_a);
  if (op == 0) fe_pow22523(r, x); else fe_invert(r, x);
  fe_towords(words, r);
}
}
