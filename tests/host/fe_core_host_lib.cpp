// Host build of the field core of zkp_amd/csrc/fe25519.h (fe_mul, fe_sq, fe_sqn and the chains on top) next to the formulation it
// replaced, for tests/test_host_fe_core.py and tests/test_gpu_fe_core.py: raw limbs in, raw limbs and canonical words out.
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
// the chains: op 0 pow22523, 1 invert; canonical words out
void t_core_chain(int op, const uint32_t* a, const uint32_t* ub_a, uint32_t* words) {
  fe x, r;
  load(x, a, ub_a);
  if (op == 0) fe_pow22523(r, x); else fe_invert(r, x);
  fe_towords(words, r);
}
}
