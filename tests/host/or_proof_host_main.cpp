// Stand-alone driver of zkp_amd/csrc/or_lane.h's assemble / respond / check / verdict items (built by tests/test_host_or_proof.py with
// g++ -fsanitize=address,undefined and run as a child process): k = 1, 2, 64 and m = 1, 11, every branch as the real one, on heap blocks
// of exactly each buffer's size, against a restatement with plain branches.  Prints "<what> <cases> <mismatches>" per check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zkp_amd/csrc/or_lane.h"

using namespace zkp;

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 7;
  g_seed ^= g_seed << 17;
  return (uint32_t)(g_seed >> 16);
}
static sc random_scalar() {
  uint32_t x[16];
  for (uint32_t& w : x) w = rnd();
  sc r;
  sc_reduce_wide(r, x);
  return r;
}
struct block {                     // a heap block of exactly n bytes: a byte past either end is the sanitizer's
  uint8_t* p;
  size_t n;
  explicit block(size_t bytes) : p((uint8_t*)std::malloc(bytes ? bytes : 1)), n(bytes) { std::memset(p, 0xa5, bytes ? bytes : 1); }
  ~block() { std::free(p); }
  block(const block&) = delete;
};
static void put(uint8_t* p, const sc& x) { std::memcpy(p, x.v, 32); }
static sc get(const uint8_t* p) {
  sc x;
  std::memcpy(x.v, p, 32);
  return x;
}
static bool same(const sc& a, const sc& b) { return std::memcmp(a.v, b.v, 32) == 0; }

int main() {
  unsigned long cases = 0, bad_rows = 0, bad_proofs = 0, bad_verdicts = 0, masks = 0, bad_masks = 0;
  for (uint32_t a = 0; a < 70; ++a)
    for (uint32_t b = 0; b < 70; ++b) {
      ++masks;
      bad_masks += or_eq_mask(a, b) != (a == b ? 0xffffffffu : 0u);
    }
  const uint32_t ks[] = {1, 2, 64}, ms[] = {1, 11};
  for (uint32_t k : ks)
    for (uint32_t m : ms) {
      // a statement of m constraints, constraint i = one term on secret (m - 1 - i), then its left-hand side
      const uint32_t nterm = 2 * m;
      std::vector<uint32_t> term_sec, term_pt(nterm, 0), msm_off;
      for (uint32_t i = 0; i < m; ++i) {
        msm_off.push_back(2 * i);
        term_sec.push_back(m - 1 - i);
        term_sec.push_back(OR_LHS);
      }
      msm_off.push_back(nterm);
      or_stmt s{};
      s.m = m; s.ns = 1; s.ni = 1; s.nc = m; s.nterm = nterm; s.k = k; s.N = 1;
      s.term_sec = term_sec.data(); s.term_pt = term_pt.data(); s.msm_off = msm_off.data();
      const size_t nd = or_drawn_count(m, k);
      for (uint32_t real = 0; real < k; ++real) {
        ++cases;
        block drawn(32 * nd), secrets(32 * (size_t)m), rows(32 * (size_t)k * nterm), c(32), chal(32 * (size_t)k), resp(32 * (size_t)k * m), flags(k), mstat((size_t)k * m);
        block wit(32 * ((size_t)m + 1));
        for (size_t i = 0; i < nd; ++i) put(drawn.p + 32 * i, random_scalar());
        for (uint32_t i = 0; i < m; ++i) {
          sc x = random_scalar();
          if (i & 1) x.v[7] |= 0xe0000000u;                           // a witness that is not reduced
          put(secrets.p + 32 * (size_t)i, x);
        }
        or_witness_item(m, secrets.p, real, wit.p);
        if (std::memcmp(wit.p, secrets.p, 32 * (size_t)m) != 0 || wit.p[32 * (size_t)m] != real) ++bad_rows;
        for (uint32_t i = 1; i < 32; ++i) bad_rows += wit.p[32 * (size_t)m + i] != 0;
        auto blind = [&](uint32_t i) { return get(drawn.p + 32 * (size_t)i); };
        auto csim = [&](uint32_t b) { return get(drawn.p + 32 * ((size_t)m + (size_t)b * (m + 1))); };
        auto ssim = [&](uint32_t b, uint32_t i) { return get(drawn.p + 32 * ((size_t)m + (size_t)b * (m + 1) + 1 + i)); };
        sc zero, sum;
        sc_zero(zero);
        sc_zero(sum);
        for (uint32_t b = 0; b < k; ++b) {
          or_assemble_item(s, b, real, drawn.p, rows.p + 32 * (size_t)b * nterm);
          sc negc;
          sc_neg(negc, b == real ? zero : csim(b));
          if (b != real) sc_add(sum, sum, csim(b));
          for (uint32_t t = 0; t < nterm; ++t) {
            const sc want = term_sec[t] == OR_LHS ? negc : (b == real ? blind(term_sec[t]) : ssim(b, term_sec[t]));
            bad_rows += !same(get(rows.p + 32 * ((size_t)b * nterm + t)), want);
          }
        }
        const sc cc = random_scalar();
        put(c.p, cc);
        or_respond_item(s, real, drawn.p, secrets.p, c.p, 1, chal.p, resp.p);
        sc c_real;
        sc_neg(sum, sum);
        sc_add(c_real, cc, sum);
        for (uint32_t b = 0; b < k; ++b) {
          bad_proofs += !same(get(chal.p + 32 * (size_t)b), b == real ? c_real : csim(b));
          for (uint32_t i = 0; i < m; ++i) {
            sc want = ssim(b, i);
            if (b == real) sc_muladd(want, c_real, get(secrets.p + 32 * (size_t)i), blind(i));
            bad_proofs += !same(get(resp.p + 32 * ((size_t)b * m + i)), want);
          }
        }
        // the verifier's rows are (responses, l - challenges); the verdict accepts the honest proof and refuses a bumped challenge, a
        // challenge of value + l, a refused point and an MSM that met a point that does not decode
        std::memset(mstat.p, 0, mstat.n);
        for (uint32_t b = 0; b < k; ++b) {
          flags.p[b] = (uint8_t)or_check_item(s, chal.p + 32 * (size_t)b, resp.p + 32 * (size_t)b * m, rows.p + 32 * (size_t)b * nterm);
          sc negc;
          sc_neg(negc, get(chal.p + 32 * (size_t)b));
          for (uint32_t t = 0; t < nterm; ++t) {
            const sc want = term_sec[t] == OR_LHS ? negc : get(resp.p + 32 * ((size_t)b * m + term_sec[t]));
            bad_rows += !same(get(rows.p + 32 * ((size_t)b * nterm + t)), want);
          }
          bad_verdicts += flags.p[b] != 0;
        }
        bad_verdicts += or_verdict_item(s, chal.p, c.p, flags.p, 0, mstat.p) != 0;
        bad_verdicts += or_verdict_item(s, chal.p, c.p, flags.p, 1, mstat.p) != 1;
        mstat.p[mstat.n - 1] = 1;
        bad_verdicts += or_verdict_item(s, chal.p, c.p, flags.p, 0, mstat.p) != 1;
        mstat.p[mstat.n - 1] = 0;
        sc one;
        sc_zero(one);
        one.v[0] = 1;
        sc bumped;
        sc_add(bumped, get(chal.p), one);
        const sc kept = get(chal.p);
        put(chal.p, bumped);
        bad_verdicts += or_verdict_item(s, chal.p, c.p, flags.p, 0, mstat.p) != 1;
        sc plus_l = kept;                                               // value + l: the same residue, not canonical
        uint64_t carry = 0;
        for (int i = 0; i < 8; ++i) {
          carry += (uint64_t)plus_l.v[i] + sc_l(i);
          plus_l.v[i] = (uint32_t)carry;
          carry >>= 32;
        }
        put(chal.p, plus_l);
        flags.p[0] = (uint8_t)or_check_item(s, chal.p, resp.p, rows.p);
        bad_verdicts += flags.p[0] != 1;
        bad_verdicts += or_verdict_item(s, chal.p, c.p, flags.p, 0, mstat.p) != 1;
        // keep = 0: zero rows
        or_respond_item(s, real, drawn.p, secrets.p, c.p, 0, chal.p, resp.p);
        for (size_t i = 0; i < chal.n; ++i) bad_proofs += chal.p[i] != 0;
        for (size_t i = 0; i < resp.n; ++i) bad_proofs += resp.p[i] != 0;
      }
    }
  std::printf("masks %lu %lu\n", masks, bad_masks);
  std::printf("rows %lu %lu\n", cases, bad_rows);
  std::printf("proofs %lu %lu\n", cases, bad_proofs);
  std::printf("verdicts %lu %lu\n", cases, bad_verdicts);
  return (bad_masks | bad_rows | bad_proofs | bad_verdicts) ? 1 : 0;
}
