// Stand-alone driver of zkp_amd/csrc/or_batch_lane.h's check and coefficient items (built by tests/test_host_or_batch.py with
// g++ -fsanitize=address,undefined and run as a child process): k = 1, 2, 64 and m = 1, 11, three proofs, on heap blocks of exactly each
// buffer's size, against a restatement with plain loops over the operands.  Prints "<what> <cases> <mismatches>" per check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zkp_amd/csrc/or_batch_lane.h"

using namespace zkp;

static uint64_t g_seed = 0x2545f4914f6cdd1dull;
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
static sc plus_l(sc x) {           // value + l: the same residue, not canonical
  uint64_t carry = 0;
  for (int i = 0; i < 8; ++i) {
    carry += (uint64_t)x.v[i] + sc_l(i);
    x.v[i] = (uint32_t)carry;
    carry >>= 32;
  }
  return x;
}

int main() {
  unsigned long check_cases = 0, bad_checks = 0, coeff_cases = 0, bad_coeffs = 0;
  const uint32_t ks[] = {1, 2, 64}, ms[] = {1, 11};
  const uint32_t N = 3, ns = 2, ni = 2;
  for (uint32_t k : ks)
    for (uint32_t m : ms) {
      // m constraints; constraint i = (secret m - 1 - i) x common point i % 2 + (secret i) x instance point i % 2, left-hand side
      // instance point (i + 1) % 2
      const uint32_t nc = m, nterm = 3 * m;
      std::vector<uint32_t> term_sec, term_pt, msm_off;
      for (uint32_t i = 0; i < m; ++i) {
        msm_off.push_back(3 * i);
        term_sec.push_back(m - 1 - i); term_pt.push_back(i % 2);
        term_sec.push_back(i);         term_pt.push_back(ns + i % 2);
        term_sec.push_back(OR_LHS);    term_pt.push_back(ns + (i + 1) % 2);
      }
      msm_off.push_back(nterm);
      or_stmt s{};
      s.m = m; s.ns = ns; s.ni = ni; s.nc = nc; s.nterm = nterm; s.k = k; s.N = N;
      s.term_sec = term_sec.data(); s.term_pt = term_pt.data(); s.msm_off = msm_off.data();
      const size_t n_blocks = (size_t)N * k, n_ops = ns + n_blocks * (ni + nc);
      block chal(32 * n_blocks), resp(32 * n_blocks * m), given(32 * n_blocks * nc), weights(16 * n_blocks * nc), scalars(32 * n_ops), partial(32 * ns * n_blocks);
      block c(32 * (size_t)N), recomputed(32 * n_blocks * nc), mstat(n_blocks * nc);
      for (size_t i = 0; i < n_blocks * m; ++i) put(resp.p + 32 * i, random_scalar());
      for (size_t i = 0; i < n_blocks * nc; ++i) put(given.p + 32 * i, random_scalar());     // (any 32 bytes that are not all zero)
      for (size_t i = 0; i < weights.n; ++i) weights.p[i] = (uint8_t)rnd();
      std::memset(weights.p, 0, 16);                                                          // a weight of 0
      std::memset(weights.p + weights.n - 16, 0xff, 16);                                      // and the largest
      for (uint32_t j = 0; j < N; ++j) {
        sc sum;
        sc_zero(sum);
        for (uint32_t b = 0; b < k; ++b) {
          const sc x = random_scalar();
          put(chal.p + 32 * ((size_t)j * k + b), x);
          sc_add(sum, sum, x);
        }
        put(c.p + 32 * (size_t)j, sum);
      }
      std::memcpy(recomputed.p, given.p, given.n);
      std::memset(mstat.p, 0, mstat.n);

      // ---- the check item and the match item, per proof
      for (uint32_t j = 0; j < N; ++j) {
        ++check_cases;
        uint8_t* chal_j = chal.p + 32 * (size_t)j * k;
        uint8_t* resp_j = resp.p + 32 * (size_t)j * k * m;
        uint8_t* given_j = given.p + 32 * (size_t)j * k * nc;
        uint8_t* re_j = recomputed.p + 32 * (size_t)j * k * nc;
        uint8_t* mstat_j = mstat.p + (size_t)j * k * nc;
        const uint8_t* c_j = c.p + 32 * (size_t)j;
        auto check = [&](uint32_t rejected) { return or_given_check_item(s, chal_j, resp_j, given_j, c_j, rejected); };
        bad_checks += check(0) != 0;
        bad_checks += check(1) != 1;
        const sc kept = get(chal_j + 32 * (size_t)(k - 1));
        sc one, bumped;
        sc_zero(one);
        one.v[0] = 1;
        sc_add(bumped, kept, one);
        put(chal_j + 32 * (size_t)(k - 1), bumped);
        bad_checks += check(0) != 1;
        put(chal_j + 32 * (size_t)(k - 1), plus_l(kept));
        bad_checks += check(0) != 1;
        put(chal_j + 32 * (size_t)(k - 1), kept);
        const sc r_kept = get(resp_j + 32 * ((size_t)k * m - 1));
        put(resp_j + 32 * ((size_t)k * m - 1), plus_l(r_kept));
        bad_checks += check(0) != 1;
        put(resp_j + 32 * ((size_t)k * m - 1), r_kept);
        const sc g_kept = get(given_j + 32 * ((size_t)k * nc - 1));
        std::memset(given_j + 32 * ((size_t)k * nc - 1), 0, 32);
        bad_checks += check(0) != 1;
        bad_checks += !or_given_rejects(s, given_j);
        put(given_j + 32 * ((size_t)k * nc - 1), g_kept);
        bad_checks += or_given_rejects(s, given_j);
        bad_checks += check(0) != 0;
        bad_checks += or_given_match_item(s, given_j, re_j, mstat_j) != 0;
        re_j[32 * (size_t)k * nc - 1] ^= 0x40;
        bad_checks += or_given_match_item(s, given_j, re_j, mstat_j) != 1;
        re_j[32 * (size_t)k * nc - 1] ^= 0x40;
        mstat_j[(size_t)k * nc - 1] = 1;
        bad_checks += or_given_match_item(s, given_j, re_j, mstat_j) != 1;
        mstat_j[(size_t)k * nc - 1] = 0;
      }

      // ---- the coefficient item: every (proof, branch), then every operand against plain loops
      for (uint32_t j = 0; j < N; ++j)
        for (uint32_t b = 0; b < k; ++b) {
          ++coeff_cases;
          const size_t blk = (size_t)j * k + b;
          or_batch_coeff_item(s, j, b, weights.p + 16 * nc * blk, chal.p + 32 * blk, resp.p + 32 * m * blk, scalars.p, partial.p);
        }
      auto weight = [&](size_t blk, uint32_t cc) {
        sc r;
        sc_zero(r);
        std::memcpy(r.v, weights.p + 16 * (nc * blk + cc), 16);
        return r;
      };
      for (uint32_t j = 0; j < N; ++j)
        for (uint32_t b = 0; b < k; ++b) {
          const size_t blk = (size_t)j * k + b;
          sc negc;
          sc_neg(negc, get(chal.p + 32 * blk));
          for (uint32_t cc = 0; cc < nc; ++cc) {
            sc want;
            sc_neg(want, weight(blk, cc));
            bad_coeffs += !same(get(scalars.p + 32 * (ns + (size_t)k * ni * N + blk * nc + cc)), want);
          }
          for (uint32_t p = 0; p < ns + ni; ++p) {
            sc want;
            sc_zero(want);
            for (uint32_t cc = 0; cc < nc; ++cc)
              for (uint32_t t = msm_off[cc]; t < msm_off[cc + 1]; ++t) {
                if (term_pt[t] != p) continue;
                sc x;
                sc_mul(x, weight(blk, cc), term_sec[t] == OR_LHS ? negc : get(resp.p + 32 * (m * blk + term_sec[t])));
                sc_add(want, want, x);
              }
            const uint8_t* got = p < ns ? partial.p + 32 * ((size_t)p * N * k + blk) : scalars.p + 32 * (ns + ((size_t)b * ni + (p - ns)) * N + j);
            bad_coeffs += !same(get(got), want);
          }
        }
    }
  std::printf("checks %lu %lu\n", check_cases, bad_checks);
  std::printf("coeffs %lu %lu\n", coeff_cases, bad_coeffs);
  return (bad_checks | bad_coeffs) ? 1 : 0;
}
