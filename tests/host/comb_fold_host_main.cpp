// Stand-alone host driver of the sign-folded radix-16 recoding (zkp_amd/csrc/sc25519.h: sc_fold_recode16) and a host model of the grouped comb
// walk in Horner order (zkp_amd/csrc/comb_tables.h: comb_group_xbar), built with g++ -fsanitize=address,undefined by tests/test_host_comb_fold.py,
// and once more with -DZKP_FE_TRACK so that the interval tracker asserts the limb bounds of the merge sequence.  The headers are one text for g++
// and hipcc: the recoding and the point formulas that run here are what the kernels compile; the walk's ORDER is restated below.
//
//   argv[1]: a file of records, one per line
//     "R <s>"              s: 64 hex digits (a reduced scalar, little-endian bytes)      -> "<flip> <e>"
//     "W <fold> <P> <s>"   fold 0 / 1, P: a ristretto255 encoding, s as above            -> "<encode(walk)> <encode(double-and-add)>"
//     "L 1 <P> <s>"        the folded ladder order on P's eight multiples                -> "<encode(ladder)> <encode(double-and-add)>"
#include "../../zkp_amd/csrc/ge25519.h"
#include "../../zkp_amd/csrc/sc25519.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace zkp;

static bool hex32(const char* s, uint32_t v[8]) {
  uint8_t b[32];
  for (int i = 0; i < 32; ++i) {
    unsigned x;
    if (sscanf(s + 2 * i, "%2x", &x) != 1) return false;
    b[i] = (uint8_t)x;
  }
  memcpy(v, b, 32);
  return true;
}
static void put(const uint32_t v[8]) {
  uint8_t b[32];
  memcpy(b, v, 32);
  for (int i = 0; i < 32; ++i) printf("%02x", b[i]);
}

constexpr int TEETH = 16, BITS = 16, ENTRIES = 8 * TEETH + 1;

// a table entry as the walks see it: limbs that came from memory, of the tight class
static void from_memory(ge_cached& c) {
  FE_TRACK(fe_set_ub_tight(c.YpX); fe_set_ub_tight(c.YmX); fe_set_ub_tight(c.Z2); fe_set_ub_tight(c.T2d));
  (void)c;
}

// comb_table_lane: entry 8 j + (k - 1) = k 2^(16 j) P; carry: the entry 2^256 P, which a call that vouches for reduced scalars does not build
static void build_table(ge_cached* tbl, const ge_p3& P, bool carry) {
  ge_p3 base = P;
  for (int j = 0; j < TEETH; ++j) {
    ge_p3 m2, m3, m4, m;
    ge_cached c1;
    ge_to_cached(c1, base);
    tbl[8 * j + 0] = c1;
    ge_double<true>(m2, base);
    ge_to_cached(tbl[8 * j + 1], m2);
    ge_add_cached(m3, m2, c1);
    ge_to_cached(tbl[8 * j + 2], m3);
    ge_double<true>(m4, m2);
    ge_to_cached(tbl[8 * j + 3], m4);
    ge_add_cached(m, m4, c1);
    ge_to_cached(tbl[8 * j + 4], m);
    ge_double<true>(m, m3);
    ge_to_cached(tbl[8 * j + 5], m);
    ge_add_cached(m, m, c1);
    ge_to_cached(tbl[8 * j + 6], m);
    ge_double<true>(base, m4);
    ge_to_cached(tbl[8 * j + 7], base);
    if (!carry && j == TEETH - 1) break;
    for (int d = 0; d < BITS - 4; ++d) ge_double<false>(base, base);
    ge_double<true>(base, base);
  }
  if (carry) ge_to_cached(tbl[8 * TEETH], base);
  for (int i = 0; i < ENTRIES - (carry ? 0 : 1); ++i) from_memory(tbl[i]);
}

static void select(ge_cached& sel, const ge_cached* row, uint32_t mag) {
  ge_cached_identity(sel);
  for (uint32_t k = 1; k <= 8; ++k) ge_cached_cmov(sel, row[k - 1], (uint32_t)(mag == k));
}

// the digit of tooth j, window w (nibble 4 j + w of e) -> sel;  raw: the digit as it stands
static void pick(ge_cached& sel, const ge_cached* tbl, const uint32_t e[8], int j, int w, bool raw) {
  const int nidx = 4 * j + w;
  const uint32_t nib = (e[nidx >> 3] >> (4 * (nidx & 7))) & 15u;
  const uint32_t neg = raw ? 0u : (uint32_t)(nib < 8u);
  const uint32_t mag = raw ? nib : (neg ? 8u - nib : nib - 8u);
  select(sel, tbl + 8 * j, mag);
  ge_cached_cneg(sel, neg);
}

// comb_group_xbar's order: pass 0 acc = S3, lo = S2; acc = 16 (16 acc + lo); pass 1 acc += S1, a fresh lo = S0; 16 acc + lo
static void walk(ge_p3& acc, const ge_cached* tbl, const uint32_t s[8], bool fold) {
  uint32_t e[8], top = 0, flip = 0;
  if (fold) flip = sc_fold_recode16(e, s);
  else sc_add_pattern(e, top, s, 0x88888888u);
  ge_p3 lo;
  ge_identity(acc);
  ge_identity(lo);
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) {
      ge_double4(acc);
      ge_cached c;
      ge_to_cached(c, lo);
      ge_add_cached(acc, acc, c);
      ge_double4(acc);
    }
    for (int j = 0; j < TEETH; ++j) {
      ge_cached sel;
      const bool top_tooth = fold && pass == 0 && j == TEETH - 1;
      if (!top_tooth) {
        pick(sel, tbl, e, j, pass ? 1 : 3, false);
        if (pass == 0 && j == 0) ge_from_cached(acc, sel);
        else ge_add_cached(acc, acc, sel);
      }
      pick(sel, tbl, e, j, pass ? 0 : 2, top_tooth);
      if (j == 0) ge_from_cached(lo, sel);
      else ge_add_cached(lo, lo, sel);
    }
  }
  ge_double4(acc);
  {
    ge_cached c;
    ge_to_cached(c, lo);
    ge_add_cached(acc, acc, c);
  }
  if (fold) ge_cneg(acc, flip);
  else {                                                   // the carry tooth (a reduced scalar never sets top: the identity is added)
    ge_cached sel;
    ge_cached_identity(sel);
    ge_cached_cmov(sel, tbl[8 * TEETH], top);
    ge_add_cached(acc, acc, sel);
  }
}

// term_ladder16's folded order on the first tooth's eight multiples: the entry of nibble 62 is the accumulator, 62 x (16 acc + entry) follow
static void ladder(ge_p3& acc, const ge_cached* tbl, const uint32_t s[8]) {
  uint32_t e[8];
  const uint32_t flip = sc_fold_recode16(e, s);
  ge_cached sel;
  select(sel, tbl, e[7] >> 24);
  ge_from_cached(acc, sel);
  for (int n = (int)SC_FOLD16_TOP_NIBBLE - 1; n >= 0; --n) {
    ge_double4(acc);
    const uint32_t nib = (e[n >> 3] >> (4 * (n & 7))) & 15u;
    const uint32_t neg = (uint32_t)(nib < 8u);
    select(sel, tbl, neg ? 8u - nib : nib - 8u);
    ge_cached_cneg(sel, neg);
    ge_add_cached(acc, acc, sel);
  }
  ge_cneg(acc, flip);
}

static void double_and_add(ge_p3& r, const ge_p3& P, const uint32_t s[8]) {
  ge_cached c;
  ge_to_cached(c, P);
  ge_identity(r);
  for (int b = 255; b >= 0; --b) {
    ge_double<true>(r, r);
    if ((s[b >> 5] >> (b & 31)) & 1u) ge_add_cached(r, r, c);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char* line = static_cast<char*>(malloc(512));
  ge_cached* tbl = static_cast<ge_cached*>(malloc(sizeof(ge_cached) * ENTRIES));          // exactly 129 entries: a read past the table shows
  ge_cached* tbl_nc = static_cast<ge_cached*>(malloc(sizeof(ge_cached) * (ENTRIES - 1)));   // exactly 128: a read of the carry entry shows
  uint32_t have[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool built = false;
  while (fgets(line, 512, f)) {
    uint32_t* s = static_cast<uint32_t*>(malloc(32));
    uint32_t* e = static_cast<uint32_t*>(malloc(32));
    if (line[0] == 'R') {
      if (strlen(line) < 2 + 64 || !hex32(line + 2, s)) return 2;
      const uint32_t flip = sc_fold_recode16(e, s);
      printf("%u ", flip);
      put(e);
      printf("\n");
    } else if (line[0] == 'W' || line[0] == 'L') {
      uint32_t pw[8];
      const int fold = line[2] - '0';
      if (strlen(line) < 4 + 64 + 1 + 64 || (fold != 0 && fold != 1) || !hex32(line + 4, pw) || !hex32(line + 4 + 65, s)) return 2;
      ge_p3 P, got, want;
      if (!ristretto_decode(P, pw)) return 3;
      if (!built || memcmp(have, pw, 32)) {                // (records come grouped by point)
        build_table(tbl, P, true);
        build_table(tbl_nc, P, false);
        memcpy(have, pw, 32);
        built = true;
      }
      if (line[0] == 'L') ladder(got, tbl_nc, s);
      else walk(got, fold ? tbl_nc : tbl, s, fold != 0);
      double_and_add(want, P, s);
      ristretto_encode(e, got);
      put(e);
      printf(" ");
      ristretto_encode(e, want);
      put(e);
      printf("\n");
    } else {
      return 2;
    }
    free(s);
    free(e);
  }
  free(tbl);
  free(tbl_nc);
  free(line);
  fclose(f);
  return 0;
}
