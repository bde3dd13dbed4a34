// Host build of ge_from_niels / ge_from_cached (zkp_amd/csrc/ge25519.h): the first entry of a chain of additions set directly instead of
// added onto the identity.  Built three times by tests/test_host_first_entry.py: plain, -DZKP_FE_TRACK (interval bound tracker) and
// -DZKP_HOST_FE51 (5 x 51-bit limbs).  Entries arrive as RAW limbs, so that the test can place them at the maxima of the tight class.
#include "../../zkp_amd/csrc/ge25519.h"
#include <cstring>
using namespace zkp;

#ifdef ZKP_HOST_FE51
constexpr int NL = 5;
#else
constexpr int NL = 9;
#endif

static void set_tight(fe& r, const uint64_t* l) {
  for (int i = 0; i < NL; ++i) r.v[i] = (decltype(r.v[0]))l[i];
  FE_TRACK(fe_set_ub_tight(r));          // the CLASS bound, whatever the value: the tracker then speaks for every tight entry
}
static void store(uint8_t* b, const fe& a) { uint32_t w[8]; fe_towords(w, a); memcpy(b, w, 32); }
static void enc(uint8_t* out, const ge_p3& p) { uint32_t w[8]; ristretto_encode(w, p); memcpy(out, w, 32); }

extern "C" {
int t_limbs(void) { return NL; }
// form 0: niels (ypx, ymx, xy2d), 1: cached (YpX, YmX, Z2, T2d) -- 3 or 4 x NL limbs, each within the tight class.
// cneg: the entry first goes through ge_niels_cneg / ge_cached_cneg(., 1) (the walks' uncarried negation).
// neg:  the _neg helper against identity - entry (ge_msub / ge_sub_cached) instead of the plain one against identity + entry.
// xyzt: the helper's coordinates, canonical; encs: encode(helper), encode(identity +- entry).
void t_first_entry(int form, int cneg, int neg, const uint64_t* limbs, uint8_t* xyzt, uint8_t* encs) {
  ge_p3 r, id, s;
  ge_identity(id);
  if (form == 0) {
    ge_niels q;
    set_tight(q.ypx, limbs); set_tight(q.ymx, limbs + NL); set_tight(q.xy2d, limbs + 2 * NL);
    if (cneg) ge_niels_cneg(q, 1);
    if (neg) { ge_from_niels_neg(r, q); ge_msub(s, id, q); }
    else { ge_from_niels(r, q); ge_madd(s, id, q); }
  } else {
    ge_cached q;
    set_tight(q.YpX, limbs); set_tight(q.YmX, limbs + NL); set_tight(q.Z2, limbs + 2 * NL); set_tight(q.T2d, limbs + 3 * NL);
    if (cneg) ge_cached_cneg(q, 1);
    if (neg) { ge_from_cached_neg(r, q); ge_sub_cached(s, id, q); }
    else { ge_from_cached(r, q); ge_add_cached(s, id, q); }
  }
  // the result is the accumulator of a chain: it must be a valid left operand of the next addition and doubling
  {
    ge_p3 u;
    ge_cached c;
    ge_to_cached(c, r);
    ge_add_cached(u, r, c);
    ge_double<true>(u, r);
    ge_niels n;
    ge_niels_identity(n);
    ge_madd(u, r, n);
  }
  store(xyzt, r.X); store(xyzt + 32, r.Y); store(xyzt + 64, r.Z); store(xyzt + 96, r.T);
  enc(encs, r);
  enc(encs + 32, s);
}
}
