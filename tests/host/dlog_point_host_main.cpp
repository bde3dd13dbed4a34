// Stand-alone driver of the host side of the bounded discrete logarithm to a base of the caller's, built with g++ -fsanitize=address,undefined by
// tests/test_host_dlog_point.py together with zkp_amd/csrc/host/host_backend.cpp: hostbk::dlog_point_n and hostbk::dlog_point_range, unsigned and
// signed, over heap blocks of exactly the size a call may touch; the basepoint forms run in between, so that the process holds several tables.
//
//   argv[1]: a file: line 1 the base (64 hex digits), then sections "signed n" (signed = 0 or 1) followed by n lines "point", 64 hex digits each
//   argv[2], argv[3]: bits, baby_bits
//   stdout:  per point: "signed k status k_ranges status_ranges" (decimal, k as int64)
//            k, status                 dlog_point_n
//            k_ranges, status_ranges   the same point halved once (dlog_point_halve, with dlog_point_shift when signed) and searched as three
//                                      ranges of giant steps (dlog_point_range), combined as the toolbox does
#include "../../zkp_amd/csrc/host/host_backend.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint8_t* block(size_t bytes) { return static_cast<uint8_t*>(malloc(bytes ? bytes : 1)); }

static bool hex32(const char* line, uint8_t out[32]) {
  if (strlen(line) < 64) return false;
  for (int i = 0; i < 32; ++i) {
    unsigned b;
    if (sscanf(line + 2 * i, "%2x", &b) != 1) return false;
    out[i] = (uint8_t)b;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const uint32_t bits = (uint32_t)atoi(argv[2]), bb = (uint32_t)atoi(argv[3]);
  char line[512];
  uint8_t* base = block(32);
  if (!fgets(line, sizeof(line), f) || !hex32(line, base)) return 2;
  if (!zkp::hostbk::dlog_point_decodes(base) || zkp::hostbk::dlog_point_prepare_table(base, bb) != 0) return 3;
  uint8_t* junk = block(32);
  memset(junk, 0xff, 32);                                                      // (no field element: not a base)
  if (zkp::hostbk::dlog_point_decodes(junk) || zkp::hostbk::dlog_point_prepare_table(junk, bb) != ZKP_DLOG_INVALID) return 3;
  free(junk);
  const uint64_t J = bits <= bb ? 1 : (uint64_t)1 << (bits - bb);
  const uint64_t cut[4] = {0, J / 3, std::max<uint64_t>(J / 3, (2 * J) / 3), J};
  int is_signed = 0;
  unsigned long n = 0;
  while (fgets(line, sizeof(line), f)) {
    if (sscanf(line, "%d %lu", &is_signed, &n) != 2 || !n) return 2;
    uint8_t* pt = block(32 * n);
    for (size_t i = 0; i < n; ++i)
      if (!fgets(line, sizeof(line), f) || !hex32(line, pt + 32 * i)) return 2;
    uint64_t* k1 = reinterpret_cast<uint64_t*>(block(8 * n));
    uint8_t* s1 = block(n);
    zkp::hostbk::dlog_point_n(base, n, pt, bits, bb, is_signed != 0, k1, s1);
    uint8_t* shift = block(zkp::hostbk::DLOG_HALF_BYTES);
    if (is_signed) zkp::hostbk::dlog_point_shift(base, bits, shift);
    for (size_t i = 0; i < n; ++i) {
      uint64_t kr = 0;
      uint8_t* half = block(zkp::hostbk::DLOG_HALF_BYTES);
      int sr = zkp::hostbk::dlog_point_halve(pt + 32 * i, is_signed ? shift : nullptr, half);
      for (int r = 0; r < 3 && sr != ZKP_DLOG_INVALID; ++r) {
        if (cut[r] >= cut[r + 1]) continue;
        uint64_t k = 0;
        const int s = zkp::hostbk::dlog_point_range(base, half, bits, bb, is_signed != 0, cut[r], cut[r + 1], &k);
        if (s == ZKP_DLOG_FOUND) { sr = s; kr = k; }
      }
      free(half);
      printf("%d %lld %u %lld %d\n", is_signed, (long long)k1[i], (unsigned)s1[i], (long long)kr, sr);
    }
    // the basepoint forms between the sections: another table in the process, and the slot of this base is found again afterwards
    uint64_t kb = 0;
    uint8_t sb = 9;
    zkp::hostbk::dlog_base_n(1, base, bits, bb + 1, &kb, &sb);
    zkp::hostbk::dlog_point_n(base, 0, nullptr, bits, bb, is_signed != 0, nullptr, nullptr);      // an empty call touches nothing
    free(shift);
    free(pt);
    free(k1);
    free(s1);
  }
  fclose(f);
  free(base);
  return 0;
}
