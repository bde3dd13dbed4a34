// Stand-alone driver of the host side of the bounded discrete logarithm to the basepoint, built with g++ -fsanitize=address,undefined by
// tests/test_host_dlog.py together with zkp_amd/csrc/host/host_backend.cpp: hostbk::dlog_base_n and hostbk::dlog_base_range over heap blocks of
// exactly the size a call may touch, at two table sizes in one process (the tables are kept per size).
//
//   argv[1]: a file of lines "point", 64 hex digits each (a ristretto255 encoding)
//   argv[2], argv[3], argv[4]: bits, baby_bits, a second baby_bits
//   stdout:  per line i: "k status k_ranges status_ranges k_second status_second" (decimal)
//            k, status                 dlog_base_n at baby_bits
//            k_ranges, status_ranges   the same point halved once (dlog_halve) and searched as three ranges of giant steps (dlog_base_range),
//                                      combined as the toolbox does
//            k_second, status_second   dlog_base_n at the second baby_bits
#include "../../zkp_amd/csrc/host/host_backend.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint8_t* block(size_t bytes) { return static_cast<uint8_t*>(malloc(bytes ? bytes : 1)); }

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const uint32_t bits = (uint32_t)atoi(argv[2]), bb = (uint32_t)atoi(argv[3]), bb2 = (uint32_t)atoi(argv[4]);
  std::vector<uint8_t> pv;
  char line[512];
  while (fgets(line, sizeof(line), f)) {
    if (strlen(line) < 64) continue;
    for (int i = 0; i < 32; ++i) {
      unsigned b;
      if (sscanf(line + 2 * i, "%2x", &b) != 1) return 2;
      pv.push_back((uint8_t)b);
    }
  }
  fclose(f);
  const size_t n = pv.size() / 32;
  if (!n) return 2;
  uint8_t* pt = block(32 * n);
  memcpy(pt, pv.data(), 32 * n);
  uint64_t* k1 = reinterpret_cast<uint64_t*>(block(8 * n));
  uint64_t* k2 = reinterpret_cast<uint64_t*>(block(8 * n));
  uint8_t *s1 = block(n), *s2 = block(n);
  zkp::hostbk::dlog_base_n(n, pt, bits, bb, k1, s1);
  zkp::hostbk::dlog_base_n(n, pt, bits, bb2, k2, s2);
  const uint64_t J = bits <= bb ? 1 : (uint64_t)1 << (bits - bb);
  const uint64_t cut[4] = {0, J / 3, std::max<uint64_t>(J / 3, (2 * J) / 3), J};
  for (size_t i = 0; i < n; ++i) {
    uint64_t kr = 0;
    uint8_t* half = block(zkp::hostbk::DLOG_HALF_BYTES);
    int sr = zkp::hostbk::dlog_halve(pt + 32 * i, half);
    for (int r = 0; r < 3 && sr != ZKP_DLOG_INVALID; ++r) {
      if (cut[r] >= cut[r + 1]) continue;
      uint64_t k = 0;
      const int s = zkp::hostbk::dlog_base_range(half, bits, bb, cut[r], cut[r + 1], &k);
      if (s == ZKP_DLOG_FOUND) { sr = s; kr = k; }
    }
    free(half);
    printf("%llu %u %llu %d %llu %u\n", (unsigned long long)k1[i], (unsigned)s1[i], (unsigned long long)kr, sr, (unsigned long long)k2[i], (unsigned)s2[i]);
  }
  zkp::hostbk::dlog_base_n(0, nullptr, bits, bb, nullptr, nullptr);          // an empty call touches nothing
  free(pt);
  free(k1);
  free(k2);
  free(s1);
  free(s2);
  return 0;
}
