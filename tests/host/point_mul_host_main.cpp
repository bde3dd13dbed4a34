// Stand-alone driver of the host side of the batched Scalar * basepoint / Scalar * point calls, built with g++ -fsanitize=address,undefined by
// tests/test_host_point_mul.py together with zkp_amd/csrc/host/host_backend.cpp: hostbk::mul_base_n and hostbk::mul_points_n over heap blocks
// of exactly the size a call may touch.
//
//   argv[1]: a file of lines "scalar point", each 64 hex digits (32 little-endian bytes / a ristretto255 encoding)
//   stdout:  per line i: "base ct vt inplace shared_point shared_scalar status"
//            base           scalar_i * B                                  (mul_base_n)
//            ct, vt         scalar_i * point_i, ZKP_CT and ZKP_VARTIME    (strides 1, 1)
//            inplace        the same, out = points                        (ZKP_CT)
//            shared_point   scalar_i * point_0                            (strides 1, 0)
//            shared_scalar  scalar_0 * point_i                            (strides 0, 1)
//            status         two hex digits: status of ct | status of shared_scalar << 4
#include "../../zkp_amd/csrc/host/host_backend.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void put(const uint8_t* p) {
  for (int i = 0; i < 32; ++i) printf("%02x", p[i]);
}
static uint8_t* block(size_t bytes) { return static_cast<uint8_t*>(malloc(bytes ? bytes : 1)); }
static bool hex32(std::vector<uint8_t>& dst, const char* s) {
  for (int i = 0; i < 32; ++i) {
    unsigned b;
    if (sscanf(s + 2 * i, "%2x", &b) != 1) return false;
    dst.push_back((uint8_t)b);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<uint8_t> sv, pv;
  char line[512];
  while (fgets(line, sizeof(line), f)) {
    if (strlen(line) < 129) continue;
    if (!hex32(sv, line) || !hex32(pv, line + 65)) return 2;
  }
  fclose(f);
  const size_t n = sv.size() / 32;
  if (!n) return 2;
  uint8_t* sc = block(32 * n);
  uint8_t* pt = block(32 * n);
  memcpy(sc, sv.data(), 32 * n);
  memcpy(pt, pv.data(), 32 * n);
  uint8_t* base = block(32 * n);
  zkp::hostbk::mul_base_n(n, sc, base);
  uint8_t *ct = block(32 * n), *st_ct = block(n);
  zkp::hostbk::mul_points_n(n, sc, 1, pt, 1, ZKP_CT, ct, st_ct);
  uint8_t *vt = block(32 * n), *st_vt = block(n);
  zkp::hostbk::mul_points_n(n, sc, 1, pt, 1, ZKP_VARTIME, vt, st_vt);
  uint8_t *inplace = block(32 * n), *st_in = block(n);
  memcpy(inplace, pt, 32 * n);
  zkp::hostbk::mul_points_n(n, sc, 1, inplace, 1, ZKP_CT, inplace, st_in);
  uint8_t *one_pt = block(32), *sp = block(32 * n), *st_sp = block(n);
  memcpy(one_pt, pt, 32);
  zkp::hostbk::mul_points_n(n, sc, 1, one_pt, 0, ZKP_CT, sp, st_sp);
  uint8_t *one_sc = block(32), *ss = block(32 * n), *st_ss = block(n);
  memcpy(one_sc, sc, 32);
  zkp::hostbk::mul_points_n(n, one_sc, 0, pt, 1, ZKP_VARTIME, ss, st_ss);
  int rc = 0;
  for (size_t i = 0; i < n; ++i) {
    if (st_ct[i] != st_vt[i] || st_ct[i] != st_in[i] || st_sp[i] != st_sp[0]) rc = 3;
    const uint8_t* cols[] = {base, ct, vt, inplace, sp, ss};
    for (int k = 0; k < 6; ++k) {
      put(cols[k] + 32 * i);
      putchar(' ');
    }
    printf("%02x\n", (unsigned)(st_ct[i] | (st_ss[i] << 4)));
  }
  // an empty call touches nothing
  zkp::hostbk::mul_base_n(0, nullptr, nullptr);
  zkp::hostbk::mul_points_n(0, nullptr, 1, nullptr, 1, ZKP_CT, nullptr, nullptr);
  for (uint8_t* p : {sc, pt, base, ct, st_ct, vt, st_vt, inplace, st_in, one_pt, sp, st_sp, one_sc, ss, st_ss}) free(p);
  return rc;
}
