// Stand-alone driver of the host side of the batched scalar calls, built with g++ -fsanitize=address,undefined by
// tests/test_host_scalar_ops.py together with zkp_amd/csrc/host/host_backend.cpp: sc_invert of sc25519.h called directly, and the
// routines behind the toolbox's host route (hostbk::sc_*_n), each over heap blocks of exactly the size the call may touch.
//
//   argv[1]: a file of 64-hex-digit lines, one 256-bit value per line (little-endian bytes)
//   stdout:  per value v (index i, w = value i + 1, wrapping): "inv direct batch inplace muladd muladd_shared muladd_nullc wide hash"
//            inv*     v^-1 three ways;  muladd  v * w + v (strides 1, out aliasing a);  muladd_shared  v * w0 + w0 (strides 1, 0, 0);
//            muladd_nullc  v * w;  wide  from_wide(v || w);  hash  hash_from_bytes(v || w as one 64-byte message of a CSR batch of all)
#define ZKP_HOST_FE51 1        // the field under host_backend.cpp's copy of the shared headers: one definition of zkp::fe in this program
#include "../../zkp_amd/csrc/sc25519.h"
#include "../../zkp_amd/csrc/host/host_backend.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void put(const uint8_t* p) {
  for (int i = 0; i < 32; ++i) printf("%02x", p[i]);
}
static uint8_t* block(size_t bytes) { return static_cast<uint8_t*>(malloc(bytes ? bytes : 1)); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<uint8_t> vals;
  char line[256];
  while (fgets(line, sizeof(line), f)) {
    if (strlen(line) < 64) continue;
    for (int i = 0; i < 32; ++i) {
      unsigned b;
      if (sscanf(line + 2 * i, "%2x", &b) != 1) return 2;
      vals.push_back((uint8_t)b);
    }
  }
  fclose(f);
  const size_t n = vals.size() / 32;
  if (!n) return 2;
  uint8_t* in = block(32 * n);
  uint8_t* next = block(32 * n);
  uint8_t* wide = block(64 * n);
  memcpy(in, vals.data(), 32 * n);
  for (size_t i = 0; i < n; ++i) {
    memcpy(next + 32 * i, in + 32 * ((i + 1) % n), 32);
    memcpy(wide + 64 * i, in + 32 * i, 32);
    memcpy(wide + 64 * i + 32, next + 32 * i, 32);
  }
  uint8_t* direct = block(32 * n);
  for (size_t i = 0; i < n; ++i) {
    zkp::sc a, r;
    memcpy(a.v, in + 32 * i, 32);
    zkp::sc_invert(r, a);
    memcpy(direct + 32 * i, r.v, 32);
  }
  uint8_t* batch = block(32 * n);
  zkp::hostbk::sc_invert_n(n, in, batch);
  uint8_t* inplace = block(32 * n);
  memcpy(inplace, in, 32 * n);
  zkp::hostbk::sc_invert_n(n, inplace, inplace);
  uint8_t* ma = block(32 * n);
  memcpy(ma, in, 32 * n);
  zkp::hostbk::sc_muladd_n(n, ma, 1, next, 1, in, 1, ma);               // out aliases a
  uint8_t* shared = block(32);
  memcpy(shared, next, 32);
  uint8_t* ms = block(32 * n);
  zkp::hostbk::sc_muladd_n(n, in, 1, shared, 0, shared, 0, ms);
  uint8_t* mn = block(32 * n);
  zkp::hostbk::sc_muladd_n(n, in, 1, next, 1, nullptr, 0, mn);
  uint8_t* fw = block(32 * n);
  zkp::hostbk::sc_from_wide_n(n, wide, fw);
  std::vector<uint64_t> off(n + 1);
  for (size_t i = 0; i <= n; ++i) off[i] = 64 * i;
  uint8_t* hs = block(32 * n);
  zkp::hostbk::sc_hash_sha512_n(n, wide, off.data(), hs);
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* cols[] = {direct, batch, inplace, ma, ms, mn, fw, hs};
    for (int k = 0; k < 8; ++k) {
      put(cols[k] + 32 * i);
      putchar(k == 7 ? '\n' : ' ');
    }
  }
  for (uint8_t* p : {in, next, wide, direct, batch, inplace, ma, shared, ms, mn, fw, hs}) free(p);
  return 0;
}
