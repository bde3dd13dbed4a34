// Stand-alone driver of the host side of the segmented scalar sums, products and dot products, built with g++ -fsanitize=address,undefined by
// tests/test_host_scalar_reduce.py together with zkp_amd/csrc/host/host_backend.cpp: hostbk::sc_reduce_n on a ragged job with index lists, over heap
// blocks of exactly the size a call may touch, for several thread counts, with the index lists and with the rows gathered beforehand (idx == NULL).
//
//   argv[1]: a job: "op n_out n_terms n_a n_b", then n_out + 1 offsets, n_terms indices into a, n_terms indices into b (op 2 only), n_a rows and
//            n_b rows (64 hex digits each)
//   stdout:  per output i: "R out" -- one thread, index lists
//   exit:    0; 3 when another thread count or the gathered form gives other bytes; 4 when an argument error wrote something or was not refused
#include "../../zkp_amd/csrc/host/host_backend.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

static uint8_t* block(size_t bytes) { return static_cast<uint8_t*>(malloc(bytes ? bytes : 1)); }
static bool hex_rows(FILE* f, uint8_t* dst, unsigned n) {
  for (unsigned i = 0; i < n; ++i) {
    char hex[80];
    if (fscanf(f, "%79s", hex) != 1 || strlen(hex) != 64) return false;
    for (int k = 0; k < 32; ++k) {
      unsigned b;
      if (sscanf(hex + 2 * k, "%2x", &b) != 1) return false;
      dst[32 * (size_t)i + k] = (uint8_t)b;
    }
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int op;
  unsigned n_out, n_terms, n_a, n_b;
  if (fscanf(f, "%d %u %u %u %u", &op, &n_out, &n_terms, &n_a, &n_b) != 5) return 2;
  const bool dot = op == ZKP_SC_DOT;
  uint32_t* off = reinterpret_cast<uint32_t*>(block(4 * (size_t)(n_out + 1)));
  uint32_t* aidx = reinterpret_cast<uint32_t*>(block(4 * (size_t)n_terms));
  uint32_t* bidx = dot ? reinterpret_cast<uint32_t*>(block(4 * (size_t)n_terms)) : nullptr;
  uint8_t* a = block(32 * (size_t)n_a);
  uint8_t* b = dot ? block(32 * (size_t)n_b) : nullptr;
  for (unsigned i = 0; i <= n_out; ++i) if (fscanf(f, "%u", &off[i]) != 1) return 2;
  for (unsigned i = 0; i < n_terms; ++i) if (fscanf(f, "%u", &aidx[i]) != 1) return 2;
  for (unsigned i = 0; dot && i < n_terms; ++i) if (fscanf(f, "%u", &bidx[i]) != 1) return 2;
  if (!hex_rows(f, a, n_a) || (dot && !hex_rows(f, b, n_b))) return 2;
  fclose(f);
  int rc = 0;
  uint8_t* want = block(32 * (size_t)n_out);
  if (zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, b, dot ? n_b : 0, bidx, 1, want) != ZKP_OK) return 2;
  uint8_t* ga = block(32 * (size_t)n_terms);
  uint8_t* gb = dot ? block(32 * (size_t)n_terms) : nullptr;
  for (unsigned t = 0; t < n_terms; ++t) {
    memcpy(ga + 32 * (size_t)t, a + 32 * (size_t)aidx[t], 32);
    if (dot) memcpy(gb + 32 * (size_t)t, b + 32 * (size_t)bidx[t], 32);
  }
  uint8_t* got = block(32 * (size_t)n_out);
  for (int threads : {1, 3, 5, 7, 64})
    for (int own : {0, 1}) {
      memset(got, 0xee, 32 * (size_t)n_out);
      const int r = own ? zkp::hostbk::sc_reduce_n(op, n_out, off, ga, n_terms, nullptr, gb, dot ? n_terms : 0, nullptr, threads, got)
                        : zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, b, dot ? n_b : 0, bidx, threads, got);
      if (r != ZKP_OK || memcmp(got, want, 32 * (size_t)n_out) != 0) {
        fprintf(stderr, "mismatch: threads %d own %d rc %d\n", threads, own, r);
        rc = 3;
      }
    }
  // argument errors are refused before anything is written
  memset(got, 0xee, 32 * (size_t)n_out);
  if (n_out >= 2 && n_terms >= 2) {
    const uint32_t nb = dot ? n_b : 0;
    if (zkp::hostbk::sc_reduce_n(3, n_out, off, a, n_a, aidx, b, nb, bidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (zkp::hostbk::sc_reduce_n(op, n_out, off, ga, n_terms + 1, nullptr, gb, dot ? n_terms : 0, nullptr, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (!dot && zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, a, n_a, nullptr, 3, got) != ZKP_ERR_ARG) rc = 4;
    const uint32_t keep = aidx[n_terms - 1];
    aidx[n_terms - 1] = n_a;
    if (zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, b, nb, bidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    aidx[n_terms - 1] = keep;
    off[0] = 1;
    if (zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, b, nb, bidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    off[0] = 0;
    const uint32_t mid = off[n_out - 1];
    off[n_out - 1] = off[n_out] + 1;
    if (zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, b, nb, bidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    off[n_out - 1] = mid;
    if (zkp::hostbk::sc_reduce_n(op, n_out, off, nullptr, n_a, aidx, b, nb, bidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, b, nb, bidx, 3, nullptr) != ZKP_ERR_ARG) rc = 4;
    for (size_t i = 0; i < 32 * (size_t)n_out; ++i) if (got[i] != 0xee) rc = 4;
  }
  if (zkp::hostbk::sc_reduce_n(op, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr) != ZKP_OK) rc = 4;      // an empty call touches nothing
  for (unsigned i = 0; i < n_out; ++i) {
    printf("R ");
    for (int k = 0; k < 32; ++k) printf("%02x", want[32 * (size_t)i + k]);
    printf("\n");
  }
  for (uint8_t* p : {reinterpret_cast<uint8_t*>(off), reinterpret_cast<uint8_t*>(aidx), reinterpret_cast<uint8_t*>(bidx), a, b, want, ga, gb, got}) free(p);
  return rc;
}
