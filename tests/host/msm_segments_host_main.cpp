// Stand-alone driver of the host side of the multiscalar sums with long segments, built with g++ -fsanitize=address,undefined by
// tests/test_host_msm_segments.py together with zkp_amd/csrc/host/host_backend.cpp: hostbk::msm_segments_n against hostbk::msm_many on a ragged job,
// over heap blocks of exactly the size a call may touch, for several thread counts and both flags.
//
//   argv[1]: a job: "n_msm n_terms n_points", then n_msm + 1 offsets, n_terms indices, n_terms scalars and n_points encodings (64 hex digits each)
//   stdout:  per segment i: "M out status" -- hostbk::msm_many, variable time
//   exit:    0; 3 when a msm_segments_n result (threads 1, 3, 7 and 64; both flags; indexed and gathered with pidx == NULL) differs from msm_many's;
//            4 when an argument error wrote something or was not refused
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
  unsigned n_msm, n_terms, n_points;
  if (fscanf(f, "%u %u %u", &n_msm, &n_terms, &n_points) != 3) return 2;
  uint32_t* off = reinterpret_cast<uint32_t*>(block(4 * (size_t)(n_msm + 1)));
  uint32_t* pidx = reinterpret_cast<uint32_t*>(block(4 * (size_t)n_terms));
  uint8_t* sc = block(32 * (size_t)n_terms);
  uint8_t* pts = block(32 * (size_t)n_points);
  for (unsigned i = 0; i <= n_msm; ++i) if (fscanf(f, "%u", &off[i]) != 1) return 2;
  for (unsigned i = 0; i < n_terms; ++i) if (fscanf(f, "%u", &pidx[i]) != 1) return 2;
  if (!hex_rows(f, sc, n_terms) || !hex_rows(f, pts, n_points)) return 2;
  fclose(f);
  int rc = 0;
  uint8_t *want = block(32 * (size_t)n_msm), *want_st = block(n_msm);
  if (zkp::hostbk::msm_many(n_msm, off, sc, pidx, pts, n_points, ZKP_VARTIME, want, want_st) != ZKP_OK) return 2;
  uint8_t* gathered = block(32 * (size_t)n_terms);
  for (unsigned t = 0; t < n_terms; ++t) memcpy(gathered + 32 * (size_t)t, pts + 32 * (size_t)pidx[t], 32);
  uint8_t *got = block(32 * (size_t)n_msm), *got_st = block(n_msm);
  for (int threads : {1, 3, 7, 64})
    for (int flags : {ZKP_VARTIME, ZKP_CT})
      for (int own : {0, 1}) {
        memset(got, 0xee, 32 * (size_t)n_msm);
        memset(got_st, 0xee, n_msm);
        const int r = own ? zkp::hostbk::msm_segments_n(n_msm, off, sc, nullptr, gathered, n_terms, flags, threads, got, got_st)
                          : zkp::hostbk::msm_segments_n(n_msm, off, sc, pidx, pts, n_points, flags, threads, got, got_st);
        if (r != ZKP_OK || memcmp(got, want, 32 * (size_t)n_msm) != 0 || memcmp(got_st, want_st, n_msm) != 0) {
          fprintf(stderr, "mismatch: threads %d flags %d own %d rc %d\n", threads, flags, own, r);
          rc = 3;
        }
      }
  // argument errors are refused before anything is written
  memset(got, 0xee, 32 * (size_t)n_msm);
  memset(got_st, 0xee, n_msm);
  if (n_msm >= 2 && n_terms >= 2) {
    if (zkp::hostbk::msm_segments_n(n_msm, off, sc, pidx, pts, n_points, 2, 3, got, got_st) != ZKP_ERR_ARG) rc = 4;
    if (zkp::hostbk::msm_segments_n(n_msm, off, sc, nullptr, gathered, n_terms + 1, ZKP_CT, 3, got, got_st) != ZKP_ERR_ARG) rc = 4;
    const uint32_t keep = pidx[n_terms - 1];
    pidx[n_terms - 1] = n_points;
    if (zkp::hostbk::msm_segments_n(n_msm, off, sc, pidx, pts, n_points, ZKP_CT, 3, got, got_st) != ZKP_ERR_ARG) rc = 4;
    pidx[n_terms - 1] = keep;
    off[0] = 1;
    if (zkp::hostbk::msm_segments_n(n_msm, off, sc, pidx, pts, n_points, ZKP_CT, 3, got, got_st) != ZKP_ERR_ARG) rc = 4;
    off[0] = 0;
    const uint32_t mid = off[n_msm - 1];
    off[n_msm - 1] = off[n_msm] + 1;
    if (zkp::hostbk::msm_segments_n(n_msm, off, sc, pidx, pts, n_points, ZKP_CT, 3, got, got_st) != ZKP_ERR_ARG) rc = 4;
    off[n_msm - 1] = mid;
    for (size_t i = 0; i < 32 * (size_t)n_msm; ++i) if (got[i] != 0xee) rc = 4;
    for (size_t i = 0; i < n_msm; ++i) if (got_st[i] != 0xee) rc = 4;
  }
  if (zkp::hostbk::msm_segments_n(0, nullptr, nullptr, nullptr, nullptr, 0, ZKP_CT, 0, nullptr, nullptr) != ZKP_OK) rc = 4;      // an empty call touches nothing
  for (unsigned i = 0; i < n_msm; ++i) {
    printf("M ");
    for (int k = 0; k < 32; ++k) printf("%02x", want[32 * (size_t)i + k]);
    printf(" %02x\n", (unsigned)want_st[i]);
  }
  for (uint8_t* p : {reinterpret_cast<uint8_t*>(off), reinterpret_cast<uint8_t*>(pidx), sc, pts, want, want_st, gathered, got, got_st}) free(p);
  return rc;
}
