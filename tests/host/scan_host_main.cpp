// Stand-alone driver of the host side of the segmented scans, built with g++ -fsanitize=address,undefined by tests/test_host_scan.py together with
// zkp_amd/csrc/host/host_backend.cpp: hostbk::sc_scan_n and hostbk::point_scan_n on a ragged job with index lists, over heap blocks of exactly the
// size a call may touch, in both modes, for several thread counts, with the index lists and with the rows gathered beforehand (idx == NULL).
//
//   argv[1]: a job: "op n_seg n_terms n_a n_points", then n_seg + 1 offsets, n_terms indices into a, n_terms indices into points, n_terms signs,
//            n_a rows and n_points rows (64 hex digits each)
//   stdout:  per mode m and term t: "S<m> row" (the scalar scan) and "P<m> row status" (the point scan) -- one thread, index lists
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
static void print_row(const char* tag, int mode, const uint8_t* row, int status) {
  printf("%s%d ", tag, mode);
  for (int k = 0; k < 32; ++k) printf("%02x", row[k]);
  if (status >= 0) printf(" %d", status);
  printf("\n");
}

int main(int argc, char** argv) {
  using namespace zkp::hostbk;
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int op;
  unsigned n_seg, T, n_a, n_pts;
  if (fscanf(f, "%d %u %u %u %u", &op, &n_seg, &T, &n_a, &n_pts) != 5) return 2;
  uint32_t* off = reinterpret_cast<uint32_t*>(block(4 * (size_t)(n_seg + 1)));
  uint32_t* aidx = reinterpret_cast<uint32_t*>(block(4 * (size_t)T));
  uint32_t* pidx = reinterpret_cast<uint32_t*>(block(4 * (size_t)T));
  uint8_t* neg = block(T);
  uint8_t* a = block(32 * (size_t)n_a);
  uint8_t* pts = block(32 * (size_t)n_pts);
  for (unsigned i = 0; i <= n_seg; ++i) if (fscanf(f, "%u", &off[i]) != 1) return 2;
  for (unsigned i = 0; i < T; ++i) if (fscanf(f, "%u", &aidx[i]) != 1) return 2;
  for (unsigned i = 0; i < T; ++i) if (fscanf(f, "%u", &pidx[i]) != 1) return 2;
  for (unsigned i = 0; i < T; ++i) { unsigned v; if (fscanf(f, "%u", &v) != 1) return 2; neg[i] = (uint8_t)v; }
  if (!hex_rows(f, a, n_a) || !hex_rows(f, pts, n_pts)) return 2;
  fclose(f);
  int rc = 0;
  uint8_t* ga = block(32 * (size_t)T);
  uint8_t* gp = block(32 * (size_t)T);
  for (unsigned t = 0; t < T; ++t) {
    memcpy(ga + 32 * (size_t)t, a + 32 * (size_t)aidx[t], 32);
    memcpy(gp + 32 * (size_t)t, pts + 32 * (size_t)pidx[t], 32);
  }
  uint8_t* want = block(32 * (size_t)T);
  uint8_t* got = block(32 * (size_t)T);
  uint8_t* wst = block(T);
  uint8_t* gst = block(T);
  for (int mode : {ZKP_SCAN_INCLUSIVE, ZKP_SCAN_EXCLUSIVE}) {
    if (sc_scan_n(op, mode, n_seg, off, a, n_a, aidx, 1, want) != ZKP_OK) return 2;
    for (unsigned t = 0; t < T; ++t) print_row("S", mode, want + 32 * (size_t)t, -1);
    for (int threads : {1, 3, 5, 7, 64})
      for (int own : {0, 1}) {
        memset(got, 0xee, 32 * (size_t)T);
        const int r = own ? sc_scan_n(op, mode, n_seg, off, ga, T, nullptr, threads, got) : sc_scan_n(op, mode, n_seg, off, a, n_a, aidx, threads, got);
        if (r != ZKP_OK || memcmp(got, want, 32 * (size_t)T) != 0) {
          fprintf(stderr, "scalar mismatch: mode %d threads %d own %d rc %d\n", mode, threads, own, r);
          rc = 3;
        }
      }
    if (point_scan_n(mode, n_seg, off, pidx, neg, pts, n_pts, 1, want, wst) != ZKP_OK) return 2;
    for (unsigned t = 0; t < T; ++t) print_row("P", mode, want + 32 * (size_t)t, wst[t]);
    for (int threads : {3, 7, 64})
      for (int own : {0, 1}) {
        memset(got, 0xee, 32 * (size_t)T);
        memset(gst, 0xee, T);
        const int r = own ? point_scan_n(mode, n_seg, off, nullptr, neg, gp, T, threads, got, gst) : point_scan_n(mode, n_seg, off, pidx, neg, pts, n_pts, threads, got, gst);
        if (r != ZKP_OK || memcmp(got, want, 32 * (size_t)T) != 0 || memcmp(gst, wst, T) != 0) {
          fprintf(stderr, "point mismatch: mode %d threads %d own %d rc %d\n", mode, threads, own, r);
          rc = 3;
        }
      }
  }
  // argument errors are refused before anything is written
  memset(got, 0xee, 32 * (size_t)T);
  memset(gst, 0xee, T);
  if (n_seg >= 2 && T >= 2) {
    if (sc_scan_n(ZKP_SC_DOT, 0, n_seg, off, a, n_a, aidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (sc_scan_n(op, 2, n_seg, off, a, n_a, aidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(2, n_seg, off, pidx, neg, pts, n_pts, 3, got, gst) != ZKP_ERR_ARG) rc = 4;
    if (sc_scan_n(op, 0, n_seg, off, ga, T + 1, nullptr, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(0, n_seg, off, nullptr, neg, gp, T - 1, 3, got, gst) != ZKP_ERR_ARG) rc = 4;
    const uint32_t keep_a = aidx[T - 1], keep_p = pidx[T - 1];
    aidx[T - 1] = n_a;
    pidx[T - 1] = n_pts;
    if (sc_scan_n(op, 0, n_seg, off, a, n_a, aidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(0, n_seg, off, pidx, neg, pts, n_pts, 3, got, gst) != ZKP_ERR_ARG) rc = 4;
    aidx[T - 1] = keep_a;
    pidx[T - 1] = keep_p;
    off[0] = 1;
    if (sc_scan_n(op, 0, n_seg, off, a, n_a, aidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(0, n_seg, off, pidx, neg, pts, n_pts, 3, got, gst) != ZKP_ERR_ARG) rc = 4;
    off[0] = 0;
    const uint32_t mid = off[n_seg - 1];
    off[n_seg - 1] = off[n_seg] + 1;
    if (sc_scan_n(op, 0, n_seg, off, a, n_a, aidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(0, n_seg, off, pidx, neg, pts, n_pts, 3, got, gst) != ZKP_ERR_ARG) rc = 4;
    off[n_seg - 1] = mid;
    if (sc_scan_n(op, 0, n_seg, off, nullptr, n_a, aidx, 3, got) != ZKP_ERR_ARG) rc = 4;
    if (sc_scan_n(op, 0, n_seg, off, a, n_a, aidx, 3, nullptr) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(0, n_seg, off, pidx, neg, nullptr, n_pts, 3, got, gst) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(0, n_seg, off, pidx, neg, pts, n_pts, 3, nullptr, gst) != ZKP_ERR_ARG) rc = 4;
    if (point_scan_n(0, n_seg, off, pidx, neg, pts, n_pts, 3, got, nullptr) != ZKP_ERR_ARG) rc = 4;
    for (size_t i = 0; i < 32 * (size_t)T; ++i) if (got[i] != 0xee) rc = 4;
    for (size_t i = 0; i < T; ++i) if (gst[i] != 0xee) rc = 4;
  }
  if (sc_scan_n(op, 0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr) != ZKP_OK) rc = 4;                  // an empty call touches nothing
  if (point_scan_n(0, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr) != ZKP_OK) rc = 4;
  for (uint8_t* p : {reinterpret_cast<uint8_t*>(off), reinterpret_cast<uint8_t*>(aidx), reinterpret_cast<uint8_t*>(pidx), neg, a, pts, ga, gp, want, got, wst, gst}) free(p);
  return rc;
}
