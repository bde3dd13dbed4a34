// Stand-alone driver of the host side of the batched point sums, built with g++ -fsanitize=address,undefined by tests/test_host_point_sum.py together
// with zkp_amd/csrc/host/host_backend.cpp: hostbk::add_points_n, sum_points_n, sum_points_partial and sum_points_finish over heap blocks of exactly
// the size a call may touch.
//
//   argv[1]: a file of lines "a b", each 64 hex digits (a ristretto255 encoding)
//   argv[2]: a sum job: "n_sums n_terms n_points", then n_sums + 1 offsets, n_terms indices, n_terms signs (0 / 1), then n_points encodings in hex
//   stdout:  per pair i: "P add sub inplace shared status"
//            add, sub   a_i + b_i, a_i - b_i                       (strides 1, 1)
//            inplace    a_i + b_i with out = a                     (strides 1, 1)
//            shared     a_i - b_0                                  (strides 1, 0)
//            status     two hex digits: status of add | status of shared << 4
//            per sum i: "S indexed gathered split status"
//            indexed    sum i through pidx and neg
//            gathered   the same terms gathered into a block of their own, pidx == NULL
//            split      sum i cut into three partial sums (sum_points_partial) added by sum_points_finish
#include "../../zkp_amd/csrc/host/host_backend.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void put(const uint8_t* p) {
  for (int i = 0; i < 32; ++i) printf("%02x", p[i]);
  putchar(' ');
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
  if (argc < 3) return 2;
  int rc = 0;
  {
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<uint8_t> av, bv;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
      if (strlen(line) < 129) continue;
      if (!hex32(av, line) || !hex32(bv, line + 65)) return 2;
    }
    fclose(f);
    const size_t n = av.size() / 32;
    if (!n) return 2;
    uint8_t *a = block(32 * n), *b = block(32 * n);
    memcpy(a, av.data(), 32 * n);
    memcpy(b, bv.data(), 32 * n);
    uint8_t *add = block(32 * n), *st_add = block(n), *sub = block(32 * n), *st_sub = block(n);
    zkp::hostbk::add_points_n(n, a, 1, b, 1, ZKP_PT_ADD, add, st_add);
    zkp::hostbk::add_points_n(n, a, 1, b, 1, ZKP_PT_SUB, sub, st_sub);
    uint8_t *inplace = block(32 * n), *st_in = block(n);
    memcpy(inplace, a, 32 * n);
    zkp::hostbk::add_points_n(n, inplace, 1, b, 1, ZKP_PT_ADD, inplace, st_in);
    uint8_t *one_b = block(32), *sh = block(32 * n), *st_sh = block(n);
    memcpy(one_b, b, 32);
    zkp::hostbk::add_points_n(n, a, 1, one_b, 0, ZKP_PT_SUB, sh, st_sh);
    for (size_t i = 0; i < n; ++i) {
      if (st_add[i] != st_sub[i] || st_add[i] != st_in[i]) rc = 3;
      printf("P ");
      put(add + 32 * i); put(sub + 32 * i); put(inplace + 32 * i); put(sh + 32 * i);
      printf("%02x\n", (unsigned)(st_add[i] | (st_sh[i] << 4)));
    }
    zkp::hostbk::add_points_n(0, nullptr, 1, nullptr, 1, ZKP_PT_ADD, nullptr, nullptr);      // an empty call touches nothing
    for (uint8_t* p : {a, b, add, st_add, sub, st_sub, inplace, st_in, one_b, sh, st_sh}) free(p);
  }
  {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned n_sums, n_terms, n_points;
    if (fscanf(f, "%u %u %u", &n_sums, &n_terms, &n_points) != 3) return 2;
    uint32_t* off = reinterpret_cast<uint32_t*>(block(4 * (size_t)(n_sums + 1)));
    uint32_t* pidx = reinterpret_cast<uint32_t*>(block(4 * (size_t)n_terms));
    uint8_t* neg = block(n_terms);
    uint8_t* pts = block(32 * (size_t)n_points);
    for (unsigned i = 0; i <= n_sums; ++i) if (fscanf(f, "%u", &off[i]) != 1) return 2;
    for (unsigned i = 0; i < n_terms; ++i) if (fscanf(f, "%u", &pidx[i]) != 1) return 2;
    for (unsigned i = 0; i < n_terms; ++i) { unsigned v; if (fscanf(f, "%u", &v) != 1) return 2; neg[i] = (uint8_t)v; }
    for (unsigned i = 0; i < n_points; ++i) {
      char hex[80];
      std::vector<uint8_t> row;
      if (fscanf(f, "%79s", hex) != 1 || strlen(hex) != 64 || !hex32(row, hex)) return 2;
      memcpy(pts + 32 * (size_t)i, row.data(), 32);
    }
    fclose(f);
    uint8_t *ind = block(32 * (size_t)n_sums), *st_ind = block(n_sums);
    zkp::hostbk::sum_points_n(n_sums, off, pidx, neg, pts, ind, st_ind);
    uint8_t* gathered = block(32 * (size_t)n_terms);
    for (unsigned t = 0; t < n_terms; ++t) memcpy(gathered + 32 * (size_t)t, pts + 32 * (size_t)pidx[t], 32);
    uint8_t *gat = block(32 * (size_t)n_sums), *st_gat = block(n_sums);
    zkp::hostbk::sum_points_n(n_sums, off, nullptr, neg, gathered, gat, st_gat);
    // sums of more than 4 terms are skipped when asked for: neither out nor status is written
    uint8_t *skip = block(32 * (size_t)n_sums), *st_skip = block(n_sums);
    memset(skip, 0xee, 32 * (size_t)n_sums);
    memset(st_skip, 0xee, n_sums);
    zkp::hostbk::sum_points_n(n_sums, off, pidx, neg, pts, skip, st_skip, 4);
    for (unsigned i = 0; i < n_sums; ++i) {
      const uint32_t lo = off[i], hi = off[i + 1], len = hi - lo;
      uint8_t* partials = block(3 * zkp::hostbk::SUM_PARTIAL_BYTES);
      const uint32_t c1 = lo + len / 3, c2 = lo + 2 * (len / 3);
      zkp::hostbk::sum_points_partial(lo, c1, pidx, neg, pts, partials);
      zkp::hostbk::sum_points_partial(c1, c2, pidx, neg, pts, partials + zkp::hostbk::SUM_PARTIAL_BYTES);
      zkp::hostbk::sum_points_partial(c2, hi, pidx, neg, pts, partials + 2 * zkp::hostbk::SUM_PARTIAL_BYTES);
      uint8_t *split = block(32), *st_split = block(1);
      zkp::hostbk::sum_points_finish(3, partials, split, st_split);
      if (st_ind[i] != st_gat[i] || st_ind[i] != *st_split) rc = 3;
      if (len > 4 ? (skip[32 * (size_t)i] != 0xee || st_skip[i] != 0xee) : (memcmp(skip + 32 * (size_t)i, ind + 32 * (size_t)i, 32) != 0 || st_skip[i] != st_ind[i])) rc = 4;
      printf("S ");
      put(ind + 32 * (size_t)i); put(gat + 32 * (size_t)i); put(split);
      printf("%02x\n", (unsigned)st_ind[i]);
      for (uint8_t* p : {partials, split, st_split}) free(p);
    }
    zkp::hostbk::sum_points_n(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    for (uint8_t* p : {reinterpret_cast<uint8_t*>(off), reinterpret_cast<uint8_t*>(pidx), neg, pts, ind, st_ind, gathered, gat, st_gat, skip, st_skip}) free(p);
  }
  return rc;
}
