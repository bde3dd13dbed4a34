// Probe of the one-limb-per-lane arithmetic (zkp_amd/csrc/rowfe.h) on chosen register images: row_probe IN OUT pushes an operand file through
// every function of the header, one wavefront per record, and writes every result as a full 64-lane image, idle lanes included.
// tests/test_gpu_row_quad_probe.py compares OUT byte for byte with tools/model/rowfe_model.py run on the same file (tests/row_quad_cases.py
// makes the operands: limb-class maxima, single-limb maxima, non-canonical zeros, curve points).  Built a second time with
// -DZKP_AB_ROW_BPERMUTE (the kept A/B variant of the moves between rows) it must write the same bytes.  tools/microbench/README.md has the
// compile command.
//
// IN (32-bit words):  header n_main, n_inv, n_horner, 0
//   n_main   x { op mask, a[64], b[64] }                       lanes 9 .. 15 of every row of a are zero, those of b are anything
//   n_inv    x { a[64] }
//   n_horner x { W, C, top[64], cached[ROW_MAX_W][64] }        the chain of k_pip_combine: W windows of C doublings and a cached addition
// OUT: n_main x ROW_OPS images (an operation the mask leaves out: zeros), n_inv images (row_invert), n_horner images.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../zkp_amd/csrc/fe_constants.h"
#include "../../zkp_amd/csrc/rowfe.h"
using namespace zkp;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

// images of a main record, in order: row_mul(a, b), row_mul(a, a), row_carry(a), row_double(a), row_add_cached(a, b), 11 doublings of a then
// row_add_cached(., b), row_sqn(a, 5), row_bcast01(a) .a .b, row_bcast23(a) .a .b, row_bcast_all(a) .r0 .. .r3
constexpr uint32_t ROW_OPS = 15, ROW_MAIN_WORDS = 129, ROW_MAX_W = 37, ROW_MAX_C = 16, ROW_HORNER_WORDS = 2 + 64 * (1 + ROW_MAX_W);
// mask bits: which operations a record's classes admit (the moves between rows run on every record)
constexpr uint32_t OP_MUL_AB = 1, OP_MUL_AA = 2, OP_CARRY = 4, OP_POINT = 8, OP_SQN = 16;

__global__ void __launch_bounds__(64) k_row_main(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const uint32_t* rec = in + (size_t)i * ROW_MAIN_WORDS;
  const uint32_t mask = rec[0], a = rec[1 + lane], b = rec[65 + lane];
  uint32_t* o = out + (size_t)i * ROW_OPS * 64 + lane;
  rowctx rc;
  row_init(rc);
  if (mask & OP_MUL_AB) o[0 * 64] = row_mul(rc, a, b);
  if (mask & OP_MUL_AA) o[1 * 64] = row_mul(rc, a, a);
  if (mask & OP_CARRY) o[2 * 64] = row_carry(rc, a);
  if (mask & OP_POINT) {
    o[3 * 64] = row_double(rc, a);
    o[4 * 64] = row_add_cached(rc, a, b);
    uint32_t r = a;
#pragma unroll 1
    for (int d = 0; d < 11; ++d) r = row_double(rc, r);
    o[5 * 64] = row_add_cached(rc, r, b);
  }
  if (mask & OP_SQN) o[6 * 64] = row_sqn(rc, a, 5);
  const rowpair p01 = row_bcast01(rc, a), p23 = row_bcast23(rc, a);
  const rowquad q = row_bcast_all(rc, a);
  o[7 * 64] = p01.a; o[8 * 64] = p01.b;
  o[9 * 64] = p23.a; o[10 * 64] = p23.b;
  o[11 * 64] = q.r0; o[12 * 64] = q.r1; o[13 * 64] = q.r2; o[14 * 64] = q.r3;
}

__global__ void __launch_bounds__(64) k_row_invert(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  rowctx rc;
  row_init(rc);
  out[(size_t)i * 64 + lane] = row_invert(rc, in[(size_t)i * 64 + lane]);
}

__global__ void __launch_bounds__(64) k_row_horner(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const uint32_t* rec = in + (size_t)i * ROW_HORNER_WORDS;
  const int W = (int)rec[0], C = (int)rec[1];
  if (W < 1 || W > (int)ROW_MAX_W || C < 1 || C > (int)ROW_MAX_C) return;       // (main refuses such a file before any launch)
  rowctx rc;
  row_init(rc);
  uint32_t acc = rec[2 + lane];
#pragma unroll 1
  for (int k = W - 1; k >= 0; --k) {
#pragma unroll 1
    for (int d = 0; d < C; ++d) acc = row_double(rc, acc);
    acc = row_add_cached(rc, acc, rec[2 + 64 * (1 + k) + lane]);
  }
  out[(size_t)i * 64 + lane] = acc;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: row_probe IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint32_t> in;
  uint32_t buf[4096];
  size_t got;
  while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  if (in.size() < 4) { fprintf(stderr, "no header\n"); return 2; }
  const uint32_t n_main = in[0], n_inv = in[1], n_horner = in[2];
  if (n_main > (1u << 16) || n_inv > (1u << 16) || n_horner > (1u << 12)) { fprintf(stderr, "too many records\n"); return 2; }
  const size_t o_main = 4, o_inv = o_main + (size_t)n_main * ROW_MAIN_WORDS, o_horner = o_inv + (size_t)n_inv * 64;
  const size_t words = o_horner + (size_t)n_horner * ROW_HORNER_WORDS;
  if (in.size() != words || !(n_main + n_inv + n_horner)) { fprintf(stderr, "operand file: %zu words, header says %zu\n", in.size(), words); return 2; }
  for (uint32_t i = 0; i < n_horner; ++i) {
    const uint32_t W = in[o_horner + (size_t)i * ROW_HORNER_WORDS], C = in[o_horner + (size_t)i * ROW_HORNER_WORDS + 1];
    if (W < 1 || W > ROW_MAX_W || C < 1 || C > ROW_MAX_C) { fprintf(stderr, "horner record %u: W = %u, C = %u\n", i, W, C); return 2; }
  }
  const size_t r_inv = (size_t)n_main * ROW_OPS * 64, r_horner = r_inv + (size_t)n_inv * 64, r_words = r_horner + (size_t)n_horner * 64;
  uint32_t *d_in, *d_out;
  CK(hipMalloc(&d_in, in.size() * 4)); CK(hipMalloc(&d_out, r_words * 4));
  CK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(d_out, 0, r_words * 4));
  if (n_main) hipLaunchKernelGGL(k_row_main, dim3(n_main), dim3(64), 0, 0, n_main, d_in + o_main, d_out);
  if (n_inv) hipLaunchKernelGGL(k_row_invert, dim3(n_inv), dim3(64), 0, 0, n_inv, d_in + o_inv, d_out + r_inv);
  if (n_horner) hipLaunchKernelGGL(k_row_horner, dim3(n_horner), dim3(64), 0, 0, n_horner, d_in + o_horner, d_out + r_horner);
  CK(hipGetLastError()); CK(hipDeviceSynchronize());
  std::vector<uint32_t> out(r_words);
  CK(hipMemcpy(out.data(), d_out, r_words * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) { perror(argv[2]); return 2; }
  printf("row_probe: %u + %u + %u records\n", n_main, n_inv, n_horner);
  return 0;
}
