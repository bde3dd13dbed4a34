// Probe kernels for the scalar layer: each loads its operands, calls ONE function of zkp_amd/csrc/sc25519.h and stores the result.  On the
// device that header runs in k_wide_reduce, k_neg_reduce, k_blind_scalars, k_responses, the batch verifier's coefficient build and every
// recoder, on operands (hash outputs, ChaCha words) no test can steer to the edges of the Montgomery code; here the operands come from a file.
// tools/microbench/README.md has the compile command.
//   sc_probe IN OUT      IN = records of 24 words: three 256-bit values (a, b, c);  OUT = 16 blocks of 8 words per record
// With a' = sc_reduce(a), b' = sc_reduce(b), c' = sc_reduce(c) (computed here, so that every precondition "< l" holds):
//   block 0 sc_reduce(a)      1 sc_to_mont(a)       2 sc_mont(a, b')        3 sc_mul(a, b')       4 sc_add(a', b')      5 sc_neg(a')
//         6 sc_from_wide(lo = a, hi = b)            7 sc_halve(a)           8 sc_halve_canonical(a')                   9 a after sc_fold_sign
//        10 word 0: the fold flag, word 1: sc_not_canonical(a)              11 .. 13 e of sc_add_pattern(a, p), p = 0x88888888, 0xAAAAAAAA, 0x80808080
//        14 words 0 .. 2: `top` of the three                                15 sc_mul(a, c') + b'  (the response of k_responses)
// tests/test_gpu_sc_probe.py compares OUT with Python integers; tests/test_host_scalar_edges.py does the same for the host build of the header.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../zkp_amd/csrc/sc25519.h"
using namespace zkp;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

constexpr uint32_t IN_WORDS = 24, OUT_WORDS = 128;

__device__ __forceinline__ void probe_load(sc& a, const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) a.v[i] = p[i];
}
__device__ __forceinline__ void probe_store(uint32_t* p, const sc& a) {
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = a.v[i];
}
constexpr uint32_t probe_pattern(int op) { return op == 11 ? 0x88888888u : op == 12 ? 0xAAAAAAAAu : 0x80808080u; }

// OP = the block it fills (10 and 14 are filled by 9 and 11 .. 13)
template <int OP>
__global__ void __launch_bounds__(64) k_probe(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  sc a, b, c, r;
  probe_load(a, in + (size_t)i * IN_WORDS);
  probe_load(b, in + (size_t)i * IN_WORDS + 8);
  probe_load(c, in + (size_t)i * IN_WORDS + 16);
  uint32_t* o = out + (size_t)i * OUT_WORDS;
  if (OP == 0) sc_reduce(r, a);
  else if (OP == 1) sc_to_mont(r, a);
  else if (OP == 2) { sc_reduce(b, b); sc_mont(r, a, b); }
  else if (OP == 3) { sc_reduce(b, b); sc_mul(r, a, b); }
  else if (OP == 4) { sc_reduce(a, a); sc_reduce(b, b); sc_add(r, a, b); }
  else if (OP == 5) { sc_reduce(a, a); sc_neg(r, a); }
  else if (OP == 6) sc_from_wide(r, a, b);
  else if (OP == 7) sc_halve(r, a);
  else if (OP == 8) { sc_reduce(a, a); sc_halve_canonical(r, a); }
  else if (OP == 9) { r = a; o[80] = sc_fold_sign(r.v); }
  else if (OP == 10) { o[81] = sc_not_canonical(a.v); return; }
  else if (OP >= 11 && OP <= 13) { uint32_t top; sc_add_pattern(r.v, top, a.v, probe_pattern(OP)); o[112 + (OP - 11)] = top; }
  else { sc t; sc_reduce(b, b); sc_reduce(c, c); sc_mul(t, a, c); sc_add(r, t, b); }
  probe_store(o + 8 * OP, r);
}

template <int OP>
static void launch(uint32_t n, const uint32_t* d_in, uint32_t* d_out) {
  hipLaunchKernelGGL(k_probe<OP>, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_in, d_out);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: sc_probe IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint32_t> in;
  uint32_t rec[IN_WORDS];
  while (fread(rec, sizeof(rec), 1, f) == 1) in.insert(in.end(), rec, rec + IN_WORDS);
  fclose(f);
  const uint32_t n = (uint32_t)(in.size() / IN_WORDS);
  if (!n) { fprintf(stderr, "no records\n"); return 2; }
  uint32_t *d_in, *d_out;
  CK(hipMalloc(&d_in, in.size() * 4)); CK(hipMalloc(&d_out, (size_t)n * OUT_WORDS * 4));
  CK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(d_out, 0, (size_t)n * OUT_WORDS * 4));
  launch<0>(n, d_in, d_out); launch<1>(n, d_in, d_out); launch<2>(n, d_in, d_out); launch<3>(n, d_in, d_out);
  launch<4>(n, d_in, d_out); launch<5>(n, d_in, d_out); launch<6>(n, d_in, d_out); launch<7>(n, d_in, d_out);
  launch<8>(n, d_in, d_out); launch<9>(n, d_in, d_out); launch<10>(n, d_in, d_out); launch<11>(n, d_in, d_out);
  launch<12>(n, d_in, d_out); launch<13>(n, d_in, d_out); launch<15>(n, d_in, d_out);
  CK(hipGetLastError()); CK(hipDeviceSynchronize());
  std::vector<uint32_t> out((size_t)n * OUT_WORDS);
  CK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) { perror(argv[2]); return 2; }
  printf("sc_probe: %u records\n", n);
  return 0;
}
