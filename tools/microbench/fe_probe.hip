// Probe kernels for reading the ISA of the field core: each loads its operands, calls ONE function of
// zkp_amd/csrc/fe25519.h and stores the result, so the VALU count of the kernel is the count of that function
// plus a fixed load / store frame (k_probe_frame).  tools/microbench/README.md has the compile command.
// Run as a program it pushes an operand file through the kernels (the device path of the field core has pinned
// mads the host path does not): fe_probe IN OUT, IN = records of 18 raw limbs (a, b), OUT = 6 x 9 limbs per record
// (a*b, b*a, a^2, a^(2^5), a^(2^10), a*d with the curve constant d: the multiplication by a constant stays on the compiler's path); tests/test_gpu_fe_core.py compares OUT with the host build of the same header.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../zkp_amd/csrc/fe_constants.h"
using namespace zkp;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

__device__ __forceinline__ void probe_load(fe& a, const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 9; ++i) a.v[i] = p[i];
}
__device__ __forceinline__ void probe_store(uint32_t* p, const fe& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) p[i] = a.v[i];
}

// OP: 0 frame only (a limb-wise add), 1 fe_mul, 2 fe_sq, 3 three squarings back to back, 4 fe_sqn(5), 5 fe_sqn(10),
// 6 fe_sqn(n) with n at run time, 7 fe_mul with the operands swapped, 8 fe_mul by a field constant (FE_D)
template <int OP>
__global__ void __launch_bounds__(64) k_probe(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t stride, int sqn) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  fe a, b, r;
  probe_load(a, in + (size_t)i * 18);
  probe_load(b, in + (size_t)i * 18 + 9);
  if (OP == 0) fe_add(r, a, b);
  else if (OP == 1) fe_mul(r, a, b);
  else if (OP == 2) fe_sq(r, a);
  else if (OP == 3) { fe_sq(r, a); fe_sq(r, r); fe_sq(r, r); }
  else if (OP == 4) fe_sqn(r, a, 5);
  else if (OP == 5) fe_sqn(r, a, 10);
  else if (OP == 6) fe_sqn(r, a, sqn);
  else if (OP == 7) fe_mul(r, b, a);
  else { fe d; fe_from_const(d, FE_D); fe_mul(r, a, d); }
  probe_store(out + (size_t)i * stride, r);
}
template __global__ void k_probe<0>(uint32_t, const uint32_t*, uint32_t*, uint32_t, int);
template __global__ void k_probe<3>(uint32_t, const uint32_t*, uint32_t*, uint32_t, int);
template __global__ void k_probe<6>(uint32_t, const uint32_t*, uint32_t*, uint32_t, int);

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: fe_probe IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint32_t> in;
  uint32_t rec[18];
  while (fread(rec, sizeof(rec), 1, f) == 1) in.insert(in.end(), rec, rec + 18);
  fclose(f);
  const uint32_t n = (uint32_t)(in.size() / 18);
  if (!n) { fprintf(stderr, "no records\n"); return 2; }
  uint32_t *d_in, *d_out;
  CK(hipMalloc(&d_in, in.size() * 4)); CK(hipMalloc(&d_out, (size_t)n * 54 * 4));
  CK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  const dim3 grid((n + 63) / 64), block(64);
  hipLaunchKernelGGL(k_probe<1>, grid, block, 0, 0, n, d_in, d_out, 54u, 0);
  hipLaunchKernelGGL(k_probe<7>, grid, block, 0, 0, n, d_in, d_out + 9, 54u, 0);
  hipLaunchKernelGGL(k_probe<2>, grid, block, 0, 0, n, d_in, d_out + 18, 54u, 0);
  hipLaunchKernelGGL(k_probe<4>, grid, block, 0, 0, n, d_in, d_out + 27, 54u, 0);
  hipLaunchKernelGGL(k_probe<5>, grid, block, 0, 0, n, d_in, d_out + 36, 54u, 0);
  hipLaunchKernelGGL(k_probe<8>, grid, block, 0, 0, n, d_in, d_out + 45, 54u, 0);
  CK(hipGetLastError()); CK(hipDeviceSynchronize());
  std::vector<uint32_t> out((size_t)n * 54);
  CK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) { perror(argv[2]); return 2; }
  printf("fe_probe: %u records\n", n);
  return 0;
}
