// Probe of the 4-lane cooperative point arithmetic (zkp_amd/csrc/quad.h) on chosen limbs: quad_probe IN OUT, one quad of lanes per record.
// IN = records of 2 x 4 x 9 raw limbs: p (X, Y, Z, T) and a second operand s, which is used as a point (q_add), as a cached operand
// (q_add_cached) and, its rows 0, 1 and 3, as an affine niels triple (y+x, y-x, 2dxy: q_load_niels).  OUT = QUAD_OPS x 4 x 9 limbs per record:
// q_double(p), q_add_cached(p, s), q_add(p, s), q_to_cached(p), q_add_cached(p, niels(s)), q_add_cached(p, -niels(s)).
// tests/test_gpu_row_quad_probe.py compares OUT byte for byte with the host build of fe25519.h making the same calls lane by lane
// (tests/host/fe_core_host_lib.cpp: t_quad_probe).  tools/microbench/README.md has the compile command.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../zkp_amd/csrc/fe_constants.h"
#include "../../zkp_amd/csrc/quad.h"
using namespace zkp;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

constexpr uint32_t QUAD_OPS = 6;

__device__ __forceinline__ void probe_store(uint32_t* p, const fe& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) p[i] = a.v[i];
}

__global__ void __launch_bounds__(256) k_quad_probe(uint32_t n, const uint32_t* __restrict__ in, const dev_niels* __restrict__ niels, uint32_t* __restrict__ out) {
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = gt >> 2;
  const int q = (int)(gt & 3u);
  if (i >= n) return;                                   // (whole quads leave together)
  qpt p, s, r;
  qcached c;
#pragma unroll
  for (int k = 0; k < 9; ++k) { p.c.v[k] = in[(size_t)i * 72 + 9 * q + k]; s.c.v[k] = in[(size_t)i * 72 + 36 + 9 * q + k]; }
  uint32_t* o = out + (size_t)i * QUAD_OPS * 36 + 9 * q;
  q_double(r, p, q);
  probe_store(o, r.c);
  c.c = s.c;
  q_add_cached(r, p, c, q);
  probe_store(o + 36, r.c);
  q_add(r, p, s, q);
  probe_store(o + 72, r.c);
  q_to_cached(c, p, q);
  probe_store(o + 108, c.c);
  q_load_niels(c, niels + i, q, 0u);
  q_add_cached(r, p, c, q);
  probe_store(o + 144, r.c);
  q_load_niels(c, niels + i, q, 1u);
  q_add_cached(r, p, c, q);
  probe_store(o + 180, r.c);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: quad_probe IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint32_t> in;
  uint32_t rec[72];
  while (fread(rec, sizeof(rec), 1, f) == 1) in.insert(in.end(), rec, rec + 72);
  fclose(f);
  const uint32_t n = (uint32_t)(in.size() / 72);
  if (!n || n > (1u << 20)) { fprintf(stderr, "no records, or too many\n"); return 2; }
  std::vector<dev_niels> nl(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* s = in.data() + (size_t)i * 72 + 36;
    for (int k = 0; k < 9; ++k) { nl[i].ypx[k] = s[k]; nl[i].ymx[k] = s[9 + k]; nl[i].xy2d[k] = s[27 + k]; }
    nl[i].valid = 1;
  }
  uint32_t *d_in, *d_out;
  dev_niels* d_nl;
  const size_t r_words = (size_t)n * QUAD_OPS * 36;
  CK(hipMalloc(&d_in, in.size() * 4)); CK(hipMalloc(&d_nl, nl.size() * sizeof(dev_niels))); CK(hipMalloc(&d_out, r_words * 4));
  CK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_nl, nl.data(), nl.size() * sizeof(dev_niels), hipMemcpyHostToDevice));
  CK(hipMemset(d_out, 0, r_words * 4));
  hipLaunchKernelGGL(k_quad_probe, dim3((n * 4 + 255) / 256), dim3(256), 0, 0, n, d_in, d_nl, d_out);
  CK(hipGetLastError()); CK(hipDeviceSynchronize());
  std::vector<uint32_t> out(r_words);
  CK(hipMemcpy(out.data(), d_out, r_words * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) { perror(argv[2]); return 2; }
  printf("quad_probe: %u records\n", n);
  return 0;
}
