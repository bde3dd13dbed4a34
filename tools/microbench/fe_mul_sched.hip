// How fast does a wave get through field multiplications and squarings, as a function of how the carries of the
// low columns travel, of the number of independent multiplications in flight per wave and of the waves per SIMD?
//   ripple : every column summed on its own (row-major), then c[k+1] += c[k] >> 29 down the columns: 8 extra 64-bit
//            adds per multiplication, short dependent chains (the library's formulation up to round 6)
//   thread : high columns first, then the low columns in sequence, column k's carry the initial addend of column
//            k+1's v_mad_u64_u32 chain: no adds, one dependent chain of ~60 mads (the library's fe_mul / fe_sq)
// CHAINS = 1 is a lone dependent chain; CHAINS = 4 is four independent ones, the shape of ge_add_cached / ge_madd.
// (The earlier question of this file, column-major against row-major product order, is answered in README.md.)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "../../zkp_amd/csrc/fe25519.h"
using namespace zkp;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

__device__ __forceinline__ void reduce_ripple(fe& r, uint64_t c[9]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c[k + 1] += c[k] >> 29;
    r.v[k] = (uint32_t)c[k] & FE_M29;
  }
  r.v[8] = (uint32_t)c[8] & FE_M23;
  const uint64_t t = c[8] >> 23;
  const uint64_t c0 = (uint64_t)r.v[0] + 19ull * (uint32_t)t;
  r.v[0] = (uint32_t)c0 & FE_M29;
  r.v[1] += (uint32_t)(c0 >> 29) + 152u * (uint32_t)(t >> 32);
}
__device__ __forceinline__ void fe_mul_ripple(fe& r, const fe& a, const fe& b) {
  uint64_t c[17];
#pragma unroll
  for (int k = 0; k < 17; ++k) c[k] = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
#pragma unroll
    for (int j = 0; j < 9; ++j) c[i + j] += (uint64_t)a.v[i] * b.v[j];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c[k] += 1216ull * (uint32_t)c[k + 9];
    c[k + 1] += 9728ull * (uint32_t)(c[k + 9] >> 32);
  }
  reduce_ripple(r, c);
}
__device__ __forceinline__ void fe_sq_ripple(fe& r, const fe& a) {
  uint32_t a2[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) a2[i] = a.v[i] << 1;
  uint64_t c[9], h[8];
#pragma unroll
  for (int k = 9; k < 17; ++k) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = k - 8; 2 * i < k; ++i) acc += (uint64_t)a2[i] * a.v[k - i];
    if ((k & 1) == 0) acc += (uint64_t)a.v[k / 2] * a.v[k / 2];
    h[k - 9] = acc;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; 2 * i < k; ++i) acc += (uint64_t)a2[i] * a.v[k - i];
    if ((k & 1) == 0) acc += (uint64_t)a.v[k / 2] * a.v[k / 2];
    if (k <= 7) acc += 1216ull * (uint32_t)h[k];
    if (k >= 1) acc += 9728ull * (uint32_t)(h[k - 1] >> 32);
    c[k] = acc;
  }
  reduce_ripple(r, c);
}

// VARIANT: 0 mul ripple, 1 mul thread, 2 sq ripple, 3 sq thread
template <int VARIANT, int CHAINS>
__global__ void __launch_bounds__(64) k_chain(uint32_t* io, int iters) {
  fe a[CHAINS], b;
#pragma unroll
  for (int i = 0; i < 9; ++i) b.v[i] = io[640 + threadIdx.x * 9 + i] & 0x1fffffff;
#pragma unroll
  for (int c = 0; c < CHAINS; ++c)
#pragma unroll
    for (int i = 0; i < 9; ++i) a[c].v[i] = (io[threadIdx.x * 9 + i] + 977u * c) & 0x1fffffff;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) {
      if (VARIANT == 0) fe_mul_ripple(a[c], a[c], b);
      else if (VARIANT == 1) fe_mul(a[c], a[c], b);
      else if (VARIANT == 2) fe_sq_ripple(a[c], a[c]);
      else fe_sq(a[c], a[c]);
    }
  }
#pragma unroll
  for (int c = 1; c < CHAINS; ++c) fe_add(a[0], a[0], a[c]);
#pragma unroll
  for (int i = 0; i < 9; ++i) io[(blockIdx.x * 64 + threadIdx.x) * 9 + i] = a[0].v[i];
}

template <int V, int CHAINS>
void run(const char* name, uint32_t* d, int waves_per_simd) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int iters = 20000 / CHAINS;
  const int blocks = 256 * 4 * waves_per_simd;
  for (int rep = 0; rep < 2; ++rep) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_chain<V, CHAINS>), dim3(blocks), dim3(64), 0, 0, d, iters);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    if (rep) printf("%-10s chains %d waves/SIMD %d : %8.3f ms  -> %7.1f ns per field op per wave, %6.1f G field-ops/s chip\n", name, CHAINS, waves_per_simd, ms,
                    ms * 1e6 / (iters * CHAINS), (double)blocks * 64 * iters * CHAINS / (ms * 1e-3) * 1e-9);
  }
}
int main() {
  uint32_t* d; CK(hipMalloc(&d, 256 * 4 * 8 * 64 * 9 * 4 + 65536)); CK(hipMemset(d, 0x5a, 65536));
  for (int w : {1, 2, 4, 8}) {
    run<0, 1>("mul-ripple", d, w); run<1, 1>("mul-thread", d, w); run<2, 1>("sq-ripple", d, w); run<3, 1>("sq-thread", d, w);
    run<0, 4>("mul-ripple", d, w); run<1, 4>("mul-thread", d, w); run<2, 4>("sq-ripple", d, w); run<3, 4>("sq-thread", d, w);
  }
  return 0;
}
