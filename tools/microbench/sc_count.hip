// What does ONE call of the scalar functions of zkp_amd/csrc/sc25519.h compile to?  Kernels that load operands, call the function and store the
// result; read the ISA and count the v_ lines and the v_mad_u64_u32 among them between a kernel's label and its s_endpgm:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -I zkp_amd/csrc tools/microbench/sc_count.hip -o sc_count.s
// -DSC_COUNT_TWO_MONT compiles the forms the callers had before the one-pass reduction (sc_mul + sc_add, sc_to_mont + sc_mont); with -I pointing
// at an older copy of the header it counts that header (profiles/r09_ab_experiments.txt, block g).
#include <hip/hip_runtime.h>
#include "sc25519.h"
using namespace zkp;
#define LD(X_, p) for (int i = 0; i < 8; ++i) X_.v[i] = p[8 * (blockIdx.x * blockDim.x + threadIdx.x) + i]
#define ST(X_, p) for (int i = 0; i < 8; ++i) p[8 * (blockIdx.x * blockDim.x + threadIdx.x) + i] = X_.v[i]
extern "C" __global__ void __launch_bounds__(256) k_muladd(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* o) {
  sc x, y, z, r; LD(x, a); LD(y, b); LD(z, c);
#ifdef SC_COUNT_TWO_MONT
  sc_mul(r, x, y); sc_add(r, r, z);
#else
  sc_muladd(r, x, y, z);
#endif
  ST(r, o);
}
extern "C" __global__ void __launch_bounds__(256) k_wide(const uint32_t* a, const uint32_t* b, uint32_t* o) {
  sc x, y, r; LD(x, a); LD(y, b); sc_from_wide(r, x, y); ST(r, o);
}
extern "C" __global__ void __launch_bounds__(256) k_w128(const uint32_t* a, const uint32_t* b, uint32_t* o) {
  sc x, y, r; LD(x, a); LD(y, b);
#ifdef SC_COUNT_TWO_MONT
  sc rm; y.v[4] = y.v[5] = y.v[6] = y.v[7] = 0; sc_to_mont(rm, y); sc_mont(r, x, rm);
#else
  sc_mul_u128(r, x, y.v);
#endif
  ST(r, o);
}
extern "C" __global__ void __launch_bounds__(256) k_mont(const uint32_t* a, const uint32_t* b, uint32_t* o) {
  sc x, y, r; LD(x, a); LD(y, b); sc_mont(r, x, y); ST(r, o);
}
