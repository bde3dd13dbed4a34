// The one-lane comb-table builder (zkp_amd/csrc/comb_tables.h: comb_table_lane) with the carry tooth skipped behind a KERNEL ARGUMENT, the form that
// AMD clang 22.0.0git (ROCm 7.2.0; roc-7.2.0 26014) compiled wrongly for gfx950 at -O3.  Kept as a reproducer; nothing in the library uses it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -c tools/microbench/lane_builder_miscompile.hip -o /tmp/lbm.o
//   clang-offload-bundler --unbundle --type=o --input=/tmp/lbm.o --targets=hip-amdgcn-amd-amdhsa--gfx950 --output=/tmp/lbm.elf
//   llvm-objdump -d /tmp/lbm.elf | less          # k_lane_runtime_flag<16>
//
// What to look for: the kernel loads the point (x[9] y[9] t[9]) with seven global_load_dwordx4; the one at offset:60 brings y[6], y[7], y[8], t[0] into
// four consecutive registers, the one at offset:32 brings x[8], y[0], y[1], y[2].  The first entry's Y + X then needs  x[8] + y[8]  and  x[0] + y[0].
// In the wrong code the sum x[0] + y[0] is WRITTEN INTO the register that holds y[8] one instruction BEFORE x[8] + y[8] reads it:
//     v_add_u32_e32 v42, v48, v37        ; x0 + y0 -> v42, which held y8
//     v_add_u32_e32 v61, v36, v42        ; x8 + (x0 + y0)
// (in comb_table_lane<16, false> and <16, true> of the library the two sums go to registers of their own).  No source construct explains a lost
// write-after-read dependency between two VALU instructions; the kernel has no aliasing pointers at that place (pts is read, comb is written later).
#include <hip/hip_runtime.h>
#include "../../zkp_amd/csrc/dev_layout.h"
#include "../../zkp_amd/csrc/sc25519.h"
#include "../../zkp_amd/csrc/hot_tables.h"
#include "../../zkp_amd/csrc/quad.h"
#include "../../zkp_amd/csrc/rowfe.h"
#include "../../zkp_amd/csrc/comb_tables.h"

namespace zkp {
template <int TEETH>
__global__ void __launch_bounds__(256, 2)
k_lane_runtime_flag(const uint32_t* __restrict__ n_slots, uint32_t max_tables, const uint32_t* __restrict__ slot_pt,
                    const dev_affine* __restrict__ pts, dev_ext* __restrict__ comb, uint32_t no_carry) {
  using cfg = comb_cfg<TEETH>;
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ns = min(*n_slots, max_tables);
  if (slot >= ns) return;
  if (slot_pt[slot] & STMT_ABSORBED) return;
  ge_p3 base;
  load_affine(base, pts + slot_pt[slot]);
  dev_ext* tbl = comb + (size_t)slot * cfg::ENTRIES;
#pragma unroll 1
  for (int j = 0; j < TEETH; ++j) {
    ge_p3 m2, m3, m4, m;
    ge_cached c1, c;
    ge_to_cached(c1, base);
    store_comb_entry(tbl + 8 * j + 0, c1);
    ge_double<true>(m2, base);
    ge_to_cached(c, m2); store_comb_entry(tbl + 8 * j + 1, c);
    ge_add_cached(m3, m2, c1);
    ge_to_cached(c, m3); store_comb_entry(tbl + 8 * j + 2, c);
    ge_double<true>(m4, m2);
    ge_to_cached(c, m4); store_comb_entry(tbl + 8 * j + 3, c);
    ge_add_cached(m, m4, c1);
    ge_to_cached(c, m); store_comb_entry(tbl + 8 * j + 4, c);
    ge_double<true>(m, m3);
    ge_to_cached(c, m); store_comb_entry(tbl + 8 * j + 5, c);
    ge_add_cached(m, m, c1);
    ge_to_cached(c, m); store_comb_entry(tbl + 8 * j + 6, c);
    ge_double<true>(base, m4);
    ge_to_cached(c, base); store_comb_entry(tbl + 8 * j + 7, c);
    if (no_carry && j == TEETH - 1) return;
#pragma unroll 1
    for (int d = 0; d < cfg::BITS - 4; ++d) ge_double<false>(base, base);
    ge_double<true>(base, base);
  }
  ge_cached c;
  ge_to_cached(c, base);
  store_comb_entry(tbl + 8 * TEETH, c);
}
template __global__ void k_lane_runtime_flag<16>(const uint32_t*, uint32_t, const uint32_t*, const dev_affine*, dev_ext*, uint32_t);
}  // namespace zkp
