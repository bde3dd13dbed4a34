// or_flows.h -- zkp_or_prove / zkp_or_verify and their _dev forms (zkp_or_mi355x.h): the batched 1-of-k OR-proofs.  Included at the end of
// zkp_kernels.hip (one translation unit: shares zkp_ctx, the workspace carving, the staging helper and the term path).  The kernels are
// or_lane.h's; this file is the order of the launches, which is the same whatever `real`, the secrets and the entropy are.
//
// Workspace behind `reserved` (the host-pointer forms' staging): [statement blob | table | off | pidx | coms | MSM status | c | flags |
// rejected | witnesses | drawn | rows] [terms_carve].  The last three regions are the nonce region: one memset clears them.
#pragma once
#include "or_meta.h"

namespace {

struct or_ws { size_t meta, table, off, pidx, coms, mstat, c, flags, rej, wit, drawn, rows, nonce_end, end; };
or_ws or_carve(size_t reserved, const or_meta& M, const or_sizes& z, uint32_t N, bool prover) {
  carve cv;
  cv.off = reserved;
  or_ws w;
  w.meta = cv.take(M.bytes());
  w.table = cv.take(32 * (size_t)z.n_points);
  w.off = cv.take(4 * ((size_t)z.n_msm + 1));
  w.pidx = cv.take(4 * (size_t)z.n_terms);
  w.coms = cv.take(32 * (size_t)z.n_msm);
  w.mstat = cv.take((size_t)z.n_msm);
  w.c = cv.take(32 * (size_t)N);
  w.flags = cv.take((size_t)z.n_blocks);
  w.rej = cv.take((size_t)N);
  w.wit = cv.take(prover ? 32 * (size_t)N * (M.m + 1) : 0);
  w.drawn = cv.take(prover ? 32 * (size_t)N * z.drawn : 0);
  w.rows = cv.take(32 * (size_t)z.n_terms);
  w.nonce_end = cv.off;
  w.end = cv.off;
  return w;
}
terms_cfg or_terms_cfg(zkp_ctx* c, uint32_t n_terms, int flags) {
  terms_cfg k;                                 // the arrays are not inspected on the host: generic bounds, as zkp_msm_many_dev
  k.teeth = c->comb_teeth;
  k.throughput = true;
  k.comb_min = flags == ZKP_CT ? c->ct_comb_min(true, n_terms) : 2u;
  return k;
}
// what both forms check before anything is touched
int or_call_check(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, or_meta& M, or_sizes& z) {
  if (!c) return fail(ZKP_ERR_ARG, "ctx is NULL");
  if (k < 1 || k > ZKP_OR_MAX_BRANCHES) return fail(ZKP_ERR_ARG, "k must be 1 .. ZKP_OR_MAX_BRANCHES");
  if (!or_meta_build(st, M)) return fail(ZKP_ERR_ARG, "malformed statement");
  if (M.nc == 0) return fail(ZKP_ERR_ARG, "a statement without constraints");
  if (!or_sizes_of(M, k, N, z)) return fail(ZKP_ERR_ARG, "N too large: N * k * (terms + constraints) must stay below 2^32");
  if (c->capturing) return fail(ZKP_ERR_ARG, "graph capture: the OR-proof calls upload the statement from host memory and cannot be recorded");
  return ZKP_OK;
}
inline void or_note(zkp_ctx* c, int kind, const char* name) {
  prof_note(c, kind, name);
  prof_mark(c, kind);
}
// the statement blob, the table [common | inst] and the CSR arrays; *s = the items' view
int or_setup(zkp_ctx* c, const or_meta& M, const or_sizes& z, const or_ws& w, uint32_t k, uint32_t N, const uint8_t* d_inst, const uint8_t* d_common,
             or_stmt* s) {
  char* base = static_cast<char*>(c->ws);
  c->or_meta_keep = M.blob;                    // the copy's source outlives the call
  HIP_TRY(hipMemcpyAsync(base + w.meta, c->or_meta_keep.data(), M.bytes(), hipMemcpyHostToDevice, c->stream));
  if (M.ns) HIP_TRY(hipMemcpyAsync(base + w.table, d_common, 32 * (size_t)M.ns, hipMemcpyDeviceToDevice, c->stream));
  if (M.ni) HIP_TRY(hipMemcpyAsync(base + w.table + 32 * (size_t)M.ns, d_inst, 32 * (size_t)z.n_blocks * M.ni, hipMemcpyDeviceToDevice, c->stream));
  *s = M.view(base + w.meta, k, N);
  hipLaunchKernelGGL(k_or_plan, grid1(z.n_blocks, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, *s, reinterpret_cast<uint32_t*>(base + w.off),
                     reinterpret_cast<uint32_t*>(base + w.pidx));
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_plan");
  HIP_TRY(hipGetLastError());
  return ZKP_OK;
}

// the prover's launches on device buffers; the workspace is sized (w.end + the term path's) and prof_begin has run
int or_prove_launches(zkp_ctx* c, const or_meta& M, const or_sizes& z, const or_ws& w, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_secrets,
                      const uint8_t* d_real, const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_entropy, uint8_t* d_chal, uint8_t* d_resp,
                      uint8_t* d_status) {
  uint8_t* base = static_cast<uint8_t*>(c->ws);
  or_stmt s;
  int rc = or_setup(c, M, z, w, k, N, d_inst, d_common, &s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_bind, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, base + w.table, 0u, base + w.rej);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_bind");
  hipLaunchKernelGGL(k_or_witness, grid1(N, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_secrets, d_real, base + w.wit);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_witness");
  HIP_TRY(hipGetLastError());
  strobe_label empty;
  strobe_label_pack(empty, "", 0);
  rc = launch_strobe_witness_rng(c, N, d_ts, empty, M.m + 1, 32, base + w.wit, d_entropy, STROBE_RNG_SCALARS, (uint32_t)z.drawn, base + w.drawn);
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_assemble, grid1(z.n_blocks, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_real, base + w.drawn, base + w.rows);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_assemble");
  HIP_TRY(hipGetLastError());
  rc = msm_terms_path(c, z.n_msm, reinterpret_cast<const uint32_t*>(base + w.off), base + w.rows, reinterpret_cast<const uint32_t*>(base + w.pidx), base + w.table,
                      z.n_points, z.n_terms, ZKP_CT, base + w.coms, base + w.mstat, nullptr, w.end, false, PH_ALL, or_terms_cfg(c, z.n_terms, ZKP_CT));
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_challenge, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, base + w.coms, base + w.rej, base + w.c);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_challenge");
  hipLaunchKernelGGL(k_or_respond, grid1(N, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_real, base + w.drawn, d_secrets, base + w.c, base + w.mstat, d_chal,
                     d_resp, d_status);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_respond");
  HIP_TRY(hipGetLastError());
  return ZKP_OK;
}
// the launches, then the wipe of the nonce region whatever they returned
int or_prove_core(zkp_ctx* c, const or_meta& M, const or_sizes& z, const or_ws& w, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_secrets,
                  const uint8_t* d_real, const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_entropy, uint8_t* d_chal, uint8_t* d_resp,
                  uint8_t* d_status) {
  const int rc = or_prove_launches(c, M, z, w, k, N, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_chal, d_resp, d_status);
  const hipError_t wiped = hipMemsetAsync(static_cast<uint8_t*>(c->ws) + w.wit, 0, w.nonce_end - w.wit, c->stream);
  if (rc) return rc;
  HIP_TRY(wiped);
  return ZKP_OK;
}

int or_verify_core(zkp_ctx* c, const or_meta& M, const or_sizes& z, const or_ws& w, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_inst,
                   const uint8_t* d_common, const uint8_t* d_chal, const uint8_t* d_resp, uint8_t* d_results) {
  uint8_t* base = static_cast<uint8_t*>(c->ws);
  or_stmt s;
  int rc = or_setup(c, M, z, w, k, N, d_inst, d_common, &s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_bind, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, base + w.table, 1u, base + w.rej);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_bind");
  hipLaunchKernelGGL(k_or_check, grid1(z.n_blocks, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_chal, d_resp, base + w.rows, base + w.flags);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_check");
  HIP_TRY(hipGetLastError());
  rc = msm_terms_path(c, z.n_msm, reinterpret_cast<const uint32_t*>(base + w.off), base + w.rows, reinterpret_cast<const uint32_t*>(base + w.pidx), base + w.table,
                      z.n_points, z.n_terms, ZKP_VARTIME, base + w.coms, base + w.mstat, nullptr, w.end, false, PH_ALL, or_terms_cfg(c, z.n_terms, ZKP_VARTIME));
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_challenge, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, base + w.coms, base + w.rej, base + w.c);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_challenge");
  hipLaunchKernelGGL(k_or_verdict, grid1(N, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_chal, base + w.c, base + w.flags, base + w.rej, base + w.mstat,
                     d_results);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_verdict");
  HIP_TRY(hipGetLastError());
  return ZKP_OK;
}

size_t or_total_ws(zkp_ctx* c, const or_ws& w, const or_sizes& z, int flags) {
  return w.end + terms_path_ws(z.n_points, z.n_terms, z.n_msm, or_terms_cfg(c, z.n_terms, flags));
}
inline bool or_all_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (!aligned16(p)) return false;
  return true;
}

}  // namespace

extern "C" {

int zkp_or_prove_dev(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_secrets, const uint8_t* d_real,
                     const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_entropy, uint8_t* d_chal, uint8_t* d_resp, uint8_t* d_status) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!d_ts || !d_real || !d_entropy || !d_chal || !d_status || (M.m && (!d_secrets || !d_resp)) || (M.ni && !d_inst) || (M.ns && !d_common))
    return fail(ZKP_ERR_ARG, "NULL device pointer");
  if (!or_all_aligned16({d_ts, d_secrets, d_inst, d_common, d_chal, d_resp})) return fail(ZKP_ERR_ARG, "device buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  const or_ws w = or_carve(0, M, z, N, true);
  rc = ensure_ws(c, or_total_ws(c, w, z, ZKP_CT));
  if (rc) return rc;
  prof_begin(c);
  return or_prove_core(c, M, z, w, k, N, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_chal, d_resp, d_status);
}

int zkp_or_verify_dev(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_inst, const uint8_t* d_common,
                      const uint8_t* d_chal, const uint8_t* d_resp, uint8_t* d_results) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!d_ts || !d_chal || !d_results || (M.m && !d_resp) || (M.ni && !d_inst) || (M.ns && !d_common)) return fail(ZKP_ERR_ARG, "NULL device pointer");
  if (!or_all_aligned16({d_ts, d_inst, d_common, d_chal, d_resp})) return fail(ZKP_ERR_ARG, "device buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  const or_ws w = or_carve(0, M, z, N, false);
  rc = ensure_ws(c, or_total_ws(c, w, z, ZKP_VARTIME));
  if (rc) return rc;
  prof_begin(c);
  return or_verify_core(c, M, z, w, k, N, d_ts, d_inst, d_common, d_chal, d_resp, d_results);
}

int zkp_or_prove(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* secrets, const uint8_t* real, const uint8_t* inst,
                 const uint8_t* common, const uint8_t* entropy, uint8_t* chal, uint8_t* resp, uint8_t* status) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!ts || !real || !entropy || !chal || !status || (M.m && (!secrets || !resp)) || (M.ni && !inst) || (M.ns && !common)) return fail(ZKP_ERR_ARG, "NULL pointer");
  if (!strobe_positions_ok(ts, N)) return fail(ZKP_ERR_ARG, "a transcript's position byte is 166 or more");
  for (uint32_t j = 0; j < N; ++j)
    if (real[j] >= k) return fail(ZKP_ERR_ARG, "real[j] must be below k");
  HIP_TRY(hipSetDevice(c->device));
  staging sg(c);
  const size_t o_ts = sg.inout(ts, ts, 208 * (size_t)N);
  const size_t o_inst = sg.in(inst, 32 * (size_t)z.n_blocks * M.ni);
  const size_t o_common = sg.in(common, 32 * (size_t)M.ns);
  const size_t o_chal = sg.out(chal, 32 * (size_t)z.n_blocks);
  const size_t o_resp = sg.out(resp, 32 * (size_t)z.n_blocks * M.m);
  const size_t o_status = sg.out(status, (size_t)N);
  const size_t o_secrets = sg.in(secrets, 32 * (size_t)N * M.m);       // secrets | real | entropy: one stretch, wiped below
  const size_t o_real = sg.in(real, (size_t)N);
  const size_t o_entropy = sg.in(entropy, 32 * (size_t)N);
  const size_t secret_end = sg.carved();
  const or_ws w = or_carve(sg.carved(), M, z, N, true);
  rc = sg.reserve(or_total_ws(c, w, z, ZKP_CT));
  if (rc) return rc;
  // from the first secret byte on the device, every way out passes the wipe of the staged secrets (the core wipes the nonce region)
  rc = sg.begin();
  if (rc == ZKP_OK)
    rc = or_prove_core(c, M, z, w, k, N, sg.at<uint8_t>(o_ts), sg.at<uint8_t>(o_secrets), sg.at<uint8_t>(o_real), sg.at<uint8_t>(o_inst), sg.at<uint8_t>(o_common),
                       sg.at<uint8_t>(o_entropy), sg.at<uint8_t>(o_chal), sg.at<uint8_t>(o_resp), sg.at<uint8_t>(o_status));
  const hipError_t wiped = hipMemsetAsync(sg.at<uint8_t>(o_secrets), 0, secret_end - o_secrets, c->stream);
  if (rc || wiped != hipSuccess) {
    const hipError_t synced = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    HIP_TRY(wiped);
    HIP_TRY(synced);
  }
  return sg.end(ZKP_OK);
}

int zkp_or_verify(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common, const uint8_t* chal,
                  const uint8_t* resp, uint8_t* results) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!ts || !chal || !results || (M.m && !resp) || (M.ni && !inst) || (M.ns && !common)) return fail(ZKP_ERR_ARG, "NULL pointer");
  if (!strobe_positions_ok(ts, N)) return fail(ZKP_ERR_ARG, "a transcript's position byte is 166 or more");
  HIP_TRY(hipSetDevice(c->device));
  staging sg(c);
  const size_t o_ts = sg.inout(ts, ts, 208 * (size_t)N);
  const size_t o_inst = sg.in(inst, 32 * (size_t)z.n_blocks * M.ni);
  const size_t o_common = sg.in(common, 32 * (size_t)M.ns);
  const size_t o_chal = sg.in(chal, 32 * (size_t)z.n_blocks);
  const size_t o_resp = sg.in(resp, 32 * (size_t)z.n_blocks * M.m);
  const size_t o_res = sg.out(results, (size_t)N);
  const or_ws w = or_carve(sg.carved(), M, z, N, false);
  rc = sg.begin(or_total_ws(c, w, z, ZKP_VARTIME));
  if (rc) return rc;
  return sg.end(or_verify_core(c, M, z, w, k, N, sg.at<uint8_t>(o_ts), sg.at<uint8_t>(o_inst), sg.at<uint8_t>(o_common), sg.at<uint8_t>(o_chal),
                               sg.at<uint8_t>(o_resp), sg.at<uint8_t>(o_res)));
}

}  // extern "C"
