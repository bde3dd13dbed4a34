// or_batch_flows.h -- the calls of zkp_or_batch_mi355x.h: the batchable form of the 1-of-k OR-proofs.  Included at the end of
// zkp_kernels.hip behind or_flows.h, whose carving, set-up and prover it shares.  The kernels are or_batch_lane.h's; this file is the
// order of the launches.
//
// zkp_or_prove_batchable     or_flows.h's prover, then one copy of its `coms` region (the host-pointer form: the download itself)
// zkp_or_verify_batchable    k_or_plan, k_or_bind, k_or_challenge over the GIVEN commitments, k_or_check, the term path (ZKP_VARTIME),
//                            k_or_given_check
// zkp_or_batch_verify        k_or_bind, k_or_challenge over the given commitments, k_or_given_check, k_or_batch_coeff, the fold of zkp_sc_reduce (ZKP_SC_SUM) over the ns
//                            segments of partials, msm_optional_impl, k_or_batch_verdict
// The batch verifier makes no size-dependent choice of its own: the fold and the MSM make theirs.
//
// Workspace of the batch verifier behind `reserved`: [statement blob | points | scalars | partials | seg | c | rejected | results |
// sum | words] [the fold's, then the MSM's].  points = [common | inst | given commitments], scalars = their coefficients.
#pragma once
#include "../../include/zkp_or_batch_mi355x.h"
#include "or_batch_lane.h"

namespace {

struct orb_ws { size_t meta, points, scalars, partial, seg, c, rej, res, sum, words, end; };
orb_ws orb_carve(size_t reserved, const or_meta& M, const or_sizes& z, uint32_t N, uint64_t n_ops) {
  carve cv;
  cv.off = reserved;
  orb_ws w;
  w.meta = cv.take(M.bytes());
  w.points = cv.take(32 * (size_t)n_ops + 32);       // (one spare row each, as zkp_msm_optional stages its operands)
  w.scalars = cv.take(32 * (size_t)n_ops + 32);
  w.partial = cv.take(32 * (size_t)M.ns * z.n_blocks);
  w.seg = cv.take(4 * ((size_t)M.ns + 1));
  w.c = cv.take(32 * (size_t)N);
  w.rej = cv.take((size_t)N);
  w.res = cv.take((size_t)N);
  w.sum = cv.take(32);
  w.words = cv.take(16);                             // [0] the MSM's status, [2] set by a rejected proof
  w.end = cv.off;
  return w;
}
// the operands of the batch check; ZKP_ERR_ARG where they, or the partials, are more than one multiscalar sum or one fold takes
int orb_sizes(const or_meta& M, const or_sizes& z, uint64_t* n_ops) {
  const uint64_t n = (uint64_t)M.ns + (uint64_t)z.n_blocks * ((uint64_t)M.ni + M.nc);
  if (n >= (1ull << 32)) return fail(ZKP_ERR_ARG, "N too large: ns + N * k * (ni + constraints) must stay below 2^32");
  if (n > 0x7fffffffull || (uint64_t)M.ns * z.n_blocks > 0x7fffffffull) return fail(ZKP_ERR_ARG, "N too large: one multiscalar sum takes at most 2^31 - 1 terms");
  *n_ops = n;
  return ZKP_OK;
}
size_t orb_total_ws(const orb_ws& w, const or_meta& M, const or_sizes& z, uint64_t n_ops) {
  return std::max(sc_reduce_ws(M.ns * z.n_blocks, w.end).total, w.end + optional_ws(n_ops));
}

int orb_verify_core(zkp_ctx* c, const or_meta& M, const or_sizes& z, const orb_ws& w, uint64_t n_ops, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_inst,
                    const uint8_t* d_common, const uint8_t* d_given, const uint8_t* d_chal, const uint8_t* d_resp, const uint8_t* d_weights, uint32_t* d_verdict) {
  uint8_t* base = static_cast<uint8_t*>(c->ws);
  uint8_t* points = base + w.points;
  uint8_t* scalars = base + w.scalars;
  uint8_t* given = points + 32 * (size_t)z.n_points;
  uint32_t* words = reinterpret_cast<uint32_t*>(base + w.words);
  c->or_meta_keep = M.blob;                    // the copy's source outlives the call
  HIP_TRY(hipMemcpyAsync(base + w.meta, c->or_meta_keep.data(), M.bytes(), hipMemcpyHostToDevice, c->stream));
  if (M.ns) HIP_TRY(hipMemcpyAsync(points, d_common, 32 * (size_t)M.ns, hipMemcpyDeviceToDevice, c->stream));
  if (M.ni) HIP_TRY(hipMemcpyAsync(points + 32 * (size_t)M.ns, d_inst, 32 * (size_t)z.n_blocks * M.ni, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(given, d_given, 32 * (size_t)z.n_msm, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(words, 0, 16, c->stream));
  const or_stmt s = M.view(base + w.meta, k, N);
  hipLaunchKernelGGL(k_or_bind, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, points, 1u, base + w.rej);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_bind");
  hipLaunchKernelGGL(k_or_challenge, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, given, base + w.rej, base + w.c);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_challenge");
  hipLaunchKernelGGL(k_or_given_check, grid1(N, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_chal, d_resp, given, base + w.c, base + w.rej,
                     (const uint8_t*)nullptr, (const uint8_t*)nullptr, base + w.res, words + 2);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_given_check");
  hipLaunchKernelGGL(k_or_batch_coeff, grid1(z.n_blocks, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_weights, d_chal, d_resp, scalars, base + w.partial,
                     reinterpret_cast<uint32_t*>(base + w.seg));
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_batch_coeff");
  HIP_TRY(hipGetLastError());
  int rc = ZKP_OK;
  if (M.ns) {
    const uint32_t n_part = M.ns * z.n_blocks;
    rc = launch_sc_reduce(c, SC_RED_SUM, M.ns, reinterpret_cast<const uint32_t*>(base + w.seg), base + w.partial, n_part, nullptr, nullptr, 0, nullptr, n_part,
                          sc_reduce_ws(n_part, w.end), scalars);
    if (rc) return rc;
  }
  rc = msm_optional_impl(c, n_ops, scalars, points, base + w.sum, words, w.end);
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_batch_verdict, dim3(1), dim3(64), 0, c->stream, base + w.sum, words, words + 2, d_verdict);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_batch_verdict");
  HIP_TRY(hipGetLastError());
  return ZKP_OK;
}

// the per-proof verifier on or_flows.h's workspace: the commitments are recomputed into `coms` and compared with the given ones
int orb_verify_each_core(zkp_ctx* c, const or_meta& M, const or_sizes& z, const or_ws& w, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_inst,
                         const uint8_t* d_common, const uint8_t* d_given, const uint8_t* d_chal, const uint8_t* d_resp, uint8_t* d_results) {
  uint8_t* base = static_cast<uint8_t*>(c->ws);
  or_stmt s;
  int rc = or_setup(c, M, z, w, k, N, d_inst, d_common, &s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_bind, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, base + w.table, 1u, base + w.rej);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_bind");
  hipLaunchKernelGGL(k_or_challenge, dim3(strobe_blocks(N)), dim3(STROBE_BLOCK), 0, c->stream, s, d_ts, d_given, base + w.rej, base + w.c);
  or_note(c, ZKP_K_TRANSCRIPT, "zkp::k_or_challenge");
  hipLaunchKernelGGL(k_or_check, grid1(z.n_blocks, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_chal, d_resp, base + w.rows, base + w.flags);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_check");
  HIP_TRY(hipGetLastError());
  rc = msm_terms_path(c, z.n_msm, reinterpret_cast<const uint32_t*>(base + w.off), base + w.rows, reinterpret_cast<const uint32_t*>(base + w.pidx), base + w.table,
                      z.n_points, z.n_terms, ZKP_VARTIME, base + w.coms, base + w.mstat, nullptr, w.end, false, PH_ALL, or_terms_cfg(c, z.n_terms, ZKP_VARTIME));
  if (rc) return rc;
  hipLaunchKernelGGL(k_or_given_check, grid1(N, OR_BLOCK), dim3(OR_BLOCK), 0, c->stream, s, d_chal, d_resp, d_given, base + w.c, base + w.rej, base + w.coms,
                     base + w.mstat, d_results, (uint32_t*)nullptr);
  or_note(c, ZKP_K_SCALARS, "zkp::k_or_given_check");
  HIP_TRY(hipGetLastError());
  return ZKP_OK;
}

// a download that a host-pointer form queues itself, behind its launches and before staging::end synchronises
int orb_download(zkp_ctx* c, void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return ZKP_OK;
}
// or_flows.h's prover and wipe, then the commitments it hashed (the _dev form: the caller's buffer is on the device)
int orb_prove_core(zkp_ctx* c, const or_meta& M, const or_sizes& z, const or_ws& w, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_secrets,
                   const uint8_t* d_real, const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_entropy, uint8_t* d_given, uint8_t* d_chal,
                   uint8_t* d_resp, uint8_t* d_status) {
  const int rc = or_prove_core(c, M, z, w, k, N, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_chal, d_resp, d_status);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(d_given, static_cast<uint8_t*>(c->ws) + w.coms, 32 * (size_t)z.n_msm, hipMemcpyDeviceToDevice, c->stream));
  return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_or_prove_batchable_dev(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_secrets, const uint8_t* d_real,
                               const uint8_t* d_inst, const uint8_t* d_common, const uint8_t* d_entropy, uint8_t* d_given, uint8_t* d_chal, uint8_t* d_resp,
                               uint8_t* d_status) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!d_ts || !d_real || !d_entropy || !d_given || !d_chal || !d_status || (M.m && (!d_secrets || !d_resp)) || (M.ni && !d_inst) || (M.ns && !d_common))
    return fail(ZKP_ERR_ARG, "NULL device pointer");
  if (!or_all_aligned16({d_ts, d_secrets, d_inst, d_common, d_given, d_chal, d_resp})) return fail(ZKP_ERR_ARG, "device buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  const or_ws w = or_carve(0, M, z, N, true);
  rc = ensure_ws(c, or_total_ws(c, w, z, ZKP_CT));
  if (rc) return rc;
  prof_begin(c);
  return orb_prove_core(c, M, z, w, k, N, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_given, d_chal, d_resp, d_status);
}

int zkp_or_verify_batchable_dev(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_inst, const uint8_t* d_common,
                                const uint8_t* d_given, const uint8_t* d_chal, const uint8_t* d_resp, uint8_t* d_results) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!d_ts || !d_given || !d_chal || !d_results || (M.m && !d_resp) || (M.ni && !d_inst) || (M.ns && !d_common)) return fail(ZKP_ERR_ARG, "NULL device pointer");
  if (!or_all_aligned16({d_ts, d_inst, d_common, d_given, d_chal, d_resp})) return fail(ZKP_ERR_ARG, "device buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  const or_ws w = or_carve(0, M, z, N, false);
  rc = ensure_ws(c, or_total_ws(c, w, z, ZKP_VARTIME));
  if (rc) return rc;
  prof_begin(c);
  return orb_verify_each_core(c, M, z, w, k, N, d_ts, d_inst, d_common, d_given, d_chal, d_resp, d_results);
}

int zkp_or_batch_verify_dev(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* d_ts, const uint8_t* d_inst, const uint8_t* d_common,
                            const uint8_t* d_given, const uint8_t* d_chal, const uint8_t* d_resp, const uint8_t* d_weights, uint32_t* d_verdict) {
  or_meta M;
  or_sizes z;
  uint64_t n_ops = 0;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc == ZKP_OK) rc = orb_sizes(M, z, &n_ops);
  if (rc) return rc;
  if (!d_verdict) return fail(ZKP_ERR_ARG, "NULL device pointer");
  HIP_TRY(hipSetDevice(c->device));
  if (N == 0) {
    HIP_TRY(hipMemsetAsync(d_verdict, 0, 4, c->stream));
    return ZKP_OK;
  }
  if (!d_ts || !d_given || !d_chal || !d_weights || (M.m && !d_resp) || (M.ni && !d_inst) || (M.ns && !d_common)) return fail(ZKP_ERR_ARG, "NULL device pointer");
  if (!or_all_aligned16({d_ts, d_inst, d_common, d_given, d_chal, d_resp, d_weights})) return fail(ZKP_ERR_ARG, "device buffers must be 16-byte aligned");
  const orb_ws w = orb_carve(0, M, z, N, n_ops);
  rc = ensure_ws(c, orb_total_ws(w, M, z, n_ops));
  if (rc) return rc;
  prof_begin(c);
  return orb_verify_core(c, M, z, w, n_ops, k, N, d_ts, d_inst, d_common, d_given, d_chal, d_resp, d_weights, d_verdict);
}

int zkp_or_prove_batchable(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* secrets, const uint8_t* real,
                           const uint8_t* inst, const uint8_t* common, const uint8_t* entropy, uint8_t* given, uint8_t* chal, uint8_t* resp, uint8_t* status) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!ts || !real || !entropy || !given || !chal || !status || (M.m && (!secrets || !resp)) || (M.ni && !inst) || (M.ns && !common))
    return fail(ZKP_ERR_ARG, "NULL pointer");
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
  // as zkp_or_prove: from the first secret byte on the device, every way out passes the wipe of the staged secrets
  rc = sg.begin();
  if (rc == ZKP_OK)
    rc = or_prove_core(c, M, z, w, k, N, sg.at<uint8_t>(o_ts), sg.at<uint8_t>(o_secrets), sg.at<uint8_t>(o_real), sg.at<uint8_t>(o_inst), sg.at<uint8_t>(o_common),
                       sg.at<uint8_t>(o_entropy), sg.at<uint8_t>(o_chal), sg.at<uint8_t>(o_resp), sg.at<uint8_t>(o_status));
  if (rc == ZKP_OK) rc = orb_download(c, given, sg.at<uint8_t>(w.coms), 32 * (size_t)z.n_msm);       // straight from the `coms` region: no copy on the device
  const hipError_t wiped = hipMemsetAsync(sg.at<uint8_t>(o_secrets), 0, secret_end - o_secrets, c->stream);
  if (rc || wiped != hipSuccess) {
    const hipError_t synced = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    HIP_TRY(wiped);
    HIP_TRY(synced);
  }
  return sg.end(ZKP_OK);
}

int zkp_or_verify_batchable(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                            const uint8_t* given, const uint8_t* chal, const uint8_t* resp, uint8_t* results) {
  or_meta M;
  or_sizes z;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc || N == 0) return rc;
  if (!ts || !given || !chal || !results || (M.m && !resp) || (M.ni && !inst) || (M.ns && !common)) return fail(ZKP_ERR_ARG, "NULL pointer");
  if (!strobe_positions_ok(ts, N)) return fail(ZKP_ERR_ARG, "a transcript's position byte is 166 or more");
  HIP_TRY(hipSetDevice(c->device));
  staging sg(c);
  const size_t o_ts = sg.inout(ts, ts, 208 * (size_t)N);
  const size_t o_inst = sg.in(inst, 32 * (size_t)z.n_blocks * M.ni);
  const size_t o_common = sg.in(common, 32 * (size_t)M.ns);
  const size_t o_given = sg.in(given, 32 * (size_t)z.n_msm);
  const size_t o_chal = sg.in(chal, 32 * (size_t)z.n_blocks);
  const size_t o_resp = sg.in(resp, 32 * (size_t)z.n_blocks * M.m);
  const size_t o_res = sg.out(results, (size_t)N);
  const or_ws w = or_carve(sg.carved(), M, z, N, false);
  rc = sg.begin(or_total_ws(c, w, z, ZKP_VARTIME));
  if (rc) return rc;
  return sg.end(orb_verify_each_core(c, M, z, w, k, N, sg.at<uint8_t>(o_ts), sg.at<uint8_t>(o_inst), sg.at<uint8_t>(o_common), sg.at<uint8_t>(o_given),
                                     sg.at<uint8_t>(o_chal), sg.at<uint8_t>(o_resp), sg.at<uint8_t>(o_res)));
}

int zkp_or_batch_verify(zkp_ctx* c, const zkp_fused_statement* st, uint32_t k, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                        const uint8_t* given, const uint8_t* chal, const uint8_t* resp, const uint8_t* weights16, int* verdict, uint8_t* debug_scalars) {
  or_meta M;
  or_sizes z;
  uint64_t n_ops = 0;
  int rc = or_call_check(c, st, k, N, M, z);
  if (rc == ZKP_OK) rc = orb_sizes(M, z, &n_ops);
  if (rc) return rc;
  if (!verdict) return fail(ZKP_ERR_ARG, "NULL pointer");
  if (N == 0) {
    *verdict = 0;
    return ZKP_OK;
  }
  if (!ts || !given || !chal || !weights16 || (M.m && !resp) || (M.ni && !inst) || (M.ns && !common)) return fail(ZKP_ERR_ARG, "NULL pointer");
  if (!strobe_positions_ok(ts, N)) return fail(ZKP_ERR_ARG, "a transcript's position byte is 166 or more");
  HIP_TRY(hipSetDevice(c->device));
  uint32_t word = 1;
  staging sg(c);
  const size_t o_ts = sg.inout(ts, ts, 208 * (size_t)N);
  const size_t o_inst = sg.in(inst, 32 * (size_t)z.n_blocks * M.ni);
  const size_t o_common = sg.in(common, 32 * (size_t)M.ns);
  const size_t o_given = sg.in(given, 32 * (size_t)z.n_msm);
  const size_t o_chal = sg.in(chal, 32 * (size_t)z.n_blocks);
  const size_t o_resp = sg.in(resp, 32 * (size_t)z.n_blocks * M.m);
  const size_t o_weights = sg.in(weights16, 16 * (size_t)z.n_msm);
  const size_t o_word = sg.out(&word, 4);
  const orb_ws w = orb_carve(sg.carved(), M, z, N, n_ops);
  rc = sg.begin(orb_total_ws(w, M, z, n_ops));
  if (rc) return rc;
  rc = orb_verify_core(c, M, z, w, n_ops, k, N, sg.at<uint8_t>(o_ts), sg.at<uint8_t>(o_inst), sg.at<uint8_t>(o_common), sg.at<uint8_t>(o_given), sg.at<uint8_t>(o_chal),
                       sg.at<uint8_t>(o_resp), sg.at<uint8_t>(o_weights), sg.at<uint32_t>(o_word));
  if (rc == ZKP_OK && debug_scalars) rc = orb_download(c, debug_scalars, sg.at<uint8_t>(w.scalars), 32 * (size_t)n_ops);
  rc = sg.end(rc);
  if (rc) return rc;
  *verdict = (int)word;
  return ZKP_OK;
}

}  // extern "C"
