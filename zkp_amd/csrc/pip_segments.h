// pip_segments.h -- zkp_msm_optional_many (zkp_mi355x.h (14)): MANY variable-time multiscalar sums with long segments by the bucket method.  Included at the
// end of zkp_kernels.hip (one translation unit: shares zkp_ctx, the workspace carving, pip_run and the term path).
//
// The kernels for many bucket MSMs side by side are pip_run's: the batch index is one more window coordinate (pip_seg::K).  What this file adds is the plan
// that turns an arbitrary CSR job into such runs, and the size rules of that plan:
//   * a RUN is pip_run<pick_c(n)> over K segments padded to n slots each, n = the longest segment of the run.  Its prepare step is k_pip_prepare_csr, which
//     reads segment seg(b) of the job for MSM b and fills the slots beyond the segment's length with the identity and all-zero digits (bin 0: the
//     histogram skips it, so a padding slot costs the prepare, histogram and scatter passes their read and no point addition); its last step is k_pip_rows,
//     which takes the K rows and status words pip_run leaves in run order to out[seg(b)] and status[seg(b)];
//   * K is bounded by the grid (K * W1 <= 65535), by the 32-bit bucket index of pip_run and by kPipRunCapTerms padded terms per run, which also bounds
//     the workspace.  A segment longer than the cap is a run of its own;
//   * runs are used for n > kSmallOptional only (the sizes the bucket kernels have ever run at); shorter segments take msm_terms_path, variable time;
//   * the host-pointer form orders the long segments by length and cuts them into CLASSES: a class is the longest segment not yet placed together with
//     every segment MORE THAN HALF as long (2 * len > longest), so a run pads no member by a factor of two or more.  Inside a class the runs take the
//     members in falling length, and n of a run is its own first member -- the later runs of a class pad less than the first.
#pragma once

namespace {

// padded terms (K * n) of one run.  profiles/msm_optional_many_bench.txt, "run cap": the smallest cap from which one, two and four runs of a 2^21-term job
// are level (32 x 65,536: 2.75, 2.90, 3.48 ns per term at caps 2^21, 2^20, 2^19); every halving below costs more (12.39 ns at 2^16)
constexpr uint64_t kPipRunCapTerms = 1u << 20;

inline bool pip_same_class(uint32_t len, uint32_t longest) { return 2 * (uint64_t)len > longest; }

inline uint32_t pip_w1(int cbits) {
  switch (cbits) {
    case 7: return pip_cfg<7>::W1;
    case 10: return pip_cfg<10>::W1;
    case 11: return pip_cfg<11>::W1;
    default: return pip_cfg<16>::W1;
  }
}
inline uint32_t pip_b1(int cbits) {
  switch (cbits) {
    case 7: return pip_cfg<7>::B1;
    case 10: return pip_cfg<10>::B1;
    case 11: return pip_cfg<11>::B1;
    default: return pip_cfg<16>::B1;
  }
}

inline uint64_t pip_run_cap(const zkp_ctx* c) {
#ifdef ZKP_BUILD_TEST_HOOKS
  if (c->debug_pip_run_cap) return c->debug_pip_run_cap;
#endif
  (void)c;
  return kPipRunCapTerms;
}

// the most MSMs of n slots one run may hold
inline uint32_t pip_run_kmax(uint32_t n, uint64_t cap) {
  const int cbits = pick_c(n);
  const uint64_t w1 = pip_w1(cbits);
  const uint64_t by_grid = 65535u / w1;                                         // grid.y = K * W1
  const uint64_t by_index = 0xffffffffull / (4u * w1 * pip_b1(cbits));          // pip_run's own check (4 * K * W1 * B1 fits 32 bits), mirrored: it cannot bind -- c = 16 means n >= 2^21, where the library's cap leaves K = 1 (only ZKP_TESTOPT_PIP_RUN_CAP can raise it), and by_grid is smaller at c <= 11
  const uint64_t by_cap = cap / n;
  return (uint32_t)std::max<uint64_t>(1, std::min(by_grid, std::min(by_index, by_cap)));
}

struct pip_many_run {
  uint32_t at, K, n;       // MSMs [at, at + K) of the run order (the seg_ids list, or the job's own order), n slots each
};

// runs over `count` MSMs whose lengths in run order are len(i) (falling inside a class), classes cut by pip_same_class; len == nullptr: one class of n_all slots
inline std::vector<pip_many_run> pip_many_plan(uint32_t count, const uint32_t* len, uint32_t n_all, uint64_t cap) {
  std::vector<pip_many_run> runs;
  uint32_t at = 0;
  while (at < count) {
    const uint32_t n = len ? len[at] : n_all;
    const uint32_t kmax = pip_run_kmax(n, cap);
    uint32_t K = 1;
    while (at + K < count && K < kmax && (!len || pip_same_class(len[at + K], n))) ++K;
    runs.push_back({at, K, n});
    at += K;
  }
  return runs;
}

inline size_t pip_many_runs_ws(const std::vector<pip_many_run>& runs) {
  size_t need = 0;
  for (const pip_many_run& r : runs) need = std::max(need, pip_ws_for(pick_c(r.n), r.n, r.K));
  return need;
}

// The runs of a plan, one after the other on the context's stream.  stage: K_max rows and K_max status words in the workspace (at ws offset o_rows / o_st), the
// buckets' own workspace from ws_reserved on.  job.first / job.seg_ids name the MSMs of run order.
int pip_many_launch(zkp_ctx* c, const std::vector<pip_many_run>& runs, pip_csr job, const uint8_t* d_scalars, const uint8_t* d_points, size_t o_rows, size_t o_st,
                    size_t ws_reserved, uint8_t* d_out, uint8_t* d_status) {
  char* base = static_cast<char*>(c->ws);
  uint8_t* rows = reinterpret_cast<uint8_t*>(base + o_rows);
  uint32_t* st = reinterpret_cast<uint32_t*>(base + o_st);
  const uint32_t first0 = job.first;
  const uint32_t* ids0 = job.seg_ids;
  for (const pip_many_run& r : runs) {
    job.first = first0 + r.at;
    job.seg_ids = ids0 ? ids0 + r.at : nullptr;
    job.at = r.at;
    pip_seg seg;
    seg.K = r.K;
    int rc;
    switch (pick_c(r.n)) {
      case 7: rc = pip_run<7>(c, r.n, d_scalars, d_points, rows, st, ws_reserved, nullptr, seg, 3, &job); break;
      case 10: rc = pip_run<10>(c, r.n, d_scalars, d_points, rows, st, ws_reserved, nullptr, seg, 3, &job); break;
      case 11: rc = pip_run<11>(c, r.n, d_scalars, d_points, rows, st, ws_reserved, nullptr, seg, 3, &job); break;
      default: rc = pip_run<16>(c, r.n, d_scalars, d_points, rows, st, ws_reserved, nullptr, seg, 3, &job); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(k_pip_rows, grid1(r.K, 256), dim3(256), 0, c->stream, r.K, job, rows, st, d_out, d_status);
  }
  HIP_TRY(hipGetLastError());
  return ZKP_OK;
}

// the generic bounds of the term path for arrays the host has not inspected, variable time (zkp_msm_many_dev's)
inline terms_cfg pip_many_terms_cfg(const zkp_ctx* c) {
  terms_cfg k;
  k.teeth = c->comb_teeth;
  k.throughput = true;
  k.comb_min = 2u;
  return k;
}

}  // namespace

extern "C" {

uint32_t zkp_msm_optional_many_min_segment(void) { return (uint32_t)kSmallOptional; }

int zkp_msm_optional_many_dev(zkp_ctx* c, uint32_t n_seg, const uint32_t* d_off, const uint8_t* d_scalars, const uint32_t* d_pidx, const uint8_t* d_points,
                              uint32_t n_points, uint32_t n_terms, uint32_t max_seg, uint8_t* d_out, uint8_t* d_status) {
  if (!c) return fail(ZKP_ERR_ARG, "ctx is NULL");
  if (n_seg == 0) return ZKP_OK;
  if (!d_off || !d_out || !d_status) return fail(ZKP_ERR_ARG, "NULL device pointer");
  if (n_terms && (!d_scalars || !d_points || n_points == 0)) return fail(ZKP_ERR_ARG, "terms without scalars/points");
  if (!d_pidx && n_points != n_terms) return fail(ZKP_ERR_ARG, "without pidx, n_points must equal the number of terms");
  if (!aligned16(d_scalars) || !aligned16(d_points) || !aligned16(d_out)) return fail(ZKP_ERR_ARG, "device buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  if (n_terms == 0 || max_seg == 0) {               // every segment is empty: the identity, status 0
    prof_begin(c);
    HIP_TRY(hipMemsetAsync(d_out, 0, 32 * (size_t)n_seg, c->stream));
    HIP_TRY(hipMemsetAsync(d_status, 0, n_seg, c->stream));
    return ZKP_OK;
  }
  if (max_seg <= kSmallOptional) {                  // the term path on the job as it stands (zkp_msm_many_dev, variable time)
    const terms_cfg k = pip_many_terms_cfg(c);
    carve cv;
    const size_t o_iota = cv.take(d_pidx ? 0 : (size_t)n_terms * 4);
    const size_t reserved = cv.off;
    const int rc = ensure_ws(c, reserved + terms_path_ws(n_points, n_terms, n_seg, k));
    if (rc) return rc;
    prof_begin(c);
    if (!d_pidx) {
      uint32_t* iota = reinterpret_cast<uint32_t*>(static_cast<char*>(c->ws) + o_iota);
      hipLaunchKernelGGL(k_iota, grid1(n_terms, 256), dim3(256), 0, c->stream, n_terms, iota);
      d_pidx = iota;
    }
    return msm_terms_path(c, n_seg, d_off, d_scalars, d_pidx, d_points, n_points, n_terms, ZKP_VARTIME, d_out, d_status, nullptr, reserved, false, PH_ALL, k);
  }
  if (max_seg > 0x7fffffffu) return fail(ZKP_ERR_ARG, "max_seg too large (max 2^31-1 terms per segment)");
  const std::vector<pip_many_run> runs = pip_many_plan(n_seg, nullptr, max_seg, pip_run_cap(c));
  uint32_t kmax = 0;
  for (const pip_many_run& r : runs) kmax = std::max(kmax, r.K);
  carve cv;
  const size_t o_rows = cv.take(32 * (size_t)kmax);
  const size_t o_st = cv.take(4 * (size_t)kmax);
  const size_t reserved = cv.off;
  const int rc = ensure_ws(c, reserved + pip_many_runs_ws(runs));
  if (rc) return rc;
  prof_begin(c);
  pip_csr job;
  job.off = d_off;
  job.pidx = d_pidx;
  job.n_seg = n_seg;
  job.n_points = n_points;
  job.n_terms = n_terms;
  return pip_many_launch(c, runs, job, d_scalars, d_points, o_rows, o_st, reserved, d_out, d_status);
}

int zkp_msm_optional_many(zkp_ctx* c, uint32_t n_seg, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points, uint32_t n_points,
                          uint8_t* out, uint8_t* status) {
  if (!c) return fail(ZKP_ERR_ARG, "ctx is NULL");
  if (n_seg == 0) return ZKP_OK;
  if (!off || !out || !status) return fail(ZKP_ERR_ARG, "NULL pointer");
  uint32_t n_terms;
  int rc = csr_check(off, n_seg, &n_terms);
  if (rc) return rc;
  if (n_terms && (!scalars || !points || n_points == 0)) return fail(ZKP_ERR_ARG, "terms without scalars/points");
  if (!pidx && n_points != n_terms) return fail(ZKP_ERR_ARG, "without pidx, n_points must equal the number of terms");
  if (!idx_in_range(pidx, n_terms, n_points)) return fail(ZKP_ERR_ARG, "pidx out of range");
  HIP_TRY(hipSetDevice(c->device));
  // the plan: empty segments are the zeroed output; short ones one CSR job of their own for the term path; the long ones in falling length
  std::vector<uint32_t> short_ids, long_ids;
  for (uint32_t i = 0; i < n_seg; ++i) {
    const uint32_t len = off[i + 1] - off[i];
    if (len == 0) continue;
    (len <= kSmallOptional ? short_ids : long_ids).push_back(i);
  }
  std::stable_sort(long_ids.begin(), long_ids.end(), [&](uint32_t a, uint32_t b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
  std::vector<uint32_t> long_len(long_ids.size());
  for (size_t j = 0; j < long_ids.size(); ++j) long_len[j] = off[long_ids[j] + 1] - off[long_ids[j]];
  if (!long_len.empty() && long_len[0] > 0x7fffffffu) return fail(ZKP_ERR_ARG, "segment too long (max 2^31-1 terms)");
  const std::vector<pip_many_run> runs = pip_many_plan((uint32_t)long_ids.size(), long_len.data(), 0, pip_run_cap(c));
  // the short segments' job, gathered on the host: offsets, scalars, and the rows they reference as a point array of its own (a handful of short segments
  // beside millions of points decodes and classifies what it uses, not the whole array), with the exact table / ladder counts zkp_msm_many derives
  const uint32_t n_short = (uint32_t)short_ids.size();
  std::vector<uint32_t> s_off(n_short + 1, 0), s_pidx;
  std::vector<uint8_t> s_sc, s_pts;
  std::unordered_map<uint32_t, uint32_t> s_row;                    // row of the job's points -> row of the short job's
  for (uint32_t j = 0; j < n_short; ++j) s_off[j + 1] = s_off[j] + (off[short_ids[j] + 1] - off[short_ids[j]]);
  const uint32_t s_terms = s_off[n_short];
  s_pidx.resize(s_terms);
  s_sc.resize(32 * (size_t)s_terms);
  for (uint32_t j = 0; j < n_short; ++j) {
    const uint32_t lo = off[short_ids[j]], len = s_off[j + 1] - s_off[j];
    memcpy(s_sc.data() + 32 * (size_t)s_off[j], scalars + 32 * (size_t)lo, 32 * (size_t)len);
    for (uint32_t i = 0; i < len; ++i) {
      const uint32_t p = pidx ? pidx[lo + i] : lo + i;
      const auto at = s_row.emplace(p, (uint32_t)s_row.size());
      if (at.second) s_pts.insert(s_pts.end(), points + 32 * (size_t)p, points + 32 * (size_t)p + 32);
      s_pidx[s_off[j] + i] = at.first->second;
    }
  }
  const uint32_t s_npts = (uint32_t)s_row.size();
  const terms_cfg k = s_terms >= 1024 ? host_terms_cfg(c, s_terms, s_pidx.data(), s_pts.data(), s_npts, 2u) : terms_cfg();
  uint32_t kmax = n_short;
  for (const pip_many_run& r : runs) kmax = std::max(kmax, r.K);
  const bool any_long = !long_ids.empty();
  carve cv;
  const size_t o_off = cv.take(any_long ? (size_t)(n_seg + 1) * 4 : 0);
  const size_t o_sc = cv.take(any_long ? (size_t)n_terms * 32 : 0);
  const size_t o_pidx = cv.take(any_long && pidx ? (size_t)n_terms * 4 : 0);
  const size_t o_pts = cv.take(any_long ? (size_t)n_points * 32 : 0);
  const size_t o_spts = cv.take((size_t)s_npts * 32);
  const size_t o_ids = cv.take(long_ids.size() * 4);
  const size_t o_soff = cv.take((size_t)(n_short + 1) * 4);
  const size_t o_ssc = cv.take((size_t)s_terms * 32);
  const size_t o_spidx = cv.take((size_t)s_terms * 4);
  const size_t o_sids = cv.take((size_t)n_short * 4);
  const size_t o_out = cv.take((size_t)n_seg * 32);
  const size_t o_stat = cv.take((size_t)n_seg);
  const size_t o_rows = cv.take(32 * (size_t)kmax);
  const size_t o_st = cv.take(4 * (size_t)kmax);
  const size_t reserved = cv.off;
  rc = ensure_ws(c, reserved + std::max(pip_many_runs_ws(runs), n_short ? terms_path_ws(s_npts, s_terms, n_short, k) : 0));
  if (rc) return rc;
  char* base = static_cast<char*>(c->ws);
  auto up = [&](size_t o, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
  if (any_long) {
    HIP_TRY(up(o_off, off, (size_t)(n_seg + 1) * 4));
    HIP_TRY(up(o_sc, scalars, (size_t)n_terms * 32));
    if (pidx) HIP_TRY(up(o_pidx, pidx, (size_t)n_terms * 4));
    HIP_TRY(up(o_ids, long_ids.data(), long_ids.size() * 4));
    HIP_TRY(up(o_pts, points, (size_t)n_points * 32));
  }
  if (n_short) {
    HIP_TRY(up(o_soff, s_off.data(), (size_t)(n_short + 1) * 4));
    HIP_TRY(up(o_ssc, s_sc.data(), (size_t)s_terms * 32));
    HIP_TRY(up(o_spidx, s_pidx.data(), (size_t)s_terms * 4));
    HIP_TRY(up(o_spts, s_pts.data(), (size_t)s_npts * 32));
    HIP_TRY(up(o_sids, short_ids.data(), (size_t)n_short * 4));
  }
  uint8_t* d_out = reinterpret_cast<uint8_t*>(base + o_out);
  uint8_t* d_status = reinterpret_cast<uint8_t*>(base + o_stat);
  const uint8_t* d_points = reinterpret_cast<uint8_t*>(base + o_pts);
  HIP_TRY(hipMemsetAsync(d_out, 0, 32 * (size_t)n_seg, c->stream));        // the empty segments: the identity, status 0
  HIP_TRY(hipMemsetAsync(d_status, 0, n_seg, c->stream));
  prof_begin(c);
  if (n_short) {
    uint8_t* rows = reinterpret_cast<uint8_t*>(base + o_rows);
    uint32_t* st = reinterpret_cast<uint32_t*>(base + o_st);
    rc = msm_terms_path(c, n_short, reinterpret_cast<uint32_t*>(base + o_soff), reinterpret_cast<uint8_t*>(base + o_ssc), reinterpret_cast<uint32_t*>(base + o_spidx),
                        reinterpret_cast<uint8_t*>(base + o_spts), s_npts, s_terms, ZKP_VARTIME, rows, nullptr, st, reserved, false, PH_ALL, k);
    if (rc) return rc;
    pip_csr ids;
    ids.seg_ids = reinterpret_cast<uint32_t*>(base + o_sids);
    ids.n_seg = n_seg;
    hipLaunchKernelGGL(k_pip_rows, grid1(n_short, 256), dim3(256), 0, c->stream, n_short, ids, rows, st, d_out, d_status);
  }
  if (any_long) {
    pip_csr job;
    job.off = reinterpret_cast<uint32_t*>(base + o_off);
    job.pidx = pidx ? reinterpret_cast<uint32_t*>(base + o_pidx) : nullptr;
    job.seg_ids = reinterpret_cast<uint32_t*>(base + o_ids);
    job.n_seg = n_seg;
    job.n_points = n_points;
    job.n_terms = n_terms;
    rc = pip_many_launch(c, runs, job, reinterpret_cast<uint8_t*>(base + o_sc), d_points, o_rows, o_st, reserved, d_out, d_status);
    if (rc) return rc;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n_seg * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(status, d_status, (size_t)n_seg, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ZKP_OK;
}

}  // extern "C"
