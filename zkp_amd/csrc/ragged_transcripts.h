// Ragged batches: the fused flows over transcripts that stand at different STROBE positions (bytes 200..202 of the blob), e.g. signatures
// over messages of different lengths.  Included by zkp_kernels.hip after fused_flows.h, before host_jobs.h.
//
// A batch splits into position classes (equal bytes 200..202: public data, labels and message lengths).  Everything of a plan but its
// transcript programs is position-free: a base plan per (flow, statement, N) holds it (plan_operands, no programs, never in fused_plans).  The
// programs are compiled per class with the same TrCompiler (compile_programs) and kept uploaded in the context; both caches drop the least
// recently used entry first.  A call then uploads a block table (one
// wavefront = one class program and up to 32 of its proofs) and the proof index list sorted stably by class, and the flows run them with
// k_transcript_run_ragged (run_program).  The class decides which program a wave runs; no secret decides anything.
#pragma once

namespace {

constexpr size_t kRaggedProgCap = 4096;        // class programs a context keeps: up to ~330 positions (pos x pos_begin) per (flow, statement, N)
constexpr size_t kRaggedBaseCap = 64;          // base plans a context keeps
constexpr uint32_t kNoPosition = 0xffffffffu;  // the position word of a base plan's key (no blob has it: byte 0 < 166)

// ---- classes and the block table (pure: zkp_debug_ragged_blocks exposes it to the tests) ------------------------------------------------
struct rg_block_ref { uint32_t cls, first, count; };
struct rg_groups {
  std::vector<uint32_t> pos;        // [classes]: the class's position word, in order of first appearance
  std::vector<uint32_t> idx;        // [N]: proof indices sorted stably by class
  std::vector<rg_block_ref> blocks; // per wavefront: class, idx[first .. first + count), count <= TR_BLOCK / 2
};
inline uint32_t blob_pos(const uint8_t* ts, uint32_t j) {
  const uint8_t* p = ts + 208 * (size_t)j + 200;
  return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}
inline void rg_group(const uint8_t* ts, uint32_t N, rg_groups& g) {
  // position word -> class: open addressing over a power-of-two table kept at most half full (a few hundred classes in practice)
  std::vector<uint32_t> slot(256, ~0u);
  auto home = [&](uint32_t p) { return (uint32_t)((p * 2654435761u) >> 8) & (uint32_t)(slot.size() - 1); };
  auto insert = [&](uint32_t p, uint32_t k) { uint32_t h = home(p); while (slot[h] != ~0u) h = (h + 1) & (uint32_t)(slot.size() - 1); slot[h] = k; };
  std::vector<uint32_t> cls(N), count;
  uint32_t last_p = ~0u, last_k = 0;
  for (uint32_t j = 0; j < N; ++j) {
    const uint32_t p = blob_pos(ts, j);
    if (p != last_p) {
      uint32_t h = home(p);
      while (slot[h] != ~0u && g.pos[slot[h]] != p) h = (h + 1) & (uint32_t)(slot.size() - 1);
      if (slot[h] == ~0u) {
        slot[h] = (uint32_t)g.pos.size();
        g.pos.push_back(p);
        count.push_back(0);
        if (2 * g.pos.size() > slot.size()) {
          slot.assign(2 * slot.size(), ~0u);
          for (uint32_t k = 0; k < (uint32_t)g.pos.size(); ++k) insert(g.pos[k], k);
          h = home(p);
          while (g.pos[slot[h]] != p) h = (h + 1) & (uint32_t)(slot.size() - 1);
        }
      }
      last_p = p;
      last_k = slot[h];
    }
    cls[j] = last_k;
    ++count[last_k];
  }
  std::vector<uint32_t> start(g.pos.size() + 1, 0);
  for (size_t k = 0; k < g.pos.size(); ++k) start[k + 1] = start[k] + count[k];
  g.idx.assign(N, 0);
  std::vector<uint32_t> fill(start.begin(), start.end() - 1);
  for (uint32_t j = 0; j < N; ++j) g.idx[fill[cls[j]]++] = j;
  constexpr uint32_t per = TR_BLOCK / 2;
  for (uint32_t k = 0; k < (uint32_t)g.pos.size(); ++k)
    for (uint32_t f = start[k]; f < start[k + 1]; f += per) g.blocks.push_back(rg_block_ref{k, f, std::min(per, start[k + 1] - f)});
}

// ---- the class program cache ---------------------------------------------------------------------------------------------------------
struct rg_prog {
  char* d_block = nullptr;          // ops A | tables A | ops B | tables B
  const tr_op* ops[2] = {nullptr, nullptr};
  const uint64_t* tables[2] = {nullptr, nullptr};
  uint32_t n[2] = {0, 0}, tail[2] = {0, 0};
  uint64_t used = 0;
};
int rg_upload_prog(zkp_ctx* c, const std::vector<tr_op>* ops, const std::vector<uint64_t>* tbl, const uint8_t (*tails)[3], int n_progs, rg_prog& out) {
  carve cv;
  size_t o_ops[2] = {0, 0}, o_tbl[2] = {0, 0};
  for (int i = 0; i < n_progs; ++i) { o_ops[i] = cv.take(ops[i].size() * sizeof(tr_op) + 64); o_tbl[i] = cv.take(tbl[i].size() * 8 + 64); }
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&out.d_block), cv.off));
  hipError_t e = hipSuccess;
  for (int i = 0; i < n_progs && e == hipSuccess; ++i) {
    if (!ops[i].empty()) e = hipMemcpy(out.d_block + o_ops[i], ops[i].data(), ops[i].size() * sizeof(tr_op), hipMemcpyHostToDevice);
    if (e == hipSuccess && !tbl[i].empty()) e = hipMemcpy(out.d_block + o_tbl[i], tbl[i].data(), tbl[i].size() * 8, hipMemcpyHostToDevice);
    out.ops[i] = reinterpret_cast<const tr_op*>(out.d_block + o_ops[i]);
    out.tables[i] = reinterpret_cast<const uint64_t*>(out.d_block + o_tbl[i]);
    out.n[i] = (uint32_t)ops[i].size();
    out.tail[i] = tails[i][0] | (uint32_t)tails[i][1] << 8 | (uint32_t)tails[i][2] << 16;
  }
  if (e != hipSuccess) { hipFree(out.d_block); out.d_block = nullptr; return fail(ZKP_ERR_HIP, std::string("class program upload: ") + hipGetErrorString(e)); }
  return ZKP_OK;
}
// the class program of `key`, compiled and uploaded by make() on a miss (*compiled counts those); stamped with the call's tick
template <typename F>
int rg_lookup(zkp_ctx* c, const std::string& key, uint64_t tick, F&& make, rg_prog** out, uint32_t* compiled) {
  auto it = c->ragged_progs.find(key);
  if (it == c->ragged_progs.end()) {
    std::unique_ptr<rg_prog> p(new rg_prog());
    const int rc = make(*p);
    if (rc) return rc;
    ++*compiled;
    it = c->ragged_progs.emplace(key, p.release()).first;
  }
  rg_prog* p = static_cast<rg_prog*>(it->second);
  p->used = tick;
  *out = p;
  return ZKP_OK;
}
// bound the cache: least recently used first, never a program of the running call (stamped `tick`); the calls are synchronous, so no
// earlier launch still reads what is freed here
void rg_evict(zkp_ctx* c, uint64_t tick) {
  while (c->ragged_progs.size() > kRaggedProgCap) {
    auto victim = c->ragged_progs.end();
    for (auto it = c->ragged_progs.begin(); it != c->ragged_progs.end(); ++it) {
      const rg_prog* p = static_cast<const rg_prog*>(it->second);
      if (p->used != tick && (victim == c->ragged_progs.end() || p->used < static_cast<const rg_prog*>(victim->second)->used)) victim = it;
    }
    if (victim == c->ragged_progs.end()) return;
    rg_prog* p = static_cast<rg_prog*>(victim->second);
    if (p->d_block) hipFree(p->d_block);
    delete p;
    c->ragged_progs.erase(victim);
  }
}

// ---- the base plans: everything of a plan but its transcript programs, per (flow, statement, N) ---------------------------------------
struct rg_base { fused_plan pl; uint64_t used = 0; };
void free_rg_base(rg_base* b) {
  if (b->pl.d_block) hipFree(b->pl.d_block);
  delete b;
}
// *built = 1 when this call compiled and uploaded it
int rg_base_plan(zkp_ctx* c, char flow, const zkp_fused_statement* st, const fused_shape& s, uint32_t N, uint64_t tick, fused_plan** out, int* built) {
  const std::string key = plan_key(flow, st, s, N, kNoPosition);
  auto it = c->ragged_bases.find(key);
  *built = 0;
  if (it == c->ragged_bases.end()) {
    std::unique_ptr<rg_base> b(new rg_base());
    fused_plan& pl = b->pl;
    pl.s = s;
    pl.N = N;
    std::vector<uint32_t> tarr;
    size_t order_at = 0, pair_at = 0;
    plan_operands(flow, st, s, pl, tarr, order_at, pair_at);
    const std::vector<uint32_t> inc = incidence_words(s);
    carve cv;
    const size_t o_t = cv.take(tarr.size() * 4 + 64);
    const size_t o_i = cv.take(inc.size() * 4 + 64);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&pl.d_block), cv.off));
    hipError_t e = tarr.empty() ? hipSuccess : hipMemcpy(pl.d_block + o_t, tarr.data(), tarr.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !inc.empty()) e = hipMemcpy(pl.d_block + o_i, inc.data(), inc.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { free_rg_base(b.release()); return fail(ZKP_ERR_HIP, std::string("base plan upload: ") + hipGetErrorString(e)); }
    pl.d_tarr = reinterpret_cast<const uint32_t*>(pl.d_block + o_t);
    pl.d_order = order_at ? pl.d_tarr + order_at : nullptr;
    pl.d_pair = pair_at ? pl.d_tarr + pair_at : nullptr;
    pl.d_inc = reinterpret_cast<const uint32_t*>(pl.d_block + o_i);
    it = c->ragged_bases.emplace(key, b.release()).first;
    *built = 1;
  }
  rg_base* b = static_cast<rg_base*>(it->second);
  b->used = tick;
  *out = &b->pl;
  while (c->ragged_bases.size() > kRaggedBaseCap) {       // (synchronous calls: no launch still reads what is freed here)
    auto victim = c->ragged_bases.end();
    for (auto v = c->ragged_bases.begin(); v != c->ragged_bases.end(); ++v) {
      const uint64_t u = static_cast<const rg_base*>(v->second)->used;
      if (u != tick && (victim == c->ragged_bases.end() || u < static_cast<const rg_base*>(victim->second)->used)) victim = v;
    }
    if (victim == c->ragged_bases.end()) break;
    free_rg_base(static_cast<rg_base*>(victim->second));
    c->ragged_bases.erase(victim);
  }
  return ZKP_OK;
}

// ---- a ragged call: the base plan with its programs A / B replaced by block tables ----------------------------------------------------
struct rg_call {
  fused_plan view;                  // a copy of the base plan (it owns nothing: the plan cache keeps the device block)
  std::vector<tr_rg_block> blk[2];  // host block tables of programs A and B (device pointers of the class programs)
  std::vector<uint32_t> idx;
  uint32_t n_classes = 0, compiled = 0;
  int base_built = 0;
  size_t bytes() const { return idx.size() * 4 + 64 + (blk[0].size() + blk[1].size()) * sizeof(tr_rg_block) + 64; }
};
// N >= 1 transcripts in at least one class; flow = FLOW_PROVE / FLOW_VERIFY / FLOW_BATCH
int rg_prepare(zkp_ctx* c, char flow, const zkp_fused_statement* st, uint32_t N, const uint8_t* ts, rg_call& r) {
  rg_groups g;
  rg_group(ts, N, g);
  for (uint32_t p : g.pos)
    if ((p & 0xff) >= 166) return fail(ZKP_ERR_ARG, "corrupt transcript blob (STROBE position out of range)");
  fused_shape s;
  int rc = check_fused_statement(st, s);
  if (rc) return rc;
  const uint64_t tick = ++c->ragged_tick;
  fused_plan* base = nullptr;
  rc = rg_base_plan(c, flow, st, s, N, tick, &base, &r.base_built);
  if (rc) return rc;
  const int n_progs = flow == FLOW_BATCH ? 1 : 2;
  std::string key = plan_key(flow, st, s, N, 0);          // (the position word sits at bytes 5..9: patched per class)
  std::vector<rg_prog*> progs(g.pos.size());
  for (size_t k = 0; k < g.pos.size(); ++k) {
    const uint32_t pos = g.pos[k];
    memcpy(&key[5], &pos, 4);
    rc = rg_lookup(c, key, tick, [&](rg_prog& out) {
      std::vector<tr_op> ops[2];
      std::vector<uint64_t> tbl[2];
      uint8_t tails[2][3] = {{0, 0, 0}, {0, 0, 0}};
      compile_programs(flow, st, s, N, pos, ops[0], tbl[0], tails[0], ops[1], tbl[1], tails[1]);
      return rg_upload_prog(c, ops, tbl, tails, n_progs, out);
    }, &progs[k], &r.compiled);
    if (rc) return rc;
  }
  rg_evict(c, tick);
  r.view = *base;
  r.view.img_bytes = 0;                                  // (no step form: no images)
  r.idx = g.idx;
  r.n_classes = (uint32_t)g.pos.size();
  for (int i = 0; i < n_progs; ++i) {
    uint32_t n_max = 0;
    for (const rg_block_ref& b : g.blocks) {
      const rg_prog* p = progs[b.cls];
      r.blk[i].push_back(tr_rg_block{p->ops[i], p->tables[i], p->n[i], p->tail[i], b.first, b.count});
      n_max = std::max(n_max, p->n[i]);
    }
    prog_dev& d = i ? r.view.b : r.view.a;
    d = prog_dev{};
    d.n = n_max;
    d.rg_blocks = (uint32_t)g.blocks.size();
  }
  if (n_progs == 1) r.view.b = prog_dev{};
  return ZKP_OK;
}
// the call's index list and block tables into the workspace at d (bytes() bytes, queued on the context's stream)
int rg_upload(zkp_ctx* c, rg_call& r, uint8_t* d) {
  carve cv;
  const size_t o_idx = cv.take(r.idx.size() * 4 + 64);
  const size_t o_a = cv.take(r.blk[0].size() * sizeof(tr_rg_block));
  const size_t o_b = cv.take(r.blk[1].size() * sizeof(tr_rg_block));
  (void)o_b;
  if (cv.off > r.bytes() + 3 * 256) return fail(ZKP_ERR_ARG, "internal: ragged tables do not fit");
  HIP_TRY(hipMemcpyAsync(d + o_idx, r.idx.data(), r.idx.size() * 4, hipMemcpyHostToDevice, c->stream));
  for (int i = 0; i < 2; ++i) {
    if (r.blk[i].empty()) continue;
    const size_t o = i ? o_b : o_a;
    HIP_TRY(hipMemcpyAsync(d + o, r.blk[i].data(), r.blk[i].size() * sizeof(tr_rg_block), hipMemcpyHostToDevice, c->stream));
    prog_dev& p = i ? r.view.b : r.view.a;
    p.rg = reinterpret_cast<const tr_rg_block*>(d + o);
    p.rg_idx = reinterpret_cast<const uint32_t*>(d + o_idx);
  }
  return ZKP_OK;
}
size_t rg_bytes(const rg_call* r) { return r ? r->bytes() + 3 * 256 : 0; }
// a batch whose blobs all stand at one position runs the aligned flow
bool rg_aligned(const uint8_t* ts, uint32_t N) {
  for (uint32_t j = 1; j < N; ++j)
    if (memcmp(ts + 208 * (size_t)j + 200, ts + 200, 3) != 0) return false;
  return true;
}

}  // namespace

void free_ragged_progs(zkp_ctx* c) {
  for (auto& kv : c->ragged_progs) {
    rg_prog* p = static_cast<rg_prog*>(kv.second);
    if (p->d_block) hipFree(p->d_block);
    delete p;
  }
  c->ragged_progs.clear();
  for (auto& kv : c->ragged_bases) free_rg_base(static_cast<rg_base*>(kv.second));
  c->ragged_bases.clear();
}

extern "C" {

// ---- hash to the group over ragged transcripts: the one-step squeeze per class --------------------------------------------------------
int zkp_fused_hash_to_group_ragged(zkp_ctx* c, uint32_t N, uint8_t* transcripts, const char* label, uint8_t* out) {
  if (!c) return fail(ZKP_ERR_ARG, "ctx is NULL");
  if (c->capturing) return fail(ZKP_ERR_ARG, "graph capture: the _ragged entry points cannot be recorded");
  if (N == 0) return ZKP_OK;
  if (!transcripts || !label || !out) return fail(ZKP_ERR_ARG, "NULL pointer");
  if (N > 0x7fffffffu) return fail(ZKP_ERR_ARG, "N too large");
  if (rg_aligned(transcripts, N)) return zkp_fused_hash_to_group(c, N, transcripts, label, out);
  rg_groups g;
  rg_group(transcripts, N, g);
  for (uint32_t p : g.pos)
    if ((p & 0xff) >= 166) return fail(ZKP_ERR_ARG, "corrupt transcript blob (STROBE position out of range)");
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t tick = ++c->ragged_tick;
  uint32_t compiled = 0;
  std::vector<tr_rg_block> blk;
  std::vector<rg_prog*> progs(g.pos.size());
  for (size_t k = 0; k < g.pos.size(); ++k) {
    const uint32_t pos = g.pos[k];
    std::string key = "H";
    key.append(reinterpret_cast<const char*>(&pos), 4);
    key += label;
    const int rc = rg_lookup(c, key, tick, [&](rg_prog& o) {
      TrCompiler tc((uint8_t)pos, (uint8_t)(pos >> 8), (uint8_t)(pos >> 16));
      tc.challenge_bytes(label, tr_ref{0, 64, 0}, 64);
      std::vector<tr_op> ops[1];
      std::vector<uint64_t> tbl[1];
      uint8_t tails[1][3];
      ops[0] = tc.finish(tails[0]);
      tbl[0] = tc.tables();
      return rg_upload_prog(c, ops, tbl, tails, 1, o);
    }, &progs[k], &compiled);
    if (rc) return rc;
  }
  rg_evict(c, tick);
  for (const rg_block_ref& b : g.blocks) blk.push_back(tr_rg_block{progs[b.cls]->ops[0], progs[b.cls]->tables[0], progs[b.cls]->n[0], progs[b.cls]->tail[0], b.first, b.count});
  carve cv;
  const size_t o_ts = cv.take((size_t)N * 208);
  const size_t o_wide = cv.take((size_t)N * 64);
  const size_t o_out = cv.take((size_t)N * 32);
  const size_t o_idx = cv.take((size_t)N * 4);
  const size_t o_blk = cv.take(blk.size() * sizeof(tr_rg_block));
  int rc = ensure_ws(c, cv.off);
  if (rc) return rc;
  char* base = static_cast<char*>(c->ws);
  HIP_TRY(hipMemcpyAsync(base + o_ts, transcripts, (size_t)N * 208, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(base + o_idx, g.idx.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(base + o_blk, blk.data(), blk.size() * sizeof(tr_rg_block), hipMemcpyHostToDevice, c->stream));
  prof_begin(c);
  ZKP_SCHED(c, RAGGED_CLASSES, g.pos.size());
  ZKP_SCHED(c, RAGGED_COMPILED, compiled);
  ZKP_SCHED(c, RAGGED_BASE, 0);
  ZKP_SCHED(c, FUSED_PLANS, c->fused_plans.size());
  prog_dev p;
  p.n = 1;
  p.rg = reinterpret_cast<const tr_rg_block*>(base + o_blk);
  p.rg_idx = reinterpret_cast<const uint32_t*>(base + o_idx);
  p.rg_blocks = (uint32_t)blk.size();
  tr_bufs bufs{};
  bufs.dst[0] = reinterpret_cast<uint8_t*>(base + o_wide);
  uint8_t* d_ts = reinterpret_cast<uint8_t*>(base + o_ts);
  run_program(c, p, N, bufs, d_ts, nullptr, nullptr, /*throughput=*/false, /*d_img=*/nullptr);
  prof_mark(c, ZKP_K_TRANSCRIPT);
  HIP_TRY(hipGetLastError());
  rc = launch_from_uniform(c, N, reinterpret_cast<uint8_t*>(base + o_wide), reinterpret_cast<uint8_t*>(base + o_out));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(transcripts, d_ts, (size_t)N * 208, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(out, base + o_out, (size_t)N * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ZKP_OK;
}

#ifdef ZKP_BUILD_TEST_HOOKS
// The class grouping of a batch (what the _ragged entry points launch): idx[N] = proof indices sorted stably by class, blocks[3 * n] =
// (class, first, count) per wavefront, classes in order of first appearance.  Returns the number of blocks (at most cap are written).
int zkp_debug_ragged_blocks(const uint8_t* transcripts, uint32_t N, uint32_t* idx, uint32_t* blocks, uint32_t cap) {
  if (!transcripts || !idx || (cap && !blocks)) return fail(ZKP_ERR_ARG, "NULL pointer");
  rg_groups g;
  rg_group(transcripts, N, g);
  memcpy(idx, g.idx.data(), (size_t)N * 4);
  for (size_t b = 0; b < g.blocks.size() && b < cap; ++b) {
    blocks[3 * b] = g.blocks[b].cls;
    blocks[3 * b + 1] = g.blocks[b].first;
    blocks[3 * b + 2] = g.blocks[b].count;
  }
  return (int)g.blocks.size();
}
#endif  // ZKP_BUILD_TEST_HOOKS

}  // extern "C"
