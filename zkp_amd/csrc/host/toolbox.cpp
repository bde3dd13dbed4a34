// Host side of the zkp toolbox on top of the MI355X engine: the Prover / Verifier / BatchVerifier flows
// of the reference (src/toolbox/{prover,verifier,batch_verifier}.rs), restructured as
//      phase A (host, all proofs, threaded)  ->  ONE GPU call  ->  phase B (host, all proofs, threaded)
// because the reference's one-MSM-per-constraint call pattern (prover.rs:93-97, verifier.rs:96-106) would
// be pure launch overhead on a GPU.  Transcript traffic is byte-identical to the reference's, so proofs
// are interchangeable with proofs made by the Rust crate.  All group arithmetic goes through
// include/zkp_mi355x.h; there is no CPU fallback here.
#include <sys/random.h>

#include <cerrno>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "merlin.hpp"
#include "scalar.hpp"

using zkp::host::Scalar;
using zkp::host::Transcript;

#include "host_backend.hpp"
#include "toolbox_internal.hpp"

using namespace zkp::host;

static std::atomic<uint32_t> g_fused_min_batch{32};
// calls whose group arithmetic is at most this many (scalar, point) terms run on the host cores (host_backend.cpp) instead of paying the
// ~1 ms launch chain of the GPU; a NULL context always does (no GPU needed at all)
static std::atomic<uint32_t> g_host_max_terms{16};
// zkp_basepoint_dlog_batch: the host table's size, and the host work per thread (n (2^(bits - baby_bits) + 128) giant steps over min(threads, 16)) up
// to which a call with a context stays on the host threads.  Measured (profiles/dlog_bench.txt): no device call goes under 0.81 ms; 2,016 steps
// take 0.51 ms on one core, 32,688 steps 0.87 ms on sixteen -- the break-even.
static std::atomic<uint32_t> g_dlog_host_baby_bits{12};
static std::atomic<uint32_t> g_dlog_host_max_steps{2048};

namespace {
inline bool on_host(const zkp_ctx* ctx, uint64_t terms) { return !ctx || terms <= g_host_max_terms.load(); }
// the engine entry points of the host-transcript route, on the GPU or -- tiny calls, or no context -- on the host
int be_msm_many(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points, uint32_t n_points, int flags,
                uint8_t* out, uint8_t* status) {
  if (on_host(ctx, n_msm ? off[n_msm] : 0)) return zkp::hostbk::msm_many(n_msm, off, scalars, pidx, points, n_points, flags, out, status);
  return zkp_msm_many(ctx, n_msm, off, scalars, pidx, points, n_points, flags, out, status);
}
int be_decode_check(zkp_ctx* ctx, bool host, uint64_t n, const uint8_t* points, uint8_t* status) {
  if (host) return zkp::hostbk::decode_check(n, points, status);
  return zkp_decode_check(ctx, n, points, status, nullptr);
}
}  // namespace

namespace zkp {
namespace host {

// false = the operating system gave no entropy (getrandom failed with anything but EINTR): callers fail closed
bool os_entropy(uint8_t* out, size_t len) {
  size_t got = 0;
  while (got < len) {
    const ssize_t r = getrandom(out + got, len - got, 0);
    if (r > 0) got += (size_t)r;
    else if (r < 0 && errno == EINTR) continue;
    else return false;
  }
  return true;
}

// ChaCha20 block function (RFC 8439 section 2.3), used as the stream generator below
inline uint32_t rotl32(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }
void chacha20_block(const uint32_t key[8], uint64_t counter, uint64_t nonce, uint8_t out[64]) {
  uint32_t st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                     (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)nonce, (uint32_t)(nonce >> 32)};
  uint32_t x[16];
  std::memcpy(x, st, sizeof(x));
#define ZKP_QR(a, b, c, d) x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 12); \
                           x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 7);
  for (int r = 0; r < 10; ++r) {
    ZKP_QR(0, 4, 8, 12) ZKP_QR(1, 5, 9, 13) ZKP_QR(2, 6, 10, 14) ZKP_QR(3, 7, 11, 15)
    ZKP_QR(0, 5, 10, 15) ZKP_QR(1, 6, 11, 12) ZKP_QR(2, 7, 8, 13) ZKP_QR(3, 4, 9, 14)
  }
#undef ZKP_QR
  for (int i = 0; i < 16; ++i) { const uint32_t v = x[i] + st[i]; std::memcpy(out + 4 * i, &v, 4); }
}

// What `thread_rng()` is to the reference (prover.rs:82, verifier.rs:153, batch_verifier.rs:179): a ChaCha stream keyed
// with 32 bytes from the operating system for every call -- getrandom() itself delivers only a few hundred MB/s, which
// for the batch verifier's 16 bytes per (constraint, proof) would cost more than the whole GPU side of the call.
bool os_random(uint8_t* out, size_t len) {
  if (len <= 256) return os_entropy(out, len);
  uint32_t key[8];
  uint64_t nonce;
  if (!os_entropy(reinterpret_cast<uint8_t*>(key), sizeof(key)) || !os_entropy(reinterpret_cast<uint8_t*>(&nonce), sizeof(nonce))) return false;
  const uint64_t blocks = (len + 63) / 64;
  parallel_for((uint32_t)std::min<uint64_t>(blocks, 0xffffffffu), 0, [&](uint32_t lo, uint32_t hi) {
    uint8_t tmp[64];
    for (uint64_t b = lo; b < hi; ++b) {
      const size_t o = (size_t)b * 64;
      if (o + 64 <= len) chacha20_block(key, b, nonce, out + o);
      else { chacha20_block(key, b, nonce, tmp); std::memcpy(out + o, tmp, len - o); }
    }
  });
  return true;
}

}  // namespace host
}  // namespace zkp

namespace {

// encoding of point variable p for proof j
inline const uint8_t* point_enc(const zkp_statement& st, uint32_t p, uint32_t j, uint32_t N, const uint8_t* inst,
                                const uint8_t* common) {
  const auto& pt = st.points[p];
  return pt.common ? common + 32 * (size_t)pt.rank : inst + 32 * ((size_t)pt.rank * N + j);
}
// index of point variable p of proof j in the device point table  common || inst (row-major [ni][N])
inline uint32_t table_index(const zkp_statement& st, uint32_t p, uint32_t j, uint32_t N) {
  const auto& pt = st.points[p];
  return pt.common ? pt.rank : st.ns + pt.rank * N + j;
}

// Scalar::from_canonical_bytes: the value must be < l = 2^252 + 27742317777372353535851937790883648493.  The reference's proofs
// reach its verifiers through serde (proofs.rs:14-32), and dalek's Deserialize refuses any other encoding of a Scalar; the
// verify entry points below take proofs as raw bytes, so they apply the same rule: a response (or challenge) >= l is a
// VerificationFailure for that proof / batch.
inline bool scalar_is_canonical(const uint8_t s[32]) {
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
  for (int i = 31; i >= 0; --i) {
    if (s[i] < L[i]) return true;
    if (s[i] > L[i]) return false;
  }
  return false;                                                      // == l
}
// proofs (of N) whose m responses are not all canonical -> flag[j] = 1; returns whether any is
bool flag_noncanonical(uint32_t N, uint32_t m, const uint8_t* responses, uint8_t* flag) {
  bool any = false;
  for (uint32_t j = 0; j < N; ++j)
    for (uint32_t i = 0; i < m; ++i)
      if (!scalar_is_canonical(responses + 32 * ((size_t)j * m + i))) { if (flag) flag[j] = 1; any = true; break; }
  return any;
}

bool all_transcripts_equal(const uint8_t* ts, uint32_t N) {
  for (uint32_t j = 1; j < N; ++j)
    if (std::memcmp(ts, ts + TB * (size_t)j, Transcript::kLiveBytes) != 0) return false;       // (the 5 padding bytes carry nothing)
  return true;
}

// Prover::new + the allocate_scalar calls that precede the first point (prover.rs:41-57) / the same on the verifier
// side.  When all N incoming transcripts are equal (the usual case) this prefix is hashed once and cloned.
void apply_prefix(const zkp_statement& st, uint32_t N, uint8_t* ts, int n_threads) {
  const uint32_t lead = st.scalar_prefix();
  auto prefix = [&](Transcript& t) {
    t.domain_sep(st.label.c_str());
    for (uint32_t a = 0; a < lead; ++a) t.append_scalar_var(st.secrets[st.alloc[a].idx].c_str());
  };
  if (N > 1 && all_transcripts_equal(ts, N)) {
    Transcript t = Transcript::from_bytes(ts);
    prefix(t);
    for (uint32_t j = 0; j < N; ++j) t.to_bytes(ts + TB * (size_t)j);
    return;
  }
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
      prefix(t);
      t.to_bytes(ts + TB * (size_t)j);
    }
  });
}

// The allocations after the scalar prefix, in the caller's order (points and any scalar allocated after a point).
// validate = the verifier-side appends, which reject the identity encoding (mod.rs:186-196); false on rejection.
bool replay_allocations(const zkp_statement& st, Transcript& t, uint32_t j, uint32_t N, const uint8_t* inst, const uint8_t* common,
                        bool validate) {
  for (uint32_t a = st.scalar_prefix(); a < st.alloc.size(); ++a) {
    const auto& al = st.alloc[a];
    if (!al.is_point) { t.append_scalar_var(st.secrets[al.idx].c_str()); continue; }
    const char* name = st.points[al.idx].name.c_str();
    const uint8_t* enc = point_enc(st, al.idx, j, N, inst, common);
    if (!validate) t.append_point_var(name, enc);
    else if (!t.validate_and_append_point_var(name, enc)) return false;
  }
  return true;
}

// point variables no constraint mentions (e.g. `B` of the CMZ statement, benches/zkp.rs:32): verify_compact
// still insists that they decompress (verifier.rs:87-92)
std::vector<uint32_t> unreferenced_points(const zkp_statement& st) {
  std::vector<char> used(st.points.size(), 0);
  for (const auto& c : st.cons) {
    used[c.lhs] = 1;
    for (const auto& t : c.lc) used[t.second] = 1;
  }
  std::vector<uint32_t> out;
  for (uint32_t p = 0; p < st.points.size(); ++p)
    if (!used[p]) out.push_back(p);
  return out;
}

std::vector<uint8_t> point_table(const zkp_statement& st, uint32_t N, const uint8_t* inst, const uint8_t* common) {
  std::vector<uint8_t> tbl(32 * ((size_t)st.ns + (size_t)st.ni * N));
  if (st.ns) std::memcpy(tbl.data(), common, 32 * (size_t)st.ns);
  if (st.ni) std::memcpy(tbl.data() + 32 * (size_t)st.ns, inst, 32 * (size_t)st.ni * N);
  return tbl;
}

}  // namespace

extern "C" {

void zkp_chacha20_block(const uint8_t key[32], uint64_t counter, uint64_t nonce, uint8_t out[64]) {
  uint32_t k[8];
  std::memcpy(k, key, 32);
  chacha20_block(k, counter, nonce, out);
}
void zkp_toolbox_set_host_max_terms(uint32_t n) { g_host_max_terms = n; }
uint32_t zkp_toolbox_get_host_max_terms(void) { return g_host_max_terms.load(); }
void zkp_toolbox_set_fused_min_batch(uint32_t n) { g_fused_min_batch = n; }
uint32_t zkp_toolbox_get_fused_min_batch(void) { return g_fused_min_batch.load(); }

// ---- transcripts / scalars -----------------------------------------------------------------------------
void zkp_transcript_init(uint8_t* t, const uint8_t* label, size_t len) { Transcript(label, len).to_bytes(t); }
// merlin's encode_usize_as_u32 asserts that lengths fit 32 bits (the > 4 GiB case of tests/sig_and_vrf_example.rs:224-241):
// an error here, never a truncated length prefix
static bool fits_u32(size_t n) { return (uint64_t)n <= 0xffffffffull; }
int zkp_transcript_append_message(uint8_t* t, const char* label, const uint8_t* msg, size_t len) {
  if (!t || !label || (len && !msg)) return ZKP_TB_BAD_STATEMENT;
  if (!fits_u32(len) || !fits_u32(std::strlen(label))) return ZKP_TB_TOO_LONG;
  Transcript x = Transcript::from_bytes(t);
  x.append_message(label, msg, len);
  x.to_bytes(t);
  return ZKP_TB_OK;
}
// merlin append_message over a CSR batch on host threads (about one Keccak-f per 166 bytes: nothing the device would gain on).  Every
// argument is checked before any transcript changes.
int zkp_transcripts_append_message_batch(uint8_t* ts, uint32_t N, int shared_initial, const char* label, const uint8_t* msgs, const uint64_t* offsets,
                                         int n_threads) {
  if (!label) return ZKP_TB_BAD_STATEMENT;
  if (!fits_u32(std::strlen(label))) return ZKP_TB_TOO_LONG;
  if (N == 0) return ZKP_TB_OK;
  if (!ts || !offsets || (offsets[N] > offsets[0] && !msgs)) return ZKP_TB_BAD_STATEMENT;
  for (uint32_t j = 0; j < N; ++j) {
    if (offsets[j + 1] < offsets[j]) return ZKP_TB_BAD_STATEMENT;
    if (!fits_u32(offsets[j + 1] - offsets[j])) return ZKP_TB_TOO_LONG;
  }
  uint8_t init[TB];
  if (shared_initial) std::memcpy(init, ts, TB);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript x = Transcript::from_bytes(shared_initial ? init : ts + TB * (size_t)j);
      x.append_message(label, msgs + offsets[j], offsets[j + 1] - offsets[j]);
      x.to_bytes(ts + TB * (size_t)j);
    }
  });
  return ZKP_TB_OK;
}
// (zkp_mi355x.h (7) takes labels of up to 248 bytes as a kernel argument; merlin's labels are short literals, a longer one stays on the host)
static bool device_label(const char* label) { return std::strlen(label) <= 248; }
static bool positions_ok(const uint8_t* ts, uint32_t n) {
  for (uint32_t j = 0; j < n; ++j)
    if (ts[TB * (size_t)j + 200] >= 166) return false;
  return true;
}
// The same with a context: the checks of the call above plus the position bytes (a position of 166 or more is no STROBE state: host
// Merlin would index past its state with it), then the host threads for ctx == NULL, N <= host_max_terms or messages of fewer than 128
// bytes on average, the device otherwise (zkp_transcripts_append_message: one lane per transcript).  Same bytes on both routes.
int zkp_transcripts_append_message_batch_ctx(zkp_ctx* ctx, uint8_t* ts, uint32_t N, int shared_initial, const char* label, const uint8_t* msgs,
                                             const uint64_t* offsets, int n_threads) {
  if (!label) return ZKP_TB_BAD_STATEMENT;
  if (!fits_u32(std::strlen(label))) return ZKP_TB_TOO_LONG;
  if (N == 0) return ZKP_TB_OK;
  if (!ts || !offsets || (offsets[N] > offsets[0] && !msgs)) return ZKP_TB_BAD_STATEMENT;
  for (uint32_t j = 0; j < N; ++j) {
    if (offsets[j + 1] < offsets[j]) return ZKP_TB_BAD_STATEMENT;
    if (!fits_u32(offsets[j + 1] - offsets[j])) return ZKP_TB_TOO_LONG;
  }
  if (!positions_ok(ts, shared_initial ? 1 : N)) return ZKP_TB_BAD_STATEMENT;
  // The device call moves every 208-byte blob over the bus, which is what the host threads pay for a message that fits the block the
  // transcript stands in; it wins once the permutations dominate (profiles/transcript_ops_bench.txt: 32-byte messages are faster on the
  // host threads at every measured N, the 0..599-byte mix and 4,096-byte messages on the device): from 128 message bytes per transcript on.
  const bool short_messages = offsets[N] - offsets[0] < 128 * (uint64_t)N;
  if (on_host(ctx, N) || short_messages || !device_label(label))
    return zkp_transcripts_append_message_batch(ts, N, shared_initial, label, msgs, offsets, n_threads);
  return zkp_transcripts_append_message(ctx, N, shared_initial, ts, label, msgs, offsets);
}
int zkp_transcript_challenge_bytes(uint8_t* t, const char* label, uint8_t* out, size_t len) {
  if (!t || !label || (len && !out)) return ZKP_TB_BAD_STATEMENT;
  if (!fits_u32(len) || !fits_u32(std::strlen(label))) return ZKP_TB_TOO_LONG;
  Transcript x = Transcript::from_bytes(t);
  x.challenge_bytes(label, out, len);
  x.to_bytes(t);
  return ZKP_TB_OK;
}
// N x challenge_bytes(label, out[j], len), routed as the append above; the transcripts advance in place
int zkp_transcripts_challenge_bytes_batch(zkp_ctx* ctx, uint8_t* ts, uint32_t N, const char* label, uint32_t len, int n_threads, uint8_t* out) {
  if (!label) return ZKP_TB_BAD_STATEMENT;
  if (!fits_u32(std::strlen(label))) return ZKP_TB_TOO_LONG;
  if (N == 0) return ZKP_TB_OK;
  if (!ts || (len && !out) || !positions_ok(ts, N)) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, N) && device_label(label)) return zkp_transcripts_challenge_bytes(ctx, N, ts, label, len, out);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript x = Transcript::from_bytes(ts + TB * (size_t)j);
      x.challenge_bytes(label, out + (size_t)len * j, len);
      x.to_bytes(ts + TB * (size_t)j);
    }
  });
  return ZKP_TB_OK;
}
void zkp_scalar_from_wide(uint8_t out[32], const uint8_t in[64]) { Scalar::from_bytes_mod_order_wide(in).to_bytes(out); }
void zkp_scalar_muladd(uint8_t out[32], const uint8_t a[32], const uint8_t b[32], const uint8_t c[32]) {
  (Scalar::from_bytes_mod_order(a) * Scalar::from_bytes_mod_order(b) + Scalar::from_bytes_mod_order(c)).to_bytes(out);
}
void zkp_scalar_neg(uint8_t out[32], const uint8_t a[32]) { (-Scalar::from_bytes_mod_order(a)).to_bytes(out); }

// ---- proof wire format (proofs.rs:14-32 under bincode 1.x; see zkp_toolbox.h) -----------------------------------------
namespace {
inline void put_u64le(uint8_t* out, uint64_t v) { for (int i = 0; i < 8; ++i) out[i] = (uint8_t)(v >> (8 * i)); }
inline uint64_t get_u64le(const uint8_t* in) { uint64_t v = 0; for (int i = 0; i < 8; ++i) v |= (uint64_t)in[i] << (8 * i); return v; }
// u64 count + count x 32 bytes at in[pos..]; false = truncated / count larger than the remaining bytes
inline bool read_vec32(const uint8_t* in, size_t len, size_t& pos, uint64_t& count) {
  if (len - pos < 8) return false;
  count = get_u64le(in + pos);
  pos += 8;
  if (count > (len - pos) / 32) return false;
  return true;
}
}  // namespace

size_t zkp_proof_compact_size(uint32_t m) { return 40 + 32 * (size_t)m; }
size_t zkp_proof_batchable_size(uint32_t nc, uint32_t m) { return 16 + 32 * ((size_t)nc + m); }

int zkp_proof_compact_encode(const uint8_t challenge[32], const uint8_t* responses, uint32_t m, uint8_t* out, size_t out_len) {
  if (!challenge || !out || (m && !responses) || out_len < zkp_proof_compact_size(m)) return ZKP_TB_BAD_STATEMENT;
  std::memcpy(out, challenge, 32);
  put_u64le(out + 32, m);
  if (m) std::memcpy(out + 40, responses, 32 * (size_t)m);
  return ZKP_TB_OK;
}
int zkp_proof_compact_decode(const uint8_t* in, size_t len, uint8_t challenge[32], uint8_t* responses, uint32_t max_m, uint32_t* m,
                             size_t* consumed) {
  if (!in || !challenge || !m || (max_m && !responses)) return ZKP_TB_BAD_STATEMENT;
  if (len < 32) return ZKP_TB_BAD_ENCODING;
  size_t pos = 32;
  uint64_t cnt = 0;
  if (!read_vec32(in, len, pos, cnt)) return ZKP_TB_BAD_ENCODING;
  if (cnt > max_m) return ZKP_TB_BAD_STATEMENT;
  if (!scalar_is_canonical(in)) return ZKP_TB_BAD_ENCODING;
  for (uint64_t i = 0; i < cnt; ++i)
    if (!scalar_is_canonical(in + pos + 32 * i)) return ZKP_TB_BAD_ENCODING;
  std::memcpy(challenge, in, 32);
  if (cnt) std::memcpy(responses, in + pos, 32 * (size_t)cnt);
  *m = (uint32_t)cnt;
  if (consumed) *consumed = pos + 32 * (size_t)cnt;
  return ZKP_TB_OK;
}
int zkp_proof_batchable_encode(const uint8_t* commitments, uint32_t nc, const uint8_t* responses, uint32_t m, uint8_t* out, size_t out_len) {
  if (!out || (nc && !commitments) || (m && !responses) || out_len < zkp_proof_batchable_size(nc, m)) return ZKP_TB_BAD_STATEMENT;
  put_u64le(out, nc);
  if (nc) std::memcpy(out + 8, commitments, 32 * (size_t)nc);
  uint8_t* q = out + 8 + 32 * (size_t)nc;
  put_u64le(q, m);
  if (m) std::memcpy(q + 8, responses, 32 * (size_t)m);
  return ZKP_TB_OK;
}
int zkp_proof_batchable_decode(const uint8_t* in, size_t len, uint8_t* commitments, uint32_t max_nc, uint32_t* nc, uint8_t* responses,
                               uint32_t max_m, uint32_t* m, size_t* consumed) {
  if (!in || !nc || !m || (max_nc && !commitments) || (max_m && !responses)) return ZKP_TB_BAD_STATEMENT;
  size_t pos = 0;
  uint64_t c = 0, r = 0;
  if (!read_vec32(in, len, pos, c)) return ZKP_TB_BAD_ENCODING;
  const size_t cpos = pos;
  pos += 32 * (size_t)c;
  if (!read_vec32(in, len, pos, r)) return ZKP_TB_BAD_ENCODING;
  if (c > max_nc || r > max_m) return ZKP_TB_BAD_STATEMENT;
  for (uint64_t i = 0; i < r; ++i)
    if (!scalar_is_canonical(in + pos + 32 * i)) return ZKP_TB_BAD_ENCODING;
  if (c) std::memcpy(commitments, in + cpos, 32 * (size_t)c);      // CompressedRistretto: any 32 bytes (validity = decompress())
  if (r) std::memcpy(responses, in + pos, 32 * (size_t)r);
  *nc = (uint32_t)c;
  *m = (uint32_t)r;
  if (consumed) *consumed = pos + 32 * (size_t)r;
  return ZKP_TB_OK;
}

// ---- statements -------------------------------------------------------------------------------------------
zkp_statement* zkp_statement_new(const char* proof_label) {
  auto* st = new zkp_statement();
  st->label = proof_label ? proof_label : "";
  return st;
}
void zkp_statement_free(zkp_statement* st) { delete st; }
int zkp_statement_add_secret(zkp_statement* st, const char* name) {
  if (!st || !name) return ZKP_TB_BAD_STATEMENT;
  st->secrets.emplace_back(name);
  st->alloc.push_back({false, (uint32_t)st->secrets.size() - 1});
  return (int)st->secrets.size() - 1;
}
int zkp_statement_add_point(zkp_statement* st, const char* name, int is_common) {
  if (!st || !name) return ZKP_TB_BAD_STATEMENT;
  st->points.push_back({name, is_common != 0, is_common ? st->ns++ : st->ni++});
  st->alloc.push_back({true, (uint32_t)st->points.size() - 1});
  return (int)st->points.size() - 1;
}
int zkp_statement_constrain(zkp_statement* st, uint32_t lhs, uint32_t n_terms, const uint32_t* secrets, const uint32_t* points) {
  if (!st || lhs >= st->points.size() || (n_terms && (!secrets || !points))) return ZKP_TB_BAD_STATEMENT;
  zkp_statement::Constraint c;
  c.lhs = lhs;
  for (uint32_t i = 0; i < n_terms; ++i) {
    if (secrets[i] >= st->secrets.size() || points[i] >= st->points.size()) return ZKP_TB_BAD_STATEMENT;
    c.lc.emplace_back(secrets[i], points[i]);
  }
  st->terms += n_terms;
  st->cons.push_back(std::move(c));
  return ZKP_TB_OK;
}
uint32_t zkp_statement_num_secrets(const zkp_statement* st) { return st ? (uint32_t)st->secrets.size() : 0; }
uint32_t zkp_statement_num_instance(const zkp_statement* st) { return st ? st->ni : 0; }
uint32_t zkp_statement_num_common(const zkp_statement* st) { return st ? st->ns : 0; }
uint32_t zkp_statement_num_constraints(const zkp_statement* st) { return st ? (uint32_t)st->cons.size() : 0; }
uint32_t zkp_statement_num_terms(const zkp_statement* st) { return st ? st->terms : 0; }

// ---- prover -----------------------------------------------------------------------------------------------
int zkp_prove_phase_a(const zkp_statement* stp, uint32_t N, uint8_t* ts, const uint8_t* secrets, const uint8_t* inst,
                      const uint8_t* common, const uint8_t* entropy, int n_threads, uint8_t* blindings, uint32_t* off,
                      uint8_t* scalars, uint32_t* pidx) {
  if (!stp || !ts || !off) return ZKP_TB_BAD_STATEMENT;
  // empty parts of a statement come with empty (possibly NULL) buffers
  if ((!stp->secrets.empty() && (!secrets || !blindings)) || (stp->terms && (!scalars || !pidx))) return ZKP_TB_BAD_STATEMENT;
  const zkp_statement& st = *stp;
  const uint32_t m = (uint32_t)st.secrets.size(), nc = (uint32_t)st.cons.size(), T = st.terms;
  apply_prefix(st, N, ts, n_threads);                                  // prover.rs:42, :54
  std::vector<uint8_t> own_entropy;
  if (!entropy) {                                                      // prover.rs:82 `thread_rng()`
    own_entropy.resize(32 * (size_t)N);
    if (!os_random(own_entropy.data(), own_entropy.size())) return ZKP_TB_NO_ENTROPY;
    entropy = own_entropy.data();
  }
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
      replay_allocations(st, t, j, N, inst, common, false);            // prover.rs:52-73 (encodings are supplied)
      zkp::host::TranscriptRng rng = t.build_rng();                    // prover.rs:78-82
      for (uint32_t i = 0; i < m; ++i) rng.rekey_with_witness_bytes("", secrets + 32 * ((size_t)j * m + i), 32);
      rng.finalize(entropy + 32 * (size_t)j);
      uint8_t* b = blindings + 32 * (size_t)j * m;
      for (uint32_t i = 0; i < m; ++i) {                               // prover.rs:85-89 Scalar::random
        uint8_t wide[64];
        rng.fill_bytes(wide, 64);
        Scalar::from_bytes_mod_order_wide(wide).to_bytes(b + 32 * i);
      }
      size_t q = (size_t)j * T;                                        // prover.rs:94-97 operand lists
      for (uint32_t k = 0; k < nc; ++k) {
        off[(size_t)j * nc + k] = (uint32_t)q;
        for (const auto& term : st.cons[k].lc) {
          std::memcpy(scalars + 32 * q, b + 32 * term.first, 32);
          pidx[q] = table_index(st, term.second, j, N);
          ++q;
        }
      }
      t.to_bytes(ts + TB * (size_t)j);
    }
  });
  off[(size_t)N * nc] = (uint32_t)((size_t)N * T);
  return ZKP_TB_OK;
}

int zkp_prove_phase_b(const zkp_statement* stp, uint32_t N, uint8_t* ts, const uint8_t* secrets, const uint8_t* blindings,
                      const uint8_t* commitments, int n_threads, uint8_t* challenges, uint8_t* responses) {
  if (!stp || !ts || !challenges || (!stp->cons.empty() && !commitments) || (!stp->secrets.empty() && !responses)) return ZKP_TB_BAD_STATEMENT;
  const zkp_statement& st = *stp;
  const uint32_t m = (uint32_t)st.secrets.size(), nc = (uint32_t)st.cons.size();
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
      for (uint32_t k = 0; k < nc; ++k)                                // prover.rs:98-100
        t.append_blinding_commitment(st.points[st.cons[k].lhs].name.c_str(), commitments + 32 * ((size_t)j * nc + k));
      uint8_t* c = challenges + 32 * (size_t)j;
      t.get_challenge("chal", c);                                      // prover.rs:106
      const Scalar cs = Scalar::from_bytes_mod_order(c);
      for (uint32_t i = 0; i < m; ++i) {                               // prover.rs:107-109  s * c + b
        const size_t o = 32 * ((size_t)j * m + i);
        (Scalar::from_bytes_mod_order(secrets + o) * cs + Scalar::from_bytes_mod_order(blindings + o)).to_bytes(responses + o);
      }
      t.to_bytes(ts + TB * (size_t)j);
    }
  });
  return ZKP_TB_OK;
}

int zkp_prove_batch(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint8_t* ts, const uint8_t* secrets,
                    const uint8_t* inst, const uint8_t* common, const uint8_t* entropy, int n_threads, uint8_t* challenges,
                    uint8_t* responses, uint8_t* commitments) {
  if (!st) return ZKP_TB_BAD_STATEMENT;                                  // (ctx == NULL: the host backend, host_backend.cpp)
  if (N == 0) return ZKP_TB_OK;
  if (ctx && ts && use_fused(ts, N)) {
    // no entropy from the caller: 40 bytes of getrandom() key a ChaCha20 stream that is expanded on the device (what thread_rng() is to prover.rs:82)
    uint8_t seed[40];
    if (!entropy && !os_entropy(seed, sizeof(seed))) return ZKP_TB_NO_ENTROPY;
    if (st->ns && N >= 32) { const int rc = zkp_ctx_prepare_fixed_points(ctx, st->ns, common); if (rc) return rc; }
    FusedView fv(*st);
    int invalid = 0;
    const int rc = entropy ? zkp_fused_prove(ctx, &fv.fs, N, ts, secrets, inst, common, entropy, challenges, responses, commitments, &invalid)
                           : zkp_fused_prove_seeded(ctx, &fv.fs, N, ts, secrets, inst, common, seed, challenges, responses, commitments, &invalid);
    if (rc) return rc;
    return invalid ? ZKP_TB_INVALID_POINT : ZKP_TB_OK;
  }
  if (ctx && ts && use_ragged(ts, N)) {                                  // the same on the device, one transcript program per position class
    uint8_t seed[40];
    if (!entropy && !os_entropy(seed, sizeof(seed))) return ZKP_TB_NO_ENTROPY;
    if (st->ns && N >= 32) { const int rc = zkp_ctx_prepare_fixed_points(ctx, st->ns, common); if (rc) return rc; }
    FusedView fv(*st);
    int invalid = 0;
    const int rc = zkp_fused_prove_ragged(ctx, &fv.fs, N, ts, secrets, inst, common, entropy, entropy ? nullptr : seed, challenges, responses, commitments, &invalid);
    if (rc) return rc;
    return invalid ? ZKP_TB_INVALID_POINT : ZKP_TB_OK;
  }
  const uint32_t m = (uint32_t)st->secrets.size(), nc = (uint32_t)st->cons.size(), T = st->terms;
  std::vector<uint8_t> blind(32 * (size_t)N * m), scalars(32 * (size_t)N * T), status((size_t)N * nc);
  std::vector<uint32_t> off((size_t)N * nc + 1), pidx((size_t)N * T);
  int rc = zkp_prove_phase_a(st, N, ts, secrets, inst, common, entropy, n_threads, blind.data(), off.data(), scalars.data(), pidx.data());
  if (rc) return rc;
  const std::vector<uint8_t> tbl = point_table(*st, N, inst, common);
  if (ctx && st->ns && N >= 32) { rc = zkp_ctx_prepare_fixed_points(ctx, st->ns, common); if (rc) return rc; }   // common points: fixed-base tables
  // prover.rs:94 RistrettoPoint::multiscalar_mul for every constraint of every proof, + compress (mod.rs:204)
  rc = be_msm_many(ctx, N * nc, off.data(), scalars.data(), pidx.data(), tbl.data(), (uint32_t)(tbl.size() / 32), ZKP_CT,
                   commitments, status.data());
  if (rc) return rc;
  for (uint8_t s : status)
    if (s) return ZKP_TB_INVALID_POINT;     // the reference prover holds decoded points; an undecodable input is a caller bug
  return zkp_prove_phase_b(st, N, ts, secrets, blind.data(), commitments, n_threads, challenges, responses);
}

// ---- single-proof verification, batched over N independent proofs -----------------------------------------
// Verifier::new + allocate_* (verifier.rs:47-77); failed[j] = 1 when an identity point is rejected
static void build_verifiers(const zkp_statement& st, uint32_t N, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                            int n_threads, uint8_t* failed) {
  apply_prefix(st, N, ts, n_threads);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
      if (!replay_allocations(st, t, j, N, inst, common, true)) failed[j] = 1;
      t.to_bytes(ts + TB * (size_t)j);
    }
  });
}

int zkp_verify_compact_batch(zkp_ctx* ctx, const zkp_statement* stp, uint32_t N, uint8_t* ts, const uint8_t* inst,
                             const uint8_t* common, const uint8_t* challenges, const uint8_t* responses, int n_threads,
                             uint8_t* results) {
  if (!stp || !ts || !results || !challenges || (!stp->secrets.empty() && !responses)) return ZKP_TB_BAD_STATEMENT;
  if (N == 0) return ZKP_TB_OK;
  const zkp_statement& st = *stp;
  if (ctx && use_fused(ts, N)) {
    if (st.ns && N >= 32) { const int rc = zkp_ctx_prepare_fixed_points(ctx, st.ns, common); if (rc) return rc; }
    FusedView fv(st);
    return zkp_fused_verify_compact(ctx, &fv.fs, N, ts, inst, common, challenges, responses, results);
  }
  if (ctx && use_ragged(ts, N)) {
    if (st.ns && N >= 32) { const int rc = zkp_ctx_prepare_fixed_points(ctx, st.ns, common); if (rc) return rc; }
    FusedView fv(st);
    return zkp_fused_verify_compact_ragged(ctx, &fv.fs, N, ts, inst, common, challenges, responses, results);
  }
  const uint32_t m = (uint32_t)st.secrets.size(), nc = (uint32_t)st.cons.size(), T1 = st.terms + nc;
  std::memset(results, 0, N);
  flag_noncanonical(N, m, responses, results);                         // proofs.rs:15-20 through serde: s >= l never reaches the verifier
  build_verifiers(st, N, ts, inst, common, n_threads, results);
  // verifier.rs:95-106: per constraint, responses over the rhs points and (-c) over the lhs point
  std::vector<uint8_t> scalars(32 * (size_t)N * T1), coms(32 * (size_t)N * nc), status((size_t)N * nc);
  std::vector<uint32_t> off((size_t)N * nc + 1), pidx((size_t)N * T1);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      uint8_t minus_c[32];
      (-Scalar::from_bytes_mod_order(challenges + 32 * (size_t)j)).to_bytes(minus_c);
      size_t q = (size_t)j * T1;
      for (uint32_t k = 0; k < nc; ++k) {
        off[(size_t)j * nc + k] = (uint32_t)q;
        for (const auto& term : st.cons[k].lc) {
          std::memcpy(scalars.data() + 32 * q, responses + 32 * ((size_t)j * m + term.first), 32);
          pidx[q++] = table_index(st, term.second, j, N);
        }
        std::memcpy(scalars.data() + 32 * q, minus_c, 32);
        pidx[q++] = table_index(st, st.cons[k].lhs, j, N);
      }
    }
  });
  off[(size_t)N * nc] = (uint32_t)((size_t)N * T1);
  const std::vector<uint8_t> tbl = point_table(st, N, inst, common);
  int rc = (ctx && st.ns && N >= 32) ? zkp_ctx_prepare_fixed_points(ctx, st.ns, common) : 0;
  if (rc) return rc;
  const bool host = on_host(ctx, (uint64_t)N * T1);
  rc = be_msm_many(ctx, N * nc, off.data(), scalars.data(), pidx.data(), tbl.data(), (uint32_t)(tbl.size() / 32),
                   ZKP_VARTIME, coms.data(), status.data());
  if (rc) return rc;
  // verifier.rs:87-92 decompresses EVERY allocated point, also those no constraint uses
  const std::vector<uint32_t> unref = unreferenced_points(st);
  if (!unref.empty()) {
    std::vector<uint8_t> encs, st8;
    std::vector<std::pair<uint32_t, int>> owner;     // (proof or ~0 for all, unused)
    for (uint32_t p : unref) {
      if (st.points[p].common) { encs.insert(encs.end(), common + 32 * (size_t)st.points[p].rank, common + 32 * (size_t)st.points[p].rank + 32); owner.emplace_back(~0u, 0); }
      else for (uint32_t j = 0; j < N; ++j) { const uint8_t* e = point_enc(st, p, j, N, inst, common); encs.insert(encs.end(), e, e + 32); owner.emplace_back(j, 0); }
    }
    st8.resize(owner.size());
    rc = be_decode_check(ctx, host, owner.size(), encs.data(), st8.data());
    if (rc) return rc;
    for (size_t i = 0; i < owner.size(); ++i)
      if (st8[i]) {
        if (owner[i].first == ~0u) std::memset(results, 1, N);
        else results[owner[i].first] = 1;
      }
  }
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      if (results[j]) continue;
      bool bad = false;
      for (uint32_t k = 0; k < nc; ++k) bad |= status[(size_t)j * nc + k] != 0;
      if (bad) { results[j] = 1; continue; }
      Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
      for (uint32_t k = 0; k < nc; ++k)                                // verifier.rs:108 (non-validating append)
        t.append_blinding_commitment(st.points[st.cons[k].lhs].name.c_str(), coms.data() + 32 * ((size_t)j * nc + k));
      uint8_t c[32];
      t.get_challenge("chal", c);                                      // verifier.rs:113-119
      // the recomputed challenge is canonical and is compared with the claimed BYTES: c + l is a different `Scalar`
      // for the reference (and does not even deserialise), so it must not verify here either
      results[j] = std::memcmp(c, challenges + 32 * (size_t)j, 32) == 0 ? 0 : 1;
      t.to_bytes(ts + TB * (size_t)j);
    }
  });
  return ZKP_TB_OK;
}

int zkp_verify_batchable_each(zkp_ctx* ctx, const zkp_statement* stp, uint32_t N, uint8_t* ts, const uint8_t* inst,
                              const uint8_t* common, const uint8_t* commitments, const uint8_t* responses,
                              const uint8_t* weights16, int n_threads, uint8_t* results) {
  if (!stp || !ts || !results || (!stp->cons.empty() && !commitments) || (!stp->secrets.empty() && !responses)) return ZKP_TB_BAD_STATEMENT;
  if (N == 0) return ZKP_TB_OK;
  const zkp_statement& st = *stp;
  const uint32_t m = (uint32_t)st.secrets.size(), nc = (uint32_t)st.cons.size(), np = (uint32_t)st.points.size();
  std::vector<uint8_t> own_w;
  if (!weights16) { own_w.resize(16 * (size_t)N * nc); if (!os_random(own_w.data(), own_w.size())) return ZKP_TB_NO_ENTROPY; weights16 = own_w.data(); }
  if (ctx && use_fused(ts, N)) {
    if (st.ns && N >= 32) { const int rc = zkp_ctx_prepare_fixed_points(ctx, st.ns, common); if (rc) return rc; }
    FusedView fv(st);
    return zkp_fused_verify_batchable(ctx, &fv.fs, N, ts, inst, common, commitments, responses, weights16, results);
  }
  if (ctx && use_ragged(ts, N)) {
    if (st.ns && N >= 32) { const int rc = zkp_ctx_prepare_fixed_points(ctx, st.ns, common); if (rc) return rc; }
    FusedView fv(st);
    return zkp_fused_verify_batchable_ragged(ctx, &fv.fs, N, ts, inst, common, commitments, responses, weights16, results);
  }
  std::memset(results, 0, N);
  flag_noncanonical(N, m, responses, results);                         // proofs.rs:27-32 through serde
  build_verifiers(st, N, ts, inst, common, n_threads, results);
  // one (np + nc)-term MSM per proof over  points || commitments   (verifier.rs:144-166)
  const uint32_t K = np + nc;
  std::vector<uint8_t> scalars(32 * (size_t)N * K), out(32 * (size_t)N), status(N);
  std::vector<uint32_t> off((size_t)N + 1), pidx((size_t)N * K);
  // point table: common || inst || commitments [N][nc]
  std::vector<uint8_t> tbl = point_table(st, N, inst, common);
  const uint32_t com_base = (uint32_t)(tbl.size() / 32);
  tbl.insert(tbl.end(), commitments, commitments + 32 * (size_t)N * nc);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    std::vector<Scalar> coeffs(K);
    for (uint32_t j = lo; j < hi; ++j) {
      off[j] = j * K;
      if (results[j]) { for (uint32_t i = 0; i < K; ++i) pidx[(size_t)j * K + i] = 0; continue; }
      Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
      for (uint32_t k = 0; k < nc && !results[j]; ++k)                 // verifier.rs:134-140
        if (!t.validate_and_append_blinding_commitment(st.points[st.cons[k].lhs].name.c_str(), commitments + 32 * ((size_t)j * nc + k)))
          results[j] = 1;
      uint8_t c[32];
      t.get_challenge("chal", c);
      t.to_bytes(ts + TB * (size_t)j);
      const Scalar minus_c = -Scalar::from_bytes_mod_order(c);         // verifier.rs:142
      std::fill(coeffs.begin(), coeffs.end(), Scalar::zero());
      for (uint32_t k = 0; k < nc; ++k) {                              // verifier.rs:151-160
        const Scalar r = Scalar::from_u128_le(weights16 + 16 * ((size_t)j * nc + k));
        coeffs[np + k] -= r;
        coeffs[st.cons[k].lhs] += r * minus_c;
        for (const auto& term : st.cons[k].lc)
          coeffs[term.second] += r * Scalar::from_bytes_mod_order(responses + 32 * ((size_t)j * m + term.first));
      }
      for (uint32_t i = 0; i < K; ++i) {
        coeffs[i].to_bytes(scalars.data() + 32 * ((size_t)j * K + i));
        pidx[(size_t)j * K + i] = i < np ? table_index(st, i, j, N) : com_base + j * nc + (i - np);
      }
    }
  });
  off[N] = N * K;
  int rc = (ctx && st.ns && N >= 32) ? zkp_ctx_prepare_fixed_points(ctx, st.ns, common) : 0;
  if (rc) return rc;
  rc = be_msm_many(ctx, N, off.data(), scalars.data(), pidx.data(), tbl.data(), (uint32_t)(tbl.size() / 32), ZKP_VARTIME,
                   out.data(), status.data());
  if (rc) return rc;
  static const uint8_t zero[32] = {0};
  for (uint32_t j = 0; j < N; ++j)                                     // verifier.rs:162-172
    if (!results[j]) results[j] = (status[j] || std::memcmp(out.data() + 32 * (size_t)j, zero, 32) != 0) ? 1 : 0;
  return ZKP_TB_OK;
}

// ---- batch verification --------------------------------------------------------------------------------------
int zkp_batch_verify_build(const zkp_statement* stp, uint32_t N, uint32_t n_transcripts, uint8_t* ts, const uint8_t* inst,
                           const uint8_t* common, const uint8_t* commitments, const uint8_t* responses,
                           const uint8_t* weights16, int n_threads, uint8_t* msm_scalars, uint8_t* msm_points) {
  if (!stp || !msm_scalars || !msm_points) return ZKP_TB_BAD_STATEMENT;
  if (n_transcripts != N) return ZKP_TB_BATCH_SIZE_MISMATCH;           // batch_verifier.rs:72-74
  const zkp_statement& st = *stp;
  const uint32_t m = (uint32_t)st.secrets.size(), nc = (uint32_t)st.cons.size(), ni = st.ni, ns = st.ns;
  const size_t rows = (size_t)ni + nc;
  if (N == 0) { std::memset(msm_scalars, 0, 32 * (size_t)ns); if (ns) std::memcpy(msm_points, common, 32 * (size_t)ns); return ZKP_TB_OK; }
  if (flag_noncanonical(N, m, responses, nullptr)) return ZKP_TB_VERIFICATION_FAILURE;   // proofs.rs:27-32 through serde
  std::vector<uint8_t> failed(N, 0);
  build_verifiers(st, N, ts, inst, common, n_threads, failed.data());  // :75-77, :92-94, :105-107, :125-128
  for (uint8_t f : failed) if (f) return ZKP_TB_VERIFICATION_FAILURE;
  std::vector<uint8_t> own_w;
  if (!weights16) { own_w.resize(16 * (size_t)N * nc); if (!os_random(own_w.data(), own_w.size())) return ZKP_TB_NO_ENTROPY; weights16 = own_w.data(); }
  uint8_t* inst_coeffs = msm_scalars + 32 * (size_t)ns;                // Matrix(rows, N), entries[cols * r + c] (util.rs:24)
  std::atomic<int> any_fail{0};
  // per-thread partial sums of the static coefficients, reduced afterwards (:187, :198 sum over the whole batch)
  unsigned n_workers = n_threads > 0 ? (unsigned)n_threads : std::thread::hardware_concurrency();
  if (n_workers == 0) n_workers = 1;
  std::vector<std::vector<Scalar>> static_parts;
  std::vector<Scalar> static_total(ns);
  std::atomic<unsigned> slot{0};
  static_parts.resize(std::max(n_workers, 128u) + 1, std::vector<Scalar>(ns));
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    std::vector<Scalar>& sp = static_parts[slot.fetch_add(1) % static_parts.size()];
    std::vector<Scalar> col(rows);
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
      for (uint32_t k = 0; k < nc; ++k)                                // :152-160
        if (!t.validate_and_append_blinding_commitment(st.points[st.cons[k].lhs].name.c_str(), commitments + 32 * ((size_t)j * nc + k))) any_fail = 1;
      uint8_t c[32];
      t.get_challenge("chal", c);                                      // :163-167
      t.to_bytes(ts + TB * (size_t)j);
      const Scalar minus_c = -Scalar::from_bytes_mod_order(c);
      std::fill(col.begin(), col.end(), Scalar::zero());
      for (uint32_t k = 0; k < nc; ++k) {                              // :176-206 (loop order swapped: proof-major)
        const Scalar r = Scalar::from_u128_le(weights16 + 16 * ((size_t)k * N + j));
        col[ni + k] -= r;                                              // :183
        const auto& lhs = st.points[st.cons[k].lhs];
        if (lhs.common) sp[lhs.rank] += r * minus_c; else col[lhs.rank] += r * minus_c;     // :185-192
        for (const auto& term : st.cons[k].lc) {                       // :194-204
          const Scalar rr = r * Scalar::from_bytes_mod_order(responses + 32 * ((size_t)j * m + term.first));
          const auto& pt = st.points[term.second];
          if (pt.common) sp[pt.rank] += rr; else col[pt.rank] += rr;
        }
      }
      for (size_t r = 0; r < rows; ++r) col[r].to_bytes(inst_coeffs + 32 * (r * N + j));
    }
  });
  if (any_fail) return ZKP_TB_VERIFICATION_FAILURE;
  for (const auto& part : static_parts)
    for (uint32_t i = 0; i < ns; ++i) static_total[i] += part[i];
  for (uint32_t i = 0; i < ns; ++i) static_total[i].to_bytes(msm_scalars + 32 * (size_t)i);
  // points: static || instance rows || commitment rows (transposed to row = constraint, column = proof) :208-217
  if (ns) std::memcpy(msm_points, common, 32 * (size_t)ns);
  if (ni) std::memcpy(msm_points + 32 * (size_t)ns, inst, 32 * (size_t)ni * N);
  uint8_t* com_rows = msm_points + 32 * ((size_t)ns + (size_t)ni * N);
  for (uint32_t j = 0; j < N; ++j)
    for (uint32_t k = 0; k < nc; ++k) std::memcpy(com_rows + 32 * ((size_t)k * N + j), commitments + 32 * ((size_t)j * nc + k), 32);
  return ZKP_TB_OK;
}

// Same checks, with the coefficient build on the GPU (zkp_batch_check): the host keeps the transcripts (validation,
// commitments, challenges :152-167), the device does :173-228 -- scalar arithmetic mod l included.
int zkp_batch_verify_coeffs(zkp_ctx* ctx, const zkp_statement* stp, uint32_t N, uint32_t n_transcripts, uint8_t* ts, const uint8_t* inst,
                            const uint8_t* common, const uint8_t* commitments, const uint8_t* responses, const uint8_t* weights16,
                            int n_threads, uint8_t* coeffs) {
  if (!stp) return ZKP_TB_BAD_STATEMENT;
  if (n_transcripts != N) return ZKP_TB_BATCH_SIZE_MISMATCH;           // batch_verifier.rs:72-74
  const zkp_statement& st = *stp;
  const uint32_t m = (uint32_t)st.secrets.size(), nc = (uint32_t)st.cons.size(), ni = st.ni, ns = st.ns;
  if (on_host(ctx, (uint64_t)ns + ((uint64_t)ni + nc) * N)) {
    // tiny batch (or no GPU context): batch_verifier.rs:67-235 entirely on the host -- the operand list of :219-228 from
    // zkp_batch_verify_build, the MSM from the host backend
    const size_t total = (size_t)ns + ((size_t)ni + nc) * N;
    std::vector<uint8_t> sc(32 * (total ? total : 1)), pts(32 * (total ? total : 1));
    const int rcb = zkp_batch_verify_build(stp, N, n_transcripts, ts, inst, common, commitments, responses, weights16, n_threads, sc.data(), pts.data());
    if (rcb) return rcb;
    if (coeffs) std::memcpy(coeffs, sc.data(), 32 * total);
    uint8_t out[32];
    int status = 1;
    const int rcm = zkp::hostbk::msm_optional(total, sc.data(), pts.data(), out, &status);
    if (rcm) return rcm;
    static const uint8_t zero32[32] = {0};
    return (!status && std::memcmp(out, zero32, 32) == 0) ? ZKP_TB_OK : ZKP_TB_VERIFICATION_FAILURE;      // :230-234
  }
  if (ts && use_fused(ts, N)) {
    FusedView fv(st);
    int verdict = 1;
    if (!weights16 && !coeffs && nc) {
      // no weights from the caller: 40 bytes of getrandom() key a ChaCha20 stream that is expanded on the device (batch_verifier.rs:179's thread_rng())
      uint8_t seed[40];
      if (!os_entropy(seed, sizeof(seed))) return ZKP_TB_NO_ENTROPY;
      const int rc = zkp_fused_batch_verify_many_seeded(ctx, &fv.fs, 1, N, ts, inst, common, commitments, responses, seed, &verdict);
      if (rc) return rc;
      return verdict ? ZKP_TB_VERIFICATION_FAILURE : ZKP_TB_OK;
    }
    std::vector<uint8_t> own_w;
    if (!weights16) { own_w.resize(16 * (size_t)N * nc); if (!os_random(own_w.data(), own_w.size())) return ZKP_TB_NO_ENTROPY; weights16 = own_w.data(); }
    const int rc = zkp_fused_batch_verify(ctx, &fv.fs, N, ts, inst, common, commitments, responses, weights16, &verdict, coeffs);
    if (rc) return rc;
    return verdict ? ZKP_TB_VERIFICATION_FAILURE : ZKP_TB_OK;
  }
  std::vector<uint8_t> minus_c(32 * (size_t)N);
  if (N) {
    if (flag_noncanonical(N, m, responses, nullptr)) return ZKP_TB_VERIFICATION_FAILURE;   // proofs.rs:27-32 through serde
    std::vector<uint8_t> failed(N, 0);
    build_verifiers(st, N, ts, inst, common, n_threads, failed.data());  // :75-77, :92-94, :105-107, :125-128
    for (uint8_t f : failed) if (f) return ZKP_TB_VERIFICATION_FAILURE;
    std::atomic<int> any_fail{0};
    parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
      for (uint32_t j = lo; j < hi; ++j) {
        Transcript t = Transcript::from_bytes(ts + TB * (size_t)j);
        for (uint32_t k = 0; k < nc; ++k)                                // :152-160
          if (!t.validate_and_append_blinding_commitment(st.points[st.cons[k].lhs].name.c_str(), commitments + 32 * ((size_t)j * nc + k))) any_fail = 1;
        uint8_t c[32];
        t.get_challenge("chal", c);                                      // :163-167
        t.to_bytes(ts + TB * (size_t)j);
        (-Scalar::from_bytes_mod_order(c)).to_bytes(minus_c.data() + 32 * (size_t)j);
      }
    });
    if (any_fail) return ZKP_TB_VERIFICATION_FAILURE;
  }
  std::vector<uint8_t> own_w;
  if (!weights16) { own_w.resize(16 * (size_t)N * nc); if (!os_random(own_w.data(), own_w.size())) return ZKP_TB_NO_ENTROPY; weights16 = own_w.data(); }
  // statement incidence in point-id form (static ids first, then instance ids)
  auto pid = [&](uint32_t v) { return st.points[v].common ? st.points[v].rank : ns + st.points[v].rank; };
  std::vector<uint32_t> lhs(nc), off(nc + 1, 0), csc, cpt;
  for (uint32_t k = 0; k < nc; ++k) {
    lhs[k] = pid(st.cons[k].lhs);
    for (const auto& term : st.cons[k].lc) { csc.push_back(term.first); cpt.push_back(pid(term.second)); }
    off[k + 1] = (uint32_t)csc.size();
  }
  zkp_batch_statement bs{m, ns, ni, nc, lhs.data(), off.data(), csc.data(), cpt.data()};
  uint8_t out[32];
  int status = 1;
  int rc = zkp_batch_check(ctx, &bs, N, minus_c.data(), responses, weights16, common, inst, commitments, out, &status, coeffs);
  if (rc) return rc;
  if (status) return ZKP_TB_VERIFICATION_FAILURE;                      // some point failed to decompress -> None
  static const uint8_t zero[32] = {0};
  return std::memcmp(out, zero, 32) == 0 ? ZKP_TB_OK : ZKP_TB_VERIFICATION_FAILURE;   // :230-234
}

// K batch verifications of a ragged batch on the device (K = 1: zkp_batch_verify); weights16 == NULL: drawn there from 40 bytes of getrandom()
static int batch_verify_ragged(zkp_ctx* ctx, const zkp_statement& st, uint32_t K, uint32_t N_each, uint8_t* ts, const uint8_t* inst, const uint8_t* common,
                               const uint8_t* commitments, const uint8_t* responses, const uint8_t* weights16, int* verdicts) {
  uint8_t seed[40];
  if (!weights16 && !st.cons.empty() && !os_entropy(seed, sizeof(seed))) return ZKP_TB_NO_ENTROPY;
  FusedView fv(st);
  const int rc = zkp_fused_batch_verify_many_ragged(ctx, &fv.fs, K, N_each, ts, inst, common, commitments, responses, weights16, weights16 ? nullptr : seed, verdicts);
  if (rc) return rc;
  for (uint32_t b = 0; b < K; ++b) verdicts[b] = verdicts[b] ? ZKP_TB_VERIFICATION_FAILURE : ZKP_TB_OK;
  return ZKP_TB_OK;
}

int zkp_batch_verify(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* ts, const uint8_t* inst,
                     const uint8_t* common, const uint8_t* commitments, const uint8_t* responses, const uint8_t* weights16,
                     int n_threads) {
  if (st && ctx && ts && n_transcripts == N && !on_host(ctx, (uint64_t)st->ns + ((uint64_t)st->ni + st->cons.size()) * N) && use_ragged(ts, N)) {
    int verdict = ZKP_TB_VERIFICATION_FAILURE;
    const int rc = batch_verify_ragged(ctx, *st, 1, N, ts, inst, common, commitments, responses, weights16, &verdict);
    return rc ? rc : verdict;
  }
  return zkp_batch_verify_coeffs(ctx, st, N, n_transcripts, ts, inst, common, commitments, responses, weights16, n_threads, nullptr);
}

int zkp_batch_verify_many(zkp_ctx* ctx, const zkp_statement* stp, uint32_t K, uint32_t N_each, uint32_t n_transcripts, uint8_t* ts, const uint8_t* inst,
                          const uint8_t* common, const uint8_t* commitments, const uint8_t* responses, const uint8_t* weights16, int n_threads,
                          int* verdicts) {
  if (!stp || !verdicts || K == 0 || N_each == 0 || (uint64_t)K * N_each > 0x7fffffffull) return ZKP_TB_BAD_STATEMENT;
  const uint32_t N = K * N_each;
  if (n_transcripts != N) return ZKP_TB_BATCH_SIZE_MISMATCH;           // batch_verifier.rs:72-74
  if (!ts) return ZKP_TB_BAD_STATEMENT;
  const zkp_statement& st = *stp;
  const uint32_t m = (uint32_t)st.secrets.size(), nc = (uint32_t)st.cons.size(), ni = st.ni;
  if (ctx && use_ragged(ts, N)) return batch_verify_ragged(ctx, st, K, N_each, ts, inst, common, commitments, responses, weights16, verdicts);
  std::vector<uint8_t> own_w;
  if (!weights16 && ctx && nc && use_fused(ts, N)) {                   // weights drawn on the device from 40 bytes of getrandom() (see zkp_batch_verify)
    uint8_t seed[40];
    if (!os_entropy(seed, sizeof(seed))) return ZKP_TB_NO_ENTROPY;
    FusedView fv(st);
    const int rc = zkp_fused_batch_verify_many_seeded(ctx, &fv.fs, K, N_each, ts, inst, common, commitments, responses, seed, verdicts);
    if (rc) return rc;
    for (uint32_t b = 0; b < K; ++b) verdicts[b] = verdicts[b] ? ZKP_TB_VERIFICATION_FAILURE : ZKP_TB_OK;
    return ZKP_TB_OK;
  }
  if (!weights16) { own_w.resize(16 * (size_t)N * nc); if (!os_random(own_w.data(), own_w.size())) return ZKP_TB_NO_ENTROPY; weights16 = own_w.data(); }
  if (ctx && use_fused(ts, N)) {
    FusedView fv(st);
    const int rc = zkp_fused_batch_verify_many(ctx, &fv.fs, K, N_each, ts, inst, common, commitments, responses, weights16, verdicts, nullptr);
    if (rc) return rc;
    for (uint32_t b = 0; b < K; ++b) verdicts[b] = verdicts[b] ? ZKP_TB_VERIFICATION_FAILURE : ZKP_TB_OK;
    return ZKP_TB_OK;
  }
  // one by one: batch b's columns of the instance rows and of the weights, gathered into arrays of its own
  std::vector<uint8_t> inst_b(32 * (size_t)ni * N_each), w_b(16 * (size_t)nc * N_each);
  for (uint32_t b = 0; b < K; ++b) {
    const size_t j0 = (size_t)b * N_each;
    for (uint32_t r = 0; r < ni; ++r) std::memcpy(inst_b.data() + 32 * (size_t)r * N_each, inst + 32 * ((size_t)r * N + j0), 32 * (size_t)N_each);
    for (uint32_t k = 0; k < nc; ++k) std::memcpy(w_b.data() + 16 * (size_t)k * N_each, weights16 + 16 * ((size_t)k * N + j0), 16 * (size_t)N_each);
    const int rc = zkp_batch_verify(ctx, stp, N_each, N_each, ts + TB * j0, inst_b.data(), common, commitments + 32 * j0 * nc, responses + 32 * j0 * m,
                                    w_b.data(), n_threads);
    if (rc < 0 || rc == ZKP_TB_BATCH_SIZE_MISMATCH) return rc;
    verdicts[b] = rc;
  }
  return ZKP_TB_OK;
}

// ---- hash to the group (RFC 9496 section 4.3.4) ----------------------------------------------------------------------
int zkp_from_uniform_bytes_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* in, int n_threads, uint8_t* out) {
  if (n == 0) return ZKP_TB_OK;
  if (!in || !out) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_from_uniform_bytes(ctx, n, in, out);
  if (n > 0xffffffffull) return ZKP_TB_BAD_STATEMENT;
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) { zkp::hostbk::from_uniform_bytes(hi - lo, in + 64 * (size_t)lo, out + 32 * (size_t)lo); });
  return ZKP_TB_OK;
}

// RistrettoPoint::hash_from_bytes::<Sha512> of n messages (CSR: message i = msgs[offsets[i], offsets[i + 1])).  The offsets are checked
// here, whichever backend runs: non-decreasing, or ZKP_TB_BAD_STATEMENT.
int zkp_hash_from_bytes_sha512_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* msgs, const uint64_t* offsets, int n_threads, uint8_t* out) {
  if (n == 0) return ZKP_TB_OK;
  if (!msgs || !offsets || !out) return ZKP_TB_BAD_STATEMENT;
  for (uint64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_hash_from_bytes_sha512(ctx, n, msgs, offsets, out);
  if (n > 0xffffffffull) return ZKP_TB_BAD_STATEMENT;
  // a thread's slice [lo, hi) is a CSR batch of its own (offsets + lo), whose buffer msgs[0, offsets[hi]) holds all of its messages
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) { zkp::hostbk::hash_from_bytes_sha512(hi - lo, msgs, offsets + lo, out + 32 * (size_t)lo); });
  return ZKP_TB_OK;
}

// ---- scalars mod l, batched (zkp_mi355x.h (6)): host threads through sc25519.h / sha512.h compiled for the host, or the device ------
int zkp_scalar_invert_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* in, int n_threads, uint8_t* out) {
  if (n == 0) return ZKP_TB_OK;
  if (!in || !out) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_sc_invert(ctx, n, in, out);
  if (n > 0xffffffffull) return ZKP_TB_BAD_STATEMENT;
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) { zkp::hostbk::sc_invert_n(hi - lo, in + 32 * (size_t)lo, out + 32 * (size_t)lo); });
  return ZKP_TB_OK;
}

int zkp_scalar_from_wide_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* in, int n_threads, uint8_t* out) {
  if (n == 0) return ZKP_TB_OK;
  if (!in || !out) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_sc_from_wide(ctx, n, in, out);
  if (n > 0xffffffffull) return ZKP_TB_BAD_STATEMENT;
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) { zkp::hostbk::sc_from_wide_n(hi - lo, in + 64 * (size_t)lo, out + 32 * (size_t)lo); });
  return ZKP_TB_OK;
}

int zkp_scalar_muladd_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, const uint8_t* c, uint32_t c_stride,
                            int n_threads, uint8_t* out) {
  if (a_stride > 1 || b_stride > 1 || c_stride > 1) return ZKP_TB_BAD_STATEMENT;
  if (n == 0) return ZKP_TB_OK;
  if (!a || !b || !out) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_sc_muladd(ctx, n, a, a_stride, b, b_stride, c, c_stride, out);
  if (n > 0xffffffffull) return ZKP_TB_BAD_STATEMENT;
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) {
    zkp::hostbk::sc_muladd_n(hi - lo, a + 32 * (size_t)lo * a_stride, a_stride, b + 32 * (size_t)lo * b_stride, b_stride, c ? c + 32 * (size_t)lo * c_stride : nullptr,
                             c_stride, out + 32 * (size_t)lo);
  });
  return ZKP_TB_OK;
}

// ---- segmented scalar sums, products and dot products (zkp_mi355x.h (12)) --------------------------------------------------------------------
// The smallest number of terms from which a call with a context runs on the device, per op.  The rule (zkp_toolbox.h): the smallest measured term
// count from which the synchronous device call is ahead of the host backend at 16 threads beyond the min-max spread of the rounds at every
// measured segment mix; none up to 2^22 terms: never.  profiles/scalar_reduce_bench.txt, the sweep (2^12 .. 2^22 terms in steps of 4, segments of 2, 32,
// 1,024 terms and one segment; device | host, ms, medians):
//   SUM      ahead at 23 of 24 cells (2^20 in one segment 0.682 | 1.379), but at 2^22 terms in segments of 2 -- 2^21 outputs to bring back -- the two are
//            level, 10.99 | 10.94 with spreads that cover each other: no size from which every mix is ahead, so NEVER
//   PRODUCT  ahead at every cell from the smallest measured size on (2^12: 0.086 to 0.098 | 0.439 to 0.457; 2^22 in segments of 2: 11.16 | 23.29): 4,096
//   DOT      ahead at every cell but one round of 2^14 x 32 (0.105 / 0.110 / 7.758 | 0.505), and at every cell from 2^16 on (0.163 to 0.252 | 0.625 to 0.669): 65,536
static std::atomic<uint64_t> g_scalar_reduce_min_terms[3] = {{UINT64_MAX}, {4096}, {65536}};
void zkp_toolbox_set_scalar_reduce_min_terms(int op, uint64_t n) {
  if (op >= 0 && op < 3) g_scalar_reduce_min_terms[op] = n;
}
static_assert(sizeof(size_t) == sizeof(uint64_t), "the getter returns the 64-bit threshold as a size_t");
size_t zkp_toolbox_get_scalar_reduce_min_terms(int op) { return op >= 0 && op < 3 ? (size_t)g_scalar_reduce_min_terms[op].load() : SIZE_MAX; }

// Every check is made by both routes before anything is written (hostbk::sc_reduce_n, zkp_sc_reduce), so they refuse the same calls.
int zkp_scalar_reduce_batch(zkp_ctx* ctx, int op, uint32_t n_out, const uint32_t* off, const uint8_t* a, uint32_t n_a, const uint32_t* aidx, const uint8_t* b,
                            uint32_t n_b, const uint32_t* bidx, int n_threads, uint8_t* out) {
  if (op != ZKP_SC_SUM && op != ZKP_SC_PRODUCT && op != ZKP_SC_DOT) return ZKP_TB_BAD_STATEMENT;
  if (n_out == 0) return ZKP_TB_OK;
  if (!off || !out) return ZKP_TB_BAD_STATEMENT;
  const uint64_t min_terms = g_scalar_reduce_min_terms[op].load();
  const bool host = !ctx || min_terms == UINT64_MAX || off[n_out] < min_terms;
  const int rc = host ? zkp::hostbk::sc_reduce_n(op, n_out, off, a, n_a, aidx, b, n_b, bidx, n_threads, out)
                      : zkp_sc_reduce(ctx, op, n_out, off, a, n_a, aidx, b, n_b, bidx, out);
  return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
}

// Scalar::hash_from_bytes::<Sha512> of n messages (CSR, checked here as zkp_hash_from_bytes_sha512_batch checks it)
int zkp_scalar_hash_from_bytes_sha512_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* msgs, const uint64_t* offsets, int n_threads, uint8_t* out) {
  if (n == 0) return ZKP_TB_OK;
  if (!msgs || !offsets || !out) return ZKP_TB_BAD_STATEMENT;
  for (uint64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_sc_hash_from_bytes_sha512(ctx, n, msgs, offsets, out);
  if (n > 0xffffffffull) return ZKP_TB_BAD_STATEMENT;
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) { zkp::hostbk::sc_hash_sha512_n(hi - lo, msgs, offsets + lo, out + 32 * (size_t)lo); });
  return ZKP_TB_OK;
}

// ---- Scalar * basepoint, Scalar * point, multiscalar products (zkp_mi355x.h (8), (1)): routed as the scalar calls above ----------------
int zkp_basepoint_mul_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* scalars, int n_threads, uint8_t* out) {
  if (n == 0) return ZKP_TB_OK;
  if (!scalars || !out || n > 0x7fffffffull) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_mul_base(ctx, n, scalars, out);
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) { zkp::hostbk::mul_base_n(hi - lo, scalars + 32 * (size_t)lo, out + 32 * (size_t)lo); });
  return ZKP_TB_OK;
}

int zkp_point_mul_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* scalars, uint32_t s_stride, const uint8_t* points, uint32_t p_stride, int flags, int n_threads,
                        uint8_t* out, uint8_t* status) {
  if (s_stride > 1 || p_stride > 1 || (flags != ZKP_CT && flags != ZKP_VARTIME)) return ZKP_TB_BAD_STATEMENT;
  if (n == 0) return ZKP_TB_OK;
  if (!scalars || !points || !out || !status || n > 0x7fffffffull) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_mul_points(ctx, n, scalars, s_stride, points, p_stride, flags, out, status);
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) {
    zkp::hostbk::mul_points_n(hi - lo, scalars + 32 * (size_t)lo * s_stride, s_stride, points + 32 * (size_t)lo * p_stride, p_stride, flags, out + 32 * (size_t)lo,
                              status + lo);
  });
  return ZKP_TB_OK;
}

// zkp_msm_many / hostbk::msm_many behind the routing (n = the number of terms) and nothing more.  The device route leaves the CSR checks to
// zkp_msm_many, which makes them before it writes anything (its ZKP_ERR_ARG is ZKP_TB_BAD_STATEMENT here); the host route makes them here,
// then cuts the MSMs into one contiguous range per thread: a range is a CSR job of its own once its offsets are rebased.
int zkp_multiscalar_mul_batch(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points,
                              uint32_t n_points, int flags, int n_threads, uint8_t* out, uint8_t* status) {
  if (flags != ZKP_CT && flags != ZKP_VARTIME) return ZKP_TB_BAD_STATEMENT;
  if (n_msm == 0) return ZKP_TB_OK;
  if (!off || !out || !status || off[0] != 0) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, off[n_msm])) {
    const int rc = zkp_msm_many(ctx, n_msm, off, scalars, pidx, points, n_points, flags, out, status);
    return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
  }
  for (uint32_t i = 0; i < n_msm; ++i)
    if (off[i + 1] < off[i]) return ZKP_TB_BAD_STATEMENT;
  const uint32_t n_terms = off[n_msm];
  if (n_terms && (!scalars || !pidx || !points || n_points == 0)) return ZKP_TB_BAD_STATEMENT;
  for (uint32_t t = 0; t < n_terms; ++t)
    if (pidx[t] >= n_points) return ZKP_TB_BAD_STATEMENT;
  std::atomic<int> rc{ZKP_OK};
  parallel_for(n_msm, n_threads, [&](uint32_t lo, uint32_t hi) {
    std::vector<uint32_t> o(hi - lo + 1);
    for (uint32_t i = lo; i <= hi; ++i) o[i - lo] = off[i] - off[lo];
    const int r = zkp::hostbk::msm_many(hi - lo, o.data(), scalars ? scalars + 32 * (size_t)off[lo] : nullptr, pidx ? pidx + off[lo] : nullptr, points, n_points, flags,
                                        out + 32 * (size_t)lo, status + lo);
    if (r) rc = r;
  });
  return rc.load() ? ZKP_TB_BAD_STATEMENT : ZKP_TB_OK;
}

// ---- multiscalar sums with long segments (zkp_mi355x.h (11)) ------------------------------------------------------------------------------
// The shortest longest-segment from which a device job folds its term axis (zkp_msm_segments) instead of summing each MSM in one lane
// (zkp_msm_many).  profiles/msm_segments_bench.txt (stream medians, fold against zkp_msm_many): of the short lengths none has the fold ahead beyond the
// spread at both output counts -- 4,096 x 2: 1.086 against 0.747; 4,096 x 11: 1.176 against 0.834; 4,096 x 32: 1.920 against 1.562; 4,096 x 128: 6.521 against 6.557; 65,536 x 2: 1.948 against 1.501; 65,536 x 11: 8.745 against 8.279; 65,536 x 32: 23.45 against 23.42; 65,536 x 128: 85.10 against 84.62 -- and 1,024 is the shortest measured length that has (1.290 against 4.194 ms at 64 segments, 12.64 against 15.96 ms at 1,024).
static std::atomic<uint32_t> g_msm_fold_min_segment{1024};
void zkp_toolbox_set_msm_fold_min_segment(uint32_t n) { g_msm_fold_min_segment = n; }
uint32_t zkp_toolbox_get_msm_fold_min_segment(void) { return g_msm_fold_min_segment.load(); }

// Every check is made here, before anything is written, so that the three routes refuse the same calls.
int zkp_multiscalar_sum_batch(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points,
                              uint32_t n_points, int flags, int n_threads, uint8_t* out, uint8_t* status) {
  if (flags != ZKP_CT && flags != ZKP_VARTIME) return ZKP_TB_BAD_STATEMENT;
  if (n_msm == 0) return ZKP_TB_OK;
  if (!off || !out || !status || off[0] != 0) return ZKP_TB_BAD_STATEMENT;
  uint32_t longest = 0;
  for (uint32_t i = 0; i < n_msm; ++i) {
    if (off[i + 1] < off[i]) return ZKP_TB_BAD_STATEMENT;
    longest = std::max(longest, off[i + 1] - off[i]);
  }
  const uint32_t n_terms = off[n_msm];
  if (n_terms && (!scalars || !points || n_points == 0)) return ZKP_TB_BAD_STATEMENT;
  if (!pidx && n_points != n_terms) return ZKP_TB_BAD_STATEMENT;
  if (pidx)
    for (uint32_t t = 0; t < n_terms; ++t)
      if (pidx[t] >= n_points) return ZKP_TB_BAD_STATEMENT;
  int rc;
  if (on_host(ctx, n_terms)) {
    rc = zkp::hostbk::msm_segments_n(n_msm, off, scalars, pidx, points, n_points, flags, n_threads, out, status);
  } else if (longest < g_msm_fold_min_segment.load()) {
    std::vector<uint32_t> iota;
    if (!pidx) {
      iota.resize(n_terms);
      for (uint32_t t = 0; t < n_terms; ++t) iota[t] = t;
    }
    rc = zkp_msm_many(ctx, n_msm, off, scalars, pidx ? pidx : iota.data(), points, n_points, flags, out, status);
  } else {
    rc = zkp_msm_segments(ctx, n_msm, off, scalars, pidx, points, n_points, flags, out, status);
  }
  return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
}

// ---- many variable-time multiscalar sums with long segments (zkp_mi355x.h (14)) ------------------------------------------------------------
// The shortest longest-segment from which a device job takes the bucket method (zkp_msm_optional_many) instead of the route
// zkp_multiscalar_sum_batch gives it.  The toolbox's standing rule: the smallest measured segment length from which the new call is ahead beyond the
// spread of the rounds at every measured segment count; 0xffffffff ("never") if there is none.  profiles/msm_optional_many_bench.txt:
// (stream medians, ms, the call against zkp_msm_segments | zkp_msm_many, all ahead beyond the spread): 256 terms at 4 segments 0.377 against 0.974 | 1.615, at 16 0.394 against 1.024 | 1.659, at 4,096 9.009 against 12.35 | 12.74; 1,024 terms at 4 segments 0.375 against 1.025 | 3.958, at 16 0.425 against 1.108 | 4.395, at 1,024 5.301 against 12.39 | 16.62.  256 is the shortest measured length; 193 to 255 terms are not measured.
static std::atomic<uint32_t> g_msm_bucket_min_segment{256};
void zkp_toolbox_set_msm_bucket_min_segment(uint32_t n) { g_msm_bucket_min_segment = n; }
uint32_t zkp_toolbox_get_msm_bucket_min_segment(void) { return g_msm_bucket_min_segment.load(); }

// zkp_multiscalar_sum_batch's checks, made before anything is written; variable time on every route.
int zkp_multiscalar_optional_batch(zkp_ctx* ctx, uint32_t n_seg, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points,
                                   uint32_t n_points, int n_threads, uint8_t* out, uint8_t* status) {
  if (n_seg == 0) return ZKP_TB_OK;
  if (!off || !out || !status || off[0] != 0) return ZKP_TB_BAD_STATEMENT;
  uint32_t longest = 0;
  for (uint32_t i = 0; i < n_seg; ++i) {
    if (off[i + 1] < off[i]) return ZKP_TB_BAD_STATEMENT;
    longest = std::max(longest, off[i + 1] - off[i]);
  }
  const uint32_t n_terms = off[n_seg];
  if (n_terms && (!scalars || !points || n_points == 0)) return ZKP_TB_BAD_STATEMENT;
  if (!pidx && n_points != n_terms) return ZKP_TB_BAD_STATEMENT;
  if (pidx)
    for (uint32_t t = 0; t < n_terms; ++t)
      if (pidx[t] >= n_points) return ZKP_TB_BAD_STATEMENT;
  if (on_host(ctx, n_terms) || longest < g_msm_bucket_min_segment.load())
    return zkp_multiscalar_sum_batch(ctx, n_seg, off, scalars, pidx, points, n_points, ZKP_VARTIME, n_threads, out, status);
  const int rc = zkp_msm_optional_many(ctx, n_seg, off, scalars, pidx, points, n_points, out, status);
  return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
}

// ---- RistrettoPoint sums (zkp_mi355x.h (9)): pairs and CSR segments behind the same routing ------------------------------------------------
int zkp_point_add_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, int op, int n_threads,
                        uint8_t* out, uint8_t* status) {
  if (a_stride > 1 || b_stride > 1 || (op != ZKP_PT_ADD && op != ZKP_PT_SUB)) return ZKP_TB_BAD_STATEMENT;
  if (n == 0) return ZKP_TB_OK;
  if (!a || !b || !out || !status || n > 0x7fffffffull) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n)) return zkp_add_points(ctx, n, a, a_stride, b, b_stride, op, out, status);
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) {
    zkp::hostbk::add_points_n(hi - lo, a + 32 * (size_t)lo * a_stride, a_stride, b + 32 * (size_t)lo * b_stride, b_stride, op, out + 32 * (size_t)lo, status + lo);
  });
  return ZKP_TB_OK;
}

// The host route cuts the work by TERMS.  With t threads and T terms a thread's share is ceil(T / t): a sum longer than that (and than 64 terms,
// below which a cut costs more than it saves) is split over all threads into partial sums that one thread then adds; the other sums go to the
// threads in contiguous ranges of about equal numbers of terms.
int zkp_point_sum_batch(zkp_ctx* ctx, uint32_t n_sums, const uint32_t* off, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points, uint32_t n_points,
                        int n_threads, uint8_t* out, uint8_t* status) {
  if (n_sums == 0) return ZKP_TB_OK;
  if (!off || !out || !status || off[0] != 0) return ZKP_TB_BAD_STATEMENT;
  for (uint32_t i = 0; i < n_sums; ++i)
    if (off[i + 1] < off[i]) return ZKP_TB_BAD_STATEMENT;
  const uint32_t n_terms = off[n_sums];
  if (n_terms && (!points || n_points == 0)) return ZKP_TB_BAD_STATEMENT;
  if (!pidx && n_points != n_terms) return ZKP_TB_BAD_STATEMENT;
  if (pidx)
    for (uint32_t t = 0; t < n_terms; ++t)
      if (pidx[t] >= n_points) return ZKP_TB_BAD_STATEMENT;
  if (!on_host(ctx, n_terms)) {
    const int rc = zkp_sum_points(ctx, n_sums, off, pidx, neg, points, n_points, out, status);
    return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
  }
  unsigned t = n_threads > 0 ? (unsigned)n_threads : std::thread::hardware_concurrency();
  t = std::max(1u, std::min(t, 128u));
  const uint32_t share = (uint32_t)(((uint64_t)n_terms + t - 1) / t);
  const uint32_t long_len = t > 1 ? std::max(share, 64u) : 0xffffffffu;
  std::vector<uint8_t> partials;
  for (uint32_t s = 0; s < n_sums && t > 1; ++s) {
    const uint32_t len = off[s + 1] - off[s];
    if (len <= long_len) continue;
    const uint32_t piece = (len + t - 1) / t, n_pieces = (len + piece - 1) / piece;
    partials.resize(zkp::hostbk::SUM_PARTIAL_BYTES * (size_t)n_pieces);
    Pool::instance().run(n_pieces, [&](unsigned k) {
      const uint32_t lo = off[s] + k * piece, hi = std::min(off[s + 1], lo + piece);
      zkp::hostbk::sum_points_partial(lo, hi, pidx, neg, points, partials.data() + zkp::hostbk::SUM_PARTIAL_BYTES * (size_t)k);
    });
    zkp::hostbk::sum_points_finish(n_pieces, partials.data(), out + 32 * (size_t)s, status + s);
  }
  const unsigned ranges = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(t, n_sums), ((uint64_t)n_terms + 63) / 64));
  std::vector<uint32_t> cut(ranges + 1, n_sums);
  cut[0] = 0;
  for (unsigned k = 1; k < ranges; ++k)          // the first sum that starts at or after term k T / ranges
    cut[k] = std::max(cut[k - 1], (uint32_t)(std::lower_bound(off, off + n_sums, (uint32_t)((uint64_t)k * n_terms / ranges)) - off));
  Pool::instance().run(ranges, [&](unsigned k) {
    const uint32_t lo = cut[k], hi = cut[k + 1];
    if (lo < hi) zkp::hostbk::sum_points_n(hi - lo, off + lo, pidx, neg, points, out + 32 * (size_t)lo, status + lo, long_len);
  });
  return ZKP_TB_OK;
}

// ---- segmented prefix sums and products of scalars, running sums of points (zkp_mi355x.h (13)) ---------------------------------------------
// The smallest number of terms from which a call with a context runs on the device (scalars: per op), by the rule of
// g_scalar_reduce_min_terms, read off the sweep of profiles/scan_bench.txt (scalars 2^12 .. 2^22 terms, points 2^6 .. 2^18, in steps of 4, in
// segments of 2, 32, 1,024 terms and one segment; device | host, ms, medians):
//   SUM      ahead at every cell up to 2^18 terms (2^12: 0.088 to 0.094 | 0.790 to 0.834; 2^18: 0.664 to 0.708 | 1.229 to 1.377), level at 2^20
//            (4.505 to 4.752 | 4.562 to 5.323, three of four mixes within the spread) and behind at 2^22 in segments of 2 and of 1,024
//            (17.25 | 16.12; 16.26 | 15.44): 32 bytes back per term.  No size from which every mix is ahead: NEVER
//   PRODUCT  ahead at every cell up to 2^18 (2^12: 0.116 to 0.122 | 0.859 to 0.985; 2^18: 0.725 to 0.797 | 1.882 to 2.910); at 2^20 the device call took
//            6 to 34 ms from round to round (medians 16.05 to 20.73 | 9.284 to 13.92: behind or within the spread); ahead at every mix at 2^22
//            (16.86 to 18.29 | 27.48 to 45.17): 4,194,304.  The 2^20 cell is unexplained -- the identical call reads 2.32 ms in the shapes part of the
//            same file -- and no property of the call; the default only keeps work on the host (zkp_toolbox.h)
//   points   ahead at every cell from the smallest measured size on (2^6: 0.365 to 0.369 | 0.400 to 0.405; 2^12: 0.632 to 0.651 | 2.538 to 4.287;
//            2^18: 1.780 to 1.969 | 118.2 to 220.9): 64
static std::atomic<uint64_t> g_scalar_scan_min_terms[2] = {{UINT64_MAX}, {4194304}};
static std::atomic<uint64_t> g_point_scan_min_terms{64};
void zkp_toolbox_set_scalar_scan_min_terms(int op, uint64_t n) {
  if (op >= 0 && op < 2) g_scalar_scan_min_terms[op] = n;
}
size_t zkp_toolbox_get_scalar_scan_min_terms(int op) { return op >= 0 && op < 2 ? (size_t)g_scalar_scan_min_terms[op].load() : SIZE_MAX; }
void zkp_toolbox_set_point_scan_min_terms(uint64_t n) { g_point_scan_min_terms = n; }
size_t zkp_toolbox_get_point_scan_min_terms(void) { return (size_t)g_point_scan_min_terms.load(); }

// Every check is made by both routes before anything is written (hostbk::sc_scan_n / point_scan_n, zkp_sc_scan / zkp_scan_points), so they refuse
// the same calls.
int zkp_scalar_scan_batch(zkp_ctx* ctx, int op, int mode, uint32_t n_seg, const uint32_t* off, const uint8_t* a, uint32_t n_a, const uint32_t* aidx, int n_threads,
                          uint8_t* out) {
  if (op != ZKP_SC_SUM && op != ZKP_SC_PRODUCT) return ZKP_TB_BAD_STATEMENT;
  if (mode != ZKP_SCAN_INCLUSIVE && mode != ZKP_SCAN_EXCLUSIVE) return ZKP_TB_BAD_STATEMENT;
  if (n_seg == 0) return ZKP_TB_OK;
  if (!off) return ZKP_TB_BAD_STATEMENT;
  const uint64_t min_terms = g_scalar_scan_min_terms[op].load();
  const bool host = !ctx || min_terms == UINT64_MAX || off[n_seg] < min_terms;
  const int rc = host ? zkp::hostbk::sc_scan_n(op, mode, n_seg, off, a, n_a, aidx, n_threads, out) : zkp_sc_scan(ctx, op, mode, n_seg, off, a, n_a, aidx, out);
  return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
}

int zkp_point_scan_batch(zkp_ctx* ctx, int mode, uint32_t n_seg, const uint32_t* off, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points, uint32_t n_points,
                         int n_threads, uint8_t* out, uint8_t* status) {
  if (mode != ZKP_SCAN_INCLUSIVE && mode != ZKP_SCAN_EXCLUSIVE) return ZKP_TB_BAD_STATEMENT;
  if (n_seg == 0) return ZKP_TB_OK;
  if (!off) return ZKP_TB_BAD_STATEMENT;
  const uint64_t min_terms = g_point_scan_min_terms.load();
  const bool host = !ctx || min_terms == UINT64_MAX || off[n_seg] < min_terms;
  const int rc = host ? zkp::hostbk::point_scan_n(mode, n_seg, off, pidx, neg, points, n_points, n_threads, out, status)
                      : zkp_scan_points(ctx, mode, n_seg, off, pidx, neg, points, n_points, out, status);
  return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
}

// ---- bounded discrete logarithms to the basepoint (zkp_mi355x.h (10)) behind the same routing ------------------------------------------------
int zkp_toolbox_set_dlog_baby_bits(uint32_t baby_bits) {
  if (baby_bits < 4 || baby_bits > 22) return ZKP_TB_BAD_STATEMENT;
  g_dlog_host_baby_bits = baby_bits;
  return ZKP_TB_OK;
}
uint32_t zkp_toolbox_get_dlog_baby_bits(void) { return g_dlog_host_baby_bits.load(); }
void zkp_toolbox_set_dlog_host_max_steps(uint32_t steps) { g_dlog_host_max_steps = steps; }
uint32_t zkp_toolbox_get_dlog_host_max_steps(void) { return g_dlog_host_max_steps.load(); }

// The host route halves every point once (spread over the threads by points), then cuts the search into (point, range of giant steps) items: with
// fewer points than threads a point's giant-step axis is split into ranges of whole inversion groups, which are searched independently (at most
// one of them finds the point's unique k).
// Routing: the host work of a call is n (J + 128) giant steps -- J = 2^(bits - host baby_bits) for a point that is not found, and 128 for its decode and
// halving, a 253-bit ladder.  A call with a context stays on the host while that work is at most host_max_steps PER THREAD, the threads counted up to 16
// (what was measured: profiles/dlog_bench.txt).
namespace {
const uint8_t kDlogBasepoint[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                    0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
unsigned dlog_threads(int n_threads) {
  const unsigned t = n_threads > 0 ? (unsigned)n_threads : std::thread::hardware_concurrency();
  return std::max(1u, std::min(t, 128u));
}
// the routing rule of both calls: group operations do not depend on the base
bool dlog_on_device(zkp_ctx* ctx, uint64_t n, uint32_t bits, unsigned t) {
  const uint32_t bb = g_dlog_host_baby_bits.load();
  const uint64_t J = bits <= bb ? 1ull : 1ull << (bits - bb);
  return ctx && n * (J + 128) > (uint64_t)g_dlog_host_max_steps.load() * std::min(t, 16u);
}
// the host route over a base that decodes (its table exists: built once, before the threads ask for it)
void dlog_host_route(const uint8_t base[32], uint64_t n, const uint8_t* points, uint32_t bits, bool is_signed, uint64_t* out, uint8_t* status, unsigned t) {
  const uint32_t bb = g_dlog_host_baby_bits.load();
  const uint64_t J = bits <= bb ? 1ull : 1ull << (bits - bb);
  constexpr size_t HB = zkp::hostbk::DLOG_HALF_BYTES;
  std::vector<uint8_t> halves(HB * (size_t)n), bad(n);
  uint8_t shift[HB];
  if (is_signed) zkp::hostbk::dlog_point_shift(base, bits, shift);
  const unsigned tp = (unsigned)std::min<uint64_t>(t, n);
  auto halve = [&](unsigned k) {
    for (uint64_t p = k; p < n; p += tp)
      bad[p] = zkp::hostbk::dlog_point_halve(points + 32 * (size_t)p, is_signed ? shift : nullptr, halves.data() + HB * (size_t)p) == ZKP_DLOG_INVALID;
  };
  if (tp <= 1) halve(0);
  else Pool::instance().run(tp, halve);
  const uint64_t groups = (J + zkp_dlog_group() - 1) / zkp_dlog_group();
  const uint64_t segs = std::max<uint64_t>(1, std::min<uint64_t>(groups, t / n));
  const uint64_t seg_len = ((groups + segs - 1) / segs) * zkp_dlog_group();
  const uint64_t items = n * segs;
  std::vector<uint64_t> ks(items);
  std::vector<uint8_t> sts(items);
  const unsigned ts = (unsigned)std::min<uint64_t>(t, items);
  auto work = [&](unsigned k) {
    for (uint64_t it = k; it < items; it += ts) {
      const uint64_t p = it / segs, lo = (it % segs) * seg_len, hi = std::min<uint64_t>(J, lo + seg_len);
      sts[it] = (uint8_t)ZKP_DLOG_NOT_FOUND;
      if (!bad[p] && lo < hi) sts[it] = (uint8_t)zkp::hostbk::dlog_point_range(base, halves.data() + HB * (size_t)p, bits, bb, is_signed, lo, hi, &ks[it]);
    }
  };
  if (ts <= 1) work(0);
  else Pool::instance().run(ts, work);
  for (uint64_t p = 0; p < n; ++p) {
    out[p] = 0;
    status[p] = bad[p] ? (uint8_t)ZKP_DLOG_INVALID : (uint8_t)ZKP_DLOG_NOT_FOUND;
    for (uint64_t s2 = 0; s2 < segs; ++s2)
      if (sts[p * segs + s2] == ZKP_DLOG_FOUND) { out[p] = ks[p * segs + s2]; status[p] = ZKP_DLOG_FOUND; }
  }
}
}  // namespace

int zkp_basepoint_dlog_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* points, uint32_t bits, uint64_t* out, uint8_t* status, int n_threads) {
  if (bits < 1 || bits > 48) return ZKP_TB_BAD_STATEMENT;
  if (n == 0) return ZKP_TB_OK;
  if (!points || !out || !status || n > 0x7fffffffull) return ZKP_TB_BAD_STATEMENT;
  const unsigned t = dlog_threads(n_threads);
  if (dlog_on_device(ctx, n, bits, t)) {
    const int rc = zkp_dlog_base(ctx, n, points, bits, out, status);
    return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
  }
  zkp::hostbk::dlog_prepare_table(g_dlog_host_baby_bits.load());
  dlog_host_route(kDlogBasepoint, n, points, bits, false, out, status, t);
  return ZKP_TB_OK;
}

// The same to a base of the caller's and over signed ranges (zkp_dlog_point).  The routing rule is the one above word for word.  On the device
// route the base's slot is the one the context already holds for it, else a free one, else the least recently used one
// (zkp_dlog_point_last_use), prepared with the default size of 2^16 rows.
int zkp_point_dlog_batch(zkp_ctx* ctx, const uint8_t base[32], uint64_t n, const uint8_t* points, uint32_t bits, int flags, uint64_t* out, uint8_t* status,
                         int n_threads) {
  if (bits < 1 || bits > 48 || (flags & ~ZKP_DLOG_SIGNED)) return ZKP_TB_BAD_STATEMENT;
  if (n == 0) return ZKP_TB_OK;
  if (!base || !points || !out || !status || n > 0x7fffffffull) return ZKP_TB_BAD_STATEMENT;
  static const uint8_t identity[32] = {};
  if (std::memcmp(base, identity, 32) == 0) return ZKP_TB_BAD_STATEMENT;
  const unsigned t = dlog_threads(n_threads);
  if (dlog_on_device(ctx, n, bits, t)) {
    int slot = zkp_dlog_point_find(ctx, base);
    if (slot < 0) {
      if (!zkp::hostbk::dlog_point_decodes(base)) return ZKP_TB_INVALID_POINT;       // (told apart from the context's other ZKP_ERR_ARG causes)
      uint64_t oldest = UINT64_MAX;
      for (uint32_t s = 0; s < ZKP_DLOG_SLOTS; ++s) {
        const uint64_t used = zkp_dlog_point_last_use(ctx, s);                 // (0: empty)
        if (used < oldest) { oldest = used; slot = (int)s; }
      }
      const int rc = zkp_ctx_prepare_dlog_point(ctx, (uint32_t)slot, base, 16);
      if (rc) return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
    }
    const int rc = zkp_dlog_point(ctx, (uint32_t)slot, n, points, bits, flags, out, status);
    return rc == ZKP_ERR_ARG ? ZKP_TB_BAD_STATEMENT : rc;
  }
  if (zkp::hostbk::dlog_point_prepare_table(base, g_dlog_host_baby_bits.load())) return ZKP_TB_INVALID_POINT;
  dlog_host_route(base, n, points, bits, (flags & ZKP_DLOG_SIGNED) != 0, out, status, t);
  return ZKP_TB_OK;
}

// n x Scalar::random (64 bytes of a ChaCha20 stream through from_bytes_mod_order_wide): element i from block i of (key, nonce)
int zkp_scalar_random_batch(zkp_ctx* ctx, uint64_t n, const uint8_t* key, uint64_t nonce, int n_threads, uint8_t* out) {
  if (n == 0) return ZKP_TB_OK;
  if (!out) return ZKP_TB_BAD_STATEMENT;
  uint8_t own[32];
  if (!key) {
    if (!os_entropy(own, sizeof(own))) return ZKP_TB_NO_ENTROPY;
    key = own;
  }
  if (!on_host(ctx, n)) return zkp_sc_random(ctx, n, key, nonce, out);
  if (n > 0xffffffffull) return ZKP_TB_BAD_STATEMENT;
  parallel_for((uint32_t)n, n_threads, [&](uint32_t lo, uint32_t hi) {
    uint8_t wide[64];
    for (uint64_t i = lo; i < hi; ++i) {
      zkp_chacha20_block(key, i, nonce, wide);
      zkp::hostbk::sc_from_wide_n(1, wide, out + 32 * (size_t)i);
    }
  });
  return ZKP_TB_OK;
}

// tests/sig_and_vrf_example.rs:36-40 for N transcripts.  Aligned batches of fused_min_batch or more squeeze on the device and map there
// (zkp_fused_hash_to_group); otherwise host Merlin on the host threads, then the map on the backend zkp_from_uniform_bytes_batch picks.
int zkp_hash_to_group_batch(zkp_ctx* ctx, uint32_t N, uint8_t* ts, const char* label, int n_threads, uint8_t* out) {
  if (!label) return ZKP_TB_BAD_STATEMENT;
  if (N == 0) return ZKP_TB_OK;
  if (!ts || !out) return ZKP_TB_BAD_STATEMENT;
  if (!fits_u32(std::strlen(label))) return ZKP_TB_TOO_LONG;
  if (ctx && use_fused(ts, N)) return zkp_fused_hash_to_group(ctx, N, ts, label, out);
  if (ctx && use_ragged(ts, N)) return zkp_fused_hash_to_group_ragged(ctx, N, ts, label, out);
  std::vector<uint8_t> wide(64 * (size_t)N);
  parallel_for(N, n_threads, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) {
      Transcript x = Transcript::from_bytes(ts + TB * (size_t)j);
      x.challenge_bytes(label, wide.data() + 64 * (size_t)j, 64);
      x.to_bytes(ts + TB * (size_t)j);
    }
  });
  return zkp_from_uniform_bytes_batch(ctx, N, wide.data(), n_threads, out);
}

int zkp_batch_verify_locate(zkp_ctx* ctx, const zkp_statement* st, uint32_t N, uint32_t n_transcripts, uint8_t* ts, const uint8_t* inst,
                            const uint8_t* common, const uint8_t* commitments, const uint8_t* responses, const uint8_t* weights16,
                            int n_threads, uint8_t* results) {
  if (!st || !results || (N && !ts)) return ZKP_TB_BAD_STATEMENT;
  if (n_transcripts != N) return ZKP_TB_BATCH_SIZE_MISMATCH;           // batch_verifier.rs:72-74
  std::memset(results, 0, N);
  const std::vector<uint8_t> saved(ts, ts + TB * (size_t)N);           // the per-proof pass starts where the batch check started
  const int rc = zkp_batch_verify(ctx, st, N, n_transcripts, ts, inst, common, commitments, responses, weights16, n_threads);
  if (rc != ZKP_TB_VERIFICATION_FAILURE || N == 0) return rc;
  std::vector<uint8_t> again(saved);
  // fresh per-proof weights (weights16 == NULL: from the OS): the batch weights are laid out [constraint][proof], these [proof][constraint]
  const int rc2 = zkp_verify_batchable_each(ctx, st, N, again.data(), inst, common, commitments, responses, nullptr, n_threads, results);
  if (rc2 < 0) return rc2;                                              // infrastructure failure: nothing may be trusted
  return ZKP_TB_VERIFICATION_FAILURE;
}

}  // extern "C"
